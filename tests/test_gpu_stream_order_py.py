"""Stream order of the Python surface: the drop-in (its unbound first call and
the shim's bound round), the proximal term's forward and backward, the
Comm.single() aggregators, the loaders and the checkpoint copy — each under
``torch.cuda.stream(S)`` through tests/streamgate.py, in arrangement A (behind
a running gate on ``S``, inputs poison before and after) and B (a gate on the
null stream, ``S`` idle), against the reference its family's test uses: the
reference loop on twins of the modules (torch's CPU or GPU order), the oracle
for the weighted round, float64 within the existing bounds for the proximal
term.  See tests/test_gpu_stream_order.py for the C ABI and the power check.

C3 runs the proximal term's forward on ``S1`` and its backward under ``S2``
behind a gate on ``S1``: autograd's contract is that the gradients are usable
on the stream that called backward().

A one-rank communicator runs every round form as one fa_reduce on the
caller's stream, so the aggregator cases here pin ``step(stream=...)`` and the
captured replay; the executor's joins between the caller's and the
communication stream need two ranks:
tests/test_gpu_loopback.py::test_loopback_rounds_behind_a_gate.

dist.py's rounds (C5) run over tests/distloop.py with every rank thread on a
side stream of its own behind its own gate; the stand-in synchronises the
sender's stream at each hand-over, so at W = 2 the gate condition covers what
a rank queues up to its first send (see _gated_loop).
"""
import copy
import functools

import numpy as np
import pytest
import torch

import feddct_amd
import prox16ref as P
import streamgate as SG
from feddct_amd import aggregate
from feddct_amd.layout import BucketLayout
from helpers import StateModule, bits_equal, buckets_to_state, states_to_buckets
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop
from test_gpu_h16_dropin import SHAPES, fill, manifest
from test_gpu_prox_edges import GRAD_BOUND, norm_bound, total_bound

pytestmark = pytest.mark.gpu

N = 5
TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


@pytest.fixture(scope="module")
def side():
    torch.cuda.set_device(0)
    S = torch.cuda.Stream()
    for arr in "AB":
        SG.power_check(arr, S)
    yield S
    print(SG.report())


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    feddct_amd.set_summation_order("torch_cpu")
    aggregate._ENGINE = None


def raw(t):
    """A tensor's bits on the host (numpy; bfloat16 as int16)."""
    return SG._np(t.detach().cpu().contiguous())


def same(got, ref_tensor, what):
    want = raw(ref_tensor)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
    iv = {2: np.uint16, 4: np.uint32, 8: np.int64}[got.dtype.itemsize]
    bad = np.nonzero(got.reshape(-1).view(iv) != want.reshape(-1).view(iv))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], got.reshape(-1)[bad[:4]],
                           want.reshape(-1)[bad[:4]])


def module_inputs(models):
    """One In per state tensor of every module; the getter follows the tensor
    into the arena its first round binds."""
    return [SG.In(v, get=(lambda m=m, k=k: m.state_dict()[k]))
            for m in models for k, v in m.state_dict().items()]


def state_list(models):
    return [v for m in models for v in m.state_dict().values()]


# ============================================================ C1: the drop-in ====
ORDERS = {
    "torch_cpu": (dict(order="torch_cpu"), "float32", "float32"),
    "torch_gpu": (dict(order="torch_gpu"), "float32", "float32"),
    "native16-fp16": (dict(order="torch_gpu", native16=True), "float16", "float16"),
    "native16-bf16": (dict(order="torch_gpu", native16=True), "bfloat16", "bfloat16"),
    "master-fp16": (dict(order="torch_gpu", native16=True, native16_master=True),
                    "float32", "float16"),
    "master-bf16": (dict(order="torch_gpu", native16=True, native16_master=True),
                    "float32", "bfloat16"),
}


def make_models(gdt, cdt, seed, shapes=SHAPES, pre="t"):
    g = fill(StateModule(manifest(gdt, shapes, pre)), 999 + seed).cuda()
    cl = [fill(StateModule(manifest(cdt, shapes, pre)), seed * 100 + i).cuda() for i in range(N)]
    return g, cl


def warm_plans(round_fn, gdt="float32", cdt="float32", **kw):
    """A round of other modules of the same layout first: plan creation
    uploads its tile table with a synchronous copy (include/fedagg.h), which
    waits for the null stream — arrangement B's gate.  The engine keeps its
    plans per layout, so the first call of the modules under test then binds
    its arenas and launches, and creates nothing."""
    wg, wcl = make_models(gdt, cdt, 50, **kw)
    round_fn(wg, wcl)
    torch.cuda.synchronize()


def reference_round(order, g, cl):
    """The reference's loop on twins: on the CPU for torch's CPU order, on the
    GPU (idle, null stream) for its GPU order."""
    rg, rc = copy.deepcopy(g), [copy.deepcopy(c) for c in cl]
    if order == "torch_cpu":
        rg, rc = rg.cpu(), [c.cpu() for c in rc]
    reference_loop(rg, rc)
    torch.cuda.synchronize()
    return rg, rc


def check_round(res, nkeys, rg, rc, what):
    k = 0
    for j, ref in enumerate([rg] + rc):
        for key, v in ref.state_dict().items():
            same(res.out[k], v, (what, "global" if j == 0 else f"client {j - 1}", key))
            k += 1
    assert k == len(res.out) == nkeys * (1 + len(rc))


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("second", [False, True], ids=["first-call", "bound-round"])
@pytest.mark.parametrize("name", sorted(ORDERS))
def test_server_aggregate(side, name, second, arr):
    """server_aggregate's first call (arenas bound, staging copies through
    torch, reduce + broadcast) and its second (the shim's bound_round), per
    summation order; then one more round on the default stream with the same
    binding."""
    kw, gdt, cdt = ORDERS[name]
    feddct_amd.set_summation_order(kw["order"], **{k: v for k, v in kw.items() if k != "order"})
    g, cl = make_models(gdt, cdt, 1)
    warm_plans(lambda a, b: feddct_amd.server_aggregate(a, b), gdt, cdt)
    if second:
        feddct_amd.server_aggregate(g, cl)
        torch.cuda.synchronize()
        assert aggregate.engine()._round is not None, "the first call bound no round"
        gen = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for c in cl:
                for v in c.state_dict().values():
                    if v.dtype == torch.int64:
                        v.add_(3)
                    else:
                        v.add_((torch.randn(v.shape, generator=gen) * 0.01).to(v.dtype).cuda())
        torch.cuda.synchronize()
    rg, rc = reference_round(kw["order"], g, cl)
    inputs = module_inputs(cl)
    calls = []
    if second:
        e = aggregate.engine()
        orig = e._run_bound
        e._run_bound = lambda r, w=None: calls.append(r) or orig(r, w)
    res = SG.run(arr, side, lambda st: feddct_amd.server_aggregate(g, cl), inputs,
                 lambda: state_list([g] + cl), (name, second), out_like=state_list([g] + cl))
    if second:
        del aggregate.engine()._run_bound
        assert len(calls) == 1 and aggregate.engine()._round is calls[0], "not the bound round"
    assert aggregate.engine().gpu_order_fallbacks == {}
    check_round(res, len(g.state_dict()), rg, rc, (name, second, arr))
    if arr == "A":
        SG.assert_poison2(res, inputs, (name, second))
    if second:      # the same binding, on the default stream
        for i in inputs:
            i.t.copy_(i.real)
        torch.cuda.synchronize()
        feddct_amd.server_aggregate(g, cl)
        torch.cuda.synchronize()
        for m, r in zip([g] + cl, [rg] + rc):
            for key, v in r.state_dict().items():
                same(raw(m.state_dict()[key]), v, (name, "default stream", key))


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("second", [False, True], ids=["first-call", "bound-round"])
def test_aggregate_weighted(side, second, arr):
    g, cl = make_models("float32", "float32", 2)
    w = T.weights_from_sizes(np.arange(10, 10 + N))
    warm_plans(lambda a, b: aggregate.aggregate_weighted(a, b, weights=w))
    if second:
        aggregate.aggregate_weighted(g, cl, weights=w)
        torch.cuda.synchronize()
    want = {}
    for key, v in g.state_dict().items():
        x = np.stack([raw(c.state_dict()[key]) for c in cl])
        if v.dtype == torch.int64:
            want[key] = T.mean_i64_trunc(x.reshape(N, -1)).reshape(v.shape)
        else:
            want[key] = T.weighted_sum0(x.reshape(N, -1), w).reshape(v.shape)
    inputs = module_inputs(cl)
    res = SG.run(arr, side, lambda st: aggregate.aggregate_weighted(g, cl, weights=w), inputs,
                 lambda: state_list([g] + cl), ("weighted", second),
                 out_like=state_list([g] + cl))
    keys = list(g.state_dict())
    for j in range(1 + N):
        for i, key in enumerate(keys):
            assert bits_equal(res.out[j * len(keys) + i], want[key]), (second, arr, j, key)
    if arr == "A":
        SG.assert_poison2(res, inputs, ("weighted", second))


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("second", [False, True], ids=["first-call", "bound-round"])
def test_server_aggregate_split(side, second, arr):
    gm, clm = make_models("float32", "float32", 3, SHAPES[:5], "m")
    gp, clp = make_models("float32", "float32", 4, SHAPES[4:], "p")
    wm, wcm = make_models("float32", "float32", 50, SHAPES[:5], "m")
    wp, wcp = make_models("float32", "float32", 51, SHAPES[4:], "p")
    aggregate.server_aggregate_split(wm, wp, wcm, wcp)
    torch.cuda.synchronize()
    if second:
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        torch.cuda.synchronize()
    rgm, rcm = reference_round("torch_cpu", gm, clm)
    rgp, rcp = reference_round("torch_cpu", gp, clp)
    inputs = module_inputs(clm + clp)
    mods = [gm] + clm + [gp] + clp
    res = SG.run(arr, side, lambda st: aggregate.server_aggregate_split(gm, gp, clm, clp), inputs,
                 lambda: state_list(mods), ("split", second), out_like=state_list(mods))
    k = 0
    for m in [rgm] + rcm + [rgp] + rcp:
        for key, v in m.state_dict().items():
            same(res.out[k], v, ("split", second, arr, key))
            k += 1
    assert k == len(res.out)
    if arr == "A":
        SG.assert_poison2(res, inputs, ("split", second))


# ==================================================== C2 / C3: the proximal term ====
MU = 0.37      # loss = 0.5 * mu * term: a MulBackward feeds the node
FORMS = {      # name -> (client dtype, global dtype, flat_grads)
    "default-node": ("float32", "float32", False),
    "flat-cpp-node": ("float32", "float32", True),
    "flat-python-bf16": ("bfloat16", "bfloat16", True),
    "flat-python-fp16": ("float16", "float16", True),
    "client16-global32": ("bfloat16", "float32", False),
}


def prox_pair(cdt, gdt, seed):
    """test_gpu_prox16_module's pair: the client the global plus 0.05 randn."""
    from test_gpu_prox16_module import Net
    torch.manual_seed(seed)
    g = Net()
    c = copy.deepcopy(g)
    with torch.no_grad():
        for p in c.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return c.to(TDT[cdt]).cuda(), g.to(TDT[gdt]).cuda()


def prox_reference(c, g):
    """The float64 model of test_gpu_prox16_module._check_step, from the
    values the pair holds now: per parameter d = w - w_t and its norm."""
    with torch.no_grad():
        d = [(w.detach().cpu() - w_t.detach().cpu()).double()
             for w, w_t in zip(c.parameters(), g.parameters())]
    return d, [float(x.norm(2)) for x in d]


def host_double(a):
    """A harness output (numpy; bfloat16 as its int16 bits) as float64."""
    a = np.atleast_1d(a)
    if a.dtype == np.int16:
        return torch.from_numpy(a).view(torch.bfloat16).double()
    return torch.from_numpy(a.astype(np.float64))


def check_prox(term, grads, prior, c, d, n64, cdt, gdt, what):
    """term and gradients (numpy, client's then global's) within the budgets
    of test_gpu_prox16_module; ``prior``: the .grad each parameter held
    before, or None."""
    pure = gdt != "float32"
    params = list(c.parameters())
    K = len(params)
    chunks = [-(-p.numel() // P.CHUNK) for p in params]
    tv = float(host_double(term)[0])
    if pure:
        beta = max(P.norm_beta(p.numel()) for p in params)
        lim = (2 * (P.U16[cdt] + beta) + 2 * (K - 1) * P.U16[cdt]) * sum(n64)
        assert abs(tv - float(torch.tensor(sum(n64)).to(TDT[cdt]))) <= lim + P.U16[cdt] * sum(n64), \
            (what, tv, sum(n64))
        scale = float(torch.tensor(0.5 * MU).to(TDT[cdt]))
    else:
        assert abs(tv - sum(n64)) <= total_bound(chunks) * sum(n64), (what, tv, sum(n64))
        scale = float(np.float32(0.5 * MU))
    k = 0
    for side, sign, dt in (("client", 1.0, cdt), ("global", -1.0, gdt)):
        for j in range(K):
            want = sign * scale * d[j] / n64[j]
            got = host_double(grads[k])
            if dt == "float32":
                lim = (GRAD_BOUND + norm_bound(chunks[j])) * want.abs()
            else:
                lim = torch.from_numpy(P.grad_limit(want.numpy(), dt))
            if prior is not None:       # one more fp32 add of the accumulation
                assert dt == "float32"
                want = want + prior[k].double()
                lim = lim + 2.0 ** -24 * want.abs()
            assert got.shape == want.shape
            assert bool(((got - want).abs() <= lim).all()), (what, side, j)
            k += 1
    assert k == len(grads)


def prox_case(name, preexisting=False):
    cdt, gdt, flat = FORMS[name]
    from feddct_amd.prox import proximal_term
    c, g = prox_pair(cdt, gdt, 51)
    params = list(c.parameters()) + list(g.parameters())
    (proximal_term(c, g, flat_grads=flat) * 0.5).backward()      # binds the arenas and the term
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    # other values than the binding call's: what that call left in the plan's
    # scratch (partial sums, norms) must not pass for this call's
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for p in c.parameters():
            p.add_((0.03 * torch.randn(p.shape, generator=gen)).to(p.dtype).cuda())
    torch.cuda.synchronize()
    d, n64 = prox_reference(c, g)
    inputs = [SG.In(p, get=(lambda p=p: p)) for p in params]
    prior = None
    if preexisting:       # .grad tensors that are not the bucket's views (a task loss's)
        gen = torch.Generator(device="cuda").manual_seed(3)
        prior = [torch.randn(p.shape, device="cuda", generator=gen) for p in params]
        for p, q in zip(params, prior):
            p.grad = q.clone()
        inputs += [SG.In(p.grad) for p in params]
        prior = [q.cpu() for q in prior]
    return SimpleCase(c, g, params, d, n64, inputs, prior, cdt, gdt, flat)


class SimpleCase:
    def __init__(self, *a):
        (self.c, self.g, self.params, self.d, self.n64, self.inputs, self.prior, self.cdt, self.gdt,
         self.flat) = a

    def like(self):
        term = torch.empty((), dtype=TDT[self.cdt] if self.gdt != "float32" else torch.float32,
                           device="cuda")
        return [term] + [torch.empty_like(p) for p in self.params]


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("name", sorted(FORMS))
def test_proximal_term_forward_and_backward_on_one_stream(side, name, arr):
    from feddct_amd.prox import proximal_term
    k = prox_case(name)
    box = {}

    def call(st):
        box["term"] = proximal_term(k.c, k.g, flat_grads=k.flat)
        (0.5 * MU * box["term"]).backward()

    res = SG.run(arr, side, call, k.inputs, lambda: [box["term"]] + [p.grad for p in k.params],
                 (name, "C2"), out_like=k.like())
    check_prox(res.out[0], res.out[1:], None, k.c, k.d, k.n64, k.cdt, k.gdt, (name, arr))
    if arr == "A":
        SG.assert_poison2(res, k.inputs, name)


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("name", ["default-node", "flat-cpp-node"])
def test_proximal_term_accumulates_onto_existing_grads(side, name, arr):
    """Every parameter already holds a .grad that is no view of the term's
    gradient bucket (a task loss's backward came first): the one-node forms
    take those over — copies made inside the node — and accumulate."""
    from feddct_amd.prox import proximal_term
    k = prox_case(name, preexisting=True)
    box = {}

    def call(st):
        box["term"] = proximal_term(k.c, k.g, flat_grads=k.flat)
        (0.5 * MU * box["term"]).backward()

    res = SG.run(arr, side, call, k.inputs, lambda: [box["term"]] + [p.grad for p in k.params],
                 (name, "C2 accumulate"), out_like=k.like())
    check_prox(res.out[0], res.out[1:], k.prior, k.c, k.d, k.n64, k.cdt, k.gdt, (name, arr))
    if arr == "A":
        SG.assert_poison2(res, k.inputs, name)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_forward_on_one_stream_backward_on_another(name):
    """C3.  Forward under S1; S2 waits for S1; a gate on S1; backward() under
    S2; the .grad read on S2.  The node's launches go to the forward's stream
    behind the gate, so the gradients are right on S2 only if the stream that
    called backward() is made to wait for them."""
    from feddct_amd.prox import proximal_term
    torch.cuda.set_device(0)
    k = prox_case(name)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    hosts = [SG._pinned_like(t) for t in k.like()]
    g_end = torch.cuda.Event()
    with torch.cuda.stream(S1):
        term = proximal_term(k.c, k.g, flat_grads=k.flat)
        loss = 0.5 * MU * term
    S2.wait_stream(S1)
    with torch.cuda.stream(S1):
        torch.cuda._sleep(SG.gate_cycles())
        g_end.record()
    with torch.cuda.stream(S2):
        loss.backward()
        for h, t in zip(hosts, [term] + [p.grad for p in k.params]):
            h.copy_(t.detach(), non_blocking=True)
    running = not g_end.query()
    S2.synchronize()
    got = [SG._np(h) for h in hosts]
    torch.cuda.synchronize()
    assert running, (name, "gate too short / call blocked the host")
    check_prox(got[0], got[1:], None, k.c, k.d, k.n64, k.cdt, k.gdt, (name, "C3"))


# ============================================== C4: Comm.single() aggregators ====
def small_layout():
    """tests/test_gpu_loopback.py::_small_layout restated, ``c`` cut to 6500
    floats (its _deep_layout): every column class the schedules separate."""
    return BucketLayout([("a", (37, 3), "float32"), ("s", (), "float32"),
                         ("b", (4101,), "float32"), ("t", (), "float32"),
                         ("c", (6500,), "float32"), ("d", (3,), "float32"),
                         ("e", (193,), "float32"), ("n1", (), "int64"),
                         ("f", (65, 65), "float32"), ("n2", (), "int64")])


@functools.lru_cache(maxsize=None)
def layout_states(n, seed):
    layout = small_layout()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        st = []
        for s in layout.slots:
            if s.kind == "i64":
                st.append((s.key, rng.integers(0, 1 << 40, s.shape).astype(np.int64)))
            else:
                st.append((s.key, (rng.standard_normal(s.shape) * 0.05).astype(np.float32)))
        out.append(st)
    return out


AGG_N = 20


def agg_weights():
    return T.weights_from_sizes(np.arange(3, 3 + AGG_N))


@functools.lru_cache(maxsize=None)
def agg_reference(weighted, r):
    """The oracle per key for round r's clients, computed once."""
    out = {}
    states = layout_states(AGG_N, 10 + r)
    for s in small_layout().slots:
        x = np.stack([dict(st)[s.key].reshape(-1) for st in states])
        if s.kind == "i64":
            out[s.key] = T.mean_i64_trunc(x).reshape(-1)
        else:
            out[s.key] = (T.weighted_sum0(x, agg_weights()) if weighted
                          else T.torch_mean0(x)).reshape(-1)
    return out


AGGS = ["NativeShardedAggregator", "NativeStripedAggregator", "NativeChainedAggregator",
        "NativeBlockedAggregator", "NativeAggregator"]      # the last: fa_reduce_multi


@pytest.fixture(scope="module")
def comm():
    from feddct_amd.comm import Comm
    torch.cuda.set_device(0)
    c = Comm.single()
    yield c
    c.set_graphs(False)


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("graphs", [False, True], ids=["issued", "captured"])
@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("agg", AGGS)
def test_native_aggregators_step_on_a_side_stream(side, comm, agg, weighted, graphs, arr):
    """Two rounds with fresh inputs, no synchronisation between them:
    ``step(stream=S.cuda_stream)`` twice inside one gated bracket, the second
    round's inputs copied in on S between them.  With graphs on, a round
    before the bracket captures on S and both steps replay there."""
    from feddct_amd import comm as C
    n = AGG_N
    layout = small_layout()
    states = [layout_states(n, 10 + r) for r in (0, 1)]
    dev = torch.device("cuda", 0)
    bk = states_to_buckets(layout, states[0], dev)
    nxt = states_to_buckets(layout, states[1], dev)
    out32 = torch.full((max(layout.f32_numel, 64),), float("nan"), device=dev)
    out64 = torch.full((max(layout.i64_numel, 1),), -7, dtype=torch.int64, device=dev)
    keep32, keep64 = torch.full_like(out32, float("nan")), torch.full_like(out64, -7)
    w = agg_weights() if weighted else None
    comm.set_graphs(graphs)
    a = getattr(C, agg)(layout, [b[0] for b in bk], [b[1] for b in bk], n, out32, out64, comm,
                        weights=None if w is None else [float(x) for x in w])
    if graphs:      # (capture needs the plan's lazy allocations made: one round first)
        a.step(stream=side.cuda_stream)
        torch.cuda.synchronize()
        out32.fill_(float("nan"))
        out64.fill_(-7)
    inputs = [SG.In(t) for b in bk for t in b] + [SG.In(t) for b in nxt for t in b]

    def call(st):
        a.step(stream=st.cuda_stream)
        keep32.copy_(out32, non_blocking=True)
        keep64.copy_(out64, non_blocking=True)
        for b, m in zip(bk, nxt):
            b[0].copy_(m[0], non_blocking=True)
            b[1].copy_(m[1], non_blocking=True)
        a.step(stream=st.cuda_stream)

    res = SG.run(arr, side, call, inputs, [keep32, keep64, out32, out64] + [t for b in bk for t in b],
                 (agg, weighted, graphs))
    comm.set_graphs(False)
    for r in (0, 1):
        got = dict(buckets_to_state(layout, torch.from_numpy(res.out[2 * r]),
                                    torch.from_numpy(res.out[2 * r + 1])))
        want = agg_reference(weighted, r)       # (one rank: every form is one fa_reduce, exact)
        for s in layout.slots:
            assert bits_equal(got[s.key].reshape(-1), want[s.key]), \
                (agg, weighted, graphs, arr, "round", r, s.key)
    for j, b in enumerate(nxt):      # a round never writes its inputs
        assert np.array_equal(res.out[4 + 2 * j], raw(inputs[2 * n + 2 * j].real)), (agg, j)
        assert np.array_equal(res.out[5 + 2 * j], raw(inputs[2 * n + 2 * j + 1].real)), (agg, j)
    if arr == "A":
        SG.assert_poison2(res, inputs, agg)


@pytest.mark.parametrize("arr", ["A", "B"])
@pytest.mark.parametrize("entry", ["fa_mean_f32_multi", "fa_mean_f32_multi_ex"])
def test_mean_f32_multi_on_a_side_stream(side, comm, entry, arr):
    """The stateless fp32 form of the default round on the one-rank
    communicator, its plan cached in the communicator by a call beforehand
    (plan creation uploads synchronously)."""
    import ctypes

    from feddct_amd import _lib
    from feddct_amd import comm as C
    n = AGG_N
    layout = small_layout()
    dev = torch.device("cuda", 0)
    bk = states_to_buckets(layout, layout_states(n, 10), dev)
    out = torch.full((max(layout.f32_numel, 64),), float("nan"), device=dev)
    ptrs = _lib.ptr_array([b[0].data_ptr() for b in bk])
    segs, nseg = _lib.seg_array(layout.segs32)
    counts = (ctypes.c_int * 1)(n)

    def call(st):
        args = (comm.handle, ptrs, counts, layout.f32_numel, out.data_ptr(), segs, nseg, 0)
        if entry == "fa_mean_f32_multi_ex":
            args += (0,)
        _lib.check(getattr(C.lib(), entry)(*args, ctypes.c_void_p(st.cuda_stream)), entry)

    call(torch.cuda.current_stream())
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    inputs = [SG.In(b[0]) for b in bk]
    res = SG.run(arr, side, call, inputs, [out], entry)
    want = agg_reference(False, 0)
    for s in layout.slots:
        if s.kind != "i64":
            assert bits_equal(res.out[0][s.offset:s.offset + s.numel], want[s.key]), (entry, arr, s.key)
    if arr == "A":
        SG.assert_poison2(res, inputs, entry)


# ================================================================ C5: dist.py ====
def _gated_loop(world):
    """tests/distloop.py's stand-in, noting per rank whether its gate still ran
    at its first hand-over to the transport.  The stand-in synchronises the
    sender's stream at every send and collective (its rule: the payload is
    complete when handed over), so from a rank's first send on its gate is
    over: at W > 1 the condition "every launch was queued while the inputs
    were poison" can hold, and is checked, for what the rank queued up to
    that point; at W = 1 nothing is sent and it is checked when step returns."""
    from distloop import LoopDist

    class GatedLoop(LoopDist):
        def __init__(self, world):
            super().__init__(world, timeout=30.0)
            self.gate_end, self.at_first_send = {}, {}

        def _payload(self, t):
            r = self.get_rank()
            if r in self.gate_end and r not in self.at_first_send:
                self.at_first_send[r] = not self.gate_end[r].query()
            return LoopDist._payload(t)

    return GatedLoop(world)


def run_dist_case(monkeypatch, W, bind):
    """Arrangement A per rank thread, each on a side stream of its own:
    ``bind(rank)`` -> (step, input tensors, output tensors) with the
    aggregator built (its plans uploaded) before the gate.  Returns per rank
    the outputs right after the step and the inputs as copied out with them."""
    import feddct_amd.dist as D
    from distloop import run_ranks
    loop = _gated_loop(W)
    monkeypatch.setattr(D, "dist", loop)
    dev = torch.device("cuda", 0)

    def fn(rank):
        step, tensors, outs = bind(rank)
        S = torch.cuda.Stream()
        inputs = [SG.In(t) for t in tensors]
        hosts = [SG._pinned_like(t) for t in outs + tensors]
        g_end = torch.cuda.Event()
        cycles = SG.gate_cycles()
        S.wait_stream(torch.cuda.current_stream())       # the set-up above, on the null stream
        with torch.cuda.stream(S):
            for i in inputs:
                i.t.fill_(i.p1)
            torch.cuda._sleep(cycles)
            g_end.record()
            loop.gate_end[rank] = g_end
            for i in inputs:
                i.t.copy_(i.real, non_blocking=True)
            step()
            running = loop.at_first_send.get(rank, not g_end.query())
            for h, t in zip(hosts, outs + tensors):
                h.copy_(t, non_blocking=True)
            for i in inputs:
                i.t.fill_(i.p2)
        S.synchronize()
        got = [SG._np(h) for h in hosts]
        after = [SG._np(i.t.cpu()) for i in inputs]
        for i, a in zip(inputs, after):
            want = SG._np(torch.empty(1, dtype=i.t.dtype).fill_(i.p2))[0]
            assert (a == want).all(), (rank, "an input written after the step's place in the stream")
        return dict(running=running, out=got[:len(outs)], ins=got[len(outs):],
                    real=[SG._np(i.real.cpu()) for i in inputs])

    res = run_ranks(W, fn, device=dev)
    for r, x in enumerate(res):
        assert x["running"], (r, "gate too short / call blocked the host")
        for a, b in zip(x["ins"], x["real"]):
            assert np.array_equal(a, b), (r, "the round wrote a client bucket")
    return res


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("form,weighted", [("striped", False), ("striped", True),
                                           ("chained", False), ("chained", True),
                                           ("sharded", False)])     # (e1 takes no weights)
def test_dist_rounds_each_rank_on_its_own_stream(monkeypatch, side, form, weighted, W):
    """StripedAggregator.step_device, ChainAggregator.step and
    ShardedAggregator.step with their HIP backends over tests/distloop.py,
    n = 5 on test_distloop_cpu's layout A, the result on every rank, against
    the references of tests/test_gpu_dist_loopback.py."""
    import feddct_amd.dist as D
    import test_distloop_cpu as DL
    n, lay = 5, "A"
    layout = DL.layout_of(lay)
    ids = tuple(range(n))
    dev = torch.device("cuda", 0)
    w = DL.sizes_weights(n, 0) if weighted else None
    counts = [n] if W == 1 else [3, 2]

    def bind(rank):
        out32, out64 = DL.fresh_out(layout, dev)
        a = sum(counts[:rank])
        b = a + counts[rank]
        bk = DL.clients_on(lay, ids[a:b], dev)
        l32, l64 = [x[0] for x in bk], [x[1] for x in bk]
        wl = None if w is None else w[a:b]
        if form == "striped":
            agg = D.StripedAggregator(layout, n, out32, out64, final="allreduce", root=0,
                                      nchunks=4, counts=counts)
            assert isinstance(agg.backend, D.HipStripeBackend)
            step = lambda: agg.step_device(l32, l64, wl)      # noqa: E731
        elif form == "chained":
            agg = D.ChainAggregator(layout, n, out32, out64, final="allreduce", root=0,
                                    nchunks=16, counts=counts)
            assert isinstance(agg.backend, D.HipChainBackend)
            step = lambda: agg.step(l32, l64, wl)             # noqa: E731
        else:
            assert (a, b) == D.shard_range(n, W, rank)
            agg = D.ShardedAggregator(layout, l32, l64, n, out32, out64, nchunks=3,
                                      final="allreduce", root=0, exchange="reduce")
            assert isinstance(agg.backend, D.HipBackend)
            step = agg.step
        return step, l32 + l64, [out32, out64]

    res = run_dist_case(monkeypatch, W, bind)
    want = DL.expected_e1(lay, ids, W) if form == "sharded" else DL.expected_exact(lay, ids, weighted, 0)
    for r, x in enumerate(res):
        DL.assert_state(layout, torch.from_numpy(x["out"][0]), torch.from_numpy(x["out"][1]), want,
                        (form, W, weighted, r))


@pytest.mark.parametrize("W", [1, 2])
def test_dist_striped_bf16_native16_each_rank_on_its_own_stream(monkeypatch, side, W):
    """The striped round on a bfloat16 ``native16`` layout (tests/round16.py's
    layout A, clients and oracle), step_device, n = 5."""
    import feddct_amd.dist as D
    import round16 as R
    dtype, n = "bfloat16", 5
    lay = R.layout_of("A", dtype)
    bits, i64 = R.clients16("A", dtype, n, seed=21)
    dev = torch.device("cuda", 0)
    counts = [n] if W == 1 else [3, 2]

    def bind(rank):
        out16 = R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype, dev)
        out64 = torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64, device=dev)
        agg = D.StripedAggregator(lay, n, out16, out64, final="allreduce", root=0, nchunks=3,
                                  counts=counts)
        assert isinstance(agg.backend, D.HipStripeBackend) and agg.backend.esize == 2
        a = sum(counts[:rank])
        b = a + counts[rank]
        l16 = [R.as_tensor(bits[k], dtype, dev) for k in range(a, b)]
        l64 = [torch.from_numpy(i64[k].copy()).to(dev) for k in range(a, b)]
        return (lambda: agg.step_device(l16, l64)), l16 + l64, [out16, out64]

    res = run_dist_case(monkeypatch, W, bind)
    exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
    for r, x in enumerate(res):
        assert R.same16(x["out"][0].view(np.uint16)[inside], exp[inside], dtype), (W, r)
        if lay.i64_numel:
            assert np.array_equal(x["out"][1][:lay.i64_numel], e64), (W, r)


# ================================================ C6: loaders and checkpoints ====
@pytest.mark.parametrize("arr", ["A", "B"])
def test_make_clients_and_reducer_on_a_side_stream(side, arr):
    """workload.make_clients (allocation, the synthetic fills) and
    Reducer.__call__(stream) queued on S: the reduce sees the filled buckets.
    The outputs are the only operands the test owns: the sentinel logic.  The
    Reducer is handed its plan: creating one uploads the tile table with a
    synchronous copy (include/fedagg.h), which waits for the null stream —
    arrangement B's gate — whatever stream the launches ride."""
    from conftest import load_manifest
    from feddct_amd import _lib, synth
    from feddct_amd.workload import Reducer, make_clients
    man = {"name": "so", "keys": load_manifest("wrn16_8_c10")["keys"][:12]}
    layout = BucketLayout.from_manifest(man)
    dev = torch.device("cuda", 0)
    out32 = torch.full((max(layout.f32_numel, 64),), float("nan"), device=dev)
    out64 = torch.full((max(layout.i64_numel, 1),), -7, dtype=torch.int64, device=dev)
    with torch.cuda.stream(side):          # the slab and torch's pool for S, before the gate
        warm = make_clients(layout, man, range(N), dev)
    torch.cuda.synchronize()
    del warm
    plan = _lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel)
    box = {}

    def call(st):
        box["cl"] = make_clients(layout, man, range(N), dev)
        box["r"] = Reducer(layout, box["cl"], out32, out64, plan=plan)
        box["r"](st.cuda_stream)

    res = SG.run(arr, side, call, [], [out32, out64], "make_clients + Reducer")
    want = dict(T.aggregate_state([synth.gen_state(man, i) for i in range(N)]))
    for key, v in buckets_to_state(layout, torch.from_numpy(res.out[0]),
                                   torch.from_numpy(res.out[1])):
        assert bits_equal(v, want[key]), (arr, key)


def test_checkpoint_copy_after_a_gated_round(side):
    """checkpoint.bucket_state_dict right after a gated server_aggregate, both
    under S: it synchronises the current stream, so the copy holds the round's
    result (arrangement A; the gate must still run when the round's call
    returns)."""
    from feddct_amd.checkpoint import bucket_state_dict
    g, cl = make_models("float32", "float32", 6)
    feddct_amd.server_aggregate(g, cl)          # bind
    torch.cuda.synchronize()
    inputs = module_inputs(cl)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for i in inputs:
            if i.real.dtype == torch.int64:
                i.real.add_(5)
            else:
                i.real.add_((torch.randn(i.real.shape, generator=gen) * 0.01).cuda())
            i.t.copy_(i.real)
    torch.cuda.synchronize()
    rg, _ = reference_round("torch_cpu", g, cl)
    for i in inputs:
        i.t.fill_(i.p1)
    torch.cuda.synchronize()
    g_end = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SG.gate_cycles())
        g_end.record()
        for i in inputs:
            i.t.copy_(i.real, non_blocking=True)
        feddct_amd.server_aggregate(g, cl)
        running = not g_end.query()
        sd = bucket_state_dict(g)
        for i in inputs:
            i.t.fill_(i.p2)
    torch.cuda.synchronize()
    assert running, "gate too short / call blocked the host"
    for key, v in rg.state_dict().items():
        same(raw(sd[key]), v, ("checkpoint", key))

