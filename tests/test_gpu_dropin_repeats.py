"""GPU: the drop-in with the global model among the clients and with a client
listed more than once.  The reference's torch.stack([...]).mean(0) accepts
both — clients sampled with replacement, a server that takes part in its own
round — and in the drop-in both reach the kernels as aliasing: one arena per
module, so server_aggregate(g, [g, c1]) launches with out == c[0] and
[c1, c2, c1] with a repeated pointer, the fused broadcast then writing one
bucket twice.  Every round is compared bit for bit, global and EVERY client,
int64 keys included, with the reference's own loop (oracle.torch_mirror
.reference_loop) on copies taken in one deepcopy of (global, clients), which
keeps the sharing; each list runs three rounds with the clients perturbed in
between, so the second and third take the bound round."""
import copy
import sys

import numpy as np
import pytest
import torch

from feddct_amd import synth
from helpers import StateModule, bits_equal
from oracle import torch_order as O
from oracle.torch_mirror import reference_loop

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")

MAN = {"keys": [{"key": "conv.weight", "shape": [16, 3, 3, 3], "dtype": "float32"},
                {"key": "bn.weight", "shape": [16], "dtype": "float32"},
                {"key": "bn.num_batches_tracked", "shape": [], "dtype": "int64"},
                {"key": "fc.weight", "shape": [10, 100], "dtype": "float32"},
                {"key": "fc.bias", "shape": [10], "dtype": "float32"},
                {"key": "odd", "shape": [3, 11], "dtype": "float32"},
                {"key": "scale", "shape": [], "dtype": "float32"}]}
MAN_B = {"keys": [{"key": "head.weight", "shape": [7, 33], "dtype": "float32"},
                  {"key": "head.bias", "shape": [7], "dtype": "float32"},
                  {"key": "steps", "shape": [], "dtype": "int64"}]}

# the bound round needs PEP 509 dict tags (CPython < 3.12); without them every
# call takes the full path and only the results are compared
HAS_FAST_PATH = sys.version_info < (3, 12)

# g: the global model; 1, 2: two more modules
LISTS = {"g12": ("g", 1, 2), "121": (1, 2, 1), "1g1": (1, "g", 1)}


def _modules(man, device, dtype=None, mode=synth.MODE_ADVERSARIAL, first=0):
    """{"g", 1, 2} -> module, every one with values of its own (the global
    too: it is a client in some lists)."""
    out = {}
    for i, name in enumerate(("g", 1, 2)):
        m = StateModule(man).load_numpy(synth.gen_state(man, first + i, mode))
        if dtype is not None:
            m = m.to(dtype)
        out[name] = m.to(device)
    return out


def _perturb(mods, step):
    with torch.no_grad():
        for i, m in enumerate(mods.values()):
            for t in m.state_dict().values():
                if t.is_floating_point():
                    t.mul_(1.0 + 0.25 * (i + 1)).add_(0.125 * (step + i))
                else:
                    t.add_(3 * i + step + 1)


def _same(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return bits_equal(a.numpy(), b.numpy())
    if a.is_floating_point():       # fp16 / bf16: no NaN in these rounds
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


def _assert_round_equals(g, clients, ref_g, ref_c, what):
    for m, r, who in [(g, ref_g, "global")] + [(c, rc, f"client {i}") for i, (c, rc)
                                                in enumerate(zip(clients, ref_c))]:
        sd, rsd = m.state_dict(), r.state_dict()
        assert list(sd) == list(rsd)
        for k in rsd:
            assert _same(sd[k], rsd[k]), (what, who, k)


def _reference(g, clients, on_cpu=True):
    """The reference's loop on ONE deepcopy of (global, clients): the copy
    keeps the same object twice, and the global inside the list."""
    ref_g, ref_c = copy.deepcopy((g, clients))
    if on_cpu:      # torch's CPU order: the default, device-independent definition
        for m in [ref_g] + list(ref_c):
            m.cpu()
    reference_loop(ref_g, ref_c)
    return ref_g, ref_c


class _Spy:
    """try_bound_round's return values, as
    test_bound_round_fast_path_sees_every_change observes them."""

    def __init__(self, attr="try_bound_round"):
        from feddct_amd import aggregate as A
        self.e, self.attr, self.calls = A.engine(), attr, []

    def __enter__(self):
        orig = getattr(self.e, self.attr)

        def spy(*a, **k):
            r = orig(*a, **k)
            self.calls.append(r)
            return r
        setattr(self.e, self.attr, spy)
        return self

    def __exit__(self, *exc):
        delattr(self.e, self.attr)


def _three_rounds(mods, names, call, on_cpu=True, expect_bound=True):
    g = mods["g"]
    clients = [mods[x] for x in names]
    with _Spy() as spy:
        for step in range(3):
            _perturb(mods, step)
            ref_g, ref_c = _reference(g, clients, on_cpu)
            spy.calls.clear()
            call(g, clients)
            torch.cuda.synchronize()
            _assert_round_equals(g, clients, ref_g, ref_c, (names, step))
            if expect_bound and HAS_FAST_PATH:    # the repeat calls take the bound round
                assert spy.calls and spy.calls[0] == (step > 0), (names, step, spy.calls)


@pytest.mark.parametrize("which", sorted(LISTS))
def test_fp32_lists_three_rounds(which):
    from feddct_amd import aggregate as A
    from feddct_amd.fedavg import server_aggregate
    mods = _modules(MAN, DEV)
    _three_rounds(mods, LISTS[which], server_aggregate)
    if HAS_FAST_PATH:
        assert A.engine()._round is not None and A.engine()._round.native is not None


def test_weighted_with_the_global_among_repeated_clients():
    """aggregate_weighted over [c1, g, c1]: fp32 keys the ordered sum of
    fp32(x * w) in torch's CPU order, int64 keys the reference mean."""
    from feddct_amd import aggregate as A
    mods = _modules(MAN, DEV)
    g, clients = mods["g"], [mods[x] for x in LISTS["1g1"]]
    sizes = [300, 50, 7]
    w = A.client_weights(sizes)
    with _Spy() as spy:
        for step in range(3):
            _perturb(mods, step)
            snap = [[(k, v.detach().cpu().numpy().copy()) for k, v in c.state_dict().items()]
                    for c in clients]
            spy.calls.clear()
            A.aggregate_weighted(g, clients, sizes=sizes)
            torch.cuda.synchronize()
            if HAS_FAST_PATH:
                assert spy.calls and spy.calls[0] == (step > 0), (step, spy.calls)
            for j, (k, v0) in enumerate(snap[0]):
                x = np.stack([s[j][1] for s in snap])
                want = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)
                for m in [g] + clients:
                    assert bits_equal(m.state_dict()[k].cpu().numpy(), want), (step, k)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_native_16_bit_round_with_the_global_among_the_clients(dtype):
    from feddct_amd import aggregate as A
    from feddct_amd.fedavg import server_aggregate
    mods = _modules(MAN, DEV, dtype=dtype, mode=synth.MODE_REALISTIC)
    assert A.engine().round_layout(mods["g"], [mods["g"], mods[1]]).native16
    _three_rounds(mods, LISTS["g12"], server_aggregate)


@pytest.mark.parametrize("which", ["g12", "121"])
def test_host_resident_lists(which):
    """CPU modules (pipeline.HostPipeline): each downloaded chunk fans out into
    the clients' host buckets while later chunks still upload from them."""
    from feddct_amd.fedavg import server_aggregate
    mods = _modules(MAN, CPU)
    _three_rounds(mods, LISTS[which], server_aggregate, expect_bound=False)
    for m in mods.values():
        assert all(v.device.type == "cpu" for v in m.state_dict().values())


def test_feddct_split_with_both_globals_among_their_clients():
    from feddct_amd.feddct import server_aggregate
    a, b = _modules(MAN, DEV), _modules(MAN_B, DEV, first=10)
    ga, gb = a["g"], b["g"]
    la, lb = [ga, a[1]], [gb, b[1]]
    with _Spy("_run_bound") as spy:
        for step in range(2):
            _perturb(a, step)
            _perturb(b, step)
            ra, rb, rla, rlb = copy.deepcopy((ga, gb, la, lb))
            for m in (ra, rb, *rla, *rlb):
                m.cpu()
            reference_loop(ra, rla)
            reference_loop(rb, rlb)
            spy.calls.clear()
            server_aggregate(ga, gb, la, lb)
            torch.cuda.synchronize()
            _assert_round_equals(ga, la, ra, rla, ("main", step))
            _assert_round_equals(gb, lb, rb, rlb, ("proxy", step))
            if HAS_FAST_PATH and step:   # the repeat call: the joint round, bound
                assert spy.calls == [True], spy.calls


def test_torch_gpu_order_with_the_global_among_the_clients():
    """set_summation_order("torch_gpu"): the reference's loop on GPU copies."""
    import feddct_amd
    from feddct_amd.fedavg import server_aggregate
    mods = _modules(MAN, DEV)
    feddct_amd.set_summation_order("torch_gpu")
    try:
        _three_rounds(mods, LISTS["g12"], server_aggregate, on_cpu=False)
    finally:
        feddct_amd.set_summation_order("torch_cpu")
