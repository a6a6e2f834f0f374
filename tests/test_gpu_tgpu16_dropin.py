"""server_aggregate on model.half() / model.bfloat16() GPU modules under
set_summation_order("torch_gpu", native16=True): the native 16-bit round in
torch-ROCm's GPU order against the reference loop run on GPU copies of the
same modules (that order's reference, as tests/test_gpu_torch_order.py takes
it), the rounds that take the CPU order on the same 16-bit buckets, the rounds
that stay staged, and switching between them on repeat calls."""
import copy
import warnings

import numpy as np
import pytest
import torch

import feddct_amd
from feddct_amd import _lib, aggregate
from feddct_amd.aggregate import engine
from helpers import StateModule
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop
from test_gpu_h16_dropin import DTYPES, SHAPES, assert_native, assert_staged, fill, manifest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    aggregate._ENGINE = None


@pytest.fixture
def native_gpu_order():
    feddct_amd.set_summation_order("torch_gpu", native16=True)
    yield
    feddct_amd.set_summation_order("torch_cpu")


def gpu_round(gman, cman, n, seed=0):
    """(global, clients) on the GPU."""
    g = fill(StateModule(gman), 999 + seed).cuda()
    return g, [fill(StateModule(cman), seed * 100 + i).cuda() for i in range(n)]


def twins(g, cl):
    return copy.deepcopy(g), [copy.deepcopy(c) for c in cl]


def nudge(a_models, b_models, seed):
    """The same in-place update on both sets of GPU modules."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for c, d in zip(a_models, b_models):
            for v, w in zip(c.state_dict().values(), d.state_dict().values()):
                if v.dtype == torch.int64:
                    v.add_(3)
                    w.add_(3)
                else:
                    step = (torch.randn(v.shape, generator=gen) * 0.01).to(v.dtype).cuda()
                    v.add_(step)
                    w.add_(step)


def nudge_one(models, seed):
    """An in-place update of GPU modules (a local training step)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for c in models:
            for v in c.state_dict().values():
                if v.dtype == torch.int64:
                    v.add_(3)
                else:
                    v.add_((torch.randn(v.shape, generator=gen) * 0.01).to(v.dtype).cuda())


def assert_same_state(ref_m, m, what):
    """Two modules (on any device) hold the same keys, dtypes and bits."""
    a, b = ref_m.state_dict(), m.state_dict()
    assert list(a) == list(b)
    for k in a:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        if x.dtype == torch.int64:
            assert torch.equal(x, y), (what, k)
        else:
            nx, ny = torch.isnan(x), torch.isnan(y)
            assert torch.equal(nx, ny), (what, k)
            bits = {2: torch.int16, 4: torch.int32}[x.element_size()]
            assert torch.equal(x.view(bits)[~nx], y.view(bits)[~ny]), (what, k)


def assert_round(rg, rc, g, cl, what):
    torch.cuda.synchronize()
    assert_same_state(rg, g, f"{what} global")
    for i, (r, c) in enumerate(zip(rc, cl)):
        assert_same_state(r, c, f"{what} client {i}")


def assert_tgpu16_bound(tdt, n):
    rb = engine()._round
    assert rb is not None and rb.native is not None and rb.order == "torch_gpu+native16"
    assert rb.plan.elem == rb.plan.out_elem == _lib.ELEM_OF_DTYPE[tdt] and rb.n == n
    # a torch-GPU-order plan: cut for this N (any other is refused), zeros as its launch form
    assert rb.plan.launch_form(n) == (0, 0, 0)
    return rb


@pytest.mark.parametrize("n", [2, 5, 20, 48])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_server_aggregate_native_rounds(native_gpu_order, dtype, n):
    tdt = DTYPES[dtype]
    g, cl = gpu_round(manifest(dtype), manifest(dtype), n)
    before = {k: v.dtype for k, v in g.state_dict().items()}
    rg, rc = twins(g, cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, tdt)
    assert {k: v.dtype for k, v in g.state_dict().items()} == before
    rb = assert_tgpu16_bound(tdt, n)
    assert_round(rg, rc, g, cl, "round 1")
    nudge(rc, cl, 7)
    reference_loop(rg, rc)
    e, calls = engine(), []
    orig = e._run_bound
    e._run_bound = lambda r, w=None: calls.append(r) or orig(r, w)
    try:
        feddct_amd.server_aggregate(g, cl)
    finally:
        del e._run_bound
    assert calls == [rb] and e._round is rb, "the second call takes the bound round"
    assert_native([g] + cl, tdt)
    assert_round(rg, rc, g, cl, "round 2")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_model_call_native(native_gpu_order, dtype):
    tdt = DTYPES[dtype]
    n = 5
    mm, pm = manifest(dtype, SHAPES[:5], "m"), manifest(dtype, SHAPES[4:], "p")
    gm, clm = gpu_round(mm, mm, n, seed=3)
    gp, clp = gpu_round(pm, pm, n, seed=4)
    rgm, rcm = twins(gm, clm)
    rgp, rcp = twins(gp, clp)
    for rnd in range(2):
        reference_loop(rgm, rcm)
        reference_loop(rgp, rcp)
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        rb = assert_tgpu16_bound(tdt, n)
        assert rb.split_ids is not None
        for a in rb.arenas:
            assert a().layout.native16 and a()._packed == [] and a().f32.dtype == tdt
        assert_round(rgm, rcm, gm, clm, f"main {rnd}")
        assert_round(rgp, rcp, gp, clp, f"proxy {rnd}")
        nudge(rcm + rcp, clm + clp, 20 + rnd)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_aggregate_weighted_takes_the_cpu_order_on_the_16_bit_arenas(native_gpu_order, dtype):
    tdt = DTYPES[dtype]
    n = 9
    g, cl = gpu_round(manifest(dtype), manifest(dtype), n, seed=2)
    cc = [copy.deepcopy(c).cpu() for c in cl]
    w = T.weights_from_sizes(np.arange(10, 10 + n))
    aggregate.aggregate_weighted(g, cl, weights=w)
    torch.cuda.synchronize()
    assert_native([g] + cl, tdt)
    rb = engine()._round
    assert rb is not None and rb.weighted and rb.plan.launch_form(n, True)[2] == 1   # a CPU-order plan
    sd = g.state_dict()
    for k, v in cc[0].state_dict().items():
        if v.dtype == torch.int64:
            want = torch.as_tensor(np.asarray(T.mean_i64_trunc(np.stack(
                [c.state_dict()[k].numpy() for c in cc]))))
            assert torch.equal(sd[k].cpu(), want.reshape(v.shape)), k
        else:
            x = np.stack([c.state_dict()[k].float().numpy() for c in cc])
            want = torch.as_tensor(np.asarray(T.weighted_sum0(x, w))).to(tdt).reshape(v.shape)
            assert torch.equal(sd[k].cpu().view(torch.int16), want.view(torch.int16)), k
    for c in cl:
        for k, v in c.state_dict().items():
            assert torch.equal(v, sd[k]), k
    # one client: N < 2 takes the CPU order too (the reference loop on host copies)
    g1, c1 = gpu_round(manifest(dtype), manifest(dtype), 1, seed=5)
    cg1, cc1 = copy.deepcopy(g1).cpu(), [copy.deepcopy(c1[0]).cpu()]
    reference_loop(cg1, cc1)
    feddct_amd.server_aggregate(g1, c1)
    torch.cuda.synchronize()
    assert_native([g1] + c1, tdt)
    assert_same_state(cg1, g1, "N = 1")


def test_outside_the_restatement_warns_counts_and_strict_raises():
    """N = 512 clients of one 1,024-element key: torch splits it across
    blocks, so the round takes the CPU order on the same 16-bit buckets, warns
    once per (layout, N), is counted in gpu_order_fallbacks, is never bound,
    and raises under strict=True."""
    n = 512
    man = {"name": "x", "keys": [{"key": "w", "shape": [1024], "dtype": "bfloat16"}]}
    assert not _lib.lib.fa_torch_gpu_config(n, 1024, None)
    g, cl = gpu_round(man, man, n, seed=6)
    cg, cc = copy.deepcopy(g).cpu(), [copy.deepcopy(c).cpu() for c in cl]
    reference_loop(cg, cc)
    e = engine()
    try:
        feddct_amd.set_summation_order("torch_gpu", native16=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            feddct_amd.server_aggregate(g, cl)
            torch.cuda.synchronize()
            assert_native([g] + cl, torch.bfloat16)
            assert_same_state(cg, g, "fallback global")
            assert_same_state(cc[-1], cl[-1], "fallback client")
            feddct_amd.server_aggregate(g, cl)
        assert sum("not restated" in str(x.message) for x in w) == 1
        assert all(issubclass(x.category, RuntimeWarning) for x in w
                   if "not restated" in str(x.message))
        sig = g._fa_arena.layout.signature
        assert e.gpu_order_fallbacks == {(sig, n): 2} and e._round is None
        feddct_amd.set_summation_order("torch_gpu", strict=True, native16=True)
        with pytest.raises(RuntimeError, match="strict"):
            feddct_amd.server_aggregate(g, cl)
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert e.strict_gpu_order is False and e.native16_gpu_order is False


def test_switching_option_and_order_between_repeat_calls():
    """Each call has its own order's bits and its own binding: the CPU order
    (native buckets), the GPU order natively, the GPU order staged (option
    off), natively again, the CPU order again."""
    tdt = torch.bfloat16
    n = 6
    g, cl = gpu_round(manifest("bfloat16"), manifest("bfloat16"), n, seed=12)
    steps = [("torch_cpu", False), ("torch_gpu", True), ("torch_gpu", True), ("torch_gpu", False),
             ("torch_gpu", True), ("torch_cpu", True), ("torch_cpu", False)]
    try:
        for step, (order, opt) in enumerate(steps):
            feddct_amd.set_summation_order(order, native16=opt)
            nudge_one(cl, 40 + step)
            rg, rc = twins(g, cl)        # the GPU order's reference: the loop on GPU copies
            if order != "torch_gpu":     # the CPU order's: on host copies
                rg, rc = rg.cpu(), [m.cpu() for m in rc]
            reference_loop(rg, rc)
            prev = engine()._round
            feddct_amd.server_aggregate(g, cl)
            torch.cuda.synchronize()
            rb = engine()._round
            if order == "torch_gpu" and not opt:
                assert_staged([g] + cl)
            else:
                assert_native([g] + cl, tdt)
            assert rb is not None and rb.order == engine().order_key
            same = step > 0 and steps[step - 1][0] == order and \
                (order == "torch_cpu" or steps[step - 1][1] == opt)
            assert (rb is prev) == same, (step, order, opt)
            assert_round(rg, rc, g, cl, f"step {step} {order} {opt}")
    finally:
        feddct_amd.set_summation_order("torch_cpu")


def test_fp32_master_over_16_bit_clients_stays_staged(native_gpu_order):
    g, cl = gpu_round(manifest("float32"), manifest("bfloat16"), 4, seed=10)
    rg, rc = twins(g, cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert not g._fa_arena.layout.master16
    assert_round(rg, rc, g, cl, "mixed")


def test_proximal_term_still_refuses(native_gpu_order):
    from feddct_amd.prox import ProximalTerm
    a, b = torch.nn.Linear(16, 8).half().cuda(), torch.nn.Linear(16, 8).half().cuda()
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(a, b)
    assert engine()._round_dtypes(a, [b]) == (None, None)
    assert engine()._device_round_dtypes(a, [b]) == ("native", torch.float16)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_option_off_is_the_staged_round(dtype):
    n = 4
    g, cl = gpu_round(manifest(dtype), manifest(dtype), n, seed=6)
    rg, rc = twins(g, cl)
    reference_loop(rg, rc)
    feddct_amd.set_summation_order("torch_gpu")
    try:
        feddct_amd.server_aggregate(g, cl)
        torch.cuda.synchronize()
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert_staged([g] + cl)
    assert engine()._round.plan.elem == _lib.FA_ELEM_F32
    assert_round(rg, rc, g, cl, "staged")
