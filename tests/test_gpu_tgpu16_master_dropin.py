"""server_aggregate with an fp32 master global over model.half() /
model.bfloat16() GPU clients under set_summation_order("torch_gpu",
native16=True, native16_master=True): the mixed native round in torch-ROCm's
GPU order against the reference loop run on GPU copies of the same modules
(the global's unrounded fp32 mean, the clients' rounded 16-bit bits), the
rounds that take the CPU order's mixed plan on the same buckets, and switching
among the orders and options on repeat calls."""
import copy
import warnings

import numpy as np
import pytest
import torch

import feddct_amd
from feddct_amd import _lib, aggregate
from feddct_amd.aggregate import engine
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop
from test_gpu_h16_dropin import DTYPES, SHAPES, assert_native, assert_staged, manifest
from test_gpu_mixed16_dropin import assert_mixed
from test_gpu_tgpu16_dropin import (assert_round, assert_same_state, gpu_round, nudge, nudge_one,
                                    twins)

pytestmark = pytest.mark.gpu

KEY = "torch_gpu+native16+master"


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    aggregate._ENGINE = None


@pytest.fixture
def master_gpu_order():
    feddct_amd.set_summation_order("torch_gpu", native16=True, native16_master=True)
    yield
    feddct_amd.set_summation_order("torch_cpu")


def assert_master_bound(g, cl, tdt, n):
    """assert_mixed's layouts, bound under the new key to a torch-GPU-order
    plan with an fp32 result (zeros as its launch form, cut for this N)."""
    assert_mixed(g, cl, tdt)
    rb = engine()._round
    assert rb.order == KEY and rb.n == n and not rb.weighted
    assert rb.plan.out_elem == _lib.FA_ELEM_F32 and rb.plan.launch_form(n) == (0, 0, 0)
    return rb


@pytest.mark.parametrize("n", [2, 5, 20, 48])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_server_aggregate_master_rounds(master_gpu_order, dtype, n):
    tdt = DTYPES[dtype]
    g, cl = gpu_round(manifest("float32"), manifest(dtype), n)
    before = {k: v.dtype for m in [g] + cl for k, v in m.state_dict().items()}
    rg, rc = twins(g, cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    rb = assert_master_bound(g, cl, tdt, n)
    assert {k: v.dtype for m in [g] + cl for k, v in m.state_dict().items()} == before
    assert_round(rg, rc, g, cl, "round 1")
    # the global holds bits no 16-bit value has: the unrounded mean
    w = g.state_dict()["t5.w"]
    assert w.dtype == torch.float32 and not torch.equal(w, w.to(tdt).float())
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
    assert_master_bound(g, cl, tdt, n)
    assert_round(rg, rc, g, cl, "round 2")
    assert e.gpu_order_fallbacks == {}


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_model_call_master(master_gpu_order, dtype):
    tdt = DTYPES[dtype]
    n = 5
    gm, clm = gpu_round(manifest("float32", SHAPES[:5], "m"), manifest(dtype, SHAPES[:5], "m"),
                        n, seed=3)
    gp, clp = gpu_round(manifest("float32", SHAPES[4:], "p"), manifest(dtype, SHAPES[4:], "p"),
                        n, seed=4)
    rgm, rcm = twins(gm, clm)
    rgp, rcp = twins(gp, clp)
    for rnd in range(2):
        reference_loop(rgm, rcm)
        reference_loop(rgp, rcp)
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        rb = engine()._round
        assert rb is not None and rb.native is not None and rb.order == KEY
        assert rb.split_ids is not None and rb.n == n
        assert rb.plan.elem == _lib.ELEM_OF_DTYPE[tdt] and rb.plan.out_elem == _lib.FA_ELEM_F32
        assert rb.plan.launch_form(n) == (0, 0, 0)
        ga, *cas = [a() for a in rb.arenas]
        assert ga.layout.master16 and ga.f32.dtype == torch.float32 and ga._packed == []
        for a in cas:
            assert a.layout.native16 and a._packed == [] and a.f32.dtype == tdt
        assert_round(rgm, rcm, gm, clm, f"main {rnd}")
        assert_round(rgp, rcp, gp, clp, f"proxy {rnd}")
        nudge(rcm + rcp, clm + clp, 20 + rnd)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_weighted_round_is_the_cpu_orders(dtype):
    """A weighted round under both options is the call made under
    "torch_cpu" on twins: §4.9's mixed plan on the same buckets."""
    tdt = DTYPES[dtype]
    n = 9
    g, cl = gpu_round(manifest("float32"), manifest(dtype), n, seed=2)
    tg, tc = twins(g, cl)
    w = T.weights_from_sizes(np.arange(10, 10 + n))
    aggregate.aggregate_weighted(tg, tc, weights=w)
    torch.cuda.synchronize()
    assert engine()._round.order == "torch_cpu"
    try:
        feddct_amd.set_summation_order("torch_gpu", native16=True, native16_master=True)
        aggregate.aggregate_weighted(g, cl, weights=w)
        torch.cuda.synchronize()
        assert_mixed(g, cl, tdt)
        rb = engine()._round
        assert rb.order == KEY and rb.weighted
        assert rb.plan.launch_form(n, True)[2] == 1     # a CPU-order plan
        assert_round(tg, tc, g, cl, "weighted")
        assert engine().gpu_order_fallbacks == {}
    finally:
        feddct_amd.set_summation_order("torch_cpu")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_one_client(master_gpu_order, dtype):
    g, cl = gpu_round(manifest("float32"), manifest(dtype), 1, seed=5)
    rg, rc = twins(g, cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, DTYPES[dtype])
    assert engine()._round.plan.launch_form(1)[2] == 1     # N < 2: a CPU-order plan
    assert_round(rg, rc, g, cl, "N = 1")


def test_outside_the_restatement_warns_counts_and_strict_raises():
    """N = 256 with keys below 32 elements: torch's block is higher than 16
    rows there, so the round takes the CPU order's mixed plan on the same
    buckets, warns once per (layout, N), is counted in gpu_order_fallbacks, is
    never bound, and raises under strict=True."""
    n = 256
    assert not _lib.lib.fa_torch_gpu_config(n, 7, None)
    g, cl = gpu_round(manifest("float32"), manifest("bfloat16"), n, seed=6)
    cg, cc = copy.deepcopy(g).cpu(), [copy.deepcopy(c).cpu() for c in cl]
    reference_loop(cg, cc)
    e = engine()
    try:
        feddct_amd.set_summation_order("torch_gpu", native16=True, native16_master=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            feddct_amd.server_aggregate(g, cl)
            torch.cuda.synchronize()
            a = g._fa_arena
            assert a.layout.master16 and a.f32.dtype == torch.float32 and a._packed == []
            assert_native(cl, torch.bfloat16)
            assert_same_state(cg, g, "fallback global")
            assert_same_state(cc[0], cl[0], "fallback client 0")
            assert_same_state(cc[-1], cl[-1], "fallback last client")
            feddct_amd.server_aggregate(g, cl)
        assert sum("not restated" in str(x.message) for x in w) == 1
        assert all(issubclass(x.category, RuntimeWarning) for x in w
                   if "not restated" in str(x.message))
        sig = cl[0]._fa_arena.layout.signature
        assert e.gpu_order_fallbacks == {(sig, n): 2} and e._round is None
        feddct_amd.set_summation_order("torch_gpu", strict=True, native16=True,
                                       native16_master=True)
        with pytest.raises(RuntimeError, match="strict"):
            feddct_amd.server_aggregate(g, cl)
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert e.strict_gpu_order is False and e.native16_master_gpu_order is False


def _key(order, opt, master):
    if order == "torch_cpu" or not opt:
        return order
    return order + "+native16" + ("+master" if master else "")


def test_switching_options_and_order_between_repeat_calls():
    """Each call has its own order's bits and its own binding: the CPU order
    (mixed buckets), native16 alone (staged, as pinned), both options
    (natively), and back.  A binding is kept exactly when the key is."""
    tdt = torch.bfloat16
    n = 6
    g, cl = gpu_round(manifest("float32"), manifest("bfloat16"), n, seed=12)
    steps = [("torch_cpu", False, False), ("torch_gpu", True, False), ("torch_gpu", True, True),
             ("torch_gpu", True, True), ("torch_gpu", True, False), ("torch_gpu", True, True),
             ("torch_cpu", True, True), ("torch_cpu", False, False), ("torch_gpu", False, False),
             ("torch_gpu", True, True)]
    try:
        for step, (order, opt, master) in enumerate(steps):
            feddct_amd.set_summation_order(order, native16=opt, native16_master=master)
            assert engine().order_key == _key(order, opt, master)
            nudge_one(cl, 40 + step)
            rg, rc = twins(g, cl)        # the GPU order's reference: the loop on GPU copies
            if order != "torch_gpu":     # the CPU order's: on host copies
                rg, rc = rg.cpu(), [m.cpu() for m in rc]
            reference_loop(rg, rc)
            prev = engine()._round
            feddct_amd.server_aggregate(g, cl)
            torch.cuda.synchronize()
            rb = engine()._round
            if order == "torch_gpu" and not master:
                assert_staged([g] + cl)
                assert not g._fa_arena.layout.master16
            else:
                assert_mixed(g, cl, tdt)
                gpu_plan = rb.plan.launch_form(n) == (0, 0, 0)
                assert gpu_plan == (order == "torch_gpu")
            assert rb is not None and rb.order == _key(order, opt, master)
            same = step > 0 and _key(*steps[step - 1]) == _key(order, opt, master)
            assert (rb is prev) == same, (step, order, opt, master)
            assert_round(rg, rc, g, cl, f"step {step} {order} {opt} {master}")
    finally:
        feddct_amd.set_summation_order("torch_cpu")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_all_16_bit_round_is_still_the_native_one(master_gpu_order, dtype):
    tdt = DTYPES[dtype]
    n = 5
    g, cl = gpu_round(manifest(dtype), manifest(dtype), n, seed=8)
    rg, rc = twins(g, cl)
    for rnd in range(2):
        reference_loop(rg, rc)
        feddct_amd.server_aggregate(g, cl)
        assert_native([g] + cl, tdt)
        rb = engine()._round
        assert rb is not None and rb.native is not None and rb.order == KEY
        assert rb.plan.elem == rb.plan.out_elem == _lib.ELEM_OF_DTYPE[tdt]
        assert rb.plan.launch_form(n) == (0, 0, 0)
        assert_round(rg, rc, g, cl, f"round {rnd}")
        nudge(rc, cl, 30 + rnd)


def test_proximal_term_still_refuses(master_gpu_order):
    from feddct_amd.prox import ProximalTerm
    a, b = torch.nn.Linear(16, 8).half().cuda(), torch.nn.Linear(16, 8).half().cuda()
    m = torch.nn.Linear(16, 8).cuda()
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(a, b)
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(a, m)
    assert engine()._round_dtypes(m, [a]) == (None, None)
    assert engine()._device_round_dtypes(m, [a]) == ("mixed", torch.float16)
