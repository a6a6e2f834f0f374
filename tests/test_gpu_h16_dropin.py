"""server_aggregate on model.half() / model.bfloat16() modules: the native
16-bit round against the reference loop on CPU copies, the rounds that must
fall back to fp32 staging, and the fixture written by the reference's own
server_aggregate (tests/golden/make_h16_golden.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import feddct_amd
from conftest import ROOT
from feddct_amd import aggregate, checkpoint
from feddct_amd.aggregate import engine
from helpers import StateModule
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
SHAPES = [[], [7], [3, 3], [33], [100], [2049], [16, 3, 3, 3], [4097]]


def manifest(dtype, shapes=SHAPES, pre="t"):
    keys = [{"key": f"{pre}{j}.w", "shape": s, "dtype": dtype} for j, s in enumerate(shapes)]
    keys.append({"key": f"{pre}.nbt", "shape": [], "dtype": "int64"})
    return {"name": "h16", "keys": keys}


def fill(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        base = torch.Generator().manual_seed(12345)
        for v in m.state_dict().values():
            if v.dtype == torch.int64:
                v.copy_(torch.randint(0, 500, v.shape, generator=g))
            else:
                b = torch.randn(v.shape, generator=base) * 0.05
                v.copy_(b * (1 + 0.01 * torch.randn(v.shape, generator=g)))
    return m


def make_round(man, n, seed=0):
    """(CPU global, CPU clients, their CUDA twins)."""
    cg = fill(StateModule(man), 999 + seed)
    cc = [fill(StateModule(man), seed * 100 + i) for i in range(n)]
    return cg, cc, copy.deepcopy(cg).cuda(), [copy.deepcopy(c).cuda() for c in cc]


def nudge(cpu_models, gpu_models, seed):
    """The same in-place update on both sides (a local training step)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for c, d in zip(cpu_models, gpu_models):
            for (k, v), w in zip(c.state_dict().items(), d.state_dict().values()):
                if v.dtype == torch.int64:
                    v.add_(3)
                    w.add_(3)
                else:
                    step = (torch.randn(v.shape, generator=g) * 0.01).to(v.dtype)
                    v.add_(step)
                    w.add_(step.cuda())


def assert_same_state(cpu_m, gpu_m, what):
    a, b = cpu_m.state_dict(), gpu_m.state_dict()
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k].cpu()
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        if x.dtype == torch.int64:
            assert torch.equal(x, y), (what, k)
        else:
            nx, ny = torch.isnan(x), torch.isnan(y)
            assert torch.equal(nx, ny), (what, k)
            bits = {2: torch.int16, 4: torch.int32}[x.element_size()]
            assert torch.equal(x.view(bits)[~nx], y.view(bits)[~ny]), (what, k)


def assert_native(models, tdt):
    for m in models:
        a = m._fa_arena
        assert a.layout.native16 and a.f32.dtype == tdt and a._packed == [] and a.valid()


def assert_staged(models):
    for m in models:
        a = m._fa_arena
        assert not a.layout.native16 and a.f32.dtype == torch.float32


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    aggregate._ENGINE = None


@pytest.mark.parametrize("n", [3, 9, 20])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_server_aggregate_native_rounds(dtype, n):
    tdt = DTYPES[dtype]
    cg, cc, g, cl = make_round(manifest(dtype), n)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, tdt)
    e = engine()
    assert e._round is not None and e._round.native is not None
    assert e._round.plan.elem == _elem(tdt)
    assert_same_state(cg, g, "round 1 global")
    for i in range(n):
        assert_same_state(cc[i], cl[i], f"round 1 client {i}")
    nudge(cc, cl, 7)
    reference_loop(cg, cc)
    rb, calls = e._round, []
    orig = e._run_bound
    e._run_bound = lambda r, w=None: calls.append(r) or orig(r, w)
    try:
        feddct_amd.server_aggregate(g, cl)
    finally:
        del e._run_bound
    assert calls == [rb] and e._round is rb, "the second call takes the bound round"
    assert_native([g] + cl, tdt)
    assert_same_state(cg, g, "round 2 global")
    for i in range(n):
        assert_same_state(cc[i], cl[i], f"round 2 client {i}")
    # the checkpoint copy of a 16-bit arena
    ck = checkpoint.bucket_state_dict(g)
    for k, v in g.state_dict().items():
        assert ck[k].dtype == v.dtype and torch.equal(ck[k], v.cpu()), k


def _elem(tdt):
    from feddct_amd import _lib
    return _lib.ELEM_OF_DTYPE[tdt]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_aggregate_weighted_native(dtype):
    tdt = DTYPES[dtype]
    n = 9
    cg, cc, g, cl = make_round(manifest(dtype), n, seed=2)
    w = T.weights_from_sizes(np.arange(10, 10 + n))
    aggregate.aggregate_weighted(g, cl, weights=w)
    assert_native([g] + cl, tdt)
    sd = g.state_dict()
    for k, v in cg.state_dict().items():
        x = np.stack([c.state_dict()[k].float().numpy() for c in cc])
        if v.dtype == torch.int64:
            want = torch.as_tensor(np.asarray(T.mean_i64_trunc(np.stack(
                [c.state_dict()[k].numpy() for c in cc]))))
            assert torch.equal(sd[k].cpu(), want.reshape(v.shape)), k
        else:
            want = torch.as_tensor(np.asarray(T.weighted_sum0(x, w))).to(tdt).reshape(v.shape)
            assert torch.equal(sd[k].cpu().view(torch.int16), want.view(torch.int16)), k
    for c in cl:
        for k, v in c.state_dict().items():
            assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_model_call_native(dtype):
    tdt = DTYPES[dtype]
    n = 5
    mm, pm = manifest(dtype, SHAPES[:5], "m"), manifest(dtype, SHAPES[4:], "p")
    cgm, ccm, gm, clm = make_round(mm, n, seed=3)
    cgp, ccp, gp, clp = make_round(pm, n, seed=4)
    for rnd in range(2):
        reference_loop(cgm, ccm)
        reference_loop(cgp, ccp)
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        rb = engine()._round
        assert rb is not None and rb.native is not None and rb.split_ids is not None
        assert rb.plan.elem == _elem(tdt)
        for a in rb.arenas:
            assert a().layout.native16 and a()._packed == [] and a().f32.dtype == tdt
        assert_same_state(cgm, gm, f"main global {rnd}")
        assert_same_state(cgp, gp, f"proxy global {rnd}")
        for i in range(n):
            assert_same_state(ccm[i], clm[i], f"main {i} {rnd}")
            assert_same_state(ccp[i], clp[i], f"proxy {i} {rnd}")
        nudge(ccm + ccp, clm + clp, 20 + rnd)


def test_fallback_one_fp32_keyed_client():
    n = 4
    man = manifest("bfloat16")
    cg, cc, g, cl = make_round(man, n, seed=5)
    odd = copy.deepcopy(man)
    odd["keys"][3]["dtype"] = "float32"
    cc[2] = fill(StateModule(odd), 77)
    cl[2] = copy.deepcopy(cc[2]).cuda()
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert_same_state(cg, g, "global")
    for i in range(n):
        assert_same_state(cc[i], cl[i], f"client {i}")


def test_fallback_torch_gpu_order_keeps_the_staged_path():
    """With the torch-GPU order set the round is today's: fp32 staging, and
    the bits of the reference loop run on the GPU modules themselves (that
    order's reference, as tests/test_gpu_torch_order.py takes it)."""
    n = 4
    _, _, g, cl = make_round(manifest("bfloat16"), n, seed=6)
    rg, rc = copy.deepcopy(g), [copy.deepcopy(c) for c in cl]
    reference_loop(rg, rc)
    feddct_amd.set_summation_order("torch_gpu")
    try:
        feddct_amd.server_aggregate(g, cl)
        torch.cuda.synchronize()
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert_staged([g] + cl)
    assert_same_state(rg.cpu(), g, "global")
    for i in range(n):
        assert_same_state(rc[i].cpu(), cl[i], f"client {i}")


def test_fallback_global_on_the_cpu():
    n = 3
    cg, cc, g, cl = make_round(manifest("float16"), n, seed=8)
    g = g.cpu()
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert_same_state(cg, g, "global")
    for i in range(n):
        assert_same_state(cc[i], cl[i], f"client {i}")


def test_a_round_that_stops_qualifying_rebinds_to_the_staged_layout():
    n = 3
    man = manifest("bfloat16")
    cg, cc, g, cl = make_round(man, n, seed=9)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, torch.bfloat16)
    with torch.no_grad():   # one client's key goes fp32
        for c, d in ((cc[1], cl[1]),):
            p = c._modules["t4"]._parameters["w"]
            p.data = p.data.float() + 0.001
            q = d._modules["t4"]._parameters["w"]
            q.data = p.data.cuda()
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert_same_state(cg, g, "global")
    for i in range(n):
        assert_same_state(cc[i], cl[i], f"client {i}")


GOLD = os.path.join(ROOT, "tests", "golden", "h16_goldens.npz")


def gold_cases():
    with open(os.path.join(ROOT, "tests", "golden", "h16_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n", [3, 17, 33])
def test_round_matches_the_reference_fixture(dtype, n):
    """tests/golden/h16_goldens.npz: the reference's own server_aggregate on
    fp16 / bf16 modules (inputs and outputs as 16-bit integers)."""
    meta = gold_cases()
    gold = np.load(GOLD)
    tdt = DTYPES[dtype]
    man = {"name": "g", "keys": [dict(e, dtype=dtype if e["dtype"] == "h16" else e["dtype"])
                                 for e in meta["keys"]]}

    def load(m, tag):
        with torch.no_grad():
            for k, v in m.state_dict().items():
                a = gold[f"{dtype}/n{n}/{tag}/{k}"]
                t = torch.from_numpy(a.copy())
                v.copy_(t if v.dtype == torch.int64 else t.view(tdt))
        return m
    cl = [load(StateModule(man), f"in{i}").cuda() for i in range(n)]
    g = StateModule(man).cuda()
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, tdt)
    for m in [g] + cl:
        for k, v in m.state_dict().items():
            want = gold[f"{dtype}/n{n}/out/{k}"]
            got = v.cpu() if v.dtype == torch.int64 else v.cpu().view(torch.int16)
            assert np.array_equal(got.numpy(), want), k
