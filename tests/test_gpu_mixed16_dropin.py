"""server_aggregate with an fp32 master global over model.half() /
model.bfloat16() clients: the mixed native round against the reference loop on
CPU twins (the global's unrounded fp32 mean, the clients' rounded 16-bit
bits), the rounds that must stay staged, re-binding in both directions, and
the fixture written by the reference's own server_aggregate
(tests/golden/make_mixed16_golden.py)."""
import copy
import os

import numpy as np
import pytest
import torch

import feddct_amd
from conftest import ROOT
from feddct_amd import _lib, aggregate, checkpoint
from feddct_amd.aggregate import engine
from helpers import StateModule
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop
from test_gpu_h16_dropin import (DTYPES, SHAPES, assert_native, assert_same_state, assert_staged,
                                 fill, gold_cases, manifest, nudge)

pytestmark = pytest.mark.gpu

GOLD16 = os.path.join(ROOT, "tests", "golden", "h16_goldens.npz")
GOLD = os.path.join(ROOT, "tests", "golden", "mixed16_goldens.npz")


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    aggregate._ENGINE = None


def make_round(gman, cman, n, seed=0):
    """(CPU global, CPU clients, their CUDA twins); the global of ``gman``."""
    cg = fill(StateModule(gman), 999 + seed)
    cc = [fill(StateModule(cman), seed * 100 + i) for i in range(n)]
    return cg, cc, copy.deepcopy(cg).cuda(), [copy.deepcopy(c).cuda() for c in cc]


def assert_mixed(g, clients, tdt):
    a = g._fa_arena
    assert a.layout.master16 and not a.layout.native16 and a.f32.dtype == torch.float32
    assert a._packed == [] and a.valid()
    assert_native(clients, tdt)
    for c in clients:
        assert c._fa_arena.layout.f32_numel == a.layout.f32_numel
        assert np.array_equal(c._fa_arena.layout.segs32, a.layout.segs32)
    rb = engine()._round
    assert rb is not None and rb.native is not None
    assert rb.plan.elem == _lib.ELEM_OF_DTYPE[tdt] and rb.plan.out_elem == _lib.FA_ELEM_F32
    assert _lib.lib.fa_plan_out_elem(rb.plan.handle) == _lib.FA_ELEM_F32


def assert_round(cg, cc, g, cl, what):
    assert_same_state(cg, g, f"{what} global")
    for i in range(len(cc)):
        assert_same_state(cc[i], cl[i], f"{what} client {i}")


@pytest.mark.parametrize("n", [3, 9, 20])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_server_aggregate_mixed_rounds(dtype, n):
    tdt = DTYPES[dtype]
    cg, cc, g, cl = make_round(manifest("float32"), manifest(dtype), n)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, tdt)
    assert_round(cg, cc, g, cl, "round 1")
    # the global holds bits no 16-bit value has: the unrounded mean
    w = g.state_dict()["t5.w"]
    assert w.dtype == torch.float32 and not torch.equal(w, w.to(tdt).float())
    nudge(cc, cl, 7)
    reference_loop(cg, cc)
    e = engine()
    rb, calls = e._round, []
    orig = e._run_bound
    e._run_bound = lambda r, w=None: calls.append(r) or orig(r, w)
    try:
        feddct_amd.server_aggregate(g, cl)
    finally:
        del e._run_bound
    assert calls == [rb] and e._round is rb, "the second call takes the bound round"
    assert_mixed(g, cl, tdt)
    assert_round(cg, cc, g, cl, "round 2")
    ck = checkpoint.bucket_state_dict(g)
    sd = g.state_dict()
    assert list(ck) == list(sd)
    for k, v in sd.items():
        assert ck[k].dtype == v.dtype and torch.equal(ck[k], v.cpu()), k


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_aggregate_weighted_mixed(dtype):
    tdt = DTYPES[dtype]
    n = 9
    cg, cc, g, cl = make_round(manifest("float32"), manifest(dtype), n, seed=2)
    w = T.weights_from_sizes(np.arange(10, 10 + n))
    aggregate.aggregate_weighted(g, cl, weights=w)
    assert_mixed(g, cl, tdt)
    sd = g.state_dict()
    for k, v in cg.state_dict().items():
        if v.dtype == torch.int64:
            want = torch.as_tensor(np.asarray(T.mean_i64_trunc(np.stack(
                [c.state_dict()[k].numpy() for c in cc])))).reshape(v.shape)
            assert torch.equal(sd[k].cpu(), want), k
            for c in cl:
                assert torch.equal(c.state_dict()[k].cpu(), want), k
            continue
        x = np.stack([c.state_dict()[k].float().numpy() for c in cc])
        want = torch.as_tensor(np.asarray(T.weighted_sum0(x, w), np.float32)).reshape(v.shape)
        assert sd[k].dtype == torch.float32
        assert torch.equal(sd[k].cpu().view(torch.int32), want.view(torch.int32)), k
        for c in cl:
            assert torch.equal(c.state_dict()[k].cpu().view(torch.int16),
                               want.to(tdt).view(torch.int16)), k


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_model_call_mixed(dtype):
    tdt = DTYPES[dtype]
    n = 5
    cgm, ccm, gm, clm = make_round(manifest("float32", SHAPES[:5], "m"),
                                   manifest(dtype, SHAPES[:5], "m"), n, seed=3)
    cgp, ccp, gp, clp = make_round(manifest("float32", SHAPES[4:], "p"),
                                   manifest(dtype, SHAPES[4:], "p"), n, seed=4)
    for rnd in range(2):
        reference_loop(cgm, ccm)
        reference_loop(cgp, ccp)
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        rb = engine()._round
        assert rb is not None and rb.native is not None and rb.split_ids is not None
        assert rb.plan.elem == _lib.ELEM_OF_DTYPE[tdt] and rb.plan.out_elem == _lib.FA_ELEM_F32
        ga, *cas = [a() for a in rb.arenas]
        assert ga.layout.master16 and ga.f32.dtype == torch.float32 and ga._packed == []
        for a in cas:
            assert a.layout.native16 and a._packed == [] and a.f32.dtype == tdt
        assert_round(cgm, ccm, gm, clm, f"main {rnd}")
        assert_round(cgp, ccp, gp, clp, f"proxy {rnd}")
        nudge(ccm + ccp, clm + clp, 20 + rnd)


# --------------------------------------------------------------- fallbacks ----
def staged_round(cg, cc, g, cl, what):
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert not g._fa_arena.layout.master16
    rb = engine()._round
    assert rb is None or rb.plan.out_elem == rb.plan.elem == _lib.FA_ELEM_F32
    assert_round(cg, cc, g, cl, what)


def test_fallback_clients_of_two_16_bit_dtypes():
    cg, cc, g, cl = make_round(manifest("float32"), manifest("bfloat16"), 4, seed=5)
    cc[2] = fill(StateModule(manifest("float16")), 77)
    cl[2] = copy.deepcopy(cc[2]).cuda()
    staged_round(cg, cc, g, cl, "two dtypes")


def test_fallback_one_client_with_an_fp32_key():
    man = manifest("bfloat16")
    cg, cc, g, cl = make_round(manifest("float32"), man, 4, seed=6)
    odd = copy.deepcopy(man)
    odd["keys"][3]["dtype"] = "float32"
    cc[1] = fill(StateModule(odd), 78)
    cl[1] = copy.deepcopy(cc[1]).cuda()
    staged_round(cg, cc, g, cl, "fp32-keyed client")


def test_fallback_global_with_one_bf16_key():
    gman = manifest("float32")
    gman["keys"][4]["dtype"] = "bfloat16"
    cg, cc, g, cl = make_round(gman, manifest("bfloat16"), 3, seed=7)
    staged_round(cg, cc, g, cl, "bf16-keyed global")


def test_fallback_the_inverse_mix():
    cg, cc, g, cl = make_round(manifest("float16"), manifest("float32"), 3, seed=8)
    staged_round(cg, cc, g, cl, "16-bit global, fp32 clients")


def test_fallback_global_on_the_cpu():
    cg, cc, g, cl = make_round(manifest("float32"), manifest("float16"), 3, seed=9)
    g = g.cpu()
    staged_round(cg, cc, g, cl, "host-resident global")


def test_fallback_torch_gpu_order_keeps_the_staged_path():
    """That order's reference is the loop run on the GPU modules themselves
    (tests/test_gpu_torch_order.py)."""
    _, _, g, cl = make_round(manifest("float32"), manifest("bfloat16"), 4, seed=10)
    rg, rc = copy.deepcopy(g), [copy.deepcopy(c) for c in cl]
    reference_loop(rg, rc)
    feddct_amd.set_summation_order("torch_gpu")
    try:
        feddct_amd.server_aggregate(g, cl)
        torch.cuda.synchronize()
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert_staged([g] + cl)
    assert not g._fa_arena.layout.master16
    assert_round(rg.cpu(), [c.cpu() for c in rc], g, cl, "torch_gpu")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_all_16_bit_rounds_keep_the_pure_plan(dtype):
    tdt = DTYPES[dtype]
    cg, cc, g, cl = make_round(manifest(dtype), manifest(dtype), 3, seed=11)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, tdt)
    assert not g._fa_arena.layout.master16
    rb = engine()._round
    assert rb.plan.elem == rb.plan.out_elem == _lib.ELEM_OF_DTYPE[tdt]
    assert_round(cg, cc, g, cl, "pure")


# ---------------------------------------------------------------- re-binds ----
def test_mixed_round_rebinds_when_the_round_changes_kind():
    tdt = torch.bfloat16
    cg, cc, g, cl = make_round(manifest("float32"), manifest("bfloat16"), 3, seed=12)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, tdt)
    assert_round(cg, cc, g, cl, "mixed")
    # the global is cast to bf16: an all-16-bit round, the pure plan
    cg, g = cg.bfloat16(), g.bfloat16()
    nudge(cc, cl, 1)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_native([g] + cl, tdt)
    rb = engine()._round
    assert rb.plan.elem == rb.plan.out_elem == _lib.FA_ELEM_BF16
    assert_round(cg, cc, g, cl, "pure after the cast")
    # ... and back to fp32: mixed again
    cg, g = cg.float(), g.float()
    nudge(cc, cl, 2)
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, tdt)
    assert_round(cg, cc, g, cl, "mixed again")
    # one client's key goes fp32: staged
    with torch.no_grad():
        p = cc[1]._modules["t4"]._parameters["w"]
        p.data = p.data.float() + 0.001
        q = cl[1]._modules["t4"]._parameters["w"]
        q.data = p.data.cuda()
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert not g._fa_arena.layout.master16
    assert_round(cg, cc, g, cl, "staged after an fp32 key")
    # ... and back to bf16: a staged round that starts qualifying
    with torch.no_grad():
        p.data = p.data.bfloat16()
        q.data = q.data.bfloat16()
    reference_loop(cg, cc)
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, tdt)
    assert_round(cg, cc, g, cl, "mixed after the key returns")


def test_client_with_an_extra_key_raises_where_the_reference_raises():
    man = manifest("bfloat16")
    cg, cc, g, cl = make_round(manifest("float32"), man, 4, seed=13)
    extra = copy.deepcopy(man)
    extra["keys"].append({"key": "more.w", "shape": [5], "dtype": "bfloat16"})
    cc[2] = fill(StateModule(extra), 79)
    cl[2] = copy.deepcopy(cc[2]).cuda()
    before = [copy.deepcopy(c) for c in cc]
    with pytest.raises(RuntimeError, match="more.w"):
        reference_loop(cg, cc)
    with pytest.raises(RuntimeError, match="more.w"):
        feddct_amd.server_aggregate(g, cl)
    torch.cuda.synchronize()
    # the global loaded and the earlier clients updated, through the
    # non-fused broadcast across dtypes; the later client as it was.  (The
    # raising client itself is left alone, as on every other path of the
    # drop-in — tests/test_gpu_parity.py; torch's load_state_dict has copied
    # its matching keys by the time it raises.)
    assert g._fa_arena.layout.master16 and g._fa_arena.f32.dtype == torch.float32
    assert_same_state(cg, g, "global")
    for i in (0, 1):
        assert_same_state(cc[i], cl[i], f"client {i} updated")
        assert cl[i]._fa_arena.layout.native16 and cl[i]._fa_arena._packed == []
    assert_same_state(cc[3], cl[3], "client 3")
    for i in (2, 3):
        assert_same_state(before[i], cl[i], f"client {i} untouched")
    assert not torch.equal(cc[0].state_dict()["t5.w"], before[0].state_dict()["t5.w"])


# ------------------------------------------------------------- the fixture ----
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n", [3, 17, 33])
def test_round_matches_the_reference_fixtures(dtype, n):
    """The reference's own server_aggregate with an fp32 global: the global's
    bits from mixed16_goldens.npz, the clients' from h16_goldens.npz (whose
    inputs the generator used, and whose outputs it found the clients equal
    to)."""
    meta = gold_cases()
    gold16, gold = np.load(GOLD16), np.load(GOLD)
    tdt = DTYPES[dtype]

    def man(dt):
        return {"name": "g", "keys": [dict(e, dtype=dt if e["dtype"] == "h16" else e["dtype"])
                                      for e in meta["keys"]]}

    def load(m, tag):
        with torch.no_grad():
            for k, v in m.state_dict().items():
                t = torch.from_numpy(gold16[f"{dtype}/n{n}/{tag}/{k}"].copy())
                v.copy_(t if v.dtype == torch.int64 else t.view(tdt))
        return m
    cl = [load(StateModule(man(dtype)), f"in{i}").cuda() for i in range(n)]
    g = StateModule(man("float32")).cuda()
    feddct_amd.server_aggregate(g, cl)
    assert_mixed(g, cl, tdt)
    for k, v in g.state_dict().items():
        want = gold[f"{dtype}/n{n}/global/{k}"]
        got = v.cpu() if v.dtype == torch.int64 else v.cpu().view(torch.int32)
        assert np.array_equal(got.numpy(), want), k
    for c in cl:
        for k, v in c.state_dict().items():
            want = gold16[f"{dtype}/n{n}/out/{k}"]
            got = v.cpu() if v.dtype == torch.int64 else v.cpu().view(torch.int16)
            assert np.array_equal(got.numpy(), want), k
