"""GPU: fp16 / bf16 buckets reduced into an fp32 result bucket in torch-ROCm's
GPU summation order (csrc/fedagg_tgpu16.hip's wide-store instances,
fa_plan_create_order_elem_out) and narrowed back into the clients, through the
raw C ABI.  Everything is compared bit for bit with torch itself on the box:
for each key the fp32 result is

    torch.stack([r.float() for r in rows], 0).mean(0)

on ``cuda`` tensors, unrounded, and every client's 16-bit bucket after the
broadcast is that fp32 bucket ``.to(dtype)`` (int64 keys: ``copy_`` of the
fp32 mean into int64); a NaN only has to be a NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import specials
import test_gpu_tgpu16_kernel as K
import tgpu16cases as C
from feddct_amd import _lib, synth
from feddct_amd.layout import KIND_I64, BucketLayout
from test_gpu_tgpu16_kernel import (DEV, DTYPES, L, SPLIT_NS, adversarial, bits, layout_clients,
                                    reduce, same_bits, torch_mean_i64)

pytestmark = pytest.mark.gpu

F32 = _lib.FA_ELEM_F32
NAN_BITS = 0x7FC0E57E        # the result bucket's fill: a NaN that no sum produces


@pytest.fixture(autouse=True)
def _device():
    torch.cuda.set_device(DEV)


def bits32(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits32(got, want):
    """fp32 tensors equal bit for bit, NaN positions as NaN."""
    assert got.dtype == want.dtype == torch.float32
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits32(got)[~gn], bits32(want)[~wn]))


def torch_mean32(rows):
    return torch.stack([r.float() for r in rows], 0).mean(0)


def master_plan(segs32, numel32, segs64=(), numel64=0, *, n, dtype, flags=C.GAPS):
    plan = _lib.Plan.for_order(segs32, numel32, segs64, numel64, n=n, elem=C.ELEMS[dtype],
                               flags=flags, out_elem=F32)
    assert L.fa_plan_elem(plan.handle) == C.ELEMS[dtype] == plan.elem
    assert L.fa_plan_out_elem(plan.handle) == F32 == plan.out_elem
    assert plan.launch_form(n) == (0, 0, 0)
    return plan


def nan_bucket(numel):
    return torch.full((numel,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def run_layout(lay, n, dtype, flags=C.GAPS):
    """The keys of ``lay`` whose fp32 (int64) result differs from torch's."""
    c16, c64 = layout_clients(lay, n, dtype)
    plan = master_plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n=n, dtype=dtype,
                       flags=flags)
    o32 = nan_bucket(lay.f32_numel)
    o64 = torch.full((max(lay.i64_numel, 1),), -7, dtype=torch.int64, device=DEV)
    assert reduce(plan, c16, c64, o32, o64) == _lib.FA_OK, L.fa_last_error()
    bad = []
    for s in lay.slots:
        if s.kind == KIND_I64:
            rows = [c[s.offset:s.offset + s.numel].view(s.shape) for c in c64]
            ok = torch.equal(o64[s.offset:s.offset + s.numel].view(s.shape), torch_mean_i64(rows))
        else:
            rows = [c[s.offset:s.offset + s.numel].view(s.shape) for c in c16]
            want = torch_mean32(rows)
            assert not torch.isnan(want).any()      # so a NaN left is a slot not written
            ok = same_bits32(o32[s.offset:s.offset + s.numel].view(s.shape), want)
        if not ok:
            bad.append(s.key)
    return bad


# ------------------------------------------------------------ row splits ----
@pytest.mark.parametrize("n", SPLIT_NS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_row_split_kernels_store_torch_gpu_fp32_mean(dtype, n):
    """S = 1 .. 16 and both inner forms (the lists of the 16-bit kernel test,
    which pins that they reach them)."""
    ent = [(f"t{j}", (m,) if m > 1 else (), dtype) for j, m in enumerate(K._kept(n))]
    lay = BucketLayout(ent + [("nbt", (), "int64")], native16=True)
    assert run_layout(lay, n, dtype) == []


# ----------------------------------------------------------- client loop ----
@functools.lru_cache(maxsize=None)
def _loop_layout(dtype):
    return BucketLayout([("a", (2048 + 17,), dtype), ("b", (5 * 2048 + 100,), dtype)],
                        native16=True)


@pytest.mark.parametrize("n", range(2, 18))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_client_loop_every_row_count(dtype, n):
    """Every row count mod 8 and the partial passes of both loop forms; full
    and partial wide tiles, and the scalar tail of a key of 2048 + 17."""
    assert run_layout(_loop_layout(dtype), n, dtype) == []


# ------------------------------------------------------------- broadcast ----
@pytest.mark.parametrize("n", [3, 25])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_broadcast_narrows_the_fp32_result_into_every_client(dtype, n):
    tdt = DTYPES[dtype]
    lay = C.manifest_layout(dtype)
    assert all(C.config(n, s.numel)[0] for s in lay.slots)
    c16, c64 = layout_clients(lay, n, dtype)
    keep, keep64 = [c.clone() for c in c16], [c.clone() for c in c64]
    plan = master_plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n=n, dtype=dtype)
    # the broadcast alone: a global of its own fp32 values (padding included)
    g32 = torch.from_numpy(synth.gen_f32(7, lay.f32_numel, 0, 0.0, 0.0,
                                         synth.MODE_ADVERSARIAL)).to(DEV)
    if dtype == "float16":
        g32 = g32 * 2.0 ** -5
    g64 = torch.arange(-3, -3 + max(lay.i64_numel, 1), dtype=torch.int64, device=DEV)
    g32_0 = g32.clone()
    assert reduce(plan, c16, c64, g32, g64, _lib.FA_F_BCAST_ONLY) == _lib.FA_OK, L.fa_last_error()
    assert torch.equal(bits32(g32), bits32(g32_0))
    for i in range(n):
        assert torch.equal(bits(c16[i]), bits(g32.to(tdt))), i
        assert torch.equal(c64[i], g64), i
    # the reduce, then that broadcast
    for c, k in zip(c16 + c64, keep + keep64):
        c.copy_(k)
    o32 = nan_bucket(lay.f32_numel)
    o32[:] = 1.5                    # (padding is narrowed too: a value, not a NaN)
    o64 = torch.full((max(lay.i64_numel, 1),), -7, dtype=torch.int64, device=DEV)
    assert reduce(plan, c16, c64, o32, o64, _lib.FA_F_BCAST) == _lib.FA_OK, L.fa_last_error()
    for s in lay.slots:
        sl = slice(s.offset, s.offset + s.numel)
        if s.kind == KIND_I64:
            assert torch.equal(o64[sl], torch_mean_i64([k[sl] for k in keep64])), s.key
        else:
            assert same_bits32(o32[sl], torch_mean32([k[sl] for k in keep])), s.key
    want16 = o32.to(tdt)
    for i in range(n):
        assert same_bits(c16[i], want16), i
        assert torch.equal(c64[i], o64), i


# -------------------------------------------------------------- raw plans ---
GUARD = 64


@pytest.mark.parametrize("flags", [0, C.GAPS])
@pytest.mark.parametrize("n", [2, 9, 17, 256])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_raw_plans_with_guard_bands(dtype, n, flags):
    """The odd-offset segment list (head and tail scalar tiles at every offset
    residue mod 8, runs cut across key boundaries): every key exact; the
    64-float guard bands on both sides of the NaN-filled fp32 result
    untouched — a store addressed in 16-bit units lands in them or in a
    neighbour —, the clients unchanged, and without the padding flag no gap
    of the result written."""
    segs, numel = C.raw_segments(n)
    assert {int(o) % 8 for o, _ in segs} == set(range(8))
    s64 = np.array([[0, 1], [3, 36]], np.int64)
    x = torch.zeros(n, numel, dtype=DTYPES[dtype])
    for j, (o, m) in enumerate(segs):
        x[:, o:o + m] = adversarial(j, int(m), n, dtype)
    x = x.to(DEV)
    before = x.clone()
    b64 = torch.from_numpy(np.stack(
        [synth.gen_i64(99, 40, i, synth.MODE_ADVERSARIAL) for i in range(n)])).to(DEV)
    before64 = b64.clone()
    res = nan_bucket(numel + 2 * GUARD)
    res64 = torch.full((40 + 16,), -7, dtype=torch.int64, device=DEV)
    o32, o64 = res[GUARD:GUARD + numel], res64[8:48]
    assert o32.data_ptr() % 16 == 0
    plan = master_plan(segs, numel, s64, 40, n=n, dtype=dtype, flags=flags)
    c16, c64 = [x[i] for i in range(n)], [b64[i] for i in range(n)]
    assert reduce(plan, c16, c64, o32, o64) == _lib.FA_OK, L.fa_last_error()
    assert torch.equal(bits(x), bits(before)) and torch.equal(b64, before64)
    assert (bits32(res[:GUARD]) == NAN_BITS).all()
    assert (bits32(res[GUARD + numel:]) == NAN_BITS).all()
    assert (res64[:8] == -7).all() and (res64[48:] == -7).all()
    covered = torch.zeros(numel, dtype=torch.bool, device=DEV)
    for o, m in segs:
        o, m = int(o), int(m)
        want = torch_mean32([c[o:o + m] for c in c16])
        assert not torch.isnan(want).any()
        assert same_bits32(o32[o:o + m], want), (o, m)
        covered[o:o + m] = True
    for o, m in s64:
        o, m = int(o), int(m)
        assert torch.equal(o64[o:o + m], torch_mean_i64([c[o:o + m] for c in c64])), (o, m)
    assert (o64[1:3] == -7).all() and (o64[39:] == -7).all()
    if not flags:
        assert (bits32(o32)[~covered] == NAN_BITS).all()


# ---------------------------------------------------------- special values --
@pytest.mark.parametrize("n", [2, 5, 33, 130])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_special_values_through_vector_scalar_and_inner_tiles(dtype, n):
    """tests/specials.py's columns (-0, subnormals, inf, NaN, overflowing
    sums, inf - inf), unrounded in fp32."""
    segs, numel, _ = specials.layout()
    kinds = {int(k) & 0xFF for k in _lib.build_order_tiles_host(
        segs, numel, n=n, elem=C.ELEMS[dtype], flags=0)[0][:, 2]}
    assert {C.K_W, C.K_SCALAR, C.K_INNER} <= kinds
    x = torch.from_numpy(specials.fill(n, seed=3)).to(DTYPES[dtype]).to(DEV)
    plan = master_plan(segs, numel, n=n, dtype=dtype, flags=0)
    o = torch.zeros(numel, dtype=torch.float32, device=DEV)
    assert reduce(plan, [x[i] for i in range(n)], None, o, None) == _lib.FA_OK, L.fa_last_error()
    nan_cols = 0
    for off, m in segs:
        off, m = int(off), int(m)
        want = torch_mean32([x[i, off:off + m] for i in range(n)])
        assert same_bits32(o[off:off + m], want), (off, m)
        nan_cols += int(torch.isnan(want).sum())
    assert nan_cols > 0


# --------------------------------------------------------------- rounding ---
@pytest.mark.parametrize("pattern", [0, 1, 2])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_narrowing_of_exact_ties_and_near_ties(dtype, pattern):
    """fp32 means that fp32 holds exactly and the 16-bit type does not: over
    every finite magnitude h, both signs, (h, succ h) — the exact tie —,
    (h, h, h, succ h) and (h, succ h, succ h, succ h), a quarter of an ulp to
    either side.  The fp32 bucket holds them unrounded, and the broadcast
    rounds them as torch's ``cuda`` ``.to(dtype)`` does."""
    tdt = DTYPES[dtype]
    rows = K._rounding_rows(dtype)[pattern].to(DEV)
    n, cols = rows.shape
    m = (cols + 7) // 8 * 8
    x = torch.zeros(n, m, dtype=tdt, device=DEV)
    x[:, :cols] = rows
    keep = x.clone()
    assert C.config(n, m) == (True, 1)
    plan = master_plan(np.array([[0, m]]), m, n=n, dtype=dtype)
    o32 = nan_bucket(m)
    c16 = [x[i] for i in range(n)]
    assert reduce(plan, c16, None, o32, None, _lib.FA_F_BCAST) == _lib.FA_OK, L.fa_last_error()
    want32 = torch_mean32([keep[i] for i in range(n)])
    assert same_bits32(o32, want32)
    # the means are exact where they are finite: float64 agrees (looked at in
    # fp32's normal range: the choice of rows is what this line checks)
    fin = torch.isfinite(want32)
    nrm = fin & (want32.abs() >= 2.0 ** -120)
    assert nrm.sum() > cols // 2
    assert torch.equal(want32[nrm].double(), keep.double().mean(0)[nrm])
    # ... and no 16-bit value (a tie or near-tie), zero and the top aside
    assert (want32[:cols][fin[:cols]] != want32[:cols].to(tdt).float()[fin[:cols]]).sum() \
        > cols // 2
    want16 = want32.to(tdt)
    for i in range(n):
        assert same_bits(c16[i], want16), i
    if pattern == 0:    # the tie goes to even: the one of (h, succ h) with bit 0 clear
        hb = bits(rows[0]).to(torch.int32) & 0xFFFF
        ok = (hb & 0x7FFF) < (0x7bff if dtype == "float16" else 0x7f00)
        even = torch.where((hb & 1) == 0, hb, hb + 1)
        got = bits(c16[0][:cols]).to(torch.int32) & 0xFFFF
        assert torch.equal(got[ok], even[ok])


# -------------------------------------------------------------- refusals ----
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_refusals_leave_poisoned_buffers_unchanged(dtype):
    tdt, n = DTYPES[dtype], 4
    segs = np.array([[0, 4096], [4096 + 200, 64]], np.int64)   # a gap of 200: no coverage
    numel = 4096 + 200 + 64
    part = master_plan(segs, numel, n=n, dtype=dtype)
    full = master_plan(np.array([[0, numel]]), numel, n=n, dtype=dtype)
    buf = torch.full((n + 1, numel), 3.0, dtype=tdt, device=DEV)
    o32 = nan_bucket(numel)
    before = buf.clone()
    c16 = [buf[i] for i in range(n + 1)]
    w = [0.25] * n

    def unchanged():
        torch.cuda.synchronize()
        return bool(torch.equal(bits(buf), bits(before))) and \
            bool((bits32(o32) == NAN_BITS).all())

    def refused(plan, what, **kw):
        rc = reduce(plan, c16[:kw.pop("n", n)], None, o32, None, **kw)
        assert rc == _lib.FA_E_INVAL, (what, rc)
        assert what.encode() in L.fa_last_error(), (what, L.fa_last_error())
        assert unchanged(), what

    refused(full, "unweighted", weights=w)
    refused(full, "cut for n=4", n=3)
    refused(full, "cut for n=4", n=5)
    refused(full, "SUM_ONLY", flags=_lib.FA_F_SUM_ONLY)
    refused(part, "FA_PLAN_GAPS_ARE_PADDING", flags=_lib.FA_F_BCAST)
    refused(part, "FA_PLAN_GAPS_ARE_PADDING", flags=_lib.FA_F_BCAST_ONLY)
    ch = _lib.FaChain(0, n, None, None, numel)
    a16 = _lib.ptr_array([c.data_ptr() for c in c16[:n]])
    assert L.fa_reduce_chain(full.handle, a16, n, None, ctypes.byref(ch), o32.data_ptr(), 0,
                             None) == _lib.FA_E_INVAL
    assert b"16-bit plan" in L.fa_last_error() and unchanged()
    # and the plans work: the refusals above were the calls', not the plans'
    assert reduce(part, c16[:n], None, o32, None) == _lib.FA_OK
    assert (o32[:4096] == 3.0).all() and (o32[4096 + 200:] == 3.0).all()
    assert torch.equal(bits(buf), bits(before))
