"""GPU: torch-ROCm's GPU summation order over fp16 / bf16 buckets
(csrc/fedagg_tgpu16.hip, fa_plan_create_order_elem) through the raw C ABI.
Everything is compared bit for bit with torch itself on the box: for each key

    torch.stack([r.float() for r in rows], 0).mean(0).to(dtype)

on ``cuda`` tensors (int64 keys: ``copy_`` of the fp32 mean into int64, as
tests/test_gpu_torch_order.py::_vs_torch); a NaN only has to be a NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import specials
import tgpu16cases as C
from feddct_amd import _lib, synth
from feddct_amd.layout import KIND_I64, BucketLayout
from oracle import torch_gpu_order as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
L = _lib.lib


@pytest.fixture(autouse=True)
def _device():
    torch.cuda.set_device(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int16)


def same_bits(got, want):
    """16-bit tensors equal bit for bit, NaN positions as NaN."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


def torch_mean(rows, tdt):
    return torch.stack([r.float() for r in rows], 0).mean(0).to(tdt)


def torch_mean_i64(rows):
    ref = torch.stack([r.float() for r in rows], 0).mean(0)
    want = torch.zeros(ref.shape, dtype=torch.int64, device=ref.device)
    want.copy_(ref)          # load_state_dict's copy_: fp32 -> int64 truncation
    return want


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def reduce(plan, c16, c64, o16, o64, flags=0, weights=None, n=None):
    n = len(c16) if n is None else n
    a16 = _lib.ptr_array([c.data_ptr() for c in c16])
    a64 = _lib.ptr_array([c.data_ptr() for c in c64]) if c64 is not None else None
    w = None if weights is None else (ctypes.c_float * n)(*[float(v) for v in weights])
    rc = L.fa_reduce(plan.handle, a16, a64, n, w, o16.data_ptr(),
                     o64.data_ptr() if o64 is not None else None, flags, stream())
    torch.cuda.synchronize()
    return rc


def adversarial(key, numel, n, dtype):
    """[n, numel] of the 16-bit dtype: synth's adversarial values (magnitudes
    2^-20 .. 2^20 of both signs), for fp16 scaled by 2^-5 so none overflows."""
    x = np.stack([synth.gen_f32(key, numel, i, 0.0, 0.0, synth.MODE_ADVERSARIAL)
                  for i in range(n)])
    if dtype == "float16":
        x = x * np.float32(2.0 ** -5)
    return torch.from_numpy(x).to(DTYPES[dtype])


def layout_clients(lay, n, dtype):
    """n client (16-bit bucket, int64 bucket) pairs over a native-16 layout."""
    x16 = torch.zeros(n, lay.f32_numel, dtype=DTYPES[dtype])
    x64 = torch.zeros(n, max(lay.i64_numel, 1), dtype=torch.int64)
    for j, s in enumerate(lay.slots):
        if s.kind == KIND_I64:
            x64[:, s.offset:s.offset + s.numel] = torch.from_numpy(np.stack(
                [synth.gen_i64(j, s.numel, i, synth.MODE_ADVERSARIAL) for i in range(n)]))
        else:
            x16[:, s.offset:s.offset + s.numel] = adversarial(j, s.numel, n, dtype)
    x16, x64 = x16.to(DEV), x64.to(DEV)
    return [x16[i] for i in range(n)], [x64[i] for i in range(n)]


def run_layout(lay, n, dtype, flags=_lib.FA_PLAN_GAPS_ARE_PADDING):
    tdt = DTYPES[dtype]
    c16, c64 = layout_clients(lay, n, dtype)
    plan = _lib.Plan.for_order(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n=n,
                               elem=C.ELEMS[dtype], flags=flags)
    o16 = torch.full((lay.f32_numel,), float("nan"), dtype=tdt, device=DEV)
    o64 = torch.full((max(lay.i64_numel, 1),), -7, dtype=torch.int64, device=DEV)
    assert reduce(plan, c16, c64, o16, o64) == _lib.FA_OK, L.fa_last_error()
    bad = []
    for s in lay.slots:
        if s.kind == KIND_I64:
            rows = [c[s.offset:s.offset + s.numel].view(s.shape) for c in c64]
            ok = torch.equal(o64[s.offset:s.offset + s.numel].view(s.shape), torch_mean_i64(rows))
        else:
            rows = [c[s.offset:s.offset + s.numel].view(s.shape) for c in c16]
            ok = same_bits(o16[s.offset:s.offset + s.numel].view(s.shape), torch_mean(rows, tdt))
        if not ok:
            bad.append(s.key)
    return bad


# ------------------------------------------------------------ row splits ----
SPLIT_MS = [1, 2, 3, 6, 8, 16, 36, 64, 100, 128, 200, 256, 1024, 4097, 65536]
SPLIT_NS = [2, 3, 9, 17, 32, 64, 127, 128, 129, 200, 256, 300]


def _kept(n):
    return [m for m in SPLIT_MS if C.config(n, m)[0]]


def test_refused_keys_are_exactly_the_high_blocks():
    """fa_torch_gpu_config refuses no key of the list up to N = 200 and
    exactly M in {2, 3, 6, 8, 16} at N = 256 and 300: torch's block is higher
    than 16 rows there (the oracle's config), no cross-block split."""
    for n in SPLIT_NS:
        dropped = set(SPLIT_MS) - set(_kept(n))
        assert dropped == (set() if n <= 200 else {2, 3, 6, 8, 16}), (n, dropped)
        for m in dropped:
            cfg = G.config(n, m)
            assert cfg["kind"] == "outer" and cfg["split"] and cfg["bh"] > 16 and not cfg["global"]
        for m in _kept(n):
            assert not G.config(n, m)["global"]


def test_row_split_lists_reach_every_split_and_both_inner_forms():
    seen, inner = set(), set()
    for n in SPLIT_NS:
        for m in _kept(n):
            if m > 1:
                seen.add(C.config(n, m)[1])
            else:
                inner.add(G.config(n, 1)["vec"])
    assert seen == {1, 2, 4, 8, 16} and inner == {False, True}


@pytest.mark.parametrize("n", SPLIT_NS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_row_split_kernels_match_torch_gpu_mean(dtype, n):
    ent = [(f"t{j}", (m,) if m > 1 else (), dtype) for j, m in enumerate(_kept(n))]
    lay = BucketLayout(ent + [("nbt", (), "int64")], native16=True)
    assert run_layout(lay, n, dtype) == []


# ----------------------------------------------------------- client loop ----
LOOP_NS = [2, 3, 4, 5, 6, 7, 8, 9, 11, 15, 16, 17, 18, 19, 21, 27, 31]


@functools.lru_cache(maxsize=None)
def _loop_layout(dtype):
    return BucketLayout([(f"w{j}", (m,), dtype)
                         for j, m in enumerate([2048 * 3, 2048 * 5 + 100, 4096, 2047, 8])],
                        native16=True)


@pytest.mark.parametrize("n", LOOP_NS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_client_loop_every_row_count(dtype, n):
    """Every row count mod 4 (and mod 8), full tiles beside partial ones."""
    lay = _loop_layout(dtype)
    assert all(C.config(n, s.numel) == (True, 1) for s in lay.slots)
    assert run_layout(lay, n, dtype) == []


# -------------------------------------------------------------- raw plans ---
GUARD = 256
POISON = 0x7e57


@pytest.mark.parametrize("flags", [0, C.GAPS])
@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_raw_plans_with_guard_bands(dtype, n, flags):
    """The CPU test's odd-offset segment list: every key against torch, the
    guard bands around the result and every client untouched, the clients
    themselves unchanged, and without the padding flag no gap element of the
    result written."""
    tdt = DTYPES[dtype]
    segs, numel = C.raw_segments(n)
    s64 = np.array([[0, 1], [3, 36]], np.int64)
    host_tiles, host_fac, host_lo = _lib.build_order_tiles_host(
        segs, numel, s64, 40, n=n, flags=flags, elem=C.ELEMS[dtype])
    C.check_table(segs, numel, s64, 40, n, flags, C.ELEMS[dtype], host_tiles, host_fac, host_lo)
    buf = torch.zeros(n + 1, numel + 2 * GUARD, dtype=tdt)
    for j, (o, m) in enumerate(segs):
        buf[:n, GUARD + o:GUARD + o + m] = adversarial(j, int(m), n, dtype)
    raw = buf.view(torch.int16)        # the poison as bits (a NaN's payload would not survive)
    raw[:, :GUARD] = POISON
    raw[:, GUARD + numel:] = POISON
    raw[n, GUARD:GUARD + numel] = POISON
    buf = buf.to(DEV)
    before = buf.clone()
    b64 = torch.zeros(n + 1, 40 + 2 * 8, dtype=torch.int64)
    b64[:n, 8:48] = torch.from_numpy(np.stack(
        [synth.gen_i64(99, 40, i, synth.MODE_ADVERSARIAL) for i in range(n)]))
    b64[n] = -7
    b64[:, :8] = -9
    b64[:, 48:] = -9
    b64 = b64.to(DEV)
    before64 = b64.clone()
    plan = _lib.Plan.for_order(segs, numel, s64, 40, n=n, elem=C.ELEMS[dtype], flags=flags)
    assert plan.info["ntiles"] == len(host_tiles)
    c16 = [buf[i, GUARD:GUARD + numel] for i in range(n)]
    c64 = [b64[i, 8:48] for i in range(n)]
    o16, o64 = buf[n, GUARD:GUARD + numel], b64[n, 8:48]
    assert reduce(plan, c16, c64, o16, o64) == _lib.FA_OK, L.fa_last_error()
    assert torch.equal(bits(buf[:n]), bits(before[:n])) and torch.equal(b64[:n], before64[:n])
    assert torch.equal(bits(buf[n, :GUARD]), bits(before[n, :GUARD]))
    assert torch.equal(bits(buf[n, GUARD + numel:]), bits(before[n, GUARD + numel:]))
    assert torch.equal(b64[n, :8], before64[n, :8]) and torch.equal(b64[n, 48:], before64[n, 48:])
    covered = torch.zeros(numel, dtype=torch.bool, device=DEV)
    for o, m in segs:
        o, m = int(o), int(m)
        want = torch_mean([c[o:o + m] for c in c16], tdt)
        assert same_bits(o16[o:o + m], want), (o, m)
        covered[o:o + m] = True
    for o, m in s64:
        o, m = int(o), int(m)
        assert torch.equal(o64[o:o + m], torch_mean_i64([c[o:o + m] for c in c64])), (o, m)
    assert (o64[1:3] == -7).all() and (o64[39:] == -7).all()
    if not flags:
        assert (bits(o16)[~covered] == POISON).all()


# --------------------------------------------------------------- rounding ---
def _rounding_rows(dtype):
    """(rows for N = 2, rows for N = 4 [two patterns]) over every finite
    magnitude h of the format, both signs: columns (h, succ h) — an exact tie
    —, (h, h, h, succ h) and (h, succ h, succ h, succ h)."""
    top = 0x7bff if dtype == "float16" else 0x7f7f
    h = np.arange(0, top + 1, dtype=np.int64)
    h = np.concatenate([h, h | 0x8000])
    s = h + 1                                   # the next magnitude, same sign
    as16 = lambda v: torch.from_numpy(v.astype(np.uint16).view(np.int16).copy()).view(DTYPES[dtype])
    h, s = as16(h), as16(s)
    return [torch.stack([h, s]), torch.stack([h, h, h, s]), torch.stack([h, s, s, s])]


@pytest.mark.parametrize("pattern", [0, 1, 2])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_rounding_of_every_finite_magnitude(dtype, pattern):
    """Once through one aligned key (vector tiles) and once through 7-element
    keys at offsets 1 mod 8 (each wholly a scalar head tile)."""
    tdt = DTYPES[dtype]
    rows = _rounding_rows(dtype)[pattern].to(DEV)
    n, cols = rows.shape
    # vector tiles: one key of every column, padded to whole 8-element vectors
    m = (cols + 7) // 8 * 8
    x = torch.zeros(n, m, dtype=tdt, device=DEV)
    x[:, :cols] = rows
    plan = _lib.Plan.for_order(np.array([[0, m]]), m, n=n, elem=C.ELEMS[dtype])
    assert all((k & 0xFF) == C.K_W for k in _lib.build_order_tiles_host(
        np.array([[0, m]]), m, n=n, elem=C.ELEMS[dtype])[0][:, 2])
    o = torch.zeros(m, dtype=tdt, device=DEV)
    assert reduce(plan, [x[i] for i in range(n)], None, o, None) == _lib.FA_OK, L.fa_last_error()
    want = torch_mean([x[i] for i in range(n)], tdt)
    assert same_bits(o, want)
    # the tie (N = 2): to even, which is the one of (h, succ h) with bit 0 clear
    # (bf16's top binade aside: there h + succ h overflows in fp32, for torch too)
    if pattern == 0:
        hb = bits(rows[0]).to(torch.int32) & 0xFFFF
        fin = (hb & 0x7FFF) < (0x7bff if dtype == "float16" else 0x7f00)
        even = torch.where((hb & 1) == 0, hb, hb + 1)
        got = bits(o[:cols]).to(torch.int32) & 0xFFFF
        assert torch.equal(got[fin], even[fin])
    # scalar tiles: the same columns as 7-element keys, each at 1 mod 8
    k = (cols + 6) // 7
    segs = np.stack([np.arange(k, dtype=np.int64) * 8 + 1, np.full(k, 7, np.int64)], 1)
    numel = 8 * k
    tiles = _lib.build_order_tiles_host(segs, numel, n=n, elem=C.ELEMS[dtype], flags=0)[0]
    assert all((kd & 0xFF) == C.K_SCALAR for kd in tiles[:, 2]) and len(tiles) == k
    y = torch.zeros(n, k, 8, dtype=tdt, device=DEV)
    pad = torch.zeros(n, 7 * k, dtype=tdt, device=DEV)
    pad[:, :cols] = rows
    y[:, :, 1:] = pad.view(n, k, 7)
    y = y.view(n, numel)
    plan = _lib.Plan.for_order(segs, numel, n=n, elem=C.ELEMS[dtype], flags=0)
    o = torch.full((numel,), 1.0, dtype=tdt, device=DEV)
    assert reduce(plan, [y[i] for i in range(n)], None, o, None) == _lib.FA_OK, L.fa_last_error()
    # torch on all keys at once ([N, k, 7]: the same S = 1 order and factor
    # 1 / N as a 7-element key's), and on every 97th key by itself
    want = torch_mean([y[i].view(k, 8)[:, 1:] for i in range(n)], tdt)
    assert same_bits(o.view(k, 8)[:, 1:], want)
    assert (o.view(k, 8)[:, 0] == 1.0).all()
    for j in range(0, k, 97):
        assert same_bits(o[8 * j + 1:8 * j + 8],
                         torch_mean([y[i, 8 * j + 1:8 * j + 8] for i in range(n)], tdt)), j


# ---------------------------------------------------------- special values --
@pytest.mark.parametrize("n", [2, 5, 33, 130])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_special_values_through_vector_scalar_and_inner_tiles(dtype, n):
    """tests/specials.py's columns (-0, subnormals, inf, NaN, overflowing
    sums, inf - inf) rounded into the 16-bit type, through its layout: keys in
    vector tiles, unaligned and short keys in scalar tiles, 0-dim keys."""
    tdt = DTYPES[dtype]
    segs, numel, _ = specials.layout()
    kinds = {int(k) & 0xFF for k in _lib.build_order_tiles_host(
        segs, numel, n=n, elem=C.ELEMS[dtype], flags=0)[0][:, 2]}
    assert {C.K_W, C.K_SCALAR, C.K_INNER} <= kinds
    x = torch.from_numpy(specials.fill(n, seed=3)).to(tdt).to(DEV)
    plan = _lib.Plan.for_order(segs, numel, n=n, elem=C.ELEMS[dtype], flags=0)
    o = torch.zeros(numel, dtype=tdt, device=DEV)
    assert reduce(plan, [x[i] for i in range(n)], None, o, None) == _lib.FA_OK, L.fa_last_error()
    nan_cols = 0
    for off, m in segs:
        off, m = int(off), int(m)
        want = torch_mean([x[i, off:off + m] for i in range(n)], tdt)
        assert same_bits(o[off:off + m], want), (off, m)
        nan_cols += int(torch.isnan(want).sum())
    assert nan_cols > 0


# ------------------------------------------------- broadcast and refusals ---
BC_SEGS = np.array([[0, 2048 + 100], [2152, 37], [2189, 1]], np.int64)
BC_NUMEL = 2198     # even, 6 elements past the last whole 16-B vector


@pytest.mark.parametrize("n", [3, 25])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_broadcast_copies_the_result_bytes_to_every_client(dtype, n):
    tdt = DTYPES[dtype]
    assert BC_NUMEL % 8 == 6
    s64 = np.array([[0, 1]], np.int64)
    plan = _lib.Plan.for_order(BC_SEGS, BC_NUMEL, s64, 1, n=n, elem=C.ELEMS[dtype])
    c16 = [adversarial(i, BC_NUMEL, 1, dtype)[0].to(DEV) for i in range(n)]
    c64 = [torch.tensor([1000 + 3 * i], dtype=torch.int64, device=DEV) for i in range(n)]
    keep = [c.clone() for c in c16]
    keep64 = [c.clone() for c in c64]
    # a result bucket whose padding (the trailing 6 elements too) is its own
    o16 = adversarial(77, BC_NUMEL, 1, dtype)[0].to(DEV)
    o64 = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert reduce(plan, c16, c64, o16, o64, _lib.FA_F_BCAST) == _lib.FA_OK, L.fa_last_error()
    for o, m in BC_SEGS:
        o, m = int(o), int(m)
        assert same_bits(o16[o:o + m], torch_mean([k[o:o + m] for k in keep], tdt)), (o, m)
    assert torch.equal(o64, torch_mean_i64(keep64))
    for i in range(n):
        assert torch.equal(bits(c16[i]), bits(o16)), i
        assert torch.equal(c64[i], o64), i
    # the broadcast alone: new global bytes into every client
    g16 = adversarial(5, BC_NUMEL, 1, dtype)[0].to(DEV)
    g64 = torch.tensor([-123], dtype=torch.int64, device=DEV)
    assert reduce(plan, c16, c64, g16, g64, _lib.FA_F_BCAST_ONLY) == _lib.FA_OK
    for i in range(n):
        assert torch.equal(bits(c16[i]), bits(g16)) and torch.equal(c64[i], g64), i


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_refusals_leave_poisoned_buffers_unchanged(dtype):
    tdt, n = DTYPES[dtype], 4
    segs = np.array([[0, 4096], [4096 + 200, 64]], np.int64)   # a gap of 200: no flat coverage
    numel = 4096 + 200 + 64
    part = _lib.Plan.for_order(segs, numel, n=n, elem=C.ELEMS[dtype])
    full = _lib.Plan.for_order(np.array([[0, numel]]), numel, n=n, elem=C.ELEMS[dtype])
    assert L.fa_plan_elem(full.handle) == C.ELEMS[dtype]
    assert L.fa_plan_out_elem(full.handle) == C.ELEMS[dtype]
    buf = torch.full((n + 2, numel), 3.0, dtype=tdt, device=DEV)
    before = buf.clone()
    c16, o16 = [buf[i] for i in range(n + 1)], buf[n + 1]
    w = [0.25] * n

    def refused(plan, what, **kw):
        rc = reduce(plan, c16[:kw.pop("n", n)], None, o16, None, **kw)
        assert rc == _lib.FA_E_INVAL, (what, rc)
        assert what.encode() in L.fa_last_error(), (what, L.fa_last_error())
        assert torch.equal(bits(buf), bits(before)), what

    refused(full, "unweighted", weights=w)
    refused(full, "cut for n=4", n=3)
    refused(full, "cut for n=4", n=5)
    refused(full, "SUM_ONLY", flags=_lib.FA_F_SUM_ONLY)
    refused(part, "flat", flags=_lib.FA_F_BCAST)
    refused(part, "flat", flags=_lib.FA_F_BCAST_ONLY)
    ch = _lib.FaChain(0, n, None, None, numel)
    a16 = _lib.ptr_array([c.data_ptr() for c in c16[:n]])
    assert L.fa_reduce_chain(full.handle, a16, n, None, ctypes.byref(ch), o16.data_ptr(), 0,
                             None) == _lib.FA_E_INVAL
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before))
    # and the plans work: the refusals above were the calls', not the plans'
    assert reduce(part, c16[:n], None, o16, None) == _lib.FA_OK
    assert (o16[:4096] == 3.0).all() and (o16[4096 + 200:] == 3.0).all()
    # the forwarding arms of the entry
    cpu = _lib.Plan.for_order(segs, numel, n=n, elem=C.ELEMS[dtype],
                              order=_lib.FA_ORDER_TORCH_CPU)
    assert L.fa_plan_elem(cpu.handle) == C.ELEMS[dtype] and cpu.launch_form(n)[2] == 1
    f32 = _lib.Plan.for_order(segs, numel, n=n, elem=_lib.FA_ELEM_F32)
    assert L.fa_plan_elem(f32.handle) == _lib.FA_ELEM_F32
