"""The mixed plan (fa_plan_create_elem_out: 16-bit clients, fp32 result)
through the C ABI on raw segment lists: the wide-store instances of the
16-bit reduce against the oracle's fp32 mean bit for bit, the narrowing
broadcast against torch's CPU ``.to(dtype)`` of the fp32 result and against a
pure 16-bit plan's broadcast, guard bands around every buffer, the refusals,
the broadcast's rounding exhaustively, and the wide store on exact-sum data
(tests/h16ref.py: no summation order enters)."""
import ctypes

import numpy as np
import pytest
import torch

import h16ref as R
from feddct_amd import _lib
from oracle import torch_order as T
from test_gpu_h16_exact import NUMEL, SEGS, gather, place
from test_gpu_h16_kernel import DATA, make_i64, make_inputs

pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float16": _lib.FA_ELEM_F16, "bfloat16": _lib.FA_ELEM_BF16}
PAD = _lib.FA_PLAN_GAPS_ARE_PADDING
GUARD = 64                      # elements on each side of every buffer
G16, G32, G64 = 0x5a5a, 0xdeadbeef, -0x0123456789abcdef
LENS = [1, 4, 5, 6, 7, 8, 33, 100, 2049, 4097]
SEGS64 = [(0, 1), (1, 5)]
NS = [1, 3, 9, 17, 24, 25, 128, 129, 257]


def seg_list(variant, residue):
    """LENS as segments -> (segs, f32_numel, plan flags).  "aligned": every
    key on the next multiple of 8 (gaps < 128: padding); "packed": back to
    back, so most offsets are no multiple of 8; "gaps": aligned and odd
    offsets across gaps that are NOT padding (flags 0).  f32_numel ends
    ``residue`` mod 8."""
    segs, off = [], 0
    for j, m in enumerate(LENS):
        if variant == "aligned":
            off = (off + 7) // 8 * 8
        elif variant == "gaps":
            off += (0, 3, 8, 13)[j % 4]
        segs.append((off, m))
        off += m
    numel = off + 1
    numel += (residue - numel) % 8
    return segs, numel, (0 if variant == "gaps" else PAD)


class Bufs:
    """n 16-bit client buckets, an fp32 result bucket and the int64 buckets on
    the device, each between two guard bands."""

    def __init__(self, dtype, bits, x64, numel):
        n = bits.shape[0]
        self.n, self.numel, self.dtype = n, numel, dtype
        self.row = (numel + 7) // 8 * 8 + 2 * GUARD          # rows stay 16-B aligned
        host = np.full((n, self.row), G16, np.uint16)
        host[:, GUARD:GUARD + numel] = bits
        self.c16 = torch.from_numpy(host.view(np.int16)).cuda()
        o = np.full(numel + 2 * GUARD, G32, np.uint32)
        self.o32 = torch.from_numpy(o.view(np.int32)).cuda()
        self.n64 = x64.shape[1]
        h64 = np.full((n, self.n64 + 2 * GUARD), G64, np.int64)
        h64[:, GUARD:GUARD + self.n64] = x64
        self.c64 = torch.from_numpy(h64).cuda()
        self.o64 = torch.full((self.n64 + 2 * GUARD,), G64, dtype=torch.int64, device="cuda")
        self.a16 = _lib.ptr_array([self.c16.data_ptr() + 2 * (self.row * i + GUARD)
                                   for i in range(n)])
        self.a64 = _lib.ptr_array([self.c64.data_ptr() + 8 * ((self.n64 + 2 * GUARD) * i + GUARD)
                                   for i in range(n)])
        self.p32 = self.o32.data_ptr() + 4 * GUARD
        self.p64 = self.o64.data_ptr() + 8 * GUARD

    def call(self, plan, flags=0, weights=None, out16=None):
        w = None if weights is None else (ctypes.c_float * self.n)(*[float(v) for v in weights])
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = _lib.lib.fa_reduce(plan.handle, self.a16, self.a64 if self.n64 else None, self.n, w,
                                self.p32 if out16 is None else out16,
                                self.p64 if self.n64 else None, flags, st)
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return [t.clone() for t in (self.c16, self.o32, self.c64, self.o64)]

    def out_bits(self):
        return self.o32.cpu().numpy().view(np.uint32)[GUARD:GUARD + self.numel]

    def client_bits(self):
        return self.c16.cpu().numpy().view(np.uint16)[:, GUARD:GUARD + self.numel]

    def assert_guards(self, what):
        o = self.o32.cpu().numpy().view(np.uint32)
        assert (o[:GUARD] == G32).all() and (o[GUARD + self.numel:] == G32).all(), (what, "out32")
        c = self.c16.cpu().numpy().view(np.uint16)
        assert (c[:, :GUARD] == G16).all() and (c[:, GUARD + self.numel:] == G16).all(), \
            (what, "client 16-bit buckets")
        o64, c64 = self.o64.cpu().numpy(), self.c64.cpu().numpy()
        assert (o64[:GUARD] == G64).all() and (o64[GUARD + self.n64:] == G64).all(), (what, "out64")
        assert (c64[:, :GUARD] == G64).all() and (c64[:, GUARD + self.n64:] == G64).all(), \
            (what, "client int64 buckets")


def mixed_plan(dtype, segs, numel, flags, segs64=(), n64=0, tile=0):
    p = _lib.Plan(np.asarray(segs, np.int64).reshape(-1, 2), numel, segs64, n64, tile_elems=tile,
                  flags=flags, elem=ELEM[dtype], out_elem=_lib.FA_ELEM_F32)
    assert p.elem == ELEM[dtype] and p.out_elem == _lib.FA_ELEM_F32
    assert _lib.lib.fa_plan_elem(p.handle) == ELEM[dtype]
    assert _lib.lib.fa_plan_out_elem(p.handle) == _lib.FA_ELEM_F32
    return p


def pure_plan(dtype, segs, numel, flags, segs64=(), n64=0):
    return _lib.Plan(np.asarray(segs, np.int64).reshape(-1, 2), numel, segs64, n64, flags=flags,
                     elem=ELEM[dtype])


def bits_of16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def to16(bits32, dtype):
    """torch's CPU .to(dtype) of fp32 bit patterns -> (uint16 bits, NaN mask)."""
    f = torch.from_numpy(np.ascontiguousarray(bits32, np.uint32).view(np.float32).copy())
    return bits_of16(f.to(TDT[dtype])), torch.isnan(f).numpy()


def assert_f32_bits(got, want, what):
    """uint32 patterns against float32 values; a NaN only has to be a NaN."""
    g = got.view(np.float32)
    gn, wn = np.isnan(g), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions")
    wb = np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.nonzero((got != wb) & ~wn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], wb[bad[:5]])


def assert_narrowed(cbits, out32, dtype, what):
    """Every client row == .to(dtype) of the fp32 bucket (NaN where it is NaN)."""
    wb, wn = to16(out32, dtype)
    for i in range(cbits.shape[0]):
        gn = np.isnan(R.widen(cbits[i], dtype))
        assert np.array_equal(gn, wn), (what, i, "NaN positions")
        bad = np.nonzero((cbits[i] != wb) & ~wn)[0]
        assert bad.size == 0, (what, i, bad[:5], cbits[i][bad[:5]], wb[bad[:5]])


def oracle(bits, dtype, segs, weights):
    xf = R.widen(bits, dtype).astype(np.float32)      # exact
    out = []
    for o, m in segs:
        with np.errstate(all="ignore"):
            v = xf[:, o:o + m]
            out.append(T.torch_mean0(v) if weights is None else T.weighted_sum0(v, weights))
    return np.concatenate(out).astype(np.float32)


def round_case(dtype, n, variant, residue, data, weighted, segs=None, numel=None, tile=0):
    if segs is None:
        segs, numel, flags = seg_list(variant, residue)
    else:
        flags = PAD
    assert numel % 8 == residue
    tdt = TDT[dtype]
    seed = 1000 * n + 8 * DATA.index(data) + residue
    bits = bits_of16(make_inputs(dtype, n, data, numel, seed))
    x64 = make_i64(n, 6, seed).numpy()
    w = T.weights_from_sizes(np.random.default_rng(seed).integers(10, 1000, n)) if weighted \
        else None
    what = (dtype, n, variant, residue, data, weighted)
    pl = mixed_plan(dtype, segs, numel, flags, SEGS64, 6, tile)
    b = Bufs(dtype, bits, x64, numel)
    inside = np.zeros(numel, bool)
    for o, m in segs:
        inside[o:o + m] = True
    # the reduce alone: the fp32 mean, unrounded, at the same element offsets
    assert b.call(pl, 0, w) == _lib.FA_OK, _lib.lib.fa_last_error()
    out = b.out_bits()
    assert_f32_bits(gather(out, segs), oracle(bits, dtype, segs, w), what)
    if not flags:
        assert (out[~inside] == G32).all(), (what, "wrote a gap that is not padding")
    want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in SEGS64])
    assert np.array_equal(b.o64.cpu().numpy()[GUARD:GUARD + 6], want64), what
    assert np.array_equal(b.client_bits(), bits), (what, "the reduce wrote a client")
    b.assert_guards(what)
    if not flags:
        return
    # reduce + broadcast: the same result, narrowed into every client over
    # [0, f32_numel) — padding and the trailing mod-8 elements included
    b2 = Bufs(dtype, bits, x64, numel)
    assert b2.call(pl, _lib.FA_F_BCAST, w) == _lib.FA_OK, _lib.lib.fa_last_error()
    out2 = b2.out_bits()
    assert np.array_equal(out2[inside], out[inside]), what
    assert_narrowed(b2.client_bits(), out2, dtype, what)
    c64 = b2.c64.cpu().numpy()[:, GUARD:GUARD + 6]
    assert (c64 == want64[None, :]).all(), what
    b2.assert_guards(what)
    # the clients' bits against a pure 16-bit plan's round on the same inputs
    # (no oracle in this check; a pure plan broadcasts an even bucket only)
    if numel % 2 == 0:
        b3 = Bufs(dtype, bits, x64, numel)
        o16 = torch.zeros(b3.row, dtype=tdt, device="cuda")
        assert b3.call(pure_plan(dtype, segs, numel, flags, SEGS64, 6), _lib.FA_F_BCAST, w,
                       out16=o16.data_ptr()) == _lib.FA_OK, _lib.lib.fa_last_error()
        got, ref = b2.client_bits()[:, inside], b3.client_bits()[:, inside]
        nan = np.isnan(R.widen(ref, dtype))
        assert np.array_equal(np.isnan(R.widen(got, dtype)), nan), what
        assert np.array_equal(got[~nan], ref[~nan]), (what, "differs from the pure 16-bit round")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k,n", list(enumerate(NS)))
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_round_matches_the_oracle(dtype, k, n, weighted):
    """Every client count, each with another f32_numel residue and data
    kind, on the aligned and the packed layout (weighted: finite data)."""
    data = ("realistic", "cancel", "subnormal")[k % 3] if weighted else DATA[k % len(DATA)]
    for j, variant in enumerate(("aligned", "packed")):
        round_case(dtype, n, variant, (k + 4 * j + (dtype == "float16")) % 8, data, weighted)


@pytest.mark.parametrize("residue", range(8))
@pytest.mark.parametrize("variant", ["aligned", "packed", "gaps"])
def test_every_residue_of_the_bucket_length(variant, residue):
    dtype = ("bfloat16", "float16")[residue % 2]
    round_case(dtype, 3 + residue, variant, residue, DATA[residue % len(DATA)], False)


@pytest.mark.parametrize("dtype", sorted(TDT))
def test_the_other_tile_width_gives_the_same_bits(dtype):
    for tile in (2048, 4096):
        round_case(dtype, 17, "aligned", 0, "realistic", False, tile=tile)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_third_cascade_level_at_4097_clients(dtype, weighted):
    segs = [(0, 40), (41, 33), (74, 7), (81, 1), (88, 100), (192, 8)]
    round_case(dtype, 4097, "small", 3, "realistic" if weighted else "cancel", weighted,
               segs=segs, numel=203)


# ---------------------------------------------------------------- refusals ----
def test_equal_types_give_the_existing_plan():
    segs, numel, flags = seg_list("aligned", 0)
    for elem in (_lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16):
        a = _lib.Plan(np.asarray(segs), numel, SEGS64, 6, flags=flags, elem=elem)
        b = _lib.Plan(np.asarray(segs), numel, SEGS64, 6, flags=flags, elem=elem, out_elem=elem)
        assert a.info == b.info and b.out_elem == elem
        assert _lib.lib.fa_plan_elem(b.handle) == elem == _lib.lib.fa_plan_out_elem(b.handle)
        assert _lib.lib.fa_plan_out_elem(a.handle) == elem
        for n in (3, 129):
            for w in (False, True):
                assert a.launch_shape(n, w) == b.launch_shape(n, w)
                assert a.launch_form(n, w) == b.launch_form(n, w)
    # a mixed plan answers as the 16-bit plan of its clients
    for dtype in TDT:
        m = mixed_plan(dtype, segs, numel, flags, SEGS64, 6)
        p = pure_plan(dtype, segs, numel, flags, SEGS64, 6)
        assert m.info == p.info
        host = _lib.build_tiles_host(np.asarray(segs), numel, SEGS64, 6, flags=flags,
                                     elem=ELEM[dtype])
        assert host[0] == m.info
        for n in (3, 129, 257):
            assert m.launch_shape(n) == p.launch_shape(n)
            assert m.launch_form(n, True) == p.launch_form(n, True)


@pytest.mark.parametrize("dtype", sorted(TDT))
def test_refusals_change_no_byte(dtype):
    L = _lib.lib
    n = 3
    cases = [seg_list("gaps", 2),                          # gaps are not padding
             ([(0, 64), (64 + 128, 64)], 320, PAD),        # a gap of 128: room for a foreign key
             ([(0, 64)], 64 + 128, PAD)]                   # ... trailing
    for segs, numel, flags in cases:
        bits = bits_of16(make_inputs(dtype, n, "realistic", numel, 5))
        b = Bufs(dtype, bits, make_i64(n, 6, 5).numpy(), numel)
        pl = mixed_plan(dtype, segs, numel, flags, SEGS64, 6)
        before = b.snapshot()
        for fl in (_lib.FA_F_BCAST, _lib.FA_F_BCAST_ONLY):
            assert b.call(pl, fl) == _lib.FA_E_INVAL
            assert b"coverage" in L.fa_last_error()
        assert b.call(pl, _lib.FA_F_SUM_ONLY) == _lib.FA_E_INVAL
        assert b"SUM_ONLY" in L.fa_last_error()
        assert b.call(pl, 8) == _lib.FA_E_INVAL
        ch = _lib.FaChain(0, n, None, None, (numel + 3) // 4 * 4)
        assert L.fa_reduce_chain(pl.handle, b.a16, n, None, ctypes.byref(ch), b.p32, 0,
                                 None) == _lib.FA_E_INVAL
        assert b"16-bit" in L.fa_last_error()
        # an fp32 result bucket that is not 16-B aligned
        w = None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.fa_reduce(pl.handle, b.a16, b.a64, n, w, b.p32 + 4, b.p64, 0,
                           st) == _lib.FA_E_ALIGN
        torch.cuda.synchronize()
        for t, t0 in zip(b.snapshot(), before):
            assert torch.equal(t, t0), (segs, "a refused call wrote")


# ------------------------------------------- the broadcast's rounding ----
def rounding_values(dtype):
    """fp32 bit patterns around every rounding decision of fp32 -> dtype."""
    top = R.FORMAT[dtype][3]
    h = np.arange(0, top, dtype=np.uint16)
    a, b = R.widen(h, dtype), R.widen(h + np.uint16(1), dtype)
    mid = ((a + b) / 2).astype(np.float32)               # one more bit: exact in fp32
    assert np.array_equal(mid.astype(np.float64), (a + b) / 2)
    pos = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)),
                          np.nextafter(mid, np.float32(-np.inf)), a.astype(np.float32)])
    main = np.concatenate([pos, -pos]).view(np.uint32)
    tb = R.widen(np.array([top], np.uint16), dtype).astype(np.float32)    # largest finite
    step = tb - R.widen(np.array([top - 1], np.uint16), dtype).astype(np.float32)
    thr = (tb.astype(np.float64) + step.astype(np.float64) / 2).astype(np.float32)  # overflows
    edge = np.concatenate([tb, thr, np.nextafter(thr, np.float32(0)),
                           np.nextafter(thr, np.float32(np.inf)),
                           np.array([np.finfo(np.float32).max], np.float32)])
    # half the smallest 16-bit subnormal (a tie with zero) and its neighbours,
    # fp32's own subnormals, the smallest normals
    tiny = R.widen(np.array([1], np.uint16), dtype).astype(np.float32)
    half = (tiny.astype(np.float64) / 2).astype(np.float32)
    small = np.concatenate([half, np.nextafter(half, np.float32(1)),
                            np.nextafter(half, np.float32(0)), tiny,
                            np.array([1, 2, 0x7fffff, 0x800000], np.uint32).view(np.float32)])
    fin = np.concatenate([edge, small])
    special = np.concatenate([
        np.concatenate([fin, -fin]).view(np.uint32),
        np.array([0, 0x80000000, 0x7f800000, 0xff800000,          # +-0, +-inf
                  0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001,  # quiet / signalling NaNs
                  0x7fffffff, 0x7f80ffff, 0x7fbfffff, 0x7f810000], np.uint32)])
    return main, special


@pytest.mark.parametrize("n", [3, 25])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_narrowing_broadcast_rounds_as_torch_rounds(dtype, n):
    """FA_F_BCAST_ONLY from a constructed fp32 bucket: for every finite
    magnitude h and its successor, both signs, the fp32 midpoint, the
    midpoint +- one fp32 ulp and h itself; the overflow threshold, results in
    the 16-bit subnormals, +-0, +-inf and NaNs — in whole parts (the
    specials lead), in the ragged last part and in the mod-8 tail (they trail
    too)."""
    main, special = rounding_values(dtype)
    vals = np.concatenate([special, np.roll(main, 1031 * n), special])
    numel = vals.size - (vals.size - 5) % 8                # f32_numel % 8 == 5
    vals = np.concatenate([vals[:numel - special.size], special])
    assert vals.size == numel and numel % 8 == 5 and numel % 2048 > special.size + 8
    assert numel // 2048 > 100
    b = Bufs(dtype, np.full((n, numel), 0x1234, np.uint16), np.zeros((n, 0), np.int64), numel)
    b.o32[GUARD:GUARD + numel] = torch.from_numpy(vals.view(np.int32).copy()).cuda()
    pl = mixed_plan(dtype, [(0, numel)], numel, PAD)
    assert b.call(pl, _lib.FA_F_BCAST_ONLY) == _lib.FA_OK, _lib.lib.fa_last_error()
    assert np.array_equal(b.out_bits(), vals), "the broadcast wrote its source"
    wb, wn = to16(vals, dtype)
    assert wn.sum() == 16 and (wb[~wn] == R.FORMAT[dtype][2]).sum() > 4    # NaNs, +inf results
    assert_narrowed(b.client_bits(), vals, dtype, (dtype, n))
    b.assert_guards((dtype, n))


# ------------------------------------------------ wide store, exact sums ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [3, 9, 17, 128, 129, 257])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_wide_store_of_exact_sums(dtype, n, weighted):
    """k * 2^e data (and dyadic weights): every fp32 product and partial sum
    is exact, so the fp32 result is the float64 sum divided once and rounded
    once to fp32 whatever the order.  (The float64 quotient rounded again to
    fp32 equals the correctly rounded fp32 quotient: 53 >= 2 * 24 + 2.)"""
    ncols = sum(m for _, m in SEGS)
    cols, w = R.exact_sum_data(dtype, n, ncols, 11 * n + weighted, weighted)
    x = R.widen(cols, dtype)
    if weighted:
        want = (x * np.asarray(w, np.float32).astype(np.float64)[:, None]).sum(0) + 0.0
    else:
        want = (x.sum(0) + 0.0) / n
    assert np.isfinite(want).all()
    want32 = want.astype(np.float32)
    bits = place(cols, SEGS, NUMEL, fill=0x7e01)
    b = Bufs(dtype, bits, np.zeros((n, 0), np.int64), NUMEL)
    pl = mixed_plan(dtype, SEGS, NUMEL, 0)
    assert b.call(pl, 0, w) == _lib.FA_OK, _lib.lib.fa_last_error()
    out = b.out_bits()
    assert_f32_bits(gather(out, SEGS), want32, (dtype, n, weighted))
    inside = np.zeros(NUMEL, bool)
    for o, m in SEGS:
        inside[o:o + m] = True
    assert (out[~inside] == G32).all(), "wrote outside the segments"
    b.assert_guards((dtype, n, weighted))
