"""GPU: chain segments of the cascade over fp16 / bf16 buckets
(fa_reduce_chain_elem, csrc/fedagg_chain16.hip), one GPU, one process, the
current stream — tests/test_gpu_chain.py on 16-bit plans.

Client groups reduced by separate launches, each continuing the previous
group's fp32 state planes in slot order, give the bits of one 16-bit fa_reduce
over all clients and the oracle's (tests/round16.expected16: every value
widened to fp32, torch's CPU order, one division, one rounding to
nearest-even).  The vector tiles chain; the layout's scalar columns (tails,
M == 1, unaligned keys, int64) go through fa_reduce over all clients' raw
rows, as the multi-GPU round gathers them.

Every comparison is bit for bit (two NaNs equal); there is no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import h16ref
import round16 as R
from feddct_amd import _lib
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import layout_tiles
from oracle import torch_order as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = list(R.DTYPES)
G = 64                      # guard band, elements, on each side of every buffer
SENT16 = 0x5A3C             # the guards of 16-bit buffers (finite in both types)
FILL32 = 0x7FC0BEEF         # state planes and fp32 results before a call: a NaN
F32 = _lib.FA_ELEM_F32


@pytest.fixture(autouse=True)
def _entry():
    """A library without the entry fails here, at symbol lookup."""
    assert _lib.lib.fa_reduce_chain_elem
    torch.cuda.set_device(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- layouts --
# a full 2048-element tile, partial tiles, a 4096-element key, unaligned keys,
# a 0-d key, an int64 key
MAN_SHAPES = [2048, 100, 2048 + 8, 33, 4096, 7, 0, 64, 1]
# tests/test_gpu_chain.py's deep layout: ~2.3 k elements, so thousands of
# clients stay cheap
DEEP_SHAPES = [100, 2048 + 8, 33, 7, 0, 64, 1]


@functools.lru_cache(maxsize=None)
def layout(name, dtype):
    if name == "raw":
        return R.RawLayout(dtype)
    shapes = MAN_SHAPES if name == "man" else DEEP_SHAPES
    return BucketLayout([(f"k{j}", (m,) if m else (), dtype) for j, m in enumerate(shapes)]
                        + [("nbt", (), "int64")], native16=True)


@functools.lru_cache(maxsize=None)
def tiles_of(name, dtype):
    """(vector tiles, the rest, mask of the elements inside a vector tile)."""
    lay = layout(name, dtype)
    _, t = layout_tiles(lay)
    vec, rest = t[t[:, 2] == 0], t[t[:, 2] != 0]
    inv = np.zeros(lay.f32_numel, bool)
    for s, c, _ in vec:
        inv[s:s + c] = True
    assert len(vec) and len(rest) and (vec[:, 0] % 8 == 0).all() and (vec[:, 1] % 8 == 0).all()
    return vec, rest, inv


@functools.lru_cache(maxsize=None)
def plans(name, dtype, mixed=False):
    """(the chain plan: vector tiles; the tails' plan; the one-launch plan)."""
    lay = layout(name, dtype)
    vec, rest, _ = tiles_of(name, dtype)
    el = R.ELEM[dtype]
    oe = F32 if mixed else None
    return (_lib.Plan.from_tiles(vec, lay.f32_numel, 0, elem=el, out_elem=oe),
            _lib.Plan.from_tiles(rest, lay.f32_numel, lay.i64_numel, elem=el, out_elem=oe),
            _lib.Plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, elem=el, out_elem=oe))


# ---------------------------------------------------------------- buffers --
class Clients:
    """n clients carved from one slab, a guard band on each side of every row."""

    def __init__(self, lay, bits, i64=None):
        n, L = bits.shape
        assert L == lay.f32_numel
        self.n, self.L = n, L
        pitch = -(-(L + 2 * G) // 64) * 64
        self.host = np.full((n, pitch), SENT16, np.uint16)
        self.host[:, G:G + L] = bits
        self.dev = torch.from_numpy(self.host.view(np.int16).copy()).to(DEV)
        self.p16 = [self.dev.data_ptr() + 2 * (i * pitch + G) for i in range(n)]
        if i64 is None:
            i64 = np.zeros((n, max(1, lay.i64_numel)), np.int64)
        self.i64 = torch.from_numpy(np.ascontiguousarray(i64)).to(DEV)
        self.p64 = [self.i64[i].data_ptr() for i in range(n)]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint16), self.host)


class Out:
    """A result bucket between two guard bands: 16-bit (fill R.FILL16), or the
    mixed plan's fp32 one (fill FILL32)."""

    def __init__(self, L, wide=False):
        self.L, self.wide = L, wide
        Lp = -(-L // 8) * 8
        if wide:
            self.t = torch.full((2 * G + Lp,), FILL32, dtype=torch.int32, device=DEV)
        else:
            self.t = torch.full((2 * G + Lp,), SENT16, dtype=torch.int16, device=DEV)
            self.t[G:G + L] = np.array([R.FILL16], np.uint16).view(np.int16)[0].item()
        self.ptr = self.t.data_ptr() + (4 if wide else 2) * G
        self.start = self.t.cpu().numpy().copy()

    def raw(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint32 if self.wide else np.uint16)

    def value(self):
        return self.raw()[G:G + self.L].copy()

    def guards_ok(self):
        a, s = self.t.cpu().numpy(), self.start
        return np.array_equal(a[:G], s[:G]) and np.array_equal(a[G + self.L:], s[G + self.L:])

    def untouched(self):
        return np.array_equal(self.t.cpu().numpy(), self.start)


class State:
    """Four fp32 planes of pitch ``plane`` pre-filled with a NaN, 64 elements
    of the fill before the first and at least 128 behind each."""

    def __init__(self, L):
        self.L = L
        self.plane = -(-L // 4) * 4 + 2 * G
        self.t = torch.full((G + 4 * self.plane,), FILL32, dtype=torch.int32, device=DEV)
        self.ptr = self.t.data_ptr() + 4 * G

    def snap(self):
        return self.t.cpu().numpy().view(np.uint32).copy()

    def check_written(self, before, lev, inv, what):
        """Against the snapshot ``before``: the planes ``lev`` names hold values
        on the vector tiles' elements, and nothing else changed."""
        now = self.snap()
        keep = np.ones(now.size, bool)
        for l in range(4):
            if lev & (1 << l):
                lo = G + l * self.plane
                got = now[lo:lo + self.L]
                assert (got[inv] != FILL32).all(), (what, l, "a named plane was not stored")
                keep[lo:lo + self.L][inv] = False
        assert np.array_equal(now[keep], before[keep]), (what, "written outside the named planes")


def _cuts(rng, n, groups):
    if groups >= n:
        return list(range(n + 1))
    c = sorted(rng.choice(np.arange(1, n), size=groups - 1, replace=False).tolist())
    return [0] + c + [n]


def _floats(w):
    return None if w is None else (ctypes.c_float * len(w))(*map(float, w))


def chained(name, dtype, cl, bounds, weights=None, inplace=True, mixed=False, discipline=False):
    """Reduce the clients as the chained groups [bounds[g], bounds[g+1]), the
    scalar columns by one fa_reduce: (result bits [f32_numel], int64 result)."""
    lay = layout(name, dtype)
    vec, rest, _ = plans(name, dtype, mixed)
    inv = tiles_of(name, dtype)[2]
    n = cl.n
    out = Out(lay.f32_numel, wide=mixed)
    out64 = torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64, device=DEV)
    st = [State(lay.f32_numel) for _ in range(1 if inplace else 2)]
    w = None if weights is None else np.asarray(weights, np.float32)
    prev = None
    for g, (a, b) in enumerate(zip(bounds, bounds[1:])):
        last = b == n
        dst = None if last else st[g % len(st)]
        assert _lib.lib.fa_chain_levels(b, n) == O.chain_levels(b, n)
        ch = _lib.FaChain(a, n, prev.ptr if prev is not None else None,
                          dst.ptr if dst is not None else None, st[0].plane)
        before = [s.snap() for s in st] if discipline else None
        _lib.check(_lib.lib.fa_reduce_chain_elem(
            vec.handle, _lib.ptr_array(cl.p16[a:b]), b - a, _floats(None if w is None else w[a:b]),
            ctypes.byref(ch), out.ptr if last else None, 0, _stream()), "fa_reduce_chain_elem")
        if discipline:
            torch.cuda.synchronize()
            for s, bef in zip(st, before):
                lev = O.chain_levels(b, n) if s is dst else 0
                s.check_written(bef, lev, inv, (n, bounds, g))
            if not last:
                assert out.untouched(), (n, bounds, g, "a segment that does not finish wrote out")
        prev = dst
    _lib.check(_lib.lib.fa_reduce(rest.handle, _lib.ptr_array(cl.p16), _lib.ptr_array(cl.p64), n,
                                  _floats(w), out.ptr, out64.data_ptr(), 0, _stream()), "tails")
    torch.cuda.synchronize()
    assert out.guards_ok(), (n, bounds, "the result's guard bands")
    return out.value(), out64.cpu().numpy()[:lay.i64_numel]


def single(name, dtype, cl, weights=None, mixed=False):
    lay = layout(name, dtype)
    full = plans(name, dtype, mixed)[2]
    out = Out(lay.f32_numel, wide=mixed)
    out64 = torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib.fa_reduce(full.handle, _lib.ptr_array(cl.p16), _lib.ptr_array(cl.p64),
                                  cl.n, _floats(weights), out.ptr, out64.data_ptr(), 0, _stream()),
               "fa_reduce")
    torch.cuda.synchronize()
    return out.value(), out64.cpu().numpy()[:lay.i64_numel]


def expected(lay, dtype, bits, i64, weights=None):
    """tests/round16.expected16; weighted: narrow(weighted_sum0(widen(bits), w))
    per segment."""
    exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
    if weights is not None:
        with np.errstate(all="ignore"):
            for o, m in lay.segs32:
                o, m = int(o), int(m)
                exp[o:o + m] = R.narrow(O.weighted_sum0(R.widen(bits[:, o:o + m], dtype),
                                                        np.asarray(weights, np.float32)), dtype)
    return exp, inside, e64


def _inside(lay):
    """Mask of the elements inside a segment."""
    m = np.zeros(lay.f32_numel, bool)
    for o, k in lay.segs32:
        m[int(o):int(o) + int(k)] = True
    return m


def _i64(n, lay, seed):
    rng = np.random.default_rng([seed, 64])
    x = rng.integers(-(1 << 40), 1 << 40, (n, max(1, lay.i64_numel))).astype(np.int64)
    x[:, :1] = rng.integers(0, 1000, (n, 1))
    return x


_cache = {}


def case(name, dtype, n, weights=None):
    """Clients, the one launch's result and the oracle's, computed once per
    (layout, type, n, weighted) and left unchanged."""
    key = (name, dtype, n, weights is not None)
    if key not in _cache:
        lay = layout(name, dtype)
        # the deep layout: client i's row depends on i alone, every n a prefix
        if name == "deep":
            if ("deepbits", dtype) not in _cache:
                _cache["deepbits", dtype] = (R.cancelling_bits(dtype, 4097, lay.f32_numel, 7),
                                             _i64(4097, lay, 7))
            bits, i64 = (x[:n] for x in _cache["deepbits", dtype])
        else:
            bits, i64 = R.cancelling_bits(dtype, n, lay.f32_numel, 11), _i64(n, lay, 11)
        cl = Clients(lay, bits, i64)
        _cache[key] = (cl, single(name, dtype, cl, weights), expected(lay, dtype, bits, i64, weights))
    return _cache[key]


def _assert_same(dtype, got, one, exp, what):
    (g16, g64), (o16, o64), (e16, inside, e64) = got, one, exp
    assert R.same16(g16[inside], o16[inside], dtype), (what, "vs one launch")
    assert R.same16(g16[inside], e16[inside], dtype), (what, "vs the oracle")
    assert np.array_equal(g64, o64) and np.array_equal(g64, e64), (what, "int64")


# ----------------------------------------------------- chained == one launch --
@pytest.mark.parametrize("n", [2, 5, 16, 20, 33, 129, 257, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_equals_one_launch(dtype, n):
    """129: the first count past the inline pointer table (a first segment of
    129 rows reads the device table; the level step is n_total's)."""
    for name in ("raw", "man"):
        cl, one, exp = case(name, dtype, n)
        sets = [[0] + [b for b in (16, 32, 256) if b < n] + [n]]
        if n == 300:
            sets.append([0, 129, 300])          # 129 and 171 local rows of 300
        for groups in (2, 3, 8):
            sets.append(_cuts(np.random.default_rng(n * 10 + groups), n, groups))
        for k, bounds in enumerate(sets):
            for inplace in ((True, False) if k < 2 else (k % 2 == 0,)):
                got = chained(name, dtype, cl, bounds, inplace=inplace)
                _assert_same(dtype, got, one, exp, (name, n, bounds, inplace))
        assert cl.unchanged(), (name, n, "clients or their guard bands changed")


@pytest.mark.parametrize("n,bounds", [(20, [0, 7, 13, 20]), (300, [0, 16, 100, 256, 300]),
                                      (257, [0, 255, 256, 257])])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_state_discipline(dtype, inplace, n, bounds):
    """Planes pre-filled with a NaN: a segment stores the planes
    fa_chain_levels names, on the vector tiles' elements, and nothing else —
    not the other planes, not the bands around every plane, not ``out``
    before the last segment, not the clients."""
    for name in ("raw", "man"):
        cl, one, exp = case(name, dtype, n)
        got = chained(name, dtype, cl, bounds, inplace=inplace, discipline=True)
        _assert_same(dtype, got, one, exp, (name, n, bounds))
        assert cl.unchanged()


# --------------------------------------------------------------------- deep --
@pytest.mark.parametrize("n", [4096, 4097])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_deep_levels(dtype, n):
    """Cuts at row 4096 (plane 3 alone is live behind it) and one row either
    side, on ~2.3 k elements."""
    cl, one, exp = case("deep", dtype, n)
    sets = [b for b in ([0, 4096, n], [0, 4095, 4097, n], [0, 4095, 4096, 4097, n],
                        [0, 256, 4096 - 16, 4096 + 16, n])]
    sets = [sorted({x for x in b if x <= n}) for b in sets]
    if n > 4096:
        assert _lib.lib.fa_chain_levels(4096, n) == 8
    for k, bounds in enumerate(s for s in sets if len(s) > 2):
        got = chained("deep", dtype, cl, bounds, inplace=k % 2 == 0, discipline=k == 0)
        _assert_same(dtype, got, one, exp, (n, bounds))
    assert cl.unchanged()


# ----------------------------------------------------------------- weighted --
@pytest.mark.parametrize("name,n,bounds", [("raw", 20, [0, 7, 13, 20]), ("man", 20, [0, 7, 13, 20]),
                                           ("deep", 4097, [0, 4096, 4097])])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_weighted(dtype, name, n, bounds):
    """The chain multiplies each client by its weight inside the kernel: the
    weighted one launch's bits and the oracle's."""
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3)
    cl, one, exp = case(name, dtype, n, weights=w)
    got = chained(name, dtype, cl, bounds, weights=w)
    _assert_same(dtype, got, one, exp, (name, n, bounds, "weighted"))
    assert cl.unchanged()


# -------------------------------------------------------------------- mixed --
@pytest.mark.parametrize("n", [20, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_mixed_plan_gives_the_fp32_bits(dtype, n):
    """out_elem F32 over 16-bit clients: the last segment stores the unrounded
    fp32 mean — the mixed one launch's fp32 bits."""
    for name in ("raw", "man"):
        cl, _, _ = case(name, dtype, n)
        o32, o64 = single(name, dtype, cl, mixed=True)
        inside = _inside(layout(name, dtype))
        for bounds in ([0, n // 2, n], [0, 16, n - 1, n]):
            g32, g64 = chained(name, dtype, cl, bounds, mixed=True, inplace=False)
            a, b = g32[inside].view(np.float32), o32[inside].view(np.float32)
            assert ((g32[inside] == o32[inside]) | (np.isnan(a) & np.isnan(b))).all(), (name, bounds)
            assert (g32[inside] != FILL32).all() and np.array_equal(g64, o64)
        assert cl.unchanged()


# ----------------------------------------------------------- order-free pins --
@pytest.mark.parametrize("n", [3, 33, 257])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_exact_sum_data(dtype, n):
    """Rows whose fp32 sums are exact: the expected bits are a float64 sum, one
    division, one rounding (tests/h16ref.py: no oracle, no order)."""
    lay = layout("man", dtype)
    bits, _ = h16ref.exact_sum_data(dtype, n, lay.f32_numel, seed=100 + n)
    cl = Clients(lay, bits)
    got, _ = chained("man", dtype, cl, [0, n // 3, n - n // 3, n])
    for o, m in lay.segs32:
        o, m = int(o), int(m)
        pat, nan = h16ref.exact_mean(bits[:, o:o + m], dtype)
        assert not nan.any() and np.array_equal(got[o:o + m], pat), o


def _chain_layout(lay, dtype, bits, bounds):
    """Any 16-bit layout without int64 keys: its vector tiles chained over
    ``bounds``, its scalar columns through fa_reduce; the result bits."""
    _, t = layout_tiles(lay)
    vec, rest = t[t[:, 2] == 0], t[t[:, 2] != 0]
    el = R.ELEM[dtype]
    assert len(vec) and not lay.i64_numel
    pv = _lib.Plan.from_tiles(vec, lay.f32_numel, 0, elem=el)
    n = len(bits)
    cl = Clients(lay, bits)
    st, out = State(lay.f32_numel), Out(lay.f32_numel)
    for a, b in zip(bounds, bounds[1:]):
        ch = _lib.FaChain(a, n, st.ptr if a else None, st.ptr if b < n else None, st.plane)
        _lib.check(_lib.lib.fa_reduce_chain_elem(
            pv.handle, _lib.ptr_array(cl.p16[a:b]), b - a, None, ctypes.byref(ch),
            out.ptr if b == n else None, 0, _stream()), "fa_reduce_chain_elem")
    if len(rest):
        pr = _lib.Plan.from_tiles(rest, lay.f32_numel, 0, elem=el)
        _lib.check(_lib.lib.fa_reduce(pr.handle, _lib.ptr_array(cl.p16), None, n, None, out.ptr,
                                      None, 0, _stream()), "tails")
    torch.cuda.synchronize()
    assert out.guards_ok() and cl.unchanged()
    return out.value()


@pytest.mark.parametrize("n,bounds", [(2, [0, 1, 2]), (4, [0, 1, 4])])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_adjacent_pair_ties(dtype, n, bounds):
    """Every pair of neighbouring 16-bit values through a two-segment chain:
    the mean is an exact tie (n = 2) or a quarter off (n = 4), and the one
    rounding sends it to the even neighbour or the nearer one.  (The key's last
    columns are its ILP-4 tail: the chain covers all but at most 31 of them.)"""
    rows = h16ref.pair_rows(dtype, n)
    m = rows.shape[1]
    lay = BucketLayout([("t", (m,), dtype)], native16=True)
    full = np.zeros((n, lay.f32_numel), np.uint16)
    full[:, :m] = rows
    got = _chain_layout(lay, dtype, full, bounds)
    pat, nan = h16ref.exact_mean(rows, dtype)
    assert not nan.any() and np.array_equal(got[:m], pat)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_special_values_in_every_row_position(dtype):
    """tests/specials.py's columns (-0, subnormals, inf, NaN, overflowing sums,
    inf - inf) cast to 16 bits, the rows rotated so that every special value
    meets every row position of a three-segment chain."""
    import specials
    n = 6
    lay = R.SpecialLayout(dtype)
    with np.errstate(all="ignore"):
        base = R.narrow(specials.fill(n, seed=3), dtype)
    for shift in range(n):
        bits = np.roll(base, shift, axis=0)
        got = _chain_layout(lay, dtype, bits, [0, 1, 4, 6])
        exp, inside, _ = R.expected16(lay, dtype, bits)
        assert R.same16(got[inside], exp[inside], dtype), shift


# ---------------------------------------------------------------- fp32 plan --
FP32_MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                     for j, m in enumerate([100, 4096, 33, 2048 + 8, 7, 0, 5000, 64, 1])]}


def _fp32_plans():
    lay = BucketLayout.from_manifest(FP32_MAN)
    _, t = layout_tiles(lay)
    vec = t[t[:, 2] == 0]
    return lay, _lib.Plan(None, lay.f32_numel, None, 0, 0, tiles=vec), \
        _lib.Plan(lay.segs32, lay.f32_numel, (), 0)


def test_chain16_fp32_plan_is_fa_reduce_chain():
    """An fp32 plan through the _elem entry: fa_reduce_chain's bits."""
    lay, vec, _ = _fp32_plans()
    n, bounds, P = 20, [0, 7, 13, 20], lay.f32_numel
    rng = np.random.default_rng(5)
    x = torch.from_numpy(np.ldexp(rng.uniform(-2, 2, (n, P)), rng.integers(-12, 12, (n, P)))
                         .astype(np.float32)).to(DEV)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3)
    for weights in (None, w):
        outs = []
        for fn in (_lib.lib.fa_reduce_chain, _lib.lib.fa_reduce_chain_elem):
            out = torch.full((P,), np.nan, device=DEV)
            st = torch.full((4 * P,), np.nan, device=DEV)
            for a, b in zip(bounds, bounds[1:]):
                ch = _lib.FaChain(a, n, st.data_ptr() if a else None,
                                  st.data_ptr() if b < n else None, P)
                _lib.check(fn(vec.handle, _lib.ptr_array([x[i].data_ptr() for i in range(a, b)]),
                              b - a, _floats(None if weights is None else weights[a:b]),
                              ctypes.byref(ch), out.data_ptr() if b == n else None, 0, _stream()))
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy().view(np.uint32))
        assert np.array_equal(outs[0], outs[1])


def test_chain16_fp32_plan_errors_are_fa_reduce_chains():
    """The same codes and the same messages, under fa_reduce_chain's name."""
    lay, vec, full = _fp32_plans()
    P = lay.f32_numel
    b = torch.zeros(4 * P, device=DEV)
    ptrs = _lib.ptr_array([b.data_ptr()] * 4)
    L = _lib.lib
    bp = b.data_ptr()
    cases = [(full, 2, _lib.FaChain(0, 4, None, bp, P), bp, 0),
             (vec, 2, _lib.FaChain(2, 4, None, None, P), bp, 0),
             (vec, 2, _lib.FaChain(0, 4, None, None, P), bp, 0),
             (vec, 3, _lib.FaChain(2, 4, bp, None, P), bp, 0),
             (vec, 2, _lib.FaChain(0, 4, None, bp, 10), bp, 0),
             (vec, 1, _lib.FaChain(0, _lib.FA_MAX_CLIENTS + 1, None, bp, P), bp, 0),
             (vec, 2, _lib.FaChain(0, 4, None, bp + 4, P), bp, 0),
             (vec, 2, _lib.FaChain(0, 4, None, bp, P), bp, 8),
             (None, 2, _lib.FaChain(0, 4, None, bp, P), bp, 0)]
    for plan, n, ch, out, flags in cases:
        h = plan.handle if plan is not None else None
        got = []
        for fn in (L.fa_reduce_chain, L.fa_reduce_chain_elem):
            rc = fn(h, ptrs, n, None, ctypes.byref(ch), out, flags, None)
            got.append((rc, L.fa_last_error()))
        assert got[0] == got[1] and got[0][0] < 0, got
        assert got[0][1].startswith(b"fa_reduce_chain:"), got
    torch.cuda.synchronize()
    assert float(b.abs().sum()) == 0.0


# ------------------------------------------------------------------- errors --
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain16_refusals_write_nothing(dtype):
    lay = layout("man", dtype)
    vec, rest, full = plans("man", dtype)
    mixed = plans("man", dtype, True)[0]
    tg = _lib.Plan.for_order(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n=4,
                             elem=R.ELEM[dtype])
    n = 4
    cl = Clients(lay, R.cancelling_bits(dtype, n, lay.f32_numel, 3))
    st, out, o32 = State(lay.f32_numel), Out(lay.f32_numel), Out(lay.f32_numel, wide=True)
    st0 = st.snap()
    L, P = _lib.lib, st.plane
    INV, ALIGN = _lib.FA_E_INVAL, _lib.FA_E_ALIGN

    def call(plan, ptrs, k, ch, o=out.ptr, flags=0):
        rc = L.fa_reduce_chain_elem(plan.handle, _lib.ptr_array(ptrs), k, None, ctypes.byref(ch),
                                    o, flags, _stream())
        msg = L.fa_last_error()
        assert rc == 0 or msg.startswith(b"fa_reduce_chain_elem:"), msg
        return rc, msg

    first = lambda: _lib.FaChain(0, n, None, st.ptr, P)
    lastc = lambda: _lib.FaChain(2, n, st.ptr, None, P)
    p = cl.p16
    rc, msg = call(tg, p[:2], 2, first())
    assert rc == INV and b"torch-GPU-order" in msg
    for plan in (full, rest):
        rc, msg = call(plan, p[:2], 2, first())
        assert rc == INV and b"scalar tiles" in msg
    rc, msg = call(vec, p[2:], 2, lastc(), flags=_lib.FA_F_SUM_ONLY)
    assert rc == INV and b"SUM_ONLY" in msg and b"16-bit" in msg
    assert call(vec, p[:2], 2, _lib.FaChain(0, n, None, st.ptr + 4, P))[0] == ALIGN
    assert call(vec, p[2:], 2, _lib.FaChain(2, n, st.ptr + 8, None, P))[0] == ALIGN
    assert call(vec, p[2:], 2, lastc(), o=out.ptr + 2)[0] == ALIGN
    assert call(mixed, p[2:], 2, lastc(), o=o32.ptr + 4)[0] == ALIGN
    assert call(vec, [p[0], None], 2, first())[0] == ALIGN
    assert call(vec, [p[0], p[1] + 2], 2, first())[0] == ALIGN
    assert call(vec, [p[0] + 8, p[1]], 2, first())[0] == ALIGN
    assert call(vec, p[:2], 2, _lib.FaChain(0, n, None, st.ptr, lay.f32_numel - 4))[0] == INV
    assert call(vec, p[:2], 2, _lib.FaChain(0, n, None, st.ptr, P + 2))[0] == INV
    assert call(vec, p[2:], 2, _lib.FaChain(2, n, None, None, P))[0] == INV   # state_in missing
    assert call(vec, p[:2], 2, _lib.FaChain(0, n, None, None, P))[0] == INV   # finish too early
    assert call(vec, p[:3], 3, _lib.FaChain(2, n, st.ptr, None, P))[0] == INV  # past n_total
    assert call(vec, p[:2], 2, first(), flags=1)[0] == INV                     # FA_F_BCAST
    torch.cuda.synchronize()
    assert np.array_equal(st.snap(), st0) and out.untouched() and o32.untouched()
    assert cl.unchanged()
    # fa_reduce_chain itself still refuses the 16-bit plan
    rc = L.fa_reduce_chain(vec.handle, _lib.ptr_array(p[:2]), 2, None, ctypes.byref(first()),
                           None, 0, _stream())
    assert rc == INV and b"16-bit plan" in L.fa_last_error()
    # and the calls the refusals were cut from go through
    assert call(vec, p[:2], 2, first(), o=None)[0] == 0
    assert call(vec, p[2:], 2, lastc())[0] == 0
    assert call(mixed, p[2:], 2, lastc(), o=o32.ptr, flags=_lib.FA_F_SUM_ONLY)[0] == 0
    torch.cuda.synchronize()
    assert not out.untouched() and out.guards_ok() and o32.guards_ok()
