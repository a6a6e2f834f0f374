"""The small kernels of the C ABI that no other test calls, bit for bit
against plain numpy: fa_div_f32 / fa_div_trunc_i64 (the /N finish of every
multi-GPU round), fa_copy_f32 (its copy step and the roofline's copy
calibration) and the two probes bench.py takes its read and write ceilings
from — a probe that skips a part, or writes fewer destinations than it
claims, raises the ceiling the headline is reported against.  Guard bands
around every buffer a kernel writes."""
import ctypes

import numpy as np
import pytest
import torch

from feddct_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on each side of every buffer
G32 = 0xdeadbeef
G64 = -0x0123456789abcdef
L = _lib.lib


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """``rows`` device buffers of ``numel`` 4- or 8-byte elements, each
    between two guard bands (every row 16-B aligned); contents as raw
    uint32 / int64 patterns."""

    def __init__(self, numel, content=None, rows=1, i64=False):
        self.numel, self.rows, self.i64 = numel, rows, i64
        self.g = G64 if i64 else G32
        self.dt = np.int64 if i64 else np.uint32
        self.row = (numel + 3) // 4 * 4 + 2 * GUARD
        h = np.full((rows, self.row), self.g, self.dt)
        if content is not None:
            h[:, GUARD:GUARD + numel] = np.asarray(content).view(self.dt) if not i64 else content
        self.t = torch.from_numpy(h.view(np.int64 if i64 else np.int32)).cuda()
        self.size = 8 if i64 else 4

    def ptr(self, r=0):
        return self.t.data_ptr() + self.size * (self.row * r + GUARD)

    def host(self):
        return self.t.cpu().numpy().view(self.dt)

    def body(self):
        h = self.host()[:, GUARD:GUARD + self.numel]
        return h[0] if self.rows == 1 else h

    def assert_guards(self, what):
        h = self.host()
        assert (h[:, :GUARD] == self.g).all() and (h[:, GUARD + self.numel:] == self.g).all(), \
            (what, "guard band written")

    def assert_unwritten(self, what):
        assert (self.host() == self.g).all(), (what, "written")


def f32_bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def assert_f32(got_bits, want, what):
    """uint32 patterns against float32 values; a NaN only has to be a NaN."""
    g = got_bits.view(np.float32)
    gn, wn = np.isnan(g), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions")
    wb = f32_bits(want)
    bad = np.nonzero((got_bits != wb) & ~wn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got_bits[bad[:5]], wb[bad[:5]])


# ------------------------------------------------------------- division ----
DIVISORS = [2, 3, 7, 20, 24, 65536, 0.1]
DIV_NUMELS = [1, 255, 256, 257, 4096 * 256 + 257]   # the last: one past grid_for's cap
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 1e-38, -1e-38, 2e-45, -2e-45,
                    1e-45, 1.1754944e-38, 1.1754942e-38, 5.877472e-39, 1.0, -1.0, 3.0, 7.0, 1 / 3,
                    16777216.0, 16777217.0, 0.1, 65536.0, 1e-30, 3.4028235e38], np.float32)


def div_inputs(numel, seed):
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):     # both ends of fp32: some round to 0, some to inf
        x = (rng.standard_normal(numel) * 10.0 ** rng.integers(-44, 38, numel)).astype(np.float32)
    sub = rng.integers(1, 1 << 23, numel).astype(np.uint32).view(np.float32)   # subnormals
    x = np.where(rng.random(numel) < 0.1, sub, x)
    k = min(numel, SPECIAL.size)
    x[:k] = np.roll(SPECIAL, -(seed % SPECIAL.size))[:k]
    x[numel - k:] = np.roll(SPECIAL, seed % SPECIAL.size)[:k]      # in the last trip too
    return x


@pytest.mark.parametrize("d", DIVISORS)
def test_div_f32_is_ieee_division(d):
    """x / d rounded to nearest with subnormal quotients kept (1e-38 / 3,
    2e-45 / 3): a reciprocal multiply or a flush-to-zero build differs."""
    d32 = np.float32(d)
    for j, numel in enumerate(DIV_NUMELS):
        x = div_inputs(numel, 7 * j + DIVISORS.index(d))
        with np.errstate(all="ignore"):
            want = x / d32
        assert want.dtype == np.float32
        if numel >= 255 and d32 > 1:
            q = want[np.isfinite(want) & (want != 0)]
            assert (np.abs(q) < np.float32(1.1754944e-38)).any(), "no subnormal quotient"
        src = Guarded(numel, x)
        out = Guarded(numel)
        assert L.fa_div_f32(src.ptr(), float(d32), out.ptr(), numel, stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        assert_f32(out.body(), want, (d, numel, "out of place"))
        out.assert_guards((d, numel))
        assert np.array_equal(src.body(), f32_bits(x)), "the source was written"
        assert L.fa_div_f32(src.ptr(), float(d32), src.ptr(), numel, stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        assert_f32(src.body(), want, (d, numel, "in place"))
        src.assert_guards((d, numel, "in place"))


def test_div_f32_reciprocal_would_differ():
    """The inputs do tell x / 3 from x * (1 / 3)."""
    x = div_inputs(257, 1)
    with np.errstate(all="ignore"):
        a, b = x / np.float32(3), x * (np.float32(1) / np.float32(3))
    fin = np.isfinite(a)
    assert (f32_bits(a[fin]) != f32_bits(b[fin])).any()


TRUNC_EXTRA = np.array([-7.9, 7.9, -0.5, 0.5, -0.99999994, 2.0 ** 62, -2.0 ** 62, -2.0 ** 63,
                        2.0 ** 63 - 2.0 ** 39, 2.0 ** 31, -2.0 ** 31 - 256, 2.0 ** 32, 2.0 ** 53,
                        8388607.5, -8388607.5], np.float32)


@pytest.mark.parametrize("d", DIVISORS + [1])
def test_div_trunc_i64_truncates_toward_zero(d):
    """trunc(x / d) for every quotient inside int64 (the result outside is
    unspecified, include/fedagg.h): negative fractions toward zero, +-2^62,
    and at d = 1 the edges -2^63 and 2^63 - 2^39."""
    d32 = np.float32(d)
    assert float(TRUNC_EXTRA[8]) == 2.0 ** 63 - 2.0 ** 39
    for j, numel in enumerate(DIV_NUMELS):
        x = div_inputs(numel, 11 * j + 3)
        x[SPECIAL.size:][:TRUNC_EXTRA.size] = TRUNC_EXTRA[:max(0, numel - SPECIAL.size)]
        with np.errstate(all="ignore"):
            q = x / d32
        inside = np.isfinite(q) & (q >= np.float32(-2.0 ** 63)) & (q < np.float32(2.0 ** 63))
        x = np.where(inside, x, np.float32(-7.9))
        if numel == 1:
            x[0] = np.float32(-7.9)
        with np.errstate(all="ignore"):
            q = x / d32
        want = np.trunc(q).astype(np.int64)
        if d == 1 and numel >= 255:
            assert {-2 ** 63, 2 ** 63 - 2 ** 39, -7, 0, 2 ** 62} <= set(want.tolist())
        src = Guarded(numel, x)
        out = Guarded(numel, i64=True)
        assert L.fa_div_trunc_i64(src.ptr(), float(d32), out.ptr(), numel,
                                  stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        got = out.body()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (d, numel, bad[:5], got[bad[:5]], want[bad[:5]], x[bad[:5]])
        out.assert_guards((d, numel))
        assert np.array_equal(src.body(), f32_bits(x)), "the source was written"


# ----------------------------------------------------------------- copy ----
def finite_bits(numel, seed):
    """Random 32-bit patterns, none of them a NaN or an infinity."""
    b = np.random.default_rng(seed).integers(0, 1 << 32, numel, dtype=np.uint64).astype(np.uint32)
    b[(b & 0x7f800000) == 0x7f800000] ^= np.uint32(0x00800000)
    return b


@pytest.mark.parametrize("numel", [1, 2, 3, 4, 5, 1023, 1024, 1027, 4099])
def test_copy_f32_copies_every_element(numel):
    bits = finite_bits(numel, numel)
    src, dst = Guarded(numel, bits), Guarded(numel)
    assert L.fa_copy_f32(src.ptr(), dst.ptr(), numel, stream()) == _lib.FA_OK
    torch.cuda.synchronize()
    assert np.array_equal(dst.body(), bits)
    dst.assert_guards(numel)
    assert np.array_equal(src.body(), bits)
    src.assert_guards(numel)


def test_copy_f32_refuses_misaligned_pointers():
    numel = 1027
    src, dst = Guarded(numel + 4, finite_bits(numel + 4, 1)), Guarded(numel + 4)
    before = src.host().copy()
    for ds, dd in ((4, 0), (0, 4), (8, 8), (0, 12)):
        assert L.fa_copy_f32(src.ptr() + ds, dst.ptr() + dd, numel, stream()) == _lib.FA_E_ALIGN
        assert b"unaligned" in L.fa_last_error()
    torch.cuda.synchronize()
    dst.assert_unwritten("misaligned copy")
    assert np.array_equal(src.host(), before)


# ---------------------------------------------------------- write probe ----
def probe_val(i):
    """write_probe_kernel's value for 32-bit index i, restated: an integer
    hash, its top 24 bits made odd, centred and scaled by 2^-23 — odd, so
    never zero, and exact in fp32."""
    i = np.asarray(i, np.uint64) & 0xffffffff
    i ^= i >> 16
    i = (i * 0x7feb352d) & 0xffffffff
    i ^= i >> 15
    i = (i * 0x846ca68b) & 0xffffffff
    i ^= i >> 16
    v = ((i >> 8) | 1).astype(np.int64) - (1 << 23)
    out = (v.astype(np.float64) / 2.0 ** 23).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * 2.0 ** 23, v.astype(np.float64))   # exact
    return out


def probe_expected(numel, seed):
    """Element e of a destination: index ((4 (e // 4)) ^ seed) + e % 4."""
    e = np.arange(numel - numel % 4, dtype=np.uint64)
    return probe_val((((e // 4 * 4) ^ np.uint64(seed)) + e % 4) & 0xffffffff)


@pytest.mark.parametrize("seed", [0, 0x9e3779b9])
@pytest.mark.parametrize("n", [1, 24, 25, 256])       # one, one, two and many groups
def test_write_probe_writes_every_destination(n, seed):
    for numel in (4, 1023, 1024, 4099):
        want = probe_expected(numel, seed)
        assert (want != 0).all() and np.unique(want).size > want.size // 2
        dst = Guarded(numel, rows=n)
        arr = _lib.ptr_array([dst.ptr(r) for r in range(n)])
        assert L.fa_write_probe_f32(arr, n, numel, seed, stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        body = dst.body().reshape(n, numel)
        nw = numel - numel % 4
        for r in range(n):
            assert np.array_equal(body[r, :nw], f32_bits(want)), (n, numel, seed, r)
        assert (body[:, nw:] == G32).all(), "the last numel % 4 elements were written"
        dst.assert_guards((n, numel, seed))


def test_write_probe_edges():
    dst = Guarded(8, rows=257)
    arr = _lib.ptr_array([dst.ptr(r) for r in range(257)])
    for numel in (0, 1, 3):
        assert L.fa_write_probe_f32(arr, 3, numel, 5, stream()) == _lib.FA_OK
    assert L.fa_write_probe_f32(arr, 257, 8, 5, stream()) == _lib.FA_E_RANGE
    assert L.fa_write_probe_f32(arr, 0, 8, 5, stream()) == _lib.FA_OK
    torch.cuda.synchronize()
    dst.assert_unwritten("numel < 4, n == 0 and n == 257")


# ----------------------------------------------------------- read probe ----
@pytest.mark.parametrize("numel", [4, 1024 * 4 + 3, 300000])
@pytest.mark.parametrize("grid", [1, 3, 64])
def test_read_probe_grid_sums_every_float4_once(grid, numel):
    """Integers in [-8, 8]: every partial sum is exact in fp32 whatever order
    the atomics land in.  Block b owns the float4s v with (v // 256) % grid
    == b (256 lanes, stride grid * 256); the last numel % 4 floats belong to
    nobody."""
    rng = np.random.default_rng(grid * 1000003 + numel)
    x = rng.integers(-8, 9, numel).astype(np.float32)
    nv = numel // 4
    x[4 * nv:] = 1000.0
    owner = (np.arange(nv) // 256) % grid
    per_v = x[:4 * nv].astype(np.float64).reshape(nv, 4).sum(1)
    want = np.array([per_v[owner == b].sum() for b in range(grid)])
    assert np.abs(want).max() < 2 ** 24 and want.sum() == x[:4 * nv].astype(np.float64).sum()
    src = Guarded(numel, x)
    out = Guarded(grid, np.zeros(grid, np.float32))
    for rep in (1, 2):          # a second call accumulates
        assert L.fa_read_probe_f32(src.ptr(), numel, out.ptr(), grid, stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        got = out.body().view(np.float32).astype(np.float64)
        assert np.array_equal(got, rep * want), (grid, numel, rep, got, want)
        assert got.sum() == rep * x[:4 * nv].astype(np.float64).sum()
        out.assert_guards((grid, numel))
    assert np.array_equal(src.body(), f32_bits(x))


def test_read_probe_tiles_read_every_part():
    """grid == 0 stores only when a tile's lane sum is the sentinel
    (1234.5, -1, 7, w): planted at float4 j of a zero source it must come
    back as out[j % 256] = w, for the first and last lanes of both halves of
    a tile, the next tile and the last float4 of a ragged last tile."""
    nv = 2 * 512 + 300
    numel = 4 * nv + 3
    marker = np.float32(-55.25)
    for j in (0, 255, 256, 511, 512, nv - 1):
        x = np.zeros(numel, np.float32)
        w = np.float32(100 + j)
        x[4 * j:4 * j + 4] = (1234.5, -1.0, 7.0, w)
        x[4 * nv:] = (1234.5, -1.0, 7.0)          # the unread tail
        src = Guarded(numel, x)
        out = Guarded(256, np.full(256, marker, np.float32))
        assert L.fa_read_probe_f32(src.ptr(), numel, out.ptr(), 0, stream()) == _lib.FA_OK
        torch.cuda.synchronize()
        want = np.full(256, marker, np.float32)
        want[j % 256] = w
        assert np.array_equal(out.body(), f32_bits(want)), (j, out.body().view(np.float32))
        out.assert_guards(j)
    # no sentinel anywhere: nothing is stored
    src = Guarded(numel, np.zeros(numel, np.float32))
    out = Guarded(256, np.full(256, marker, np.float32))
    assert L.fa_read_probe_f32(src.ptr(), numel, out.ptr(), 0, stream()) == _lib.FA_OK
    torch.cuda.synchronize()
    assert (out.body() == f32_bits(marker)).all()
