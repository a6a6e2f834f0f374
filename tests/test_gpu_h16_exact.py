"""The 16-bit reduce kernels (csrc/fedagg_h16.hip) through the C ABI against
tests/h16ref.py only — expected bits that no summation order enters
(exhaustive neighbouring values, the identity at N = 1, exact-sum data) and
an order-independent error bound on arbitrary data.  The oracle is not
imported here: these tests stand if the cascade is ever re-tuned, and they do
not share its arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import h16ref as R
from feddct_amd import _lib
from test_gpu_h16_kernel import make_inputs

pytestmark = pytest.mark.gpu

ELEM = {"float16": _lib.FA_ELEM_F16, "bfloat16": _lib.FA_ELEM_BF16}
TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
OUT_PAT = 0xabcd


def reduce_bits(dtype, bits, segs, numel, tile=0, weights=None, plan_flags=0):
    """fa_reduce over client rows ``bits[n, numel]`` (uint16) on a raw plan
    of floating segments only; returns the result bucket's bits, gaps still
    holding OUT_PAT."""
    n = bits.shape[0]
    assert bits.shape[1] == numel
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    row = (numel + 7) // 8 * 8               # every client bucket 16-B aligned
    host = np.zeros((n, row), np.uint16)
    host[:, :numel] = bits
    x = torch.from_numpy(host.view(np.int16)).to(dev)
    out = torch.from_numpy(np.full(row, OUT_PAT, np.uint16).view(np.int16).copy()).to(dev)
    plan = _lib.Plan(np.asarray(segs, np.int64).reshape(-1, 2), numel, tile_elems=tile,
                     flags=plan_flags, elem=ELEM[dtype])
    if tile:
        assert plan.info["tile_elems"] == tile
    w = None if weights is None else (ctypes.c_float * n)(*[float(v) for v in weights])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = _lib.ptr_array([x.data_ptr() + 2 * row * i for i in range(n)])
    _lib.check(_lib.lib.fa_reduce(plan.handle, ptrs, None, n, w, out.data_ptr(), None, 0, st),
               "fa_reduce")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)[:numel]


def is_nan_bits(b, dtype):
    return np.isnan(R.widen(b, dtype))


def assert_bits(got, want, what):
    """got: uint16; want: (bits, is-NaN) of h16ref."""
    wb, wn = want
    gn = is_nan_bits(got, what[0])
    assert np.array_equal(gn, wn), (what, "NaN positions", np.nonzero(gn != wn)[0][:5])
    bad = np.nonzero((got != wb) & ~wn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], wb[bad[:5]])


def place(cols, segs, numel, fill=0):
    """Rows ``cols[n, m]`` laid into the segments in order: bits[n, numel]."""
    out = np.full((cols.shape[0], numel), fill, np.uint16)
    c = 0
    for o, m in segs:
        out[:, o:o + m] = cols[:, c:c + m]
        c += m
    assert c == cols.shape[1]
    return out


def gather(res, segs):
    return np.concatenate([res[o:o + m] for o, m in segs])


# ------------------------------------------------------ exhaustive rounding ----
def scalar_slice(dtype):
    """Indices into the adjacent-pair columns: every 8th magnitude, and all
    magnitudes within 16 of a binade boundary (the subnormal boundary is the
    first of them) and of the top of the format."""
    p, _, _, top = R.FORMAT[dtype]
    ncol = top                                   # magnitudes 0 .. top - 1
    keep = np.zeros(ncol, bool)
    keep[::8] = True
    for edge in list(range(1 << (p - 1), top, 1 << (p - 1))) + [top]:
        keep[max(0, edge - 16):min(ncol, edge + 17)] = True
    return np.nonzero(keep)[0]


def scalar_layout(ncols):
    """Keys of 1, 3 and 7 elements back to back (inner, ILP-4, and the
    4-column cascade body that a 16-bit plan keeps scalar), then one long key
    at an odd offset (scalar cascade body, ILP-4 tail)."""
    segs, off, left = [], 0, ncols
    small = ncols // 2
    j = 0
    while ncols - left < small:
        m = (1, 3, 7)[j % 3]
        segs.append((off, m))
        off, left, j = off + m, left - m, j + 1
    off += 1 - off % 2                           # an odd offset
    segs.append((off, left))
    return segs, off + left + 3


@pytest.mark.parametrize("layout", ["long", "scalar"])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("tile", [2048, 4096])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_adjacent_pair_rounds_to_nearest_even(dtype, tile, n, layout):
    """(h, h+1): an exact tie; (h, h, h, h+1) and (h, h+1, h+1, h+1): a
    quarter and three quarters — for every finite magnitude h of the format
    and both signs, through the vector tiles' narrow2 (one long key) and
    through the scalar columns' narrow (short keys and an odd offset)."""
    rows = np.concatenate([R.pair_rows(dtype, n, 0), R.pair_rows(dtype, n, 1)], 1)
    if layout == "scalar":
        ncol = R.FORMAT[dtype][3]
        idx = scalar_slice(dtype)
        assert 3000 < idx.size < 14000
        idx = np.concatenate([idx + k * ncol for k in range(rows.shape[1] // ncol)])
        rows = rows[:, idx]
        segs, numel = scalar_layout(rows.shape[1])
    else:
        segs, numel = [(0, rows.shape[1])], rows.shape[1] + 5
    want = R.exact_mean(rows, dtype)
    assert not want[1].any()
    res = reduce_bits(dtype, place(rows, segs, numel), segs, numel, tile)
    assert_bits(gather(res, segs), want, (dtype, tile, n, layout))
    inside = np.zeros(numel, bool)
    for o, m in segs:
        inside[o:o + m] = True
    assert (res[~inside] == OUT_PAT).all(), "wrote outside the segments"


# ------------------------------------------------------------- identity ----
@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_one_client_gives_its_own_bits_back(dtype, layout):
    """All 65,536 patterns: widening, + 0, / 1 and narrowing change no
    non-NaN pattern except -0, which the +0-seeded sum turns into +0; a NaN
    stays a NaN."""
    bits = np.arange(1 << 16, dtype=np.uint16)[None, :]
    segs, numel = ([(0, 1 << 16)], 1 << 16) if layout == "vector" else ([(1, 1 << 16)], 65540)
    res = gather(reduce_bits(dtype, place(bits, segs, numel), segs, numel), segs)
    nan = is_nan_bits(bits[0], dtype)
    assert nan.sum() == 2 * ((1 << (R.FORMAT[dtype][0] - 1)) - 1)
    assert np.array_equal(is_nan_bits(res, dtype), nan)
    want = bits[0].copy()
    want[0x8000] = 0
    bad = np.nonzero((res != want) & ~nan)[0]
    assert bad.size == 0, (dtype, layout, bad[:5], res[bad[:5]])
    assert_bits(res, R.exact_mean(bits, dtype), (dtype, layout))


# -------------------------------------------------------- exact-sum data ----
# M == 1, ILP-4 only, the scalar 4-column body, a scalar cascade at an odd
# offset, two vector tiles + a ragged one, an aligned body with a tail, and
# again an odd offset; flags 0: the gaps are not padding
SEGS = [(0, 1), (1, 3), (4, 7), (11, 33), (48, 4096 + 64), (4208, 100), (4309, 64)]
NUMEL = 4378
# (the 4,097-client set: a vector body with its tail, a scalar cascade at an
# odd offset, the scalar 4-column body, M == 1)
SEGS_SMALL = [(0, 40), (41, 33), (74, 7), (81, 1)]
NUMEL_SMALL = 86


def key_set(n):
    return (SEGS_SMALL, NUMEL_SMALL) if n > 4096 else (SEGS, NUMEL)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [3, 9, 17, 128, 129, 257, 4097])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_exact_sum_data_gives_the_exact_mean(dtype, n, weighted):
    """k * 2^e values (and dyadic weights): every fp32 product and partial
    sum is exact, so the expected bits hold for any order."""
    segs, numel = key_set(n)
    ncols = sum(m for _, m in segs)
    cols, w = R.exact_sum_data(dtype, n, ncols, 7 * n + weighted, weighted)
    want = R.exact_mean(cols, dtype, w)
    for tile in (2048, 4096) if n in (9, 129) else (0,):
        res = reduce_bits(dtype, place(cols, segs, numel, fill=0x7e01), segs, numel, tile, w)
        assert_bits(gather(res, segs), want, (dtype, n, weighted, tile))


# ------------------------------------------------------------- the bound ----
def sizes_weights(n, seed):
    s = np.random.default_rng(seed).integers(10, 1000, n).astype(np.float64)
    return (s / s.sum()).astype(np.float32)       # w_i = fp32(n_i / sum n), not dyadic


WORST = {}


@pytest.mark.parametrize("data", ["realistic", "cancel", "range", "naninf"])
@pytest.mark.parametrize("n,weighted", [(128, True), (129, True), (4097, True), (4097, False)])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_arbitrary_data_stays_inside_the_bound(dtype, n, weighted, data):
    segs, numel = key_set(n)
    x = make_inputs(dtype, n, data, numel, 13 * n + weighted)
    bits = x.contiguous().view(torch.int16).numpy().view(np.uint16)
    w = sizes_weights(n, n) if weighted else None
    res = gather(reduce_bits(dtype, bits, segs, numel, 0, w), segs)
    cols = np.concatenate([bits[:, o:o + m] for o, m in segs], 1)
    m, err, bnd = R.bound(cols, dtype, w, res)
    rv = R.widen(res, dtype)
    # NaN and +-inf where the float64 reference has them
    assert np.array_equal(np.isnan(rv), np.isnan(m)), (dtype, n, data, "NaN positions")
    inf = np.isinf(m)
    assert np.array_equal(rv[inf], m[inf]), (dtype, n, data, "inf positions")
    fin = np.isfinite(m)
    # a column whose fp32 partial sums can round to inf although its mean is
    # finite — sum |t_i| (1 + g(n)) reaches fp32's overflow threshold; bf16
    # 'range' values next to the top, 4,097 of them unweighted: the reference
    # sums in fp32, so +-inf of the mean's sign is a legal result there
    _, s = R.mean64(cols, dtype, w)
    k = n * R.U32
    risky = fin & (s * (1 if weighted else n) * (1 + k / (1 - k)) >= 2.0 ** 128 * (1 - 2.0 ** -25))
    legal_inf = risky & np.isinf(rv) & (np.sign(rv) == np.sign(m))
    check = fin & ~legal_inf
    assert risky.sum() == 0 or (dtype == "bfloat16" and data == "range" and not weighted)
    ratio = float((err[check] / bnd[check]).max())
    WORST[dtype, n, weighted, data] = ratio
    print(f"bound ratio {dtype} n={n} weighted={weighted} {data}: {ratio:.6f} "
          f"(overall worst so far {max(WORST.values()):.6f})")
    assert ratio <= 1.0, (dtype, n, weighted, data, int(np.argmax(err / bnd)))
