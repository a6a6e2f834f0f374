"""tests/h16ref.py checked where no GPU is needed — against torch's own CPU
arithmetic and against the oracle — so that the GPU tests built on it rest on
something verified; and the raw fuzz cases of test_gpu_h16_fuzz.py through
the host tile planner."""
import numpy as np
import pytest
import torch

import h16ref as R
from feddct_amd import _lib
from oracle import torch_order as O
from test_gpu_h16_fuzz import SEEDS, case, gaps_of, inside_mask, may_write_mask
from test_gpu_h16_kernel import make_inputs

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def from_bits(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()) \
        .view(TDT[dtype])


def to_bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def oracle_bits(bits, dtype, weights=None):
    """The expected value of the GPU tests: the oracle on the widened rows,
    then torch's CPU .to(dtype); (bits, is-NaN)."""
    xf = from_bits(bits, dtype).float().numpy()
    with np.errstate(all="ignore"):
        r = O.torch_mean0(xf) if weights is None else O.weighted_sum0(xf, weights)
    t = torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(TDT[dtype])
    return to_bits(t), torch.isnan(t).numpy()


def same(a, b):
    """Columns on which two (bits, is-NaN) results differ."""
    return np.nonzero((a[1] != b[1]) | ((a[0] != b[0]) & ~a[1]))[0]


# ------------------------------------------------------------ conversions ----
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_widen_and_rne16_against_torch_on_every_pattern(dtype):
    bits = np.arange(1 << 16, dtype=np.uint16)
    t = from_bits(bits, dtype)
    v = R.widen(bits, dtype)
    nan = torch.isnan(t).numpy()
    assert np.array_equal(np.isnan(v), nan)
    assert np.array_equal(v[~nan], t.double().numpy()[~nan])
    assert np.array_equal(np.signbit(v[~nan]), np.signbit(t.double().numpy()[~nan]))
    # round trip, and fp32 values between the patterns: the midpoints (ties),
    # and one fp32 ulp to either side of them
    fin = np.nonzero(np.isfinite(v))[0]
    b, n = R.rne16(v[fin].astype(np.float32), dtype)
    assert not n.any() and np.array_equal(b, bits[fin])
    lo = v[fin]
    hi = R.widen((bits[fin] + np.uint16(1)), dtype)
    ok = np.isfinite(hi)
    mid = ((lo[ok] + hi[ok]) / 2).astype(np.float32)        # exact in fp32
    assert np.array_equal(mid.astype(np.float64), (lo[ok] + hi[ok]) / 2)
    for x in (mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))):
        got, gn = R.rne16(x, dtype)
        want = torch.from_numpy(x.copy()).to(TDT[dtype])
        assert not gn.any() and np.array_equal(got, to_bits(want))
    # past the top: the last value that stays finite, the first that does not
    top = R.widen(np.array([R.FORMAT[dtype][3]], np.uint16), dtype)[0]
    edge = np.float32(top + R.ulp16(top, dtype) / 2)
    for x, want in ((np.nextafter(edge, np.float32(0)), R.FORMAT[dtype][3]),
                    (edge, R.FORMAT[dtype][2])):
        for sgn, sb in ((1, 0), (-1, 0x8000)):
            got, _ = R.rne16(np.array([sgn * x], np.float32), dtype)
            assert got[0] == want | sb
            assert to_bits(torch.tensor([sgn * float(x)]).to(TDT[dtype]))[0] == want | sb
    assert R.rne16(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), dtype)[1].tolist() == \
        [True, False, False, False]
    assert R.rne16(np.array([-0.0], np.float32), dtype)[0][0] == 0x8000


# ------------------------------------------------- exhaustive neighbours ----
OVERFLOW_COLUMNS = {("float16", 2): 0, ("float16", 4): 0, ("bfloat16", 2): 127, ("bfloat16", 4): 255}


@pytest.mark.parametrize("sign", [0, 1])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_adjacent_pair_rounds_as_torch_and_the_oracle_round_it(dtype, n, sign):
    rows = R.pair_rows(dtype, n, sign)
    ncol = {"float16": 31743, "bfloat16": 32639}[dtype]
    assert rows.shape == (n, ncol * (n // 2))
    gb, gn, over = R.exact_mean(rows, dtype, return_overflow=True)
    t = from_bits(rows, dtype).float().mean(0).to(TDT[dtype])
    torch_res = (to_bits(t), torch.isnan(t).numpy())
    assert same((gb, gn), torch_res).size == 0
    assert same((gb, gn), oracle_bits(rows, dtype)).size == 0
    assert not gn.any()
    # the +-inf rule decided exactly the columns whose fp32 sum overflows
    # while the mean itself is a finite value of the format: per sign 127
    # bf16 columns at N = 2, 255 at N = 4 (counted over the tie columns /
    # over either of the quarter columns), none for fp16
    per_kind = over.reshape(n // 2, ncol).sum(1)
    assert (per_kind == OVERFLOW_COLUMNS[dtype, n]).all(), per_kind
    inf = R.FORMAT[dtype][2] | (0x8000 if sign else 0)
    assert (gb[over] == inf).all() and (gb[~over] != inf).all()
    with np.errstate(all="ignore"):
        plain = (R.widen(rows, dtype).sum(0) / n).astype(np.float32)
    pb, _ = R.rne16(plain, dtype)
    assert np.array_equal(np.nonzero(pb != gb)[0], np.nonzero(over)[0])


def test_exact_mean_special_columns():
    for dtype in R.DTYPES:
        inf, top = R.FORMAT[dtype][2], R.FORMAT[dtype][3]
        one = 0x3c00 if dtype == "float16" else 0x3f80
        rows = np.array([[0x8000, inf, inf, one, 0x8000, top, 0x0001],
                         [0x8000, inf | 0x8000, one, inf | 1, 0x0000, top, 0x8001],
                         [0x8000, one, one, one, 0x8000, top, 0x0000]], np.uint16)
        b, n = R.exact_mean(rows, dtype)
        assert n.tolist() == [False, True, False, True, False, False, False]
        assert b[0] == 0 and b[2] == inf and b[4] == 0 and b[6] == 0
        # three times the largest value: an fp32 value for fp16, past fp32 for bf16
        assert b[5] == (top if dtype == "float16" else inf)
        assert same((b, n), oracle_bits(rows, dtype)).size == 0


# -------------------------------------------------------- exact-sum data ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 129, 257])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_exact_sum_data_matches_the_oracle(dtype, n, weighted):
    bits, w = R.exact_sum_data(dtype, n, 700, 100 * n + weighted, weighted)
    assert (w is None) == (not weighted)
    if weighted:
        assert float(np.asarray(w, np.float64).sum()) == 1.0
    got = R.exact_mean(bits, dtype, w)
    # 1-D keys of every column rule: M == 1, ILP-4 tails, cascade bodies
    for o, m in ((0, 1), (1, 7), (8, 33), (41, 659)):
        want = oracle_bits(bits[:, o:o + m], dtype, w)
        assert same((got[0][o:o + m], got[1][o:o + m]), want).size == 0, (o, m)
    assert not got[1].any()
    assert (got[0][1::41] == 0).all(), "-0 in every client gives +0"


def test_exact_sum_data_is_exact_in_every_order():
    """The generator's promise, checked in fp32 itself: forward, backward and
    pairwise sums of the (weighted) rows agree bit for bit."""
    for dtype in R.DTYPES:
        for weighted in (False, True):
            bits, w = R.exact_sum_data(dtype, 4097, 64, 5, weighted)
            t = R.widen(bits, dtype).astype(np.float32)
            if weighted:
                t = t * np.asarray(w, np.float32)[:, None]
                assert np.array_equal(t.astype(np.float64),
                                      R.widen(bits, dtype) * np.asarray(w, np.float64)[:, None])
            fwd, bwd = np.zeros(64, np.float32), np.zeros(64, np.float32)
            for i in range(4097):
                fwd = fwd + t[i]
                bwd = bwd + t[4096 - i]
            assert fwd.dtype == np.float32
            assert np.array_equal(fwd, bwd)
            assert np.array_equal(fwd.astype(np.float64), t.astype(np.float64).sum(0))


# ------------------------------------------------------------- the bound ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [3, 17, 129, 257])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_the_oracles_result_is_inside_the_bound(dtype, n, weighted):
    worst = 0.0
    for k, data in enumerate(("realistic", "cancel", "subnormal")):
        x = make_inputs(dtype, n, data, 3000, 10 * n + k)
        bits = to_bits(x)
        w = O.weights_from_sizes(np.random.default_rng(n).integers(10, 1000, n)) \
            if weighted else None
        rb, rn = oracle_bits(bits, dtype, w)
        assert not rn.any()
        m, err, bnd = R.bound(bits, dtype, w, rb)
        assert np.isfinite(m).all()
        ratio = float((err / bnd).max())
        print(f"bound ratio {dtype} n={n} weighted={weighted} {data}: {ratio:.6f}")
        worst = max(worst, ratio)
    assert worst <= 1.0


def test_the_bound_catches_what_it_should():
    """Truncation, a dropped client, a wrong divisor and a swapped weight
    break the bound; another summation order does not."""
    for dtype in R.DTYPES:
        n = 17
        bits = to_bits(make_inputs(dtype, n, "realistic", 3000, 3))
        w = O.weights_from_sizes(np.arange(1, n + 1) * 10)
        xf = R.widen(bits, dtype).astype(np.float32)

        def broken(res32):
            _, err, bnd = R.bound(bits, dtype, None, R.rne16(res32, dtype)[0])
            return float((err / bnd).max())
        s = np.zeros(3000, np.float32)
        for i in reversed(range(n)):
            s = s + xf[i]
        assert broken(s / np.float32(n)) <= 1.0                         # another order
        assert broken(s / np.float32(n + 1)) > 1.0                      # divisor
        assert broken((s - xf[n - 1]) / np.float32(n)) > 1.0            # a client dropped
        trunc = (s / np.float32(n)).view(np.uint32) & np.uint32(0xffff0000 if dtype == "bfloat16"
                                                                else 0xffffe000)
        _, err, bnd = R.bound(bits, dtype, None,
                              (trunc >> np.uint32(16)).astype(np.uint16) if dtype == "bfloat16"
                              else trunc.view(np.float32).astype(np.float16).view(np.uint16))
        assert float((err / bnd).max()) > 1.0                           # truncation
        ws = np.zeros(3000, np.float32)
        w_bad = w.copy()
        w_bad[n - 1] = w[0]
        for i in range(n):
            ws = ws + xf[i] * w_bad[i]
        _, err, bnd = R.bound(bits, dtype, w, R.rne16(ws, dtype)[0])
        assert float((err / bnd).max()) > 1.0                           # a weight swapped


# ------------------------------------------------- planner fuzz, on the host ----
@pytest.mark.parametrize("seed", SEEDS)
def test_host_tile_table_of_the_raw_fuzz_cases(seed):
    c = case(seed)
    flags = _lib.FA_PLAN_GAPS_ARE_PADDING if c["gaps_pad"] else 0
    info, tiles = _lib.build_tiles_host(c["segs"], c["numel"], c["segs64"], c["numel64"],
                                        c["tile"], flags=flags,
                                        elem=_lib.ELEM_OF_DTYPE[TDT[c["dtype"]]])
    assert info["tile_elems"] == c["tile"] and info["ntiles"] == len(tiles)
    inside, may = inside_mask(c), may_write_mask(c)
    cover = np.zeros(c["numel"], np.int64)
    cover64 = np.zeros(max(1, c["numel64"]), np.int64)
    for start, count, kind in tiles:
        assert count >= 1 and start >= 0
        if kind >= 4:
            assert start + count <= c["numel64"]
            cover64[start:start + count] += 1
            continue
        assert start + count <= c["numel"] and count <= (c["tile"] if kind == 0 else 256)
        cover[start:start + count] += 1
        if kind == 0:      # 16-B vectors of 8 elements, whole ones
            assert start % 8 == 0 and count % 8 == 0, (seed, start, count)
        assert inside[start:start + count].any(), (seed, start, count, kind, "a tile of gap only")
        if kind != 0:      # scalar columns never reach over a gap
            assert inside[start:start + count].all(), (seed, start, count, kind)
    assert (cover[inside] == 1).all(), (seed, "every segment element exactly once")
    assert cover.max(initial=0) <= 1, (seed, "two tiles over one element")
    if not c["gaps_pad"]:
        assert (cover[~inside] == 0).all(), (seed, "a tile over a gap that is no padding")
    # with the flag, only the gap between two segments that a vector run
    # joins — all of it, the run is contiguous — and never the bucket's head
    # or tail
    assert (cover[~may] == 0).all(), seed
    live = [(int(o), int(m)) for o, m in c["segs"] if m]
    for (o0, m0), (o1, _) in zip(live, live[1:]):
        gap = cover[o0 + m0:o1]
        assert gap.size == 0 or gap.min() == gap.max(), (seed, o0 + m0, o1, "a gap half covered")
    want64 = np.zeros(max(1, c["numel64"]), np.int64)
    for o, m in c["segs64"]:
        want64[o:o + m] = 1
    assert np.array_equal(cover64, want64), (seed, "int64 tiles")
    if not c["gaps_pad"]:   # (with the flag the count includes the padding a run spans)
        assert info["cascade_elems"] + info["tail_elems"] == int(c["segs"][:, 1].sum())
    # the fp32 element type is the existing entry point's table
    a = _lib.build_tiles_host(c["segs"], c["numel"], c["segs64"], c["numel64"], c["tile"],
                              flags=flags)
    b = _lib.build_tiles_host(c["segs"], c["numel"], c["segs64"], c["numel64"], c["tile"],
                              flags=flags, elem=_lib.FA_ELEM_F32)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert len(gaps_of(c["segs"], c["numel"])) >= 2
