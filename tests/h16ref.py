"""A reference for the 16-bit reduce that shares no code with the oracle.

"Widen every fp16 / bf16 value exactly to fp32, sum in fp32, divide by N (or
weight each value first), round to nearest-even once into the 16-bit type" is
restated here in numpy float64 and integer arithmetic only: nothing is
imported from ``oracle/`` or from ``feddct_amd``.  Two kinds of check come
out of it:

* ``exact_mean``: expected *bits* for inputs whose fp32 sums are exact by
  construction, so no summation order enters the expected value;
* ``bound``: an error bound against the float64 mean that holds for every
  summation order, for arbitrary data.

16-bit values travel as uint16 bit patterns, dtypes as the strings
"float16" / "bfloat16".
"""
import numpy as np

DTYPES = ("float16", "bfloat16")
U32 = 2.0 ** -24                       # fp32 unit roundoff
F32_OVERFLOW = 2.0 ** 128              # first magnitude fp32 cannot hold
# (precision p, minimum normal exponent, bits of +inf, largest finite bits)
FORMAT = {"float16": (11, -14, 0x7c00, 0x7bff), "bfloat16": (8, -126, 0x7f80, 0x7f7f)}


def widen(bits, dtype):
    """uint16 patterns -> float64, exactly (every fp16 / bf16 value is an
    fp32 value, every fp32 value a float64 value; NaN stays NaN, -0 stays -0)."""
    bits = np.ascontiguousarray(bits, np.uint16)
    with np.errstate(invalid="ignore"):      # (a signalling NaN pattern may raise the flag)
        if dtype == "float16":
            return bits.view(np.float16).astype(np.float64)
        if dtype == "bfloat16":
            return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    raise ValueError(dtype)


def rne16(x32, dtype):
    """float32 -> (uint16 patterns, is-NaN mask), round to nearest-even.

    fp16: numpy's float32 -> float16 cast (IEEE: overflow to +-inf from
    65520, subnormal results kept).  bf16: on the fp32 bits u, add 0x7fff
    plus the lowest kept bit and drop the low half — the carry out of the
    low 16 bits is the round-up, the "+ kept bit" sends a tie to the even
    neighbour, and a carry out of the mantissa walks into the exponent (the
    next binade, or inf from 0x7f7f8000).  A NaN is reported in the mask, not
    as a pattern (its payload is nobody's contract); its pattern slot holds 0.
    """
    x32 = np.ascontiguousarray(x32, np.float32)
    nan = np.isnan(x32)
    if dtype == "float16":
        with np.errstate(all="ignore"):
            out = x32.astype(np.float16).view(np.uint16).copy()
    elif dtype == "bfloat16":
        u = x32.view(np.uint32).astype(np.uint64)
        out = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1)))
               >> np.uint64(16)).astype(np.uint16)
    else:
        raise ValueError(dtype)
    out[nan] = 0
    return out, nan


def _terms(bits, dtype, weights):
    """The n x m float64 terms of the sum: x_i, or w_i * x_i with the fp32
    weight widened — an exact product in float64 (24 x 11 significant bits)."""
    x = widen(bits, dtype)
    if x.ndim != 2:
        raise ValueError("bits must be [n, m]")
    if weights is None:
        return x
    w = np.asarray(weights, np.float32).astype(np.float64)
    if w.shape != (x.shape[0],):
        raise ValueError("one weight per row")
    with np.errstate(all="ignore"):
        return x * w[:, None]


def exact_mean(bits, dtype, weights=None, return_overflow=False):
    """Expected result bits of the reduce over rows ``bits[n, m]`` whose fp32
    sums are exact by construction; returns (uint16 patterns, is-NaN mask)
    and, with ``return_overflow``, the mask of columns the overflow rule
    decided.

    The caller guarantees that every partial sum of the (weighted) rows, in
    any order, is an fp32 value: then each fp32 add of the kernel is exact,
    every order gives the same sum, and that sum is the float64 running sum
    computed here (exact for the same reason: 53 bits hold what 24 hold).
    What remains is a chain of single, correct roundings:

    1. weighted: w_i * x_i is exact in fp32 by construction (dyadic weights)
       and exact in float64 always;
    2. unweighted: the kernel rounds s / n once to fp32.  Here s / n is
       rounded to float64 and then to fp32.  The double rounding is
       innocuous: s and n are fp32 values, so a quotient that is not itself
       a midpoint between two fp32 values (24 bits, or fewer in fp32's
       subnormal range) differs from every such midpoint by a relative
       2^-38 at least for n < 2^13, far more than float64's 2^-53 can move
       it; and a quotient that is a midpoint or an fp32 value is a float64
       value and is not moved at all;
    3. ``rne16`` rounds that fp32 value once to the 16-bit type.

    Special columns, as the fp32 arithmetic of the reference defines them:
    a running sum that reaches 2^128 in magnitude is +-inf from there on (an
    exact fp32 partial sum is at most 2^128 - 2^104, so "reaches 2^128" is
    "overflows fp32"; rows are added in index order, which matters only to
    columns of mixed sign near the top of bf16 — the callers have none); a
    NaN, or +inf and -inf together, gives NaN; a column of -0 only gives +0,
    because the sum starts from +0.
    """
    t = _terms(bits, dtype, weights)
    n, m = t.shape
    s = np.zeros(m, np.float64)         # +0: the accumulators' start
    over = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = s + t[i]
            hit = np.isfinite(s) & (np.abs(s) >= F32_OVERFLOW)
            s[hit] = np.copysign(np.inf, s[hit])
            over |= hit
        q = s if weights is not None else s / np.float64(n)
        r32 = q.astype(np.float32)
    out = rne16(r32, dtype)
    return (out + (over,)) if return_overflow else out


def ulp16(v, dtype):
    """Spacing of the 16-bit format at magnitude |v| (float64 in, float64
    out): 2^(e - p + 1) with e = floor(log2 |v|), floored at the subnormal
    spacing and capped at the top binade's (an overflowed result is measured
    on the grid continued one step past the largest finite value)."""
    p, emin, _, _ = FORMAT[dtype]
    emax = 15 if dtype == "float16" else 127
    a = np.abs(np.asarray(v, np.float64))
    e = np.full(a.shape, emin, np.int64)
    pos = a > 0
    e[pos] = np.floor(np.log2(a[pos])).astype(np.int64)   # log2 is exact at powers of two
    e = np.clip(e, emin, emax)
    return np.ldexp(1.0, (e - (p - 1)).astype(np.int64))


def mean64(bits, dtype, weights=None):
    """The mean (or weighted sum) in extended precision, returned as float64,
    with s = sum |w_i x_i| (or sum |x_i| / n).  The terms are exact; their
    sum is taken in x87 extended precision where numpy has it (64 significant
    bits: the reference's own error is then 2^-40 of the bound's second term)
    and by math.fsum (exact) elsewhere."""
    t = _terms(bits, dtype, weights)
    n = t.shape[0]
    with np.errstate(all="ignore"):
        if np.finfo(np.longdouble).nmant >= 63:
            tl = t.astype(np.longdouble)
            m, s = tl.sum(0), np.abs(tl).sum(0)
            if weights is None:
                m, s = m / n, s / n
            return m.astype(np.float64), s.astype(np.float64)
        import math
        m = np.array([math.fsum(c) if np.isfinite(c).all() else float(np.sum(c)) for c in t.T])
        s = np.array([math.fsum(c) if np.isfinite(c).all() else float(np.sum(c))
                      for c in np.abs(t).T])
        if weights is None:
            m, s = m / n, s / n
        return m, s


def bound(bits, dtype, weights, r):
    """Error bound of a result ``r`` (uint16 patterns, finite or +-inf where
    the mean is finite) against the float64 mean m of arbitrary rows
    ``bits[n, m]``; returns (m, err, bnd): assert ``err <= bnd`` on the
    columns whose mean is finite.

        |r - m| <= 1/2 ulp16(max(|r|, |m|)) + g(n+1) * s + 2^-149,
        g(k) = k u / (1 - k u),  u = 2^-24,
        s = sum |w_i x_i|   (weighted)   or   sum |x_i| / n.

    Derivation.  Let S be the fp32 value that the kernel narrows.
    Weighted: t_i = fl(w_i x_i) = w_i x_i (1 + d_i), |d_i| <= u, and a sum of
    n terms takes n - 1 adds in whatever order, each exact up to a factor
    (1 + d), |d| <= u; every term passes through at most n - 1 of them, so
    S = sum w_i x_i (1 + th_i) with |th_i| <= g(n) (Higham, Accuracy and
    Stability, lemma 3.1 and section 4.2: the bound is the same for every
    order).  Unweighted: the x_i are exact in fp32, the n - 1 adds give
    factors within g(n-1), the one division another (1 + d): again g(n).
    g(n+1) >= g(n) leaves one rounding spare.  fp32 adds never lose anything
    to underflow (a subnormal sum of fp32 values is exact); the product or
    the division can, by at most half of fp32's subnormal spacing, 2^-150 per
    event: the 2^-149 covers the division, or two products.  (A weighted sum
    of bf16 values so small that more than two products land below 2^-126 can
    in principle lose 2^-150 per term; that is 2^-16 of bf16's subnormal
    half-ulp per term and no test here has come near it.)  So
    |S - m| <= g(n+1) s + 2^-149.  Narrowing is
    one rounding to nearest: |r - S| <= 1/2 ulp16 at S, and S lies between r
    and m or next to them, so the spacing at max(|r|, |m|) is an upper bound
    for the spacing at S (the subnormal spacing is the floor).  An
    overflowed r stands for the first value past the largest finite one
    (2^16, 2^128): rounding sends S there exactly when S is within half a
    top-binade ulp of it.

    What breaks it: truncation instead of rounding (up to a whole ulp16), a
    dropped client or weight (an error of the size of a term, |x| / n), a
    wrong divisor (m / n relative).  What does not: any legal order.
    """
    p, emin, inf_bits, _ = FORMAT[dtype]
    m, s = mean64(bits, dtype, weights)
    n = np.shape(bits)[0]
    r = np.ascontiguousarray(r, np.uint16)
    rv = widen(r, dtype)
    past = np.ldexp(1.0, 16 if dtype == "float16" else 128)
    rv = np.where(np.isinf(rv), np.copysign(past, rv), rv)
    k = (n + 1) * U32
    with np.errstate(all="ignore"):
        err = np.abs(rv - m)
        big = np.maximum(np.abs(rv), np.abs(m))
        big = np.where(np.isfinite(big), big, 0.0)
        bnd = 0.5 * ulp16(big, dtype) + k / (1 - k) * s + 2.0 ** -149
    return m, err, bnd


# ------------------------------------------------------------ test data ----
def adjacent_pairs(dtype, sign=0):
    """Every finite magnitude h that has a finite successor, as patterns
    (h, h + 1): 31,743 columns for fp16, 32,639 for bf16; ``sign`` 1 sets the
    sign bit of both."""
    top = FORMAT[dtype][3]
    h = np.arange(0, top, dtype=np.uint16)
    sb = np.uint16(0x8000 if sign else 0)
    return h | sb, (h + np.uint16(1)) | sb


def pair_rows(dtype, n, sign=0):
    """The adjacent-pair columns as rows of an n-client reduce: (h, h+1) at
    n = 2, an exact tie; (h, h, h, h+1) and (h, h+1, h+1, h+1) side by side
    at n = 4, a quarter and three quarters.  Sums of 2 or 4 neighbours are
    exact in fp32 (12 or 9 significant bits, far below 24)."""
    lo, hi = adjacent_pairs(dtype, sign)
    if n == 2:
        return np.stack([lo, hi])
    if n == 4:
        return np.stack([np.concatenate([lo, lo]), np.concatenate([lo, hi]),
                         np.concatenate([lo, hi]), np.concatenate([hi, hi])])
    raise ValueError(n)


def exact_sum_data(dtype, n, m, seed, weighted=False):
    """Rows whose every fp32 partial sum is exact: (bits[n, m], weights).

    Unweighted: x = k * 2^e with |k| < 2^10 (fp16) or 2^7 (bf16) and one e
    per column; any partial sum of up to 4,097 rows is an integer multiple of
    2^e below 2^23 * 2^e, an fp32 value.  Weighted: w_i = c_i / 2^12 with
    positive integers c_i summing to 2^12, and |k| small enough that
    sum c_i |k_i| < 2^24 (|k| < 2^10 or 2^7 always is: the c_i sum to 2^12);
    the products c_i k_i * 2^(e-12) and all their partial sums are again
    exact.  e is drawn so that values and sums stay inside the 16-bit
    format's normal and subnormal range and every product inside fp32's."""
    rng = np.random.default_rng(seed)
    kmax = 1 << (10 if dtype == "float16" else 7)
    k = rng.integers(-kmax + 1, kmax, (n, m))
    # a few columns of one repeated value, of zeros, and of -0 only
    k[:, 0::37] = k[0, 0::37]
    if dtype == "float16":
        e = rng.integers(-24, 6, m)      # k * 2^e: multiples of the subnormal spacing, < 2^15
    else:
        e = rng.integers(-120, 100, m)
    x = np.ldexp(k.astype(np.float64), e[None, :])
    if dtype == "float16":
        bits = x.astype(np.float16).view(np.uint16).copy()
    else:
        bits = (x.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    assert np.array_equal(widen(bits, dtype), x), "k * 2^e must be a value of the format"
    bits[:, 1::41] = 0x8000              # -0 in every client
    w = None
    if weighted:
        # positive steps of 1/4096 summing to 1; beyond 4,096 clients the
        # surplus clients weigh 0 (0 * x is exact too)
        live = min(n, 4096)
        c = np.zeros(n, np.int64)
        idx = rng.permutation(n)[:live]
        c[idx] = 1 + rng.multinomial(4096 - live, np.ones(live) / live)
        assert c.sum() == 4096
        w = (c / 4096.0).astype(np.float32)
    return bits, w
