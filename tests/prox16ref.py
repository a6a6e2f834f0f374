"""The proximal term of fp16 / bf16 models, restated.

What ``(w - w_t).norm(2)``, the running ``proximal_term += ...`` and their
backward compute for 16-bit tensors on torch's CPU, written out in numpy
float32 / float64 and the integer roundings of ``h16ref``: nothing is
imported from ``feddct_amd`` or from ``oracle/``, and nothing from torch.
tests/test_prox16_cpu.py checks this restatement against CPU torch bit for
bit; the GPU tests check the kernels against it.

16-bit values travel as uint16 bit patterns, dtypes as "float16" / "bfloat16".
"""
import math

import numpy as np

from h16ref import FORMAT, rne16, widen

U32 = 2.0 ** -24                        # fp32 unit roundoff
U16 = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
TINY16 = {"float16": 2.0 ** -24, "bfloat16": 2.0 ** -133}   # smallest subnormal
CHUNK = 4096                            # elements per partial-sum workgroup


def f32(bits, dtype):
    """uint16 patterns -> float32, exactly."""
    return widen(bits, dtype).astype(np.float32)


def rn16(x32, dtype):
    """float32 -> uint16 patterns, round to nearest-even; NaN -> 0x7fc0 / 0x7e00."""
    out, nan = rne16(np.asarray(x32, np.float32), dtype)
    out = out.copy()
    out[nan] = 0x7e00 if dtype == "float16" else 0x7fc0
    return out


def diff16(a, b, dtype):
    """w - w_t: rn16(fp32(w) - fp32(w_t))."""
    with np.errstate(all="ignore"):
        return rn16(f32(a, dtype) - f32(b, dtype), dtype)


def norm64(d, dtype):
    """sqrt(sum d16^2) in float64 (squares and their sum far inside its range)."""
    x = widen(d, dtype)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.sum(x * x)))


def norm_beta(count):
    """Relative bound of the fp32 norm the pure kernel rounds to 16 bits, for a
    segment of ``count`` elements, to first order in u = 2^-24, from the order
    csrc/prox_h16.hip documents.  The differences are the restated 16-bit
    values themselves (no rounding of the kernel's own) and their squares are
    exact in fp32 (16 or 22 significant bits).  The terms are non-negative, so
    the sum's relative error is at most the longest chain of adds one term
    passes through:
      16 in-lane adds (4 groups of four per lane: 3 adds inside each, 1 into
         the accumulator),
      1  the scalar-tail add,
      6  wave shuffles,
      3  cross-wave adds (4 waves, the first onto 0 exact),
      ceil(c/64) + 6 in the finish (lane l: partials l, l + 64, ...; then the
         shuffle tree), c = ceil(count / 4096) chunks.
    The square root halves a relative error and adds one rounding."""
    c = -(-int(count) // CHUNK)
    depth = 16 + 1 + 6 + 3 + -(-c // 64) + 6
    return (depth / 2 + 1) * U32


def _f32_down(x):
    y = np.float32(x)
    return y if float(y) <= x else np.nextafter(y, np.float32(-np.inf))


def _f32_up(x):
    y = np.float32(x)
    return y if float(y) >= x else np.nextafter(y, np.float32(np.inf))


def norm16_interval(d, dtype):
    """(rn16(lo), rn16(hi)) as uint16 patterns: the float64 norm of d16 scaled by
    1 -+ beta, rounded outward to fp32, then narrowed.  Where the two are equal
    the 16-bit norm is determined whatever the fp32 summation order."""
    n = norm64(d, dtype)
    beta = norm_beta(len(d))
    lo, hi = _f32_down(n * (1 - beta)), _f32_up(n * (1 + beta))
    with np.errstate(all="ignore"):
        return int(rn16([lo], dtype)[0]), int(rn16([hi], dtype)[0])


def running_total(norm_bits, dtype):
    """proximal_term += n16[k], in 16 bits, in order, from n16[0]; an empty
    list gives +0."""
    norm_bits = np.asarray(norm_bits, np.uint16).reshape(-1)
    if len(norm_bits) == 0:
        return 0
    run = f32(norm_bits[:1], dtype)
    with np.errstate(all="ignore"):
        for k in range(1, len(norm_bits)):
            run = f32(rn16(run + f32(norm_bits[k:k + 1], dtype), dtype), dtype)
    return int(rn16(run, dtype)[0])


def grad16(d, n_bits, gout_bits, dtype):
    """grad_w = rn16(gout16 * rn16(d16 / n16)), zero where n16 == 0; the
    division is IEEE fp32.  grad_w_t is its negation (the sign bit flipped)."""
    d = np.asarray(d, np.uint16)
    n = f32(np.array([n_bits], np.uint16), dtype)[0]
    if n == 0:
        return np.zeros_like(d)
    g = f32(np.array([gout_bits], np.uint16), dtype)[0]
    with np.errstate(all="ignore"):
        q = f32(rn16(f32(d, dtype) / n, dtype), dtype)
        return rn16(g * q, dtype)


def neg16(bits):
    return np.asarray(bits, np.uint16) ^ np.uint16(0x8000)


def acc16(old, new, dtype):
    """AccumulateGrad in 16 bits: rn16(fp32(old) + fp32(new))."""
    with np.errstate(all="ignore"):
        return rn16(f32(old, dtype) + f32(new, dtype), dtype)


def grad_limit(want64, dtype):
    """|got - want64| <= 3.1 u16 |want64| + 2 (smallest subnormal): three 16-bit
    roundings (the difference is exact input; the norm, the quotient, the
    product) plus the fp32 terms."""
    return 3.1 * U16[dtype] * np.abs(want64) + 2 * TINY16[dtype]


assert math.isclose(U16["float16"], 2.0 ** -FORMAT["float16"][0])


# ------------------------------------------------------------ test data ----
# the 8-element vector edge, the 2048-element load-slot edge, the chunk edge
# and the ragged multi-chunk case
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 1023, 1024, 0, 1025, 2047, 2048, 2049,
           4095, 4096, 4097, 8191, 8193, 3 * 4096 + 7]
ZERO_SEG = LENGTHS.index(1024)     # the segment with a == b


def place(lengths, lead=8):
    """Segments of the given lengths at offsets that are multiples of 8, with
    gaps of 8 to 23 elements between them, ``lead`` in front and 8 behind:
    (segs[k] = (offset, numel), bucket numel)."""
    segs, off = [], lead
    for k, n in enumerate(lengths):
        segs.append((off, n))
        off = -(-(off + n + 8) // 8) * 8 + 8 * (k % 2)
    return np.array(segs, np.int64).reshape(-1, 2), off + 8


def inputs(numel, seed, dtype, same=()):
    """b = randn, a = b + 0.05 randn, both narrowed: (a bits, b bits); a == b
    over every (offset, numel) of ``same``."""
    rng = np.random.default_rng(seed)
    b32 = rng.standard_normal(numel).astype(np.float32)
    a32 = (b32 + np.float32(0.05) * rng.standard_normal(numel).astype(np.float32))
    a, b = rn16(a32, dtype), rn16(b32, dtype)
    for o, m in same:
        a[o:o + m] = b[o:o + m]
    return a, b


def exact_share(segs, a, b, dtype):
    """(segments whose 16-bit norm every legal summation order agrees on,
    non-empty segments, the (lo, hi) patterns per segment)."""
    iv = [norm16_interval(diff16(a[o:o + m], b[o:o + m], dtype), dtype) for o, m in segs]
    live = [k for k, (_, m) in enumerate(segs) if m > 0]
    return sum(iv[k][0] == iv[k][1] for k in live), len(live), iv
