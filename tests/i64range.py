"""int64 keys over the whole range of the type: the shared generator of
tests/test_gpu_int64_range.py (the kernels) and tests/test_oracle.py (the
oracle against torch's CPU arithmetic).  No GPU, no library."""
import numpy as np

# the key sizes of test_gpu_parity.test_int64_adversarial: the M == 1 inner,
# ILP-4 and cascade orders and the packed-column staging
KEYS = [1, 1, 3, 9, 40, 300]            # [] and [1] are both one element
SEGS64 = []
for _m in KEYS:
    SEGS64.append((sum(m for _, m in SEGS64), _m))
NUMEL = sum(KEYS)
NS = [1, 2, 7, 9, 20, 33, 129]

# .float() ties at and above 2^24 (to even), the 2^31 / 2^32 word boundary,
# beyond 2^40 and 2^53
FIXED = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6,
         2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 2 ** 8, 2 ** 40 + 12345, 2 ** 53 + 1]


def magnitudes(n):
    """The fixed list with both signs, and next to the largest power of two
    whose n-fold sum stays inside int64: 2^k - 1, 2^k - 2^(k-25) and -2^k with
    k = 62 - ceil(log2 n), so no partial sum of n such values leaves the range
    (n * 2^k <= 2^62) and every fp32 mean is inside int64."""
    k = 62 - int(n - 1).bit_length()
    vals = [s * m for m in FIXED for s in (1, -1)]
    vals += [2 ** k - 1, -(2 ** k - 1), 2 ** k - 2 ** (k - 25), -(2 ** k - 2 ** (k - 25)), -2 ** k]
    return vals


def values(n, seed=0):
    """[n, NUMEL] int64: per client and column one of magnitudes(n), by a
    seeded draw; the first len(magnitudes) columns of the 300-element key and
    client 0 of the small keys walk the list, so every value occurs.  n == 1
    also holds INT64_MIN and 2^63 - 2^39 (both exact in fp32, both in range)."""
    mags = np.array(magnitudes(n), np.int64)
    rng = np.random.default_rng(1000 * n + seed)
    x = mags[rng.integers(0, len(mags), (n, NUMEL))]
    o300 = SEGS64[-1][0]
    for i in range(n):
        x[i, o300:o300 + len(mags)] = np.roll(mags, i)
    assert len(mags) <= o300
    x[0, :len(mags)] = mags
    if n == 1:
        x[0, o300 + 40] = -2 ** 63
        x[0, o300 + 41] = 2 ** 63 - 2 ** 39
        x[0, 0] = -2 ** 63
        x[0, 2] = 2 ** 63 - 2 ** 39
    return x
