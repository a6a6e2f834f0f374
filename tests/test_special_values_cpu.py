"""No GPU: the references of tests/test_gpu_special_values.py agree with each
other.  On the planted patterns (tests/specials.py: signed zeros, subnormals,
infinities, NaN, sums that overflow) and under both weight variants (zero,
negative, subnormal and infinite weights) the oracle's restatement equals
torch's own single-threaded CPU sum bit for bit, so the oracle alone pins the
kernels where torch's CPU order cannot be run; and the planted layout sends
every pattern through every column rule of the plan."""
import numpy as np
import pytest

import specials as S
from helpers import bits_equal

NS = [1, 2, 3, 8, 17, 129, 300, 4097]
MS = [1, 2, 5, 8, 9, 40, 300, 2088]


@pytest.mark.parametrize("n", NS)
def test_oracle_equals_torch_cpu_on_special_values(n):
    rng = np.random.default_rng(n)
    for phase, m in enumerate(MS):
        x = S.pattern_matrix(n, m, phase, rng)
        assert m < S.NPAT or {(j + phase) % S.NPAT for j in range(m)} == set(range(S.NPAT))
        for mode in S.MODES:
            w = S.mode_weights(n, mode)
            cols = [x] if m > 1 else [x[:, 0], x]   # a 0-d key, and shape [1]
            for c in cols:
                want = S.oracle(c, mode, w)
                ref = S.torch_cpu(c, mode, w)
                assert bits_equal(want, ref), (n, m, mode, c.shape)
    # the nine 0-d keys of the layout, one pattern each
    for p in range(S.NPAT):
        x = S.pattern_matrix(n, 1, p, rng)[:, 0]
        for mode in S.MODES:
            w = S.mode_weights(n, mode)
            assert bits_equal(S.oracle(x, mode, w), S.torch_cpu(x, mode, w)), (n, p, mode)


def test_patterns_are_what_they_claim():
    n = 17
    x = S.pattern_matrix(n, S.NPAT, 0, np.random.default_rng(0))
    assert (x[:, 1].view(np.uint32) == 0x80000000).all()
    assert (np.abs(x[:, 2]) < np.float32(1.2e-38)).all() and np.any(x[:, 2] != 0)
    assert np.isposinf(x[:, 3]).sum() == 1 and np.isnan(x[:, 4]).sum() == 1
    assert np.isposinf(x[0, 7]) and np.isneginf(x[n - 1, 7])
    mean = S.oracle(x, "mean")
    assert mean.view(np.uint32)[1] == 0
    assert np.isposinf(mean[3]) and np.isnan(mean[4]) and np.isposinf(mean[5])
    assert 0 < mean[6] < np.float32(1.2e-38) and np.isnan(mean[7]) and np.isneginf(mean[8])
    for v in (1, 2):
        w = S.weights(n, v)
        assert w[0] == 0 and w[n - 1] < 0 and 0 < w[1] < np.float32(1.2e-38)
        assert np.isinf(w[2]) == (v == 2)
    # 0 * inf: variant 2 turns P7's row-0 infinity under w[0] = 0 into a NaN product
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.float32(0.0) * x[0, 7])


@pytest.mark.parametrize("gaps", [True, False])
def test_layout_sends_every_pattern_through_every_column_rule(gaps):
    """The plan's host tile table over specials.layout(): the vector cascade
    (a full tile and partial ones), the scalar cascade, the ILP-4 tail and the
    M == 1 order each hold columns of all nine patterns."""
    from feddct_amd import _lib
    segs, numel, phases = S.layout()
    pat = np.full(numel, -1)
    for (o, m), ph in zip(segs, phases):
        pat[o:o + m] = (np.arange(m) + ph) % S.NPAT
    _, tiles = _lib.build_tiles_host(segs, numel,
                                     flags=_lib.FA_PLAN_GAPS_ARE_PADDING if gaps else 0)
    te = 2048
    seen = {}
    for start, count, kind in tiles:
        rule = {0: "vec_full" if count == te else "vec_partial", 1: "casc_scalar", 2: "ilp4",
                3: "inner"}[int(kind)]
        seen.setdefault(rule, set()).update(int(p) for p in pat[start:start + count] if p >= 0)
    want = set(range(S.NPAT))
    assert set(seen) == {"vec_full", "vec_partial", "casc_scalar", "ilp4", "inner"}
    for rule, pats in seen.items():
        assert pats == want, (rule, pats)
