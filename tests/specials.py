"""Special-value columns for the fp32 reduce: the patterns, the raw layout that
sends them through every column rule, the weight vectors, and the two
references (the oracle, and torch's own CPU sum run single-threaded).  Shared
by tests/test_special_values_cpu.py and tests/test_gpu_special_values.py."""
import numpy as np
import torch

from oracle import torch_order as O

NPAT = 9
# P0 ordinary normals; P1 all -0.0 (the result's bits are 0); P2 subnormal
# multiples float32(1e-45) * integers(-5, 5); P3 normals with one +inf; P4
# normals with one NaN; P5 all 3e38 (the sum overflows); P6 all 1e-40; P7
# normals with +inf in row 0 and -inf in row N - 1 (inf - inf); P8 all -3e38.

# (numel, offset past the 64-float boundary).  The 9-element key sits at an
# offset that is not a multiple of 4 (nine ILP-4 columns); the second 40-element
# key does too, which sends its 32 cascade columns down the scalar cascade
# (the 5-element key alone gives that rule four columns, fewer than patterns).
KEYS = [(2, 0), (5, 0), (9, 2), (40, 0), (40, 1), (300, 0), (2048 + 40, 0)]
MODES = ["mean", "sum", "w1", "w2"]


def _round_up(x, a):
    return (x + a - 1) // a * a


def layout():
    """(segs [k, 2] int64, bucket numel, phase per segment).  Column j of
    segment i carries pattern (j + phase[i]) % 9; the nine trailing
    one-element segments are the 0-d keys (the M == 1 order), one per pattern."""
    segs, phases, off = [], [], 0
    for i, (m, shift) in enumerate(KEYS):
        off = _round_up(off, 64) + shift
        segs.append((off, m))
        phases.append(i)
        off += m
    for p in range(NPAT):
        off = _round_up(off, 64)
        segs.append((off, 1))
        phases.append(p)
        off += 1
    return np.array(segs, np.int64), _round_up(off, 64), phases


def pattern_matrix(n, m, phase, rng):
    """[n, m] float32, column j carrying pattern (j + phase) % 9."""
    x = rng.standard_normal((n, m)).astype(np.float32)
    pat = (np.arange(m) + phase) % NPAT
    for j in range(m):
        p = pat[j]
        if p == 1:
            x[:, j] = np.float32(-0.0)
        elif p == 2:
            x[:, j] = (np.float32(1e-45) * rng.integers(-5, 5, n)).astype(np.float32)
        elif p == 3:
            x[int(rng.integers(0, n)), j] = np.inf
        elif p == 4:
            x[int(rng.integers(0, n)), j] = np.nan
        elif p == 5:
            x[:, j] = np.float32(3e38)
        elif p == 6:
            x[:, j] = np.float32(1e-40)
        elif p == 7:
            x[0, j] = np.inf
            x[n - 1, j] = -np.inf
        elif p == 8:
            x[:, j] = np.float32(-3e38)
    return x


def fill(n, seed=0):
    """[n, numel] float32 client buckets over layout(): every segment's
    columns planted, the gaps ordinary normals."""
    segs, numel, phases = layout()
    rng = np.random.default_rng(1000003 * seed + n)
    x = rng.standard_normal((n, numel)).astype(np.float32)
    for (o, m), ph in zip(segs, phases):
        x[:, o:o + m] = pattern_matrix(n, int(m), ph, rng)
    return x


def weights(n, variant):
    """Variant 1: ordinary client weights with w[N-1] < 0, w[0] = 0 and w[1] =
    float32(1e-41) (a subnormal weight); variant 2 adds w[2] = inf, so 0 * inf
    and inf - inf appear.  Later entries win where N is too small for all."""
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3).astype(np.float32)
    w[n - 1] = -w[n - 1]
    w[0] = 0.0
    if n > 1:
        w[1] = np.float32(1e-41)
    if variant == 2 and n > 2:
        w[2] = np.inf
    return w


def mode_weights(n, mode):
    return weights(n, int(mode[1])) if mode[0] == "w" else None


def oracle(x, mode, w=None):
    """The main reference, per tensor: x [n, ...] float32."""
    with np.errstate(all="ignore"):
        if mode == "mean":
            return O.torch_mean0(x)
        if mode == "sum":
            return O.torch_sum0(x)
        return O.weighted_sum0(x, w)


def torch_cpu(x, mode, w=None):
    """The second reference: torch's CPU itself, single-threaded."""
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = torch.from_numpy(np.array(x, np.float32))      # (a copy: x may be read-only)
        if mode == "mean":
            r = t.mean(0)
        elif mode == "sum":
            r = t.sum(0)
        else:
            wt = torch.from_numpy(np.asarray(w, np.float32))
            r = (t * wt.reshape((-1,) + (1,) * (t.dim() - 1))).sum(0)
        return r.numpy()
    finally:
        torch.set_num_threads(nthr)
