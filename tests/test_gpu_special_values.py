"""GPU: non-finite and subnormal values through every column rule and kernel
form of the fp32 reduce.  tests/specials.py plants nine column patterns
(signed zeros, subnormals, +-inf, NaN, sums that overflow) over a layout whose
tile table holds the vector cascade (full and partial tiles), the scalar
cascade, the ILP-4 tail and the M == 1 order; the mean, FA_F_SUM_ONLY and two
weighted variants (zero, negative, subnormal and infinite weights) run at
client counts that take the batch-of-16 kernel and its tail (17), the pointer
table (129), the deep cascade (300) and the packed scalar tiles' direct loads
with the cascade's fourth level (4097); the client-loop instances see the
patterns in the long launch's first full and last partial tile.  Bit for bit
against the oracle and against torch's own single-threaded CPU sum (NaN
positions equal, payloads free)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import specials as S
from helpers import bits_equal
from longlaunch import end_window, head_window, long_launch_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NS = [1, 3, 17, 129, 300, 4097]


@pytest.fixture(scope="module")
def lib():
    from feddct_amd import _lib
    torch.cuda.set_device(DEV)
    return _lib


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(host [n, numel], its device copy): shared by the four modes of one
    client count and never written (the result goes to a bucket of its own)."""
    x = S.fill(n)
    x.setflags(write=False)
    return x, torch.from_numpy(x.copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _plan():
    from feddct_amd import _lib
    segs, numel, _ = S.layout()
    return _lib.Plan(segs, numel)


def _call(lib, plan, rows, n, mode, w, out):
    wa = None if w is None else (ctypes.c_float * n)(*[float(v) for v in w])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([rows[i].data_ptr() for i in range(n)]),
                                None, n, wa, out.data_ptr(), None,
                                lib.FA_F_SUM_ONLY if mode == "sum" else 0, st), "fa_reduce")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("n", NS)
def test_special_values_through_every_column_rule(lib, n, mode):
    segs, numel, phases = S.layout()
    x, xd = _inputs(n)
    w = S.mode_weights(n, mode)
    out = torch.full((numel,), 7.25, device=DEV)
    _call(lib, _plan(), xd, n, mode, w, out)
    got = out.cpu().numpy()
    for (o, m), ph in zip(segs, phases):
        cols = x[:, o:o + m] if m > 1 else x[:, o]      # a one-element segment: a 0-d key
        g = got[o:o + m].reshape(cols.shape[1:])
        assert bits_equal(g, S.oracle(cols, mode, w)), (n, mode, int(o), int(m), "oracle")
        assert bits_equal(g, S.torch_cpu(cols, mode, w)), (n, mode, int(o), int(m), "torch")
        if w is None:      # P1, all -0.0: the +0-seeded sum is +0
            zero = [j for j in range(int(m)) if (j + ph) % S.NPAT == 1]
            assert (got[o:o + m].view(np.uint32)[zero] == 0).all(), (n, mode, int(o))


@pytest.mark.parametrize("n,mode", [(3, "mean"), (3, "w1"), (17, "mean"), (17, "w2"),
                                    (256, "mean")])
def test_special_values_in_the_client_loop_instances(lib, n, mode):
    """The long launch (pipe 1 below 256 clients, pipe 2 at 256): the patterns
    planted over the long key's head window (its first full tiles) and end
    window (its last vector tile, partial, and the ILP-4 tail)."""
    w = S.mode_weights(n, mode)
    layout, plan, x, _ = long_launch_case(lib, n, w is not None, DEV, seed=7)
    assert plan.launch_form(n, w is not None)[2] == (2 if n >= 256 else 1)
    planted = [head_window(layout), end_window(layout)]
    # the plain tile table: a full vector tile inside the head window, and the
    # long key's last vector tile, a partial one, inside the end window
    _, tiles = lib.build_tiles_host(layout.segs32, layout.f32_numel)
    vec = tiles[tiles[:, 2] == 0]
    (ho, hm), (eo, em) = planted
    assert any(c == 2048 and ho <= s and s + c <= ho + hm for s, c, _ in vec)
    last = vec[(vec[:, 0] < eo + em) & (vec[:, 0] + vec[:, 1] > eo)][-1]
    assert eo <= last[0] and last[0] + last[1] <= eo + em and last[1] < 2048, last
    rng = np.random.default_rng(n)
    host = []
    for ph, (o, m) in enumerate(planted):
        cols = S.pattern_matrix(n, m, 3 * ph, rng)
        x[:, o:o + m] = torch.from_numpy(cols).to(DEV)
        host.append(cols)
    out = torch.full((x.shape[1],), float("nan"), device=DEV)
    _call(lib, plan, x, n, mode, w, out)
    for (o, m), cols in zip(planted, host):
        g = out[o:o + m].cpu().numpy()
        assert bits_equal(g, S.oracle(cols, mode, w)), (n, mode, o, m, "oracle")
        assert bits_equal(g, S.torch_cpu(cols, mode, w)), (n, mode, o, m, "torch")
