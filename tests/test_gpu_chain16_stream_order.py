"""Stream order of fa_reduce_chain_elem: every launch of a chain over 16-bit
buckets rides the stream it is handed (tests/streamgate.py, arrangements A and
B, as tests/test_gpu_stream_order.py runs every other entry point).

The cases are registered in that module's table (``case``), so its guard over
both headers — every entry point with a ``void *stream`` has a stream-order
case — counts them: the two modules belong together, and the guard holds
whenever both are collected (the whole suite, or the two files).

The cases run in a fresh child process (this file as a script): the harness
needs a side stream that does not share a hardware queue with the null
stream, which its power check verifies — and which side stream a module gets
depends on how many the process has handed out before.  One more side stream
taken here, in the suite's process, moved the stream-order modules after this
one onto other streams (one of them onto a stream without that property); a
child takes its own first one and leaves the suite's untouched."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import round16 as R
import streamgate as SG
import test_gpu_chain16 as C
import test_gpu_stream_order as S
from feddct_amd import _lib
from oracle import torch_order as O

L = _lib.lib
NAMES = []


def chain16(dtype, weighted):
    """Three segments (n_total = 20 cut 7 + 7 + 6) queued back to back on the
    "man" layout's vector tiles, the fp32 state planes carried on the device."""
    n, cuts = 20, [0, 7, 14, 20]
    lay = C.layout("man", dtype)
    vec, _, _ = C.plans("man", dtype)
    inv = C.tiles_of("man", dtype)[2]
    bits = R.cancelling_bits(dtype, n, lay.f32_numel, 41)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3) if weighted else None
    cl = C.Clients(lay, bits)
    st, out = C.State(lay.f32_numel), C.Out(lay.f32_numel)
    exp, inside, _ = C.expected(lay, dtype, bits, None, w)
    arrs = [_lib.ptr_array(cl.p16[a:z]) for a, z in zip(cuts, cuts[1:])]
    was = [C._floats(None if w is None else w[a:z]) for a, z in zip(cuts, cuts[1:])]
    chs = [_lib.FaChain(a, n, st.ptr if a else None, st.ptr if z < n else None, st.plane)
           for a, z in zip(cuts, cuts[1:])]
    inputs = [SG.In(cl.dev, kind="f16bits" if dtype == "float16" else "bf16bits")]
    what = ("chain16", dtype, weighted)

    def call(s):
        for k, (a, z) in enumerate(zip(cuts, cuts[1:])):
            rc = L.fa_reduce_chain_elem(vec.handle, arrs[k], z - a, was[k], ctypes.byref(chs[k]),
                                        out.ptr if z == n else None, 0, S.sp(s))
            assert rc == _lib.FA_OK, (what, k, L.fa_last_error())

    def check(res, arr):
        o16, c16 = res.out[0].view(np.uint16), res.out[1].view(np.uint16)
        G, Lf = C.G, lay.f32_numel
        assert (o16[:G] == C.SENT16).all() and (o16[G + Lf:] == C.SENT16).all(), (what, "guards")
        got = o16[G:G + Lf]
        seg = inv & inside
        assert seg.sum() > 4096
        assert R.same16(got[seg], exp[seg], dtype), what
        assert (got[~inv] == R.FILL16).all(), (what, "outside the vector tiles")
        assert np.array_equal(c16, cl.host), (what, "a client written")
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[out.t, cl.dev], check=check)


for _d in C.DTYPES:
    for _w in (False, True):
        _name = f"chain16-{_d}-{'weighted' if _w else 'mean'}"
        S.case(_name, ["fa_reduce_chain_elem"])(lambda d=_d, w=_w: chain16(d, w))
        NAMES.append(_name)


def main():
    """Every case in both arrangements on one side stream, after the harness's
    power check; prints one line per case."""
    torch.cuda.set_device(0)
    side = torch.cuda.Stream()
    for arr in "AB":
        SG.power_check(arr, side)
    for name in NAMES:
        for arr in S.CASES[name].arrs:
            k = S.CASES[name].build()
            torch.cuda.synchronize()
            res = SG.run(arr, side, k.call, k.inputs, k.outputs, name)
            k.check(res, arr)
            print("ok", name, arr, flush=True)
    print(SG.report())


@pytest.mark.gpu
def test_chain16_stream_order():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=here, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    done = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert sorted(done) == sorted([n, a] for n in NAMES for a in "AB"), r.stdout


if __name__ == "__main__":
    main()
