"""GPU: the chained multi-GPU round on fp16 / bf16 buckets over
torch.distributed — feddct_amd/dist.py's ChainAggregator with its opt-in and
HipChainBackend on 16-bit plans (fa_reduce_chain_elem, fp32 state planes, a
16-bit compact tail plan), at W = 1, 2, 3 and 8 ranks as threads of one
process over the in-process stand-in (tests/distloop.py), one GPU, the
current stream; tests/test_gpu_dist_loopback.py::test_chained_round on
native 16-bit layouts.

Results against the oracle (tests/round16.expected16, weighted:
tests/chain16.expected16w); one case per W also against one GPU's 16-bit
fa_reduce.  Ranks that are no result ranks keep their fill, inputs stay
unchanged.  Every comparison is bit for bit, two NaNs equal."""
import ctypes

import numpy as np
import pytest
import torch

import chain16 as K
import feddct_amd.dist as D
import round16 as R
from distloop import LoopDist, run_ranks
from feddct_amd import _lib
from oracle import torch_order as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HOLES = [0, 3, 0, 4, 5, 0, 8, 0]     # no clients first, in the middle, last: finisher 6


@pytest.fixture(autouse=True)
def _entry():
    """A library without the entry fails here, at symbol lookup."""
    assert _lib.lib.fa_reduce_chain_elem
    torch.cuda.set_device(DEV)


def _fill_out(lay, dtype):
    return (R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype, DEV),
            torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64, device=DEV))


def _single_gpu(lay, dtype, bits, i64, w):
    """One GPU's 16-bit fa_reduce over all clients (weighted: with weights)."""
    n = len(bits)
    c16 = [R.as_tensor(bits[k], dtype, DEV) for k in range(n)]
    c64 = [torch.from_numpy(i64[k].copy()).to(DEV) for k in range(n)]
    o32, o64 = _fill_out(lay, dtype)
    plan = _lib.Plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, elem=R.ELEM[dtype])
    wa = None if w is None else (ctypes.c_float * n)(*map(float, w))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.fa_reduce(plan.handle, _lib.ptr_array([t.data_ptr() for t in c16]),
                                  _lib.ptr_array([t.data_ptr() for t in c64]), n, wa,
                                  o32.data_ptr(), o64.data_ptr(), 0, st), "fa_reduce")
    torch.cuda.synchronize()
    return R.bits_of(o32).copy(), o64.cpu().numpy().copy()


CASES = [
    # layout, counts, final, root, nchunks, weighted, rounds, single
    ("A", [20], "reduce", 0, 16, False, 2, True),
    ("raw", [20], "allreduce", 0, 1, True, 1, False),
    ("B", [7, 13], "allreduce", 0, 16, True, 2, True),
    ("A", [260, 40], "reduce", 1, 16, False, 1, False),       # plane 2 travels
    ("raw", [7, 13], "reduce", 0, 1, False, 1, False),        # root != finisher 1
    ("raw", [0, 3, 2], "reduce", 0, 1, True, 1, False),       # root holds no clients
    ("B", [9, 0, 11], "allreduce", 0, 16, False, 2, True),
    ("A", [260, 40, 0], "reduce", 1, 16, True, 1, False),
    ("B", HOLES, "reduce", 6, 16, True, 2, True),             # root == finisher
    ("raw", HOLES, "reduce", 0, 1, False, 1, False),          # root != finisher, no clients
    ("A", [1, 1, 1, 1, 1, 0, 0, 0], "allreduce", 0, 16, False, 1, False),
    ("C", [1, 1, 1, 1, 1, 0, 0, 0], "reduce", 2, 1, True, 1, False),
]


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("name,counts,final,root,nchunks,weighted,rounds,single", CASES)
def test_dist_chain16_hip_backend(monkeypatch, name, counts, final, root, nchunks, weighted,
                                  rounds, single, dtype):
    W, n = len(counts), sum(counts)
    assert W <= 8
    loop = LoopDist(W, timeout=30.0)
    monkeypatch.setattr(D, "dist", loop)
    lay = R.layout_of(name, dtype)
    data = [R.clients16(name, dtype, n, seed=51 + k) for k in range(rounds)]
    ws = [O.weights_from_sizes(np.arange(1, n + 1) * (3 + k) + 2 + k) if weighted else None
          for k in range(rounds)]

    def fn(rank):
        out32, out64 = _fill_out(lay, dtype)
        agg = D.ChainAggregator(lay, n, out32, out64, final=final, root=root, nchunks=nchunks,
                                counts=counts, native16=True)
        assert isinstance(agg.backend, D.HipChainBackend)
        assert agg.backend.elem == R.ELEM[dtype]
        assert agg.state.dtype == torch.float32
        assert agg.state.numel() == (4 if n >= 256 else 2) * agg.plane
        assert agg.stack32.dtype == agg.gather32.dtype == lay.float_dtype
        a = sum(counts[:rank])
        res = []
        for (bits, i64), w in zip(data, ws):
            o0, _ = _fill_out(lay, dtype)
            out32.copy_(o0)
            out64.fill_(-7)
            loc = [R.as_tensor(bits[k], dtype, DEV) for k in range(a, a + counts[rank])]
            l64 = [torch.from_numpy(i64[k].copy()).to(DEV) for k in range(a, a + counts[rank])]
            agg.step(loc, l64, None if w is None else w[a:a + counts[rank]])
            torch.cuda.synchronize()
            same = all(np.array_equal(R.bits_of(t), bits[a + j]) for j, t in enumerate(loc)) and \
                all(np.array_equal(t.cpu().numpy(), i64[a + j]) for j, t in enumerate(l64))
            res.append(dict(o16=R.bits_of(out32).copy(), o64=out64.cpu().numpy().copy(),
                            inputs=same))
            loop.barrier()
        return res

    res = run_ranks(W, fn, device=DEV)
    roots = set(range(W)) if final == "allreduce" else {root}
    for k, ((bits, i64), w) in enumerate(zip(data, ws)):
        exp, inside, e64 = (R.expected16(lay, dtype, bits, i64) if w is None
                            else K.expected16w(lay, dtype, bits, w, i64))
        one = _single_gpu(lay, dtype, bits, i64, w) if single and k == 0 else None
        for r in range(W):
            got = res[r][k]
            assert got["inputs"], (r, k, "client buckets changed")
            if r not in roots:
                assert (got["o16"] == R.FILL16).all() and (got["o64"] == -7).all(), (r, k)
                continue
            assert R.same16(got["o16"][inside], exp[inside], dtype), (r, k)
            if lay.i64_numel:
                assert np.array_equal(got["o64"][:lay.i64_numel], e64), (r, k)
            if one is not None:
                assert R.same16(got["o16"][inside], one[0][inside], dtype), (r, k, "1gpu")
                assert np.array_equal(got["o64"][:lay.i64_numel], one[1][:lay.i64_numel])


@pytest.mark.parametrize("dtype", list(R.DTYPES))
def test_aggregator_chain16_reports_the_chained_form(monkeypatch, dtype):
    """Aggregator(chain16=True): the chained form where the model picks it
    (2 ranks x 300 clients of layout B: 600 rows of every stripe would cross
    the link, against three state planes) and with weights; the default stays
    striped, and weights stay refused without the opt-in."""
    W, counts = 2, [300, 300]
    n = sum(counts)
    monkeypatch.setattr(D, "dist", LoopDist(W, timeout=30.0))
    lay = R.layout_of("B", dtype)
    bits, i64 = R.clients16("B", dtype, n, seed=77)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 3 + 2)
    assert D.exact_form(counts, lay, root_all=True, chain16=True) == "chained"
    assert D.exact_form(counts, lay, root_all=True) == "striped"
    assert D.exact_form([3, 2], lay, root_all=True, chain16=True) == "striped"

    def fn(rank):
        a = sum(counts[:rank])
        loc = [R.as_tensor(bits[k], dtype, DEV) for k in range(a, a + counts[rank])]
        l64 = [torch.from_numpy(i64[k].copy()).to(DEV) for k in range(a, a + counts[rank])]
        forms, outs = [], []
        for weights, chain16 in ((None, False), (None, True), (w[a:a + counts[rank]], True)):
            out32, out64 = _fill_out(lay, dtype)
            agg = D.Aggregator(lay, loc, l64, n, out32, out64, final="allreduce", counts=counts,
                               weights=weights, native=False, chain16=chain16)
            agg.step()
            torch.cuda.synchronize()
            forms.append(agg.form)
            outs.append((R.bits_of(out32).copy(), out64.cpu().numpy().copy()))
        with pytest.raises(ValueError, match="weighted rounds on 16-bit buckets"):
            D.Aggregator(lay, loc, l64, n, out32, out64, counts=counts, native=False,
                         weights=w[a:a + counts[rank]])
        return forms, outs

    res = run_ranks(W, fn, device=DEV)
    exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
    expw = K.expected16w(lay, dtype, bits, w, i64)[0]
    for r in range(W):
        forms, outs = res[r]
        assert forms == ["striped/torch.distributed", "chained/torch.distributed",
                         "chained/torch.distributed"], forms
        for (o16, o64), want in zip(outs, (exp, exp, expw)):
            assert R.same16(o16[inside], want[inside], dtype), r
            assert np.array_equal(o64[:lay.i64_numel], e64), r
