"""GPU: the 16-bit striped round over torch.distributed.

* comm.py's native aggregators run on fp32 buckets only: on a native 16-bit
  layout each raises, with the result bucket still holding its fill.
* feddct_amd/dist.py's StripedAggregator with its HipStripeBackend (16-bit
  tile-subset plans, client pointers moved back by 2 * base) at W = 1, 2, 3
  and 8 ranks over the in-process stand-in for torch.distributed
  (tests/distloop.py), N = 5, 20 and 300, through step_device and step_host
  with pinned 16-bit stripes, two rounds on one aggregator (cancellation-heavy
  data); one round each on the special values of tests/specials.py and on
  exact-sum data whose expected bits no summation order enters.  The receive
  matrix carries a sentinel in its row padding and in one guard row.  Results
  against the oracle (tests/round16.expected16); one case per W also against
  one GPU's 16-bit fa_reduce.

Every comparison is bit for bit, two NaNs equal; there is no tolerance."""
import numpy as np
import pytest
import torch

import feddct_amd.dist as D
import round16 as R
from distloop import LoopDist, run_ranks
from feddct_amd import _lib
from feddct_amd import comm as C
from feddct_amd.workload import Reducer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT16 = 0x5A3C        # (a finite value in both types)


@pytest.fixture(autouse=True)
def _elem_entries():
    """A library without the 16-bit round fails here, at symbol lookup, before
    anything could hand 16-bit buckets to fp32 kernels."""
    assert C.lib().fa_describe_round_elem and C.lib().fa_round_model_elem
    assert hasattr(D, "refuse_native16")


def _fill_out(lay, dtype):
    return (R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype, DEV),
            torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64, device=DEV))


def _single_gpu(lay, dtype, bits, i64):
    """One GPU's 16-bit fa_reduce over all clients."""
    n = len(bits)
    clients = [(R.as_tensor(bits[k], dtype, DEV), torch.from_numpy(i64[k].copy()).to(DEV))
               for k in range(n)]
    o32, o64 = _fill_out(lay, dtype)
    plan = _lib.Plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, elem=R.ELEM[dtype])
    Reducer(lay, clients, o32, o64, plan=plan)()
    torch.cuda.synchronize()
    return R.bits_of(o32).copy(), o64.cpu().numpy().copy()


def test_native_aggregators_refuse_16bit_layouts():
    """The native rounds run on fp32 buckets: every comm.py aggregator raises
    on a native 16-bit layout, with the result bucket still holding its fill."""
    torch.cuda.set_device(DEV)
    dtype, n = "bfloat16", 5
    lay = R.layout_of("A", dtype)
    bits, i64 = R.clients16("A", dtype, n, seed=9)
    loc = [R.as_tensor(bits[k], dtype, DEV) for k in range(n)]
    c64 = [torch.from_numpy(i64[k].copy()).to(DEV) for k in range(n)]
    o32, o64 = _fill_out(lay, dtype)
    comm = C.Comm.single()
    try:
        for cls in (C.NativeShardedAggregator, C.NativeChainedAggregator,
                    C.NativeBlockedAggregator, C.NativeStripedAggregator, C.NativeAggregator):
            with pytest.raises(ValueError, match="native rounds run on fp32 buckets"):
                cls(lay, loc, c64, n, o32, o64, comm)
        torch.cuda.synchronize()
        assert (R.bits_of(o32) == R.FILL16).all() and bool((o64 == -7).all())
    finally:
        comm.close()


# ------------------------------------- dist.py with HipStripeBackend, W ranks --
def _guard_recv(agg, dtype):
    """One guard row behind the receive matrix; the row padding [L, lpad) and
    the guard row hold a sentinel (tests/test_gpu_dist_loopback._guard_recv)."""
    n, pitch = agg.recv.shape
    full = R.as_tensor(np.zeros((n + 1) * pitch, np.uint16), dtype, DEV).view(n + 1, pitch)
    sent = R.as_tensor(np.array([SENT16], np.uint16), dtype, DEV)[0]
    L = agg.hi - agg.lo
    full[:, L:] = sent
    full[n] = sent
    agg.recv = full[:n]
    return full, L


def _guard_ok(guard):
    full, L = guard
    n = full.shape[0] - 1
    b = full.view(torch.int16)
    s = np.array([SENT16], np.uint16).view(np.int16)[0].item()
    return bool((b[n] == s).all()) and bool((b[:n, L:] == s).all())


DIST_CASES = [
    # name, W, n, host, final, root, nchunks, counts, single
    ("A", 1, 20, False, "allreduce", 0, 4, None, True),
    ("B", 1, 5, True, "reduce", 0, 3, None, False),
    ("B", 2, 20, False, "allreduce", 0, 1, None, True),
    ("raw", 2, 300, False, "reduce", 1, 4, None, False),
    ("A", 2, 5, True, "reduce", 0, 3, None, False),
    ("B", 3, 20, False, "reduce", 2, 3, [9, 0, 11], True),
    ("C", 3, 300, True, "allreduce", 0, 4, None, False),
    ("raw", 3, 5, False, "allreduce", 0, 1, None, False),
    ("B", 8, 20, False, "reduce", 7, 4, [2, 0, 3, 1, 0, 4, 2, 8], True),
    ("A", 8, 5, False, "allreduce", 0, 3, None, False),
    ("B", 8, 300, False, "reduce", 0, 1, None, False),
    ("raw", 8, 20, True, "allreduce", 0, 4, None, False),
]


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("name,W,n,host,final,root,nchunks,counts,single", DIST_CASES)
def test_dist_striped_hip_backend(monkeypatch, name, W, n, host, final, root, nchunks, counts,
                                  single, dtype):
    loop = LoopDist(W, timeout=30.0)
    monkeypatch.setattr(D, "dist", loop)
    lay = R.layout_of(name, dtype)
    rounds = [R.clients16(name, dtype, n, seed=21 + k) for k in range(2)]

    def fn(rank):
        out32, out64 = _fill_out(lay, dtype)
        agg = D.StripedAggregator(lay, n, out32, out64, final=final, root=root, nchunks=nchunks,
                                  counts=counts)
        assert isinstance(agg.backend, D.HipStripeBackend) and agg.backend.esize == 2
        assert agg.recv.dtype == lay.float_dtype
        guard = _guard_recv(agg, dtype)
        a, b = agg.shards[rank]
        res = []
        for bits, i64 in rounds:
            out32.copy_(R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype, DEV))
            out64.fill_(-7)
            if host:
                st = [R.as_tensor(bits[k, agg.lo:agg.hi], dtype).pin_memory() for k in range(n)]
                agg.step_host(st, [torch.from_numpy(i64[k].copy()).pin_memory() for k in range(n)])
                same = True
            else:
                loc = [R.as_tensor(bits[k], dtype, DEV) for k in range(a, b)]
                agg.step_device(loc, [torch.from_numpy(i64[k].copy()).to(DEV)
                                      for k in range(a, b)])
                torch.cuda.synchronize()
                same = all(np.array_equal(R.bits_of(t), bits[a + j]) for j, t in enumerate(loc))
            torch.cuda.synchronize()
            res.append(dict(o16=R.bits_of(out32).copy(), o64=out64.cpu().numpy().copy(),
                            guard=_guard_ok(guard), inputs=same))
        return res

    res = run_ranks(W, fn, device=DEV)
    roots = set(range(W)) if final == "allreduce" else {root}
    for k, (bits, i64) in enumerate(rounds):
        exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
        one = _single_gpu(lay, dtype, bits, i64) if single and k == 0 else None
        for r in range(W):
            got = res[r][k]
            assert got["guard"], (r, k, "receive matrix padding / guard row written")
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


def _run_device_round(monkeypatch, lay, dtype, bits, W, final, root, nchunks, counts=None):
    """One step_device round of ``bits[n, numel]`` (no int64 data beyond zeros)
    at W ranks; returns every rank's result bits."""
    n = len(bits)
    monkeypatch.setattr(D, "dist", LoopDist(W, timeout=30.0))

    def fn(rank):
        out32, out64 = _fill_out(lay, dtype)
        agg = D.StripedAggregator(lay, n, out32, out64, final=final, root=root, nchunks=nchunks,
                                  counts=counts)
        assert agg.backend.esize == 2
        a, b = agg.shards[rank]
        z64 = [torch.zeros(max(1, lay.i64_numel), dtype=torch.int64, device=DEV)
               for _ in range(a, b)]
        agg.step_device([R.as_tensor(bits[k], dtype, DEV) for k in range(a, b)], z64)
        torch.cuda.synchronize()
        return R.bits_of(out32).copy()

    return run_ranks(W, fn, device=DEV)


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("W,n,final,root,nchunks,counts", [
    (2, 20, "allreduce", 0, 3, None), (8, 5, "reduce", 4, 1, None),
    (3, 300, "reduce", 2, 4, [150, 0, 150])])
def test_dist_striped_special_values(monkeypatch, W, n, final, root, nchunks, counts, dtype):
    """tests/specials.py's columns (-0, subnormals, inf, NaN, overflowing sums,
    inf - inf) cast to 16 bits, through every column rule of the raw layout."""
    import specials
    lay = R.SpecialLayout(dtype)
    with np.errstate(all="ignore"):
        bits = R.narrow(specials.fill(n, seed=3), dtype)
    exp, inside, _ = R.expected16(lay, dtype, bits)
    res = _run_device_round(monkeypatch, lay, dtype, bits, W, final, root, nchunks, counts)
    for r in (range(W) if final == "allreduce" else [root]):
        assert R.same16(res[r][inside], exp[inside], dtype), r


@pytest.mark.parametrize("dtype", list(R.DTYPES))
@pytest.mark.parametrize("name,W,n,final,root,nchunks", [
    ("B", 8, 20, "allreduce", 0, 4), ("raw", 3, 300, "reduce", 1, 3), ("A", 2, 5, "reduce", 0, 1)])
def test_dist_striped_exact_sum_data(monkeypatch, name, W, n, final, root, nchunks, dtype):
    """Rows whose fp32 sums are exact (tests/h16ref.exact_sum_data): expected
    bits that no summation order and no oracle enters (a float64 sum, one
    division, one rounding)."""
    import h16ref
    lay = R.layout_of(name, dtype)
    bits, _ = h16ref.exact_sum_data(dtype, n, lay.f32_numel, seed=100 + n)
    res = _run_device_round(monkeypatch, lay, dtype, bits, W, final, root, nchunks)
    for r in (range(W) if final == "allreduce" else [root]):
        for o, m in lay.segs32:
            o, m = int(o), int(m)
            pat, nan = h16ref.exact_mean(bits[:, o:o + m], dtype)
            assert not nan.any()
            assert np.array_equal(res[r][o:o + m], pat), (r, o)
