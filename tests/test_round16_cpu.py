"""The striped multi-GPU round on fp16 / bf16 buckets, without a GPU: the
16-bit schedules (fa_describe_round_elem) and cost model (fa_round_model_elem)
of libfedagg_comm.so (host only: the library has no 16-bit executor), every
rank's schedule replayed together on uint16 buffers (tests/round16.Sim16), and
feddct_amd/dist.py's StripedAggregator on
native 16-bit layouts over the in-process torch.distributed stand-in
(tests/distloop.py) with an oracle arithmetic backend.

Layouts: tests/test_distloop_cpu.MANS A / B / C cast to each 16-bit dtype
(``BucketLayout(native16=True)``) and a raw segment list (an offset that is no
multiple of 8, a 5-element key, a bucket length of residue 5 modulo 8).
Every expectation is the oracle's ``torch_mean0`` over the widened values of a
whole key, rounded once to the 16-bit type."""
import ctypes

import numpy as np
import pytest
import torch

import feddct_amd.dist as D
import round16 as R
from distloop import LoopDist, run_ranks
from feddct_amd import _lib
from feddct_amd import comm as C
from feddct_amd.partition import layout_tiles
from test_distloop_cpu import MANS, fresh_out

DTYPE_NAMES = ("float16", "bfloat16")
STRIPED = C.FA_MODE_STRIPED


@pytest.fixture(autouse=True)
def _elem_entries():
    """A library or a comm.py without the 16-bit round fails here, at symbol
    lookup, not by cutting a 16-bit layout as if it held floats."""
    assert C.lib().fa_describe_round_elem and C.lib().fa_round_model_elem
    assert hasattr(D, "refuse_native16")


def _counts(n, world):
    return D.shard_counts(n, world)


def _scheds(lay, counts, nchunks, root):
    return [C.describe(STRIPED, lay, counts, r, nchunks=nchunks, root=root)
            for r in range(len(counts))]


# ---------------------------------------------------------------- schedules --
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", R.LAYOUTS)
def test_schedules_tile_the_bucket_and_pair_up(name, dtype):
    """W = 1..8, every rank: the stripes' chunks tile [0, f32_numel) in 16-bit
    elements, every cut is a multiple of 128 elements or the bucket's end, per
    ordered pair of ranks the sends match the receives in posting order and
    count, and each K_STRIPE follows the step that delivered its rows."""
    lay = R.layout_of(name, dtype)
    F = lay.f32_numel
    for W in range(1, 9):
        for n, nchunks, root in ((5, 3, -1), (20, 4, W - 1), (300, 1, 0)):
            counts = _counts(n, W)
            sch = _scheds(lay, counts, nchunks, root)
            chunks = sorted({(x["offset"], x["count"]) for s in sch for x in s
                             if x["op"] == "K_STRIPE"})
            pos = 0
            for off, cnt in chunks:
                assert off == pos and cnt > 0, (W, chunks)
                assert off % 128 == 0, (W, off)
                pos = off + cnt
            assert pos == F, (W, pos, F)
            for a in range(W):
                for b in range(W):
                    if a == b:
                        continue
                    sends = [(x["offset"], x["count"]) for x in sch[a]
                             if x["op"] == "SEND" and x["peer"] == b]
                    recvs = [(x["offset"], x["count"]) for x in sch[b]
                             if x["op"] == "RECV" and x["peer"] == a]
                    assert sends == recvs, (W, a, b)
            for r, s in enumerate(sch):
                for x in s:
                    if x["op"] != "K_STRIPE":
                        continue
                    rows = [y for y in s if y["op"] == "RECV" and y["dst"] == "RECV"
                            and y["offset"] == x["offset"]]
                    assert len(rows) == n - counts[r], (W, r, x)
                    assert all(y["step"] < x["step"] and y["count"] == x["count"] for y in rows)


CASES = [  # layout, W, N or counts, nchunks, root
    ("A", 2, 5, 3, -1), ("A", 3, 20, 4, 2), ("A", 8, 5, 1, 4), ("A", 8, 300, 3, -1),
    ("B", 2, 20, 4, 0), ("B", 3, 300, 1, -1), ("B", 8, 20, 4, 7), ("B", 8, [4, 3, 0, 5, 0, 1, 6, 1], 3, 0),
    ("C", 3, 5, 4, 0), ("C", 8, 20, 3, -1), ("raw", 2, 300, 4, 1), ("raw", 3, 20, 3, -1),
    ("raw", 8, 5, 1, 0), ("A", 1, 20, 4, 0), ("raw", 3, [7, 0, 13], 4, 2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_replayed_round_is_the_single_bucket_result(case):
    """All ranks' schedules replayed on uint16 buffers: every result rank holds
    the single-bucket expectation bit for bit, int64 keys included; the other
    ranks' result buckets keep their fill."""
    name, W, n, nchunks, root = case
    counts = list(n) if isinstance(n, list) else _counts(n, W)
    n = sum(counts)
    for dtype in DTYPE_NAMES:
        lay = R.layout_of(name, dtype)
        bits, i64 = R.clients16(name, dtype, n, seed=W + nchunks)
        exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
        _, tiles = layout_tiles(lay)
        sim = R.Sim16(lay, dtype, tiles, counts, list(bits), list(i64[:, :max(1, lay.i64_numel)]))
        bufs = sim.run(_scheds(lay, counts, nchunks, root))
        for r in range(W):
            out = bufs[r]["OUT"]
            if root < 0 or root == r:
                assert R.same16(out[inside], exp[inside], dtype), (case, dtype, r)
                if lay.i64_numel:
                    assert np.array_equal(bufs[r]["OUT64"][:lay.i64_numel], e64), (case, dtype, r)
            else:
                assert (out == R.FILL16).all() and (bufs[r]["OUT64"] == -7).all(), (case, r)


def _raw_describe(entry, lay, counts, rank, nchunks, root, weighted, mode, tail):
    n = ctypes.c_int()
    args = (mode, len(counts), rank, C._counts(counts), *C._layout_args(lay), nchunks, 0,
            _lib.FA_PLAN_GAPS_ARE_PADDING, root, weighted)
    rc = entry(*args, None, 0, ctypes.byref(n), *tail)
    if rc:
        return rc, None
    arr = (C.FaXfer * max(1, n.value))()
    rc = entry(*args, arr, n.value, ctypes.byref(n), *tail)
    return rc, bytes(arr)[:n.value * ctypes.sizeof(C.FaXfer)]


@pytest.mark.parametrize("mode", [C.FA_MODE_SHARDED, STRIPED, C.FA_MODE_CHAINED,
                                  C.FA_MODE_BLOCKED])
def test_elem_f32_is_the_fp32_entry(mode):
    """elem = FA_ELEM_F32 returns fa_describe_round's ops and fa_round_model's
    cost, for every form, weighted too."""
    lib = C.lib()
    lay = R.fp32_layout_of("B")
    counts = [9, 8, 0, 7]
    for weighted in (0, 1):
        for rank in range(4):
            a = _raw_describe(lib.fa_describe_round, lay, counts, rank, 3, 1, weighted, mode, ())
            b = _raw_describe(lib.fa_describe_round_elem, lay, counts, rank, 3, 1, weighted, mode,
                              (_lib.FA_ELEM_F32,))
            assert a[0] == 0 and a == b
        ca, cb = C.FaRoundCost(), C.FaRoundCost()
        args = (mode, 4, C._counts(counts), *C._layout_args(lay), 3, 0,
                _lib.FA_PLAN_GAPS_ARE_PADDING, 1, weighted)
        assert lib.fa_round_model(*args, ctypes.byref(ca)) == 0
        assert lib.fa_round_model_elem(*args, ctypes.byref(cb), _lib.FA_ELEM_F32) == 0
        assert bytes(ca) == bytes(cb)


# -------------------------------------------------------------------- model --
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_link_bytes_halve_on_layout_c(dtype):
    """Layout C has no int64 key and every key is a multiple of 128 elements,
    so the fp32 and 16-bit cuts coincide: the 16-bit round's largest link byte
    count is exactly half the fp32 round's, groups and steps are equal."""
    l16, l32 = R.layout_of("C", dtype), R.fp32_layout_of("C")
    assert l16.f32_numel == l32.f32_numel and not l16.i64_numel
    for counts, nchunks, root in (([3, 2], 4, 0), ([7, 7, 6], 3, -1), ([1, 1, 1, 1, 1, 0, 0, 0], 1, 4),
                                  (_counts(300, 8), 4, 7)):
        a = C.round_model(STRIPED, l32, counts, nchunks, root=root)
        b = C.round_model(STRIPED, l16, counts, nchunks, root=root)
        assert a["link_bytes_max"] > 0
        assert b["link_bytes_max"] * 2 == a["link_bytes_max"], (counts, a, b)
        assert (a["groups"], a["steps"]) == (b["groups"], b["steps"])
        assert b["hbm_bytes_max"] * 2 == a["hbm_bytes_max"]
        assert b["model_us"] <= a["model_us"]
    one32 = C.round_model(STRIPED, l32, [5], 1, root=0)
    one16 = C.round_model(STRIPED, l16, [5], 1, root=0)
    assert one16["hbm_bytes_max"] * 2 == one32["hbm_bytes_max"]


# ---------------------------------------------------------------- refusals --
@pytest.mark.parametrize("elem", [_lib.FA_ELEM_F16, _lib.FA_ELEM_BF16])
def test_elem_entries_refuse_other_forms_and_weights(elem):
    lib = C.lib()
    lay = R.layout_of("A", "float16" if elem == _lib.FA_ELEM_F16 else "bfloat16")
    counts = [3, 2]
    head = (2, C._counts(counts), *C._layout_args(lay), 2, 0, _lib.FA_PLAN_GAPS_ARE_PADDING, 0)
    cost, n = C.FaRoundCost(), ctypes.c_int()
    for mode in (C.FA_MODE_SHARDED, C.FA_MODE_CHAINED, C.FA_MODE_BLOCKED):
        assert lib.fa_round_model_elem(mode, *head, 0, ctypes.byref(cost), elem) == _lib.FA_E_INVAL
        assert b"striped" in _lib.lib.fa_last_error()
        assert lib.fa_describe_round_elem(mode, 2, 0, *head[1:], 0, None, 0, ctypes.byref(n),
                                          elem) == _lib.FA_E_INVAL
        assert b"striped" in _lib.lib.fa_last_error()
    assert lib.fa_round_model_elem(STRIPED, *head, 1, ctypes.byref(cost), elem) == _lib.FA_E_INVAL
    assert b"weighted" in _lib.lib.fa_last_error()
    assert _lib.lib.fa_last_error().startswith(b"fa_round_model_elem:")   # the entry called
    assert lib.fa_round_model_elem(STRIPED, *head, 0, None, elem) == _lib.FA_E_INVAL
    assert _lib.lib.fa_last_error().startswith(b"fa_round_model_elem: out is NULL")
    assert lib.fa_describe_round_elem(STRIPED, 2, 0, *head[1:], 0, None, 0, None,
                                      elem) == _lib.FA_E_INVAL
    assert _lib.lib.fa_last_error().startswith(b"fa_describe_round_elem: nops is NULL")
    assert lib.fa_describe_round_elem(STRIPED, 2, 0, *head[1:], 1, None, 0, ctypes.byref(n),
                                      elem) == _lib.FA_E_INVAL
    assert b"weighted" in _lib.lib.fa_last_error()
    assert lib.fa_round_model_elem(STRIPED, *head, 0, ctypes.byref(cost), 7) == _lib.FA_E_INVAL
    assert lib.fa_round_model_elem(STRIPED, *head, 0, ctypes.byref(cost), elem) == 0
    with pytest.raises(_lib.FedaggError, match="weighted"):
        C.round_model(STRIPED, lay, counts, 2, weighted=True)
    with pytest.raises(_lib.FedaggError, match="striped"):
        C.describe(C.FA_MODE_CHAINED, lay, counts, 0)


# ------------------------------------------------- dist.py over the stand-in --
def _loop(monkeypatch, world):
    loop = LoopDist(world, timeout=60.0)
    monkeypatch.setattr(D, "dist", loop)
    return loop


def _out16(lay, dtype):
    o32 = R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype)
    return o32, torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64)


@pytest.mark.parametrize("name,world,n,host,final,nchunks,root", [
    ("A", 1, 5, False, "reduce", 4, 0), ("A", 2, 20, False, "allreduce", 4, 0),
    ("B", 3, 20, False, "reduce", 3, 2), ("B", 8, 5, False, "reduce", 1, 4),
    ("raw", 8, 20, False, "allreduce", 3, 0), ("C", 3, 5, True, "allreduce", 4, 0),
    ("A", 8, 20, True, "reduce", 3, 6), ("raw", 2, 300, True, "allreduce", 1, 0),
    ("B", 2, 300, False, "reduce", 4, 1), ("B", 1, 20, True, "allreduce", 3, 0)])
def test_striped_aggregator_native16_loop(monkeypatch, name, world, n, host, final, nchunks,
                                          root):
    """dist.StripedAggregator on native 16-bit layouts through step_device and
    step_host, two rounds on one aggregator with fresh data."""
    _loop(monkeypatch, world)
    for dtype in DTYPE_NAMES:
        lay = R.layout_of(name, dtype)
        rounds = [R.clients16(name, dtype, n, seed=11 + k) for k in range(2)]

        def fn(rank):
            out32, out64 = _out16(lay, dtype)
            agg = D.StripedAggregator(lay, n, out32, out64,
                                      backend=R.OracleStripeBackend16(lay, dtype), final=final,
                                      root=root, nchunks=nchunks)
            assert agg.recv.dtype == lay.float_dtype and agg.recv.shape[1] % 8 == 0
            assert agg.lo % 128 == 0 or agg.lo == agg.hi == lay.f32_numel   # (an empty stripe)
            got = []
            for bits, i64 in rounds:
                out32.copy_(R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype))
                out64.fill_(-7)
                c64 = [torch.from_numpy(i64[k].copy()) for k in range(n)]
                if host:
                    agg.step_host([R.as_tensor(bits[k, agg.lo:agg.hi], dtype) for k in range(n)],
                                  c64)
                else:
                    a, b = agg.shards[rank]
                    agg.step_device([R.as_tensor(bits[k], dtype) for k in range(a, b)], c64[a:b])
                got.append((R.bits_of(out32).copy(), out64.numpy().copy()))
            return got

        res = run_ranks(world, fn)
        for k, (bits, i64) in enumerate(rounds):
            exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
            for r in range(world):
                o16, o64 = res[r][k]
                if final == "reduce" and r != root:
                    assert (o16 == R.FILL16).all() and (o64 == -7).all(), (dtype, k, r)
                else:
                    assert R.same16(o16[inside], exp[inside], dtype), (dtype, k, r)
                    if lay.i64_numel:
                        assert np.array_equal(o64[:lay.i64_numel], e64), (dtype, k, r)


def test_native16_refusals_and_choice(monkeypatch):
    """The TypeError / ValueError paths of the 16-bit round, the other
    aggregators' refusals, and Aggregator choosing the striped form."""
    world = 2
    _loop(monkeypatch, world)
    dtype = "float16"
    lay = R.layout_of("A", dtype)
    n = 5
    bits, i64 = R.clients16("A", dtype, n, seed=3)
    exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
    be = R.OracleStripeBackend16(lay, dtype)
    assert D.exact_form([3, 2], lay) == "striped"
    assert D.exact_form([40, 40], lay, root_all=True) == "striped"

    def fn(rank):
        a, b = D.shard_range(n, world, rank)
        loc = [R.as_tensor(bits[k], dtype) for k in range(a, b)]
        c64 = [torch.from_numpy(i64[k].copy()) for k in range(a, b)]
        out32, out64 = _out16(lay, dtype)
        f32out, _ = fresh_out(lay)
        with pytest.raises(TypeError, match="float32"):
            D.StripedAggregator(lay, n, f32out, out64, backend=be)
        agg = D.StripedAggregator(lay, n, out32, out64, backend=be, final="allreduce")
        with pytest.raises(TypeError, match="bfloat16"):
            agg.step_device([t.to(torch.bfloat16) for t in loc], c64)
        with pytest.raises(ValueError, match="weighted"):
            agg.step_device(loc, c64, weights=[0.5] * (b - a))
        with pytest.raises(TypeError, match="float32"):
            agg.step_host([t.float() for t in loc], c64)
        assert (R.bits_of(out32) == R.FILL16).all()        # nothing ran
        with pytest.raises(ValueError, match="striped round only"):
            D.ShardedAggregator(lay, loc, c64, n, out32, out64, backend=object())
        with pytest.raises(ValueError, match="striped round only"):
            D.ChainAggregator(lay, n, out32, out64, backend=object())
        with pytest.raises(ValueError, match="stripe_backend"):
            D.Aggregator(lay, loc, c64, n, out32, out64, backend=object())
        with pytest.raises(ValueError, match="weighted"):
            D.Aggregator(lay, loc, c64, n, out32, out64, stripe_backend=be,
                         weights=[0.5] * (b - a))
        with pytest.raises(ValueError, match="striped round only"):
            D.Aggregator(lay, loc, c64, n, out32, out64, exact=False, backend=object())
        top = D.Aggregator(lay, loc, c64, n, out32, out64, stripe_backend=be, final="allreduce")
        assert top.form == "striped/torch.distributed"
        top.step()
        return R.bits_of(out32).copy(), out64.numpy().copy()

    for o16, o64 in run_ranks(world, fn):
        assert R.same16(o16[inside], exp[inside], dtype)
        assert np.array_equal(o64[:lay.i64_numel], e64)


def test_native_wrappers_refuse_before_the_library(monkeypatch):
    """comm.py's aggregators run on fp32 buckets only: on a native 16-bit
    layout each raises ValueError before the library or the communicator is
    touched (the communicator here is a stub that fails on any use; they used
    to hand 16-bit buckets to fp32 kernels)."""
    class NoComm:
        def info(self):
            raise AssertionError("the communicator was used")

    dtype = "bfloat16"
    lay = R.layout_of("A", dtype)
    loc = [R.as_tensor(np.zeros(lay.f32_numel, np.uint16), dtype) for _ in range(3)]
    c64 = [torch.zeros(lay.i64_numel, dtype=torch.int64) for _ in range(3)]
    out32, out64 = _out16(lay, dtype)
    monkeypatch.setattr(C, "_clib", None)
    monkeypatch.setattr(C, "_load", lambda: (_ for _ in ()).throw(AssertionError("loaded")))
    for cls in (C.NativeShardedAggregator, C.NativeChainedAggregator, C.NativeBlockedAggregator,
                C.NativeStripedAggregator, C.NativeAggregator):
        with pytest.raises(ValueError, match="native rounds run on fp32 buckets"):
            cls(lay, loc, c64, 3, out32, out64, NoComm())
    assert (R.bits_of(out32) == R.FILL16).all()
