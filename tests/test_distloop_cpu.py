"""The in-process stand-in for torch.distributed (tests/distloop.py) checked
against what is already known: feddct_amd/dist.py's rounds on CPU tensors
with the oracle backends of tests/test_dist_gloo.py, W ranks as W threads.
The cases are those the gloo tests run over real torch.distributed
(test_sharded_round_gloo, test_striped_round_is_exact_gloo,
test_chained_round_is_exact_gloo), plus W = 8 and ranks without clients.

Every result rank must hold the oracle's bits (O.aggregate_state,
O.weighted_sum0, O.mean_i64_trunc); for the re-associated e1 round the
ascending-rank-order fp32 sum of the per-rank oracle partials, divided by N
in fp32 (the stand-in's documented SUM order).  The stand-in gives the answers
real gloo gives, so tests/test_gpu_dist_loopback.py may run the HIP backends
over it.

The helpers below (layouts, client buckets, expectations, the bit compare)
are shared with tests/test_gpu_dist_loopback.py."""
import functools

import numpy as np
import pytest
import torch

import feddct_amd.dist as D
from distloop import LoopDist, LoopError, run_ranks
from feddct_amd import synth
from feddct_amd.dist import (ChainAggregator, ShardedAggregator, StripedAggregator,
                             chunk_segments, shard_range)
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import chain_cut
from oracle import torch_order as O
from test_dist_gloo import (MAN, OracleBackend, OracleChainBackend, OracleStripeBackend,
                            _bucket)


def _man(f32, i64=()):
    return {"keys": [{"key": f"k{j}", "shape": [m], "dtype": "float32"}
                     for j, m in enumerate(f32)]
            + [{"key": f"n{j}", "shape": list(s), "dtype": "int64"} for j, s in enumerate(i64)]}


# A: test_dist_gloo.MAN.  B: enough vector tiles for 8 non-empty stripes.
# C: vector tiles only - no scalar column (T == 0), no int64 key.
MANS = {"A": MAN,
        "B": _man([3 * 2048 + 40, 4097, 33, 1, 7, 2049, 8193, 5], [(), (5,)]),
        "C": _man([2048, 4096])}
FRESH = 1000    # client ids of a second round's fresh data: FRESH + slot


@functools.lru_cache(maxsize=None)
def layout_of(name):
    return BucketLayout.from_manifest(MANS[name])


@functools.lru_cache(maxsize=None)
def _state(name, client):
    return synth.gen_state(MANS[name], client, synth.MODE_ADVERSARIAL)


@functools.lru_cache(maxsize=None)
def cpu_bucket(name, client):
    """Client ``client``'s (fp32, int64) buckets, placed as test_dist_gloo._bucket
    places them.  Shared: clone before use."""
    return _bucket(layout_of(name), _state(name, client))


def clients_on(name, ids, device="cpu"):
    out = []
    for c in ids:
        f32, i64 = cpu_bucket(name, c)
        out.append((f32.clone().to(device), i64.clone().to(device)))
    return out


def sizes_weights(n, salt=0):
    """n_total fp32 weights (O.weights_from_sizes); ``salt`` varies them."""
    return O.weights_from_sizes(np.arange(1, n + 1) * (3 + salt) + 2 + salt)


@functools.lru_cache(maxsize=None)
def expected_exact(name, ids, weighted=False, salt=0):
    """{key: the single-process reference's result} over client ids ``ids``."""
    states = [_state(name, c) for c in ids]
    if not weighted:
        return dict(O.aggregate_state(states))
    w = sizes_weights(len(ids), salt)
    exact = {}
    for j, (k, _) in enumerate(states[0]):
        x = np.stack([np.asarray(st[j][1]) for st in states])
        exact[k] = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)
    return exact


@functools.lru_cache(maxsize=None)
def expected_e1(name, ids, world):
    """The e1 round under the stand-in's SUM: per rank the oracle's torch-order
    sum of its shard (O.torch_sum0), the partials added in ascending rank
    order in fp32, then / N in fp32; int64 keys exact over all clients."""
    n = len(ids)
    states = [_state(name, c) for c in ids]
    exact = {}
    for j, (k, _) in enumerate(states[0]):
        x = np.stack([np.asarray(st[j][1]).reshape(-1) for st in states])
        if x.dtype == np.int64:
            exact[k] = O.mean_i64_trunc(x)
            continue
        tot = None
        for r in range(world):
            a, b = shard_range(n, world, r)
            part = O.torch_sum0(x[a:b]).astype(np.float32)
            tot = part if tot is None else (tot + part).astype(np.float32)
        exact[k] = (tot / np.float32(n)).astype(np.float32)
    return exact


def same_bits(got, want):
    """Bit for bit, NaNs compared as NaNs."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and got[~gn].tobytes() == want[~wn].tobytes()


def assert_state(layout, o32, o64, exact, tag):
    """Every key's elements of the result buckets equal ``exact``'s."""
    o32, o64 = o32.cpu().numpy(), o64.cpu().numpy()
    for s in layout.slots:
        src = o64 if s.kind == "i64" else o32
        assert same_bits(src[s.offset:s.offset + s.numel], np.asarray(exact[s.key])), (tag, s.key)


def assert_untouched(o32, o64, tag):
    """A rank that is no result rank keeps its fill (NaN / -7)."""
    assert bool(torch.isnan(o32).all()), (tag, "out32 written on a non-result rank")
    assert bool((o64 == -7).all()), (tag, "out64 written on a non-result rank")


def fresh_out(layout, device="cpu"):
    return (torch.full((layout.f32_numel,), float("nan"), device=device),
            torch.full((max(1, layout.i64_numel),), -7, dtype=torch.int64, device=device))


def _loop(monkeypatch, world):
    loop = LoopDist(world, timeout=60.0)
    monkeypatch.setattr(D, "dist", loop)
    return loop


# ----------------------------------------------------------- the stand-in --
def test_sum_is_ascending_rank_order_fp32(monkeypatch):
    """reduce / all_reduce / reduce_scatter_tensor add ((p0 + p1) + p2) + p3 in
    fp32, on values where every other association differs."""
    W = 4
    loop = _loop(monkeypatch, W)
    vals = np.array([[1e8, 3.0], [1.0, 2.0 ** -24], [-1e8, 1.0], [1.0, 2.0 ** -24]], np.float32)
    want = vals[0]
    for r in range(1, W):
        want = (want + vals[r]).astype(np.float32)
    assert not np.array_equal(want, (vals[0] + vals[2]) + (vals[1] + vals[3]))

    def fn(rank):
        mine = torch.from_numpy(np.tile(vals[rank], W))       # W shares of 2
        a = mine.clone()
        loop.all_reduce(a, op=loop.ReduceOp.SUM)
        b = mine.clone()
        loop.reduce(b, dst=2, op=loop.ReduceOp.SUM, async_op=True).wait()
        c = torch.zeros(2)
        loop.reduce_scatter_tensor(c, mine, op=loop.ReduceOp.SUM)
        return a.numpy(), b.numpy(), c.numpy()

    for r, (a, b, c) in enumerate(run_ranks(W, fn)):
        assert same_bits(a, np.tile(want, W))
        assert same_bits(b, np.tile(want if r == 2 else vals[r], W))   # only dst is written
        assert same_bits(c, want)


def test_messages_match_per_pair_in_posting_order(monkeypatch):
    """The k-th receive posted for a (source, destination) pair takes the
    pair's k-th send whatever the wait order, pairs do not mix, and a send
    hands over a copy; gather / all_gather / broadcast place by rank."""
    W = 3
    loop = _loop(monkeypatch, W)

    def fn(rank):
        got = {}
        if rank == 0:
            for dst in (1, 2):
                t = torch.tensor([10.0 * dst])
                for k in range(3):
                    loop.isend(t + k, dst).wait()
                    t += 100                      # after the send: must not be seen
        else:
            bufs = [torch.zeros(1) for _ in range(3)]
            reqs = loop.batch_isend_irecv([loop.P2POp(loop.irecv, b, 0) for b in bufs])
            for q in reversed(reqs):
                q.wait()
            got["p2p"] = [float(b) for b in bufs]
        allg = torch.zeros(W, 2)
        loop.all_gather_into_tensor(allg, torch.full((2,), float(rank)))
        lst = [torch.zeros(1) for _ in range(W)] if rank == 1 else None
        loop.gather(torch.tensor([float(rank + 5)]), lst, dst=1, async_op=True).wait()
        bc = torch.tensor([float(rank)])
        loop.broadcast(bc, src=2)
        loop.barrier()
        got.update(allg=allg.tolist(), gather=lst and [float(x) for x in lst], bc=float(bc))
        return got

    res = run_ranks(W, fn)
    for r in (1, 2):
        assert res[r]["p2p"] == [10.0 * r, 10.0 * r + 101, 10.0 * r + 202]
    for r in range(W):
        assert res[r]["allg"] == [[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]
        assert res[r]["bc"] == 2.0
        assert res[r]["gather"] == ([5.0, 6.0, 7.0] if r == 1 else None)
    assert loop.get_backend() not in ("gloo",) and "nccl" not in loop.get_backend()


def test_one_rank_failing_ends_the_others_at_once(monkeypatch):
    """The first exception is re-raised by run_ranks, and a rank blocked in a
    wait raises instead of waiting for its 60 s limit; a wrong-sized message is
    an error, not a broadcasting copy."""
    loop = _loop(monkeypatch, 2)
    seen = []

    def fn(rank):
        if rank == 0:
            raise KeyError("rank 0 gives up")
        try:
            loop.irecv(torch.zeros(4), 0).wait()
        except LoopError as e:
            seen.append(str(e))
            raise

    with pytest.raises(KeyError, match="gives up"):
        run_ranks(2, fn)
    assert len(seen) == 1 and "another rank failed" in seen[0]

    loop = _loop(monkeypatch, 2)

    def sizes(rank):
        if rank == 0:
            loop.isend(torch.zeros(1), 1).wait()
        else:
            loop.irecv(torch.zeros(4), 0).wait()

    with pytest.raises(LoopError, match="posted receive"):
        run_ranks(2, sizes)


# ------------------------------------------------------------- the rounds --
@pytest.mark.parametrize("world,n_total,final,exchange,nchunks", [
    (2, 20, "allreduce", "reduce", 3), (3, 7, "allreduce", "reduce", 3),
    (2, 20, "reduce", "reduce", 3), (3, 7, "reduce", "reduce", 3),
    (2, 20, "reduce", "rs_gather", 3), (3, 7, "allreduce", "rs_gather", 3),
    (3, 7, "reduce", "rs_gather", 3), (8, 20, "reduce", "rs_gather", 3),
    (8, 9, "allreduce", "reduce", 3), (3, 7, "reduce", "rs_gather", 120)])
def test_sharded_round_loop(monkeypatch, world, n_total, final, exchange, nchunks):
    """test_sharded_round_gloo's cases (and W = 8): the stand-in's cross-rank
    sum is exactly the ascending-rank-order fp32 sum of the oracle partials.
    With 120 chunks the 4096-float key is a chunk of its own, whose last
    4096 % 3 floats take rs_gather's plain reduce."""
    _loop(monkeypatch, world)
    layout = layout_of("A")
    chunks = chunk_segments(layout, nchunks)

    def fn(rank):
        lo, hi = shard_range(n_total, world, rank)
        bk = clients_on("A", range(lo, hi))
        out32, out64 = fresh_out(layout)
        agg = ShardedAggregator(layout, [b[0] for b in bk], [b[1] for b in bk], n_total, out32,
                                out64, nchunks=nchunks, backend=OracleBackend(layout, chunks),
                                final=final, exchange=exchange)
        agg.step()
        return out32, out64

    want = expected_e1("A", tuple(range(n_total)), world)
    for r, (o32, o64) in enumerate(run_ranks(world, fn)):
        if final == "reduce" and r != 0:
            assert_untouched(o32, o64, r)
        else:
            assert_state(layout, o32, o64, want, r)


@pytest.mark.parametrize("world,n_total,host,final,weighted,nchunks,root", [
    (2, 20, False, "allreduce", False, 4, 0), (3, 7, False, "allreduce", False, 2, 0),
    (2, 9, True, "allreduce", False, 4, 0), (3, 7, False, "reduce", False, 1, 0),
    (3, 8, False, "reduce", True, 3, 0), (2, 5, False, "allreduce", True, 4, 0),
    (8, 5, False, "reduce", True, 2, 6), (8, 9, True, "allreduce", False, 3, 0)])
def test_striped_round_is_exact_loop(monkeypatch, world, n_total, host, final, weighted, nchunks,
                                     root):
    """test_striped_round_is_exact_gloo's cases, plus W = 8 with ranks that hold
    no clients (5 slots) and W = 8 host ingress."""
    _loop(monkeypatch, world)
    layout = layout_of("A")
    w = sizes_weights(n_total) if weighted else None

    def fn(rank):
        out32, out64 = fresh_out(layout)
        agg = StripedAggregator(layout, n_total, out32, out64,
                                backend=OracleStripeBackend(layout), final=final, root=root,
                                nchunks=nchunks)
        if host:
            allb = clients_on("A", range(n_total))
            agg.step_host([b[0][agg.lo:agg.hi].clone() for b in allb], [b[1] for b in allb])
        else:
            a, b = shard_range(n_total, world, rank)
            bk = clients_on("A", range(a, b))
            agg.step_device([x[0] for x in bk], [x[1] for x in bk],
                            None if w is None else w[a:b])
        return out32, out64

    want = expected_exact("A", tuple(range(n_total)), weighted)
    for r, (o32, o64) in enumerate(run_ranks(world, fn)):
        if final == "reduce" and r != root:
            assert_untouched(o32, o64, r)
        else:
            assert_state(layout, o32, o64, want, r)


@pytest.mark.parametrize("counts,final,weighted,root", [
    ([10, 10], "reduce", False, 0), ([3, 4, 2], "allreduce", False, 0),
    ([0, 6, 3], "reduce", False, 0), ([5, 17], "allreduce", True, 0),
    ([9, 0, 8], "reduce", True, 0), ([2, 0, 3, 1, 0, 4, 2, 0], "reduce", True, 3),
    ([0, 0, 1, 1, 1, 1, 1, 0], "allreduce", False, 0)])
def test_chained_round_is_exact_loop(monkeypatch, counts, final, weighted, root):
    """test_chained_round_is_exact_gloo's cases, plus W = 8 with ranks without
    clients first, in the middle and last."""
    world, n = len(counts), sum(counts)
    _loop(monkeypatch, world)
    layout = layout_of("A")
    chunks, compact, _, _ = chain_cut(layout, 3)
    w = sizes_weights(n) if weighted else None

    def fn(rank):
        a = sum(counts[:rank])
        bk = clients_on("A", range(a, a + counts[rank]))
        out32, out64 = fresh_out(layout)
        agg = ChainAggregator(layout, n, out32, out64,
                              backend=OracleChainBackend(layout, chunks, compact), final=final,
                              root=root, nchunks=3, counts=counts)
        agg.step([x[0] for x in bk], [x[1] for x in bk],
                 None if w is None else w[a:a + counts[rank]])
        return out32, out64

    want = expected_exact("A", tuple(range(n)), weighted)
    for r, (o32, o64) in enumerate(run_ranks(world, fn)):
        if final == "reduce" and r != root:
            assert_untouched(o32, o64, r)
        else:
            assert_state(layout, o32, o64, want, r)
