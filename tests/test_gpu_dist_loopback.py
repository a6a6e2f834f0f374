"""GPU: feddct_amd/dist.py's rounds with their own HIP backends (HipBackend,
HipStripeBackend, HipChainBackend) at W = 1, 2, 3 and 8 ranks on the one GPU
of the box, over the in-process stand-in for torch.distributed
(tests/distloop.py, validated against the oracle by
tests/test_distloop_cpu.py).  The Python counterpart of
tests/test_gpu_loopback.py, which does the same for the native rounds.

What runs here and nowhere else on a GPU at more than one rank:
HipStripeBackend.reduce_chunk (client pointers moved back by the stripe's
base, rows of a padded receive matrix, own clients and pre-multiplied received
rows mixed in weighted rounds), StripedAggregator.step_host (pinned-host
stripe uploads, int64 buckets uploaded and reduced), HipChainBackend.chain /
.tails (FaChain's state_in / state_out / plane, 2 and 4 state planes, the
compact tail plan), HipBackend.partial_sum / .divide per key-aligned chunk,
and Aggregator's choice of form and the weights it passes down.

Layouts (test_distloop_cpu.MANS): A = test_dist_gloo.MAN; B has enough vector
tiles for 8 non-empty stripes; C has vector tiles only (no scalar column, no
int64 key).  n_total: 5 (ranks without clients at W = 8), 20, and 300 on A
(past FA_INLINE_CLIENTS: the pointer table; past 256: four state planes).

Every comparison is bit for bit, NaNs as NaNs; there is no tolerance.  On
every result rank every key equals the oracle's result (O.aggregate_state /
O.weighted_sum0 / O.mean_i64_trunc; e1: the per-rank O.torch_sum0 partials
added in ascending rank order in fp32 - the stand-in's SUM - then / N); in
one case per form also one GPU's fa_reduce over all clients.  Non-result
ranks keep their fill (NaN / -7), client buckets are unchanged after every
round, and the striped forms' receive matrix keeps a sentinel in its row
padding [L, lpad) and in one guard row behind it.  One case per form runs two
rounds on one aggregator, the second on fresh data and weights."""
import functools

import numpy as np
import pytest
import torch

import feddct_amd.dist as D
from distloop import LoopDist, run_ranks
from feddct_amd.dist import (Aggregator, ChainAggregator, ShardedAggregator, StripedAggregator,
                             exact_form, shard_counts)
from test_distloop_cpu import (FRESH, assert_state, assert_untouched, clients_on, cpu_bucket,
                               expected_e1, expected_exact, fresh_out, layout_of, same_bits,
                               sizes_weights)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -12345.5


def _loop(monkeypatch, world):
    loop = LoopDist(world, timeout=30.0)
    monkeypatch.setattr(D, "dist", loop)
    return loop


def _ids(n, rd):
    """Client ids of round ``rd``'s n slots (round 1: fresh data)."""
    return tuple(rd * FRESH + k for k in range(n))


def _weights(n, rd, weighted):
    return sizes_weights(n, salt=rd) if weighted else None


@functools.lru_cache(maxsize=None)
def _single_gpu(lay, ids, weighted, salt):
    """One GPU's fa_reduce over all clients (tests/test_gpu_comm._single_gpu)."""
    from feddct_amd.workload import Reducer
    layout = layout_of(lay)
    torch.cuda.set_device(DEV)
    clients = clients_on(lay, ids, DEV)
    o32, o64 = fresh_out(layout, DEV)
    w = sizes_weights(len(ids), salt) if weighted else None
    Reducer(layout, clients, o32, o64, weights=None if w is None else list(map(float, w)))()
    torch.cuda.synchronize()
    return o32.cpu(), o64.cpu()


def _pin(t):
    return t.pin_memory()


def _guard_recv(agg):
    """Give the striped aggregator's receive matrix one guard row and fill the
    row padding [L, lpad) and the guard row with a sentinel."""
    n, pitch = agg.recv.shape
    full = torch.zeros((n + 1, pitch), dtype=torch.float32, device=agg.recv.device)
    L = agg.hi - agg.lo
    full[:, L:] = SENTINEL
    full[n] = SENTINEL
    agg.recv = full[:n]
    return full, L


def _guard_ok(guard):
    full, L = guard
    n = full.shape[0] - 1
    return bool((full[n] == SENTINEL).all()) and bool((full[:n, L:] == SENTINEL).all())


def _unchanged(lay, ids, tensors32, tensors64):
    """The clients' buckets still hold what was put there."""
    for c, x, y in zip(ids, tensors32, tensors64):
        f32, i64 = cpu_bucket(lay, c)
        if not (same_bits(x.cpu().numpy(), f32.numpy()) and torch.equal(y.cpu(), i64)):
            return False
    return True


def _refill(lay, ids, tensors32, tensors64):
    """Fresh client data written in place (buckets bound at construction)."""
    for c, x, y in zip(ids, tensors32, tensors64):
        f32, i64 = cpu_bucket(lay, c)
        x.copy_(f32)
        y.copy_(i64)


def _snap(out32, out64, **flags):
    torch.cuda.synchronize()
    return dict(flags, o32=out32.cpu().clone(), o64=out64.cpu().clone())


def _reset(out32, out64):
    out32.fill_(float("nan"))
    out64.fill_(-7)


def _check(lay, res, n, rounds, roots, weighted=False, e1_world=0, single=False):
    """res[rank][round] against the expectations; ``roots``: the result ranks."""
    layout = layout_of(lay)
    for rd in range(rounds):
        ids = _ids(n, rd)
        want = (expected_e1(lay, ids, e1_world) if e1_world
                else expected_exact(lay, ids, weighted, rd))
        for r, per_round in enumerate(res):
            got = per_round[rd]
            tag = (r, rd)
            assert got.get("inputs", True), (tag, "client buckets changed")
            assert got.get("guard", True), (tag, "receive matrix padding / guard row written")
            if r in roots:
                assert_state(layout, got["o32"], got["o64"], want, tag)
            else:
                assert_untouched(got["o32"], got["o64"], tag)
        if single:
            s32, s64 = _single_gpu(lay, ids, weighted, rd)
            want1 = {}
            for s in layout.slots:
                src = s64 if s.kind == "i64" else s32
                want1[s.key] = src[s.offset:s.offset + s.numel].numpy()
            for r in roots:
                assert_state(layout, res[r][rd]["o32"], res[r][rd]["o64"], want1, (r, rd, "1gpu"))


def _roots(world, final, root):
    return set(range(world)) if final == "allreduce" else {root}


# ------------------------------------------- StripedAggregator.step_device --
STRIPED_DEVICE = [
    # lay, W, n, final, root, nchunks, weighted, counts, rounds, single
    ("A", 1, 20, "allreduce", 0, 4, False, None, 1, False),
    ("B", 2, 20, "allreduce", 0, 1, True, None, 1, True),
    ("A", 2, 5, "reduce", 1, 13, False, [0, 5], 1, False),
    ("A", 2, 300, "reduce", 0, 4, True, None, 1, False),
    ("B", 2, 20, "reduce", 0, 13, True, [13, 7], 1, False),
    ("B", 3, 20, "reduce", 1, 4, True, [9, 0, 11], 1, False),
    ("A", 3, 5, "allreduce", 0, 13, False, None, 1, False),
    ("A", 3, 20, "reduce", 0, 4, True, None, 1, False),
    ("C", 3, 20, "reduce", 2, 1, False, None, 1, False),
    ("B", 8, 20, "allreduce", 0, 4, True, None, 2, False),
    ("A", 8, 5, "reduce", 3, 13, False, None, 1, False),
    ("A", 8, 20, "reduce", 0, 4, False, None, 1, False),
    ("B", 8, 20, "reduce", 7, 1, False, [2, 0, 3, 1, 0, 4, 2, 8], 1, False),
    ("C", 8, 5, "allreduce", 0, 4, True, None, 1, False),
]


@pytest.mark.parametrize("lay,W,n,final,root,nchunks,weighted,counts,rounds,single",
                         STRIPED_DEVICE)
def test_striped_device_round(monkeypatch, lay, W, n, final, root, nchunks, weighted, counts,
                              rounds, single):
    loop = _loop(monkeypatch, W)
    layout = layout_of(lay)

    def fn(rank):
        out32, out64 = fresh_out(layout, DEV)
        agg = StripedAggregator(layout, n, out32, out64, final=final, root=root,
                                nchunks=nchunks, counts=counts)
        assert isinstance(agg.backend, D.HipStripeBackend)
        guard = _guard_recv(agg)
        a, b = agg.shards[rank]
        res = []
        for rd in range(rounds):
            ids = _ids(n, rd)[a:b]
            bk = clients_on(lay, ids, DEV)
            w = _weights(n, rd, weighted)
            agg.step_device([x[0] for x in bk], [x[1] for x in bk],
                            None if w is None else w[a:b])
            res.append(_snap(out32, out64, guard=_guard_ok(guard),
                             inputs=_unchanged(lay, ids, [x[0] for x in bk], [x[1] for x in bk])))
            loop.barrier()
            _reset(out32, out64)
        return res

    res = run_ranks(W, fn, device=DEV)
    _check(lay, res, n, rounds, _roots(W, final, root), weighted, single=single)


# --------------------------------------------- StripedAggregator.step_host --
STRIPED_HOST = [
    # lay, W, n, final, root, nchunks, rounds, single
    ("A", 1, 20, "allreduce", 0, 4, 1, False),
    ("A", 2, 300, "allreduce", 0, 1, 1, True),
    ("A", 2, 20, "reduce", 0, 4, 1, False),
    ("B", 2, 20, "reduce", 1, 4, 1, False),
    ("A", 3, 20, "reduce", 1, 4, 1, False),
    ("B", 3, 20, "allreduce", 0, 1, 1, False),
    ("C", 3, 20, "reduce", 0, 4, 1, False),
    ("A", 8, 300, "reduce", 7, 4, 1, False),
    ("B", 8, 20, "allreduce", 0, 4, 2, False),
    ("B", 8, 20, "reduce", 3, 1, 1, False),
    ("C", 8, 20, "reduce", 0, 1, 1, False),
]


@pytest.mark.parametrize("lay,W,n,final,root,nchunks,rounds,single", STRIPED_HOST)
def test_striped_host_round(monkeypatch, lay, W, n, final, root, nchunks, rounds, single):
    loop = _loop(monkeypatch, W)
    layout = layout_of(lay)

    def fn(rank):
        out32, out64 = fresh_out(layout, DEV)
        agg = StripedAggregator(layout, n, out32, out64, final=final, root=root,
                                nchunks=nchunks)
        assert isinstance(agg.backend, D.HipStripeBackend)
        guard = _guard_recv(agg)
        lo, hi = agg.lo, agg.hi
        res = []
        for rd in range(rounds):
            ids = _ids(n, rd)
            # this rank's stripe of every client in one pinned matrix, the int64
            # buckets on the host
            m = (_pin(torch.stack([cpu_bucket(lay, c)[0][lo:hi] for c in ids])) if hi > lo
                 else torch.zeros((n, 0)))
            keep = m.clone()
            c64 = [cpu_bucket(lay, c)[1].clone() for c in ids]
            agg.step_host(list(m.unbind(0)), c64)
            ok = _guard_ok(guard)
            res.append(_snap(out32, out64, guard=ok))
            res[-1]["inputs"] = same_bits(m.numpy(), keep.numpy()) and all(
                torch.equal(t, cpu_bucket(lay, c)[1]) for t, c in zip(c64, ids))
            loop.barrier()
            _reset(out32, out64)
        return res

    res = run_ranks(W, fn, device=DEV)
    _check(lay, res, n, rounds, _roots(W, final, root), single=single)


# ----------------------------------------------------- ChainAggregator.step --
ZEROS8 = [0, 3, 0, 4, 5, 0, 8, 0]     # no clients first, in the middle, last: finisher 6
CHAINED = [
    # lay, counts, final, root, nchunks, weighted, rounds, single
    ("A", [20], "reduce", 0, 16, False, 1, False),
    ("A", [7, 13], "allreduce", 0, 16, True, 1, True),
    ("B", [20, 0], "reduce", 1, 1, False, 1, False),          # root != finisher 0
    ("A", [260, 40], "reduce", 1, 16, True, 1, False),        # plane 2 travels
    ("A", [0, 3, 2], "reduce", 0, 1, False, 1, False),        # root != finisher 2
    ("B", [9, 0, 11], "allreduce", 0, 16, True, 1, False),
    ("A", [260, 40, 0], "reduce", 1, 16, False, 1, False),    # root == finisher 1, not last
    ("C", [5, 0, 15], "reduce", 1, 16, True, 1, False),       # the root holds no clients
    ("A", ZEROS8, "reduce", 6, 16, True, 2, False),           # root == finisher
    ("B", ZEROS8, "reduce", 0, 1, False, 1, False),           # root != finisher
    ("A", [1, 1, 1, 1, 1, 0, 0, 0], "allreduce", 0, 16, False, 1, False),
    ("A", [0, 17, 40, 40, 40, 40, 83, 40], "allreduce", 0, 1, True, 1, False),
    ("C", [3, 3, 3, 3, 2, 2, 2, 2], "allreduce", 0, 1, False, 1, False),
]


@pytest.mark.parametrize("lay,counts,final,root,nchunks,weighted,rounds,single", CHAINED)
def test_chained_round(monkeypatch, lay, counts, final, root, nchunks, weighted, rounds, single):
    W, n = len(counts), sum(counts)
    loop = _loop(monkeypatch, W)
    layout = layout_of(lay)

    def fn(rank):
        out32, out64 = fresh_out(layout, DEV)
        agg = ChainAggregator(layout, n, out32, out64, final=final, root=root, nchunks=nchunks,
                              counts=counts)
        assert isinstance(agg.backend, D.HipChainBackend)
        assert agg.state.numel() == (4 if n >= 256 else 2) * agg.plane
        a = sum(counts[:rank])
        res = []
        for rd in range(rounds):
            ids = _ids(n, rd)[a:a + counts[rank]]
            bk = clients_on(lay, ids, DEV)
            w = _weights(n, rd, weighted)
            agg.step([x[0] for x in bk], [x[1] for x in bk],
                     None if w is None else w[a:a + counts[rank]])
            res.append(_snap(out32, out64,
                             inputs=_unchanged(lay, ids, [x[0] for x in bk], [x[1] for x in bk])))
            loop.barrier()
            _reset(out32, out64)
        return res

    res = run_ranks(W, fn, device=DEV)
    _check(lay, res, n, rounds, _roots(W, final, root), weighted, single=single)


# --------------------------------------------------- ShardedAggregator.step --
SHARDED = [
    # lay, W, n, final, root, exchange, nchunks, rounds, single
    ("A", 1, 20, "reduce", 0, "reduce", 3, 1, True),      # one rank: no re-association
    ("A", 2, 20, "reduce", 1, "rs_gather", 3, 1, False),
    ("B", 2, 20, "allreduce", 0, "reduce", 8, 1, False),
    ("A", 2, 300, "reduce", 0, "rs_gather", 3, 1, False),
    ("B", 3, 20, "allreduce", 0, "rs_gather", 3, 1, False),
    ("A", 3, 20, "reduce", 1, "reduce", 1, 1, False),
    ("A", 3, 20, "reduce", 2, "rs_gather", 120, 1, False),    # a remainder inside a key
    ("A", 3, 20, "allreduce", 0, "rs_gather", 120, 1, False),
    ("B", 8, 20, "reduce", 5, "rs_gather", 3, 2, False),
    ("A", 8, 20, "allreduce", 0, "reduce", 8, 1, False),
    ("C", 8, 20, "allreduce", 0, "rs_gather", 2, 1, False),
]


def _remainder_in_a_key(layout, W, nchunks):
    """Some chunk's last len % W floats (rs_gather: the plain reduce's share)
    hold key elements, not layout padding."""
    for _, lo, hi in D.chunk_segments(layout, nchunks):
        rlo = lo + W * ((hi - lo) // W)
        if any(o < hi and o + m > rlo for o, m in layout.segs32):
            return True
    return False


@pytest.mark.parametrize("lay,W,n,final,root,exchange,nchunks,rounds,single", SHARDED)
def test_sharded_round(monkeypatch, lay, W, n, final, root, exchange, nchunks, rounds, single):
    loop = _loop(monkeypatch, W)
    layout = layout_of(lay)
    if nchunks == 120:      # k1 (4096 floats) is a chunk of its own: 4096 % 3 == 1
        assert exchange == "rs_gather" and _remainder_in_a_key(layout, W, nchunks)

    def fn(rank):
        out32, out64 = fresh_out(layout, DEV)
        a, b = D.shard_range(n, W, rank)
        bk = clients_on(lay, _ids(n, 0)[a:b], DEV)
        l32, l64 = [x[0] for x in bk], [x[1] for x in bk]
        agg = ShardedAggregator(layout, l32, l64, n, out32, out64, nchunks=nchunks, final=final,
                                root=root, exchange=exchange)
        assert isinstance(agg.backend, D.HipBackend)
        res = []
        for rd in range(rounds):
            ids = _ids(n, rd)[a:b]
            _refill(lay, ids, l32, l64)
            agg.step()
            res.append(_snap(out32, out64, inputs=_unchanged(lay, ids, l32, l64)))
            loop.barrier()
            _reset(out32, out64)
        return res

    res = run_ranks(W, fn, device=DEV)
    _check(lay, res, n, rounds, _roots(W, final, root), e1_world=W, single=single)


# -------------------------------------------------- Aggregator, the default --
DEFAULT = [
    # lay, counts, final, weighted, model's form, exact, rounds, single
    ("A", [20], "reduce", False, "blocked", True, 1, False),          # one rank: chained here
    ("A", [10, 10], "reduce", True, "striped", True, 1, True),
    ("A", [150, 150], "reduce", False, "chained", True, 1, False),
    ("A", [7, 0, 13], "allreduce", False, "striped", True, 1, False),
    ("A", [0, 20, 0], "reduce", True, "chained", True, 1, False),
    ("B", [3, 3, 3, 2, 2, 2, 2, 3], "reduce", True, "striped", True, 2, False),
    ("A", [0, 0, 0, 20, 0, 0, 0, 0], "allreduce", False, "chained", True, 1, False),
    ("A", [10, 10], "reduce", False, None, False, 1, False),           # exact=False: e1
    ("B", [7, 7, 6], "allreduce", False, None, False, 1, False),
    ("A", [3, 3, 3, 3, 2, 2, 2, 2], "reduce", False, None, False, 1, False),
]


@pytest.mark.parametrize("lay,counts,final,weighted,model,exact,rounds,single", DEFAULT)
def test_default_entry(monkeypatch, lay, counts, final, weighted, model, exact, rounds, single):
    W, n = len(counts), sum(counts)
    loop = _loop(monkeypatch, W)
    layout = layout_of(lay)
    if exact:       # ask the model on the host first
        assert exact_form(counts, layout, root_all=final != "reduce") == model
        form = ("striped" if model == "striped" else "chained") + "/torch.distributed"
    else:
        assert counts == shard_counts(n, W)
        form = "e1/torch.distributed"
    root = max(r for r in range(W) if counts[r] > 0)    # the entry's default root

    def fn(rank):
        out32, out64 = fresh_out(layout, DEV)
        a = sum(counts[:rank])
        bk = clients_on(lay, _ids(n, 0)[a:a + counts[rank]], DEV)
        l32, l64 = [x[0] for x in bk], [x[1] for x in bk]
        w = _weights(n, 0, weighted)
        agg = Aggregator(layout, l32, l64, n, out32, out64, final=final, counts=counts,
                         weights=None if w is None else w[a:a + counts[rank]], exact=exact)
        assert agg.form == form, agg.form
        assert agg._agg.root == (-1 if exact and final != "reduce" else root)
        assert isinstance(agg._agg.backend, (D.HipBackend, D.HipStripeBackend,
                                             D.HipChainBackend))
        res = []
        for rd in range(rounds):
            ids = _ids(n, rd)[a:a + counts[rank]]
            _refill(lay, ids, l32, l64)
            w = _weights(n, rd, weighted)
            agg.weights = None if w is None else w[a:a + counts[rank]]
            agg.step()
            res.append(_snap(out32, out64, inputs=_unchanged(lay, ids, l32, l64)))
            loop.barrier()
            _reset(out32, out64)
        return res

    res = run_ranks(W, fn, device=DEV)
    _check(lay, res, n, rounds, _roots(W, final, root), weighted, e1_world=0 if exact else W,
           single=single)
