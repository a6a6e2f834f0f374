"""The native multi-GPU schedules (libfedagg_comm.so), all ranks at once, on
a CPU: fa_describe_round (the schedule builders of
feddct_amd/csrc/sched_host.cpp, the library's HIP-free host unit) gives each
rank's exact list of exchanges and kernels; tests/schedsim.py replays the lists of every
rank together under RCCL's group/matching rules with the oracle as the
arithmetic.  Covers world sizes 2-8, uneven and empty shards, every root,
weighted rounds, and both e1 exchanges:

* chained and striped rounds must give the single-process reference's bits;
* the sharded round's int64 keys are exact and its fp32 keys stay within
  the re-association bound;
* no schedule may deadlock;
* the native cut points and peers agree with partition.split_tiles /
  dist.shard_range and the Python aggregators' own send/receive lists.
"""
import numpy as np
import pytest
import torch

from feddct_amd import comm as C
from feddct_amd import synth
from feddct_amd.dist import shard_range
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import layout_tiles, split_tiles
from oracle import torch_order as O
from schedsim import Deadlock, Hazard, Sim

MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                for j, m in enumerate([100, 4096, 33, 2048 + 8, 7, 0, 5000, 1, 64, 3000])]
       + [{"key": "nbt", "shape": [], "dtype": "int64"},
          {"key": "nbt2", "shape": [], "dtype": "int64"}]}


def _buckets(layout, states):
    c32, c64 = [], []
    for st in states:
        f32 = np.full(layout.f32_numel, np.nan, np.float32)   # padding must never leak
        i64 = np.zeros(max(1, layout.i64_numel), np.int64)
        for k, v in st:
            s = layout.by_key[k]
            tgt = i64 if s.kind == "i64" else f32
            tgt[s.offset:s.offset + s.numel] = np.asarray(v).reshape(-1)
        c32.append(f32)
        c64.append(i64)
    return c32, c64


def _expected(states, weights):
    if weights is None:
        return dict(O.aggregate_state(states))
    out = {}
    for j, (k, v0) in enumerate(states[0]):
        x = np.stack([np.asarray(s[j][1]) for s in states])
        out[k] = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, weights)
    return out


def _run(mode, counts, root, weighted=False, exchange=C.FA_XCHG_REDUCE, nchunks=5, man=MAN):
    layout = BucketLayout.from_manifest(man)
    n = sum(counts)
    states = [synth.gen_state(man, c, synth.MODE_ADVERSARIAL) for c in range(n)]
    c32, c64 = _buckets(layout, states)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 5 + 1) if weighted else None
    _, tiles = layout_tiles(layout)
    scheds = [C.describe(mode, layout, counts, r, nchunks=nchunks, exchange=exchange, root=root,
                         weighted=weighted) for r in range(len(counts))]
    bufs = Sim(layout, tiles, counts, c32, c64, w, root).run(scheds)
    return layout, states, w, bufs, scheds


def _result_ranks(W, root):
    return range(W) if root < 0 else [root]


COUNTS = [[10, 10], [7, 0, 13], [3, 3, 3, 3, 3, 3, 3, 3], [0, 5, 1, 14], [4, 9, 0, 2, 5],
          [1, 1, 1, 17], [16, 16, 1], [2, 30, 2, 0, 0, 1, 3, 2]]


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("root", [0, -1, "last", 1])
def test_chained_schedule_is_exact(counts, root):
    W = len(counts)
    root = W - 1 if root == "last" else root
    layout, states, _, bufs, _ = _run(C.FA_MODE_CHAINED, counts, root)
    want = _expected(states, None)
    for r in _result_ranks(W, root):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (r, s.key)


@pytest.mark.parametrize("counts", [[10, 10], [4, 9, 0, 2, 5], [2, 30, 2, 0, 0, 1, 3, 2]])
def test_chained_schedule_weighted_is_exact(counts):
    layout, states, w, bufs, _ = _run(C.FA_MODE_CHAINED, counts, 0, weighted=True)
    want = _expected(states, w)
    for s in layout.slots:
        src = bufs[0]["OUT64"] if s.kind == "i64" else bufs[0]["OUT"]
        got = src[s.offset:s.offset + s.numel].reshape(s.shape)
        assert got.tobytes() == np.asarray(want[s.key]).tobytes(), s.key


def test_chained_schedule_deep_levels():
    """n_total >= 256: four state planes, level-2 promotions across hops."""
    counts = [100, 156, 44]
    layout, states, _, bufs, scheds = _run(C.FA_MODE_CHAINED, counts, -1, nchunks=3)
    want = _expected(states, None)
    for s in layout.slots:
        src = bufs[2]["OUT64"] if s.kind == "i64" else bufs[2]["OUT"]
        assert src[s.offset:s.offset + s.numel].tobytes() == np.asarray(want[s.key]).tobytes()
    planes = {x["src_index"] for x in scheds[1] if x["op"] == "SEND"}
    assert planes == set(i for i in range(4) if O.chain_levels(256, 300) & (1 << i))


STRIPE_COUNTS = [[9], [10, 10], [7, 0, 13], [0, 5, 1, 14], [4, 9, 0, 2, 5], [1, 2, 3, 4, 5, 6],
                 [1, 1, 1, 17, 0, 2, 3], [3, 3, 3, 3, 3, 3, 3, 3], [2, 30, 2, 0, 0, 1, 3, 2]]


@pytest.mark.parametrize("counts", STRIPE_COUNTS)
@pytest.mark.parametrize("root", [0, -1, 1])
@pytest.mark.parametrize("nchunks", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_striped_schedule_is_exact(counts, root, nchunks, weighted):
    """r06: the link-parallel striped round (every peer in one group per
    column chunk, the chunk reduce beside the next chunk's exchange, the
    finished chunks two steps later), W = 1..8, weighted too: the
    single-process reference's bits on every result rank, no deadlock, no
    stream hazard (schedsim)."""
    W = len(counts)
    if root >= W:
        pytest.skip("root beyond the world")
    layout, states, w, bufs, scheds = _run(C.FA_MODE_STRIPED, counts, root, weighted=weighted,
                                           nchunks=nchunks)
    want = _expected(states, w)
    for r in _result_ranks(W, root):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (r, s.key)


@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_striped_groups_are_link_parallel(W):
    """Every exchange step of the striped round is ONE group holding all the
    rank's peers (r06, VERDICT r05 next 1: r02-r05 one partner per group), and
    the round has nchunks + 2 such steps; one stripe reduce per nonempty
    chunk, each in the step after its rows arrive."""
    big = {"keys": [{"key": f"b{j}", "shape": [40000 + 7 * j], "dtype": "float32"}
                    for j in range(12)]}
    layout = BucketLayout.from_manifest(big)
    counts = [3] * W
    for r in range(W):
        ops = C.describe(C.FA_MODE_STRIPED, layout, counts, r, nchunks=4, root=-1)
        by_step = {}
        for x in ops:
            if x["op"] in ("SEND", "RECV") and (x["src"] == "CLIENT" or x["dst"] == "RECV"):
                by_step.setdefault(x["step"], set()).add(x["peer"])
        assert by_step and all(v == set(range(W)) - {r} for v in by_step.values()), by_step
        recv_step = {}
        for x in ops:
            if x["op"] == "RECV" and x["dst"] == "RECV":
                recv_step[x["chunk"]] = x["step"]
        for x in ops:
            if x["op"] == "K_STRIPE":
                assert x["step"] == recv_step[x["chunk"]] + 1


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("exchange", [C.FA_XCHG_REDUCE, C.FA_XCHG_RS_GATHER])
@pytest.mark.parametrize("root", [0, -1])
@pytest.mark.parametrize("weighted", [False, True])
def test_sharded_schedule(counts, exchange, root, weighted):
    W = len(counts)
    layout, states, w, bufs, _ = _run(C.FA_MODE_SHARDED, counts, root, weighted, exchange)
    want = _expected(states, w)
    n = sum(counts)
    for r in _result_ranks(W, root):
        for s in layout.slots:
            if s.kind == "i64":
                assert np.array_equal(bufs[r]["OUT64"][s.offset:s.offset + s.numel],
                                      np.asarray(want[s.key]).reshape(-1)), s.key
                continue
            got = bufs[r]["OUT"][s.offset:s.offset + s.numel].astype(np.float64)
            x = np.stack([dict(st)[s.key].reshape(-1) for st in states]).astype(np.float64)
            if w is not None:
                x = x * w[:, None]
            mag = np.abs(x).mean(0) if w is None else np.abs(x).sum(0)
            err = np.abs(got - np.asarray(want[s.key], np.float64).reshape(-1))
            assert (err <= 2 * n * 2.0 ** -24 * mag + 1e-38).all(), (r, s.key)


@pytest.mark.parametrize("W", [2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("root", [-1, 0])
def test_striped_cuts_and_peers_match_python(W, root):
    """The native stripe bounds are partition.split_tiles', its chunk bounds
    partition.stripe_chunks', the shards dist.shard_range's, and the native
    exchange and reduce steps are exactly the Python StripedAggregator's
    (dist.stripe_schedule), op for op and step for step."""
    from feddct_amd.dist import stripe_schedule
    from feddct_amd.partition import stripe_chunks
    layout = BucketLayout.from_manifest(MAN)
    n = 3 * W + 2
    counts = [b - a for a, b in (shard_range(n, W, r) for r in range(W))]
    _, tiles = layout_tiles(layout)
    parts = split_tiles(tiles, W, layout.f32_numel)
    chunks = stripe_chunks(tiles, W, layout.f32_numel, 3)
    bounds = [[c[0] for c in ch] + [ch[-1][1]] for ch in chunks]
    assert [(b[0], b[-1]) for b in bounds] == [p[:2] for p in parts]
    shards = [shard_range(n, W, q) for q in range(W)]
    for r in range(W):
        ops = C.describe(C.FA_MODE_STRIPED, layout, counts, r, nchunks=3, root=root)
        native = {}
        for x in ops:
            if x["op"] == "SEND" and x["src"] == "CLIENT":
                t = ("send", x["peer"], sum(counts[:r]) + x["src_index"], x["offset"], x["count"])
            elif x["op"] == "RECV" and x["dst"] == "RECV":
                t = ("recv", x["peer"], x["dst_index"], x["offset"], x["count"])
            elif x["op"] == "SEND":
                t = ("send_out", x["peer"], x["offset"], x["count"])
            elif x["op"] == "RECV" and x["dst"] == "OUT":
                t = ("recv_out", x["peer"], x["offset"], x["count"])
            elif x["op"] == "K_STRIPE":
                t = ("reduce", x["chunk"], x["offset"], x["count"])
            else:
                continue
            native.setdefault(x["step"], []).append(t)
        py = stripe_schedule(bounds, shards, r, root)
        assert [native.get(k + 2, []) for k in range(len(py))] == py
        assert all(2 <= k <= len(py) + 1 for k in native), sorted(native)


@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_chained_hops_follow_slot_order(W):
    """Each rank receives only from rank-1 and sends only to rank+1 (slot
    order), one op per nonzero state plane per chunk, and the chunks tile the
    vector columns."""
    layout = BucketLayout.from_manifest(MAN)
    n = 2 * W + 9
    counts = [b - a for a, b in (shard_range(n, W, r) for r in range(W))]
    _, tiles = layout_tiles(layout)
    vec = tiles[tiles[:, 2] == 0]
    for r in range(W):
        ops = C.describe(C.FA_MODE_CHAINED, layout, counts, r, nchunks=4, root=W - 1)
        first = sum(counts[:r])
        for x in ops:
            if x["op"] == "SEND" and x["src"] == "STATE":
                assert x["peer"] == r + 1
                assert O.chain_levels(first + counts[r], n) & (1 << x["src_index"])
            if x["op"] == "RECV" and x["dst"] == "STATE":
                assert x["peer"] == r - 1
                assert O.chain_levels(first, n) & (1 << x["dst_index"])
        ks = [x for x in ops if x["op"] == "K_CHAIN"]
        assert all(k["row0"] == first and k["nrows"] == counts[r] for k in ks)
        covered = sum(int(((vec[:, 0] >= k["offset"]) & (vec[:, 0] < k["offset"] + k["count"]))
                          .sum()) for k in ks)
        assert covered == len(vec)


def test_describe_errors():
    from feddct_amd import _lib
    layout = BucketLayout.from_manifest(MAN)
    with pytest.raises(_lib.FedaggError, match="mode"):
        C.describe(7, layout, [1, 1], 0)
    with pytest.raises(_lib.FedaggError, match="root"):
        C.describe(C.FA_MODE_CHAINED, layout, [1, 1], 0, root=2)
    with pytest.raises(_lib.FedaggError, match="clients in total"):
        C.describe(C.FA_MODE_CHAINED, layout, [0, 0], 0)


def test_stream_hazard_is_detected():
    """The replay's stream rules: a compute-stream chunk reduce placed in the
    same step as the group that receives its rows is reported (the executor
    would run the two concurrently)."""
    layout = BucketLayout.from_manifest(MAN)
    counts = [2, 2]
    states = [synth.gen_state(MAN, c, synth.MODE_ADVERSARIAL) for c in range(4)]
    c32, c64 = _buckets(layout, states)
    _, tiles = layout_tiles(layout)
    scheds = [C.describe(C.FA_MODE_STRIPED, layout, counts, r, nchunks=2, root=-1)
              for r in range(2)]
    for o in scheds:
        for x in o:
            if x["op"] == "K_STRIPE":
                x["step"] -= 1   # beside its own rows' receives
        o.sort(key=lambda x: x["step"])
    with pytest.raises(Hazard):
        Sim(layout, tiles, counts, c32, c64, None, -1).run(scheds)


def test_deadlock_is_detected():
    """The replay itself: a schedule whose ranks both receive first is
    reported, not hung."""
    layout = BucketLayout.from_manifest(MAN)
    counts = [2, 2]
    states = [synth.gen_state(MAN, c, synth.MODE_ADVERSARIAL) for c in range(4)]
    c32, c64 = _buckets(layout, states)
    _, tiles = layout_tiles(layout)
    bad = [[{"step": 0, "op": "RECV", "peer": 1 - r, "chunk": -1, "src": "NONE",
             "src_index": -1, "dst": "OUT", "dst_index": -1, "offset": 0, "count": 4,
             "row0": 0, "nrows": 0},
            {"step": 1, "op": "SEND", "peer": 1 - r, "chunk": -1, "src": "CLIENT",
             "src_index": 0, "dst": "NONE", "dst_index": -1, "offset": 0, "count": 4,
             "row0": 0, "nrows": 0}] for r in range(2)]
    with pytest.raises(Deadlock):
        Sim(layout, tiles, counts, c32, c64).run(bad)


BLOCK_COUNTS = [[20], [10, 10], [7, 0, 13], [16, 16, 1], [20, 20, 20], [20] * 8,
                [12, 9, 30, 0, 14, 8], [100, 156, 44],
                [250, 10]]    # the spanning block ends at 256: its sum sent and copied from CONT plane 2


@pytest.mark.parametrize("counts", BLOCK_COUNTS)
@pytest.mark.parametrize("root", [0, -1, "last", 1])
def test_blocked_schedule_is_exact(counts, root):
    """Block sums where they lie, spanning partials relayed through the
    stripe owners, the owners' folds: the single-process reference's bits
    (incl. n_total >= 256: the fold's level-2 promotion)."""
    W = len(counts)
    root = W - 1 if root == "last" else root
    if root >= W:
        pytest.skip("root beyond the world")
    layout, states, _, bufs, _ = _run(C.FA_MODE_BLOCKED, counts, root)
    want = _expected(states, None)
    for r in _result_ranks(W, root):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (r, s.key)


@pytest.mark.parametrize("counts", [[10, 10], [20] * 8, [12, 9, 30, 0, 14, 8], [100, 156, 44],
                                    [250, 10]])
def test_blocked_schedule_weighted_is_exact(counts):
    layout, states, w, bufs, _ = _run(C.FA_MODE_BLOCKED, counts, -1, weighted=True)
    want = _expected(states, w)
    for r in range(len(counts)):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (r, s.key)


# N_total > 4096 (FA_MAX_CLIENTS is 65536): the chained state's fourth plane,
# the fold's level-3 promotion after every 256th block
SMALL_MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                      for j, m in enumerate([40, 3, 0, 64 + 5])]
             + [{"key": "nbt", "shape": [], "dtype": "int64"}]}


@pytest.mark.parametrize("mode,counts", [(C.FA_MODE_BLOCKED, [2000, 2500, 700]),
                                         (C.FA_MODE_BLOCKED, [4100, 0, 1]),
                                         (C.FA_MODE_CHAINED, [3000, 2200]),
                                         (C.FA_MODE_CHAINED, [1, 4200, 17])])
def test_exact_schedules_beyond_4096_clients(mode, counts):
    layout, states, _, bufs, _ = _run(mode, counts, 0, man=SMALL_MAN)
    want = _expected(states, None)
    for s in layout.slots:
        src = bufs[0]["OUT64"] if s.kind == "i64" else bufs[0]["OUT"]
        got = src[s.offset:s.offset + s.numel].reshape(s.shape)
        assert got.tobytes() == np.asarray(want[s.key]).tobytes(), s.key


# The counts the GPU loopback runs at depth (tests/test_gpu_loopback.py
# test_loopback_deep_cascade), replayed here: a spanning block that ends on a
# multiple of 256 / 4096 (its sum in CONT plane 2 / 3), N = 4096 exactly (the
# spanning block is the last: a finishing continuation, 256 pieces), 257 and
# 515 pieces, a chain hop that carries plane 3 alone.
DEEP_CASES = [(C.FA_MODE_BLOCKED, [250, 10], 0), (C.FA_MODE_BLOCKED, [250, 10], -1),
              (C.FA_MODE_BLOCKED, [4090, 10], 0), (C.FA_MODE_BLOCKED, [4090, 6], -1),
              (C.FA_MODE_BLOCKED, [4090, 4110, 30], -1),
              (C.FA_MODE_BLOCKED, [4090, 22], 0),     # 257 whole blocks, no remainder
              (C.FA_MODE_BLOCKED, [4096, 16], 1),     # no spanning block: 257 local sums
              (C.FA_MODE_CHAINED, [4096, 5], 1), (C.FA_MODE_CHAINED, [4090, 4110, 30], -1)]


@pytest.mark.parametrize("mode,counts,root", DEEP_CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_deep_cascade_schedules_are_exact(mode, counts, root, weighted):
    layout, states, w, bufs, scheds = _run(mode, counts, root, weighted=weighted, man=SMALL_MAN)
    want = _expected(states, w)
    for r in _result_ranks(len(counts), root):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (r, s.key)
    if mode == C.FA_MODE_CHAINED and counts == [4096, 5]:
        sent = {x["src_index"] for x in scheds[0] if x["op"] == "SEND" and x["src"] == "STATE"}
        assert sent == {3}


@pytest.mark.parametrize("counts,plane", [([250, 10], 2), ([4090, 10], 3), ([4090, 6], 0)])
def test_blocked_cont_planes(counts, plane):
    """The holder of a spanning block leaves the block's sum in the CONT plane
    the cascade's promotions at the block's last row name: a block ending on
    a multiple of 256 in plane 2, of 4096 in plane 3, a finishing continuation
    (the block ends the reduction) in plane 0 — and its sends to the owners
    and its own copy into the fold's rows read that plane."""
    holder = 1
    # SMALL_MAN (the deep replay's layout) is one stripe, owned by rank 0: the
    # holder sends; on MAN it owns a stripe too and copies its own part
    for man, root in [(SMALL_MAN, 0), (SMALL_MAN, -1), (MAN, 0), (MAN, -1)]:
        layout = BucketLayout.from_manifest(man)
        ops = C.describe(C.FA_MODE_BLOCKED, layout, counts, holder, root=root)
        cont = [x for x in ops if x["op"] == "K_CONT"]
        assert len(cont) == 1 and cont[0]["dst"] == "CONT" and cont[0]["dst_index"] == plane
        assert cont[0]["row0"] == counts[0] and cont[0]["nrows"] == 16 - counts[0] % 16
        piece = counts[0] // 16
        sends = [x for x in ops if x["op"] == "SEND" and x["src"] == "CONT"]
        copies = [x for x in ops if x["op"] == "K_COPY" and x["src"] == "CONT"]
        assert sends and all(x["step"] > cont[0]["step"] for x in sends + copies)
        assert {x["src_index"] for x in sends} == {plane}
        assert ([(x["src_index"], x["dst"], x["dst_index"]) for x in copies]
                == ([(plane, "BLK", piece)] if man is MAN else []))
        # the starter's side: no continuation, and nothing of its own in CONT
        other = C.describe(C.FA_MODE_BLOCKED, layout, counts, 0, root=root)
        assert not [x for x in other if x["op"] == "K_CONT" or x["src"] == "CONT"]


@pytest.mark.parametrize("counts", [[4, 9, 0, 2, 5], [1, 1, 1, 17], [3] * 8])
def test_blocked_refuses_blocks_over_three_ranks(counts):
    from feddct_amd._lib import FedaggError
    layout = BucketLayout.from_manifest(MAN)
    with pytest.raises(FedaggError, match="more than two"):
        C.describe(C.FA_MODE_BLOCKED, layout, counts, 0, root=0)


def test_blocked_relays_spread_over_owners():
    """W=8, 20 slots per rank: every spanning partial leaves its starter in
    W-1 pieces (2 direct to the holder, W-3 through the other owners), and no
    rank sends more than one piece to any peer per step."""
    layout = BucketLayout.from_manifest(MAN)
    W = 8
    counts = [20] * W
    for r in range(W):
        ops = C.describe(C.FA_MODE_BLOCKED, layout, counts, r, root=0)
        parts = [x for x in ops if x["op"] == "SEND" and x["src"] == "TAILP"]
        if parts:
            peers = [x["peer"] for x in parts]
            assert sorted(set(peers)) == sorted(set(range(W)) - {r}), peers
        by_step = {}
        for x in ops:
            if x["op"] == "SEND" and x["src"] in ("TAILP", "RELAY"):
                key = (x["step"], x["peer"], x["src"])
                by_step[key] = by_step.get(key, 0) + 1
        assert all(v <= 2 for v in by_step.values())


def test_blocked_and_chained_scalar_only_layout():
    """A layout with no vector columns (0-d keys, 3-element tensors, int64):
    no blocks to sum, only the raw stacked columns — still exact."""
    man = {"keys": [{"key": "a", "shape": [], "dtype": "float32"},
                    {"key": "b", "shape": [3], "dtype": "float32"},
                    {"key": "n", "shape": [], "dtype": "int64"}]}
    layout = BucketLayout.from_manifest(man)
    for mode in (C.FA_MODE_BLOCKED, C.FA_MODE_CHAINED):
        counts = [10, 10, 5]
        n = sum(counts)
        states = [synth.gen_state(man, c, synth.MODE_ADVERSARIAL) for c in range(n)]
        c32, c64 = _buckets(layout, states)
        _, tiles = layout_tiles(layout)
        scheds = [C.describe(mode, layout, counts, r, root=-1) for r in range(3)]
        bufs = Sim(layout, tiles, counts, c32, c64, None, -1).run(scheds)
        want = _expected(states, None)
        for r in range(3):
            for s in layout.slots:
                src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
                got = src[s.offset:s.offset + s.numel].reshape(s.shape)
                assert got.tobytes() == np.asarray(want[s.key]).tobytes(), (mode, r, s.key)


# The counts, roots and weight vectors the GPU loopback runs under special
# values (tests/test_gpu_loopback.py), replayed here with the oracle as the
# arithmetic: the schedule half of those rounds, so a difference on the GPU is
# the executor's.
SPECIAL_COUNTS = [[10, 10], [7, 0, 13], [16, 16, 1], [100, 156, 44]]


def _special_states(man, n, seed):
    """Client states over ``man``: every fp32 key's columns carry the nine
    specials.py patterns (phase = the key's index), int64 keys the generator's."""
    import specials
    rng = np.random.default_rng(seed)
    cols = []
    for j, e in enumerate(man["keys"]):
        shape = tuple(e["shape"])
        m = int(np.prod(shape)) if shape else 1
        if e["dtype"] == "int64":
            cols.append([synth.gen_i64(j, m, c).reshape(shape) for c in range(n)])
        else:
            x = specials.pattern_matrix(n, m, j, rng)
            cols.append([x[c].reshape(shape) for c in range(n)])
    return [[(e["key"], cols[j][c]) for j, e in enumerate(man["keys"])] for c in range(n)]


@pytest.mark.parametrize("counts", SPECIAL_COUNTS)
@pytest.mark.parametrize("root", [0, -1])
@pytest.mark.parametrize("wmode", ["mean", "w1", "w2"])
@pytest.mark.parametrize("mode", [C.FA_MODE_CHAINED, C.FA_MODE_STRIPED, C.FA_MODE_BLOCKED])
def test_exact_schedules_under_special_values(mode, counts, root, wmode):
    """inf, NaN, -0.0, subnormals, overflowing and cancelling columns, and
    weights that are 0, subnormal, negative and inf, through the chained,
    striped and blocked schedules: every result rank holds the single-process
    reference's bits (NaNs where it has NaNs), int64 keys included."""
    import specials
    from helpers import bits_equal
    layout = BucketLayout.from_manifest(MAN)
    n = sum(counts)
    states = _special_states(MAN, n, 977 * n + len(counts))
    c32, c64 = _buckets(layout, states)
    w = specials.mode_weights(n, wmode)
    _, tiles = layout_tiles(layout)
    scheds = [C.describe(mode, layout, counts, r, nchunks=3, root=root, weighted=w is not None)
              for r in range(len(counts))]
    with np.errstate(all="ignore"):
        bufs = Sim(layout, tiles, counts, c32, c64, w, root).run(scheds)
        want = {}
        for j, (k, _) in enumerate(states[0]):
            x = np.stack([np.asarray(s[j][1]) for s in states])
            want[k] = (O.mean_i64_trunc(x) if x.dtype == np.int64
                       else specials.oracle(x, wmode, w))
    for r in _result_ranks(len(counts), root):
        for s in layout.slots:
            src = bufs[r]["OUT64"] if s.kind == "i64" else bufs[r]["OUT"]
            got = src[s.offset:s.offset + s.numel].reshape(s.shape)
            assert bits_equal(got, np.asarray(want[s.key])), (r, s.key)
