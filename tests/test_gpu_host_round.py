"""GPU: the host-resident round — clients and global in host memory, staged
through the GPU chunk by chunk on three streams (pipeline.HostPipeline,
Engine._reduce_host) — directly and through the drop-in.

What these tests are built to notice:

* a reduce that runs before its upload has landed, a download that is
  skipped or runs before its kernel, a fan-out that copies a chunk before it
  is in host memory.  Every round gets FRESH inputs, written in place into the
  same host buckets or modules, and every host bucket the round must write is
  filled with a sentinel first (7.25 / -3, values no input produces): stale
  device staging buffers, a stale device result and an unwritten target are
  then wrong values, not accidentally right ones;
* tile-subset plans (the chunks) at the client counts where the launch
  changes — batch of 8 / 16, inline / table pointers, the deep cascade — with
  and without weights;
* cuts with empty ranges, layouts without int64 or without floating keys;
* the drop-in's surface on host modules: goldens at every N, weights,
  broadcast=False, the split call, staged dtypes, the summation-order switch,
  the reference's errors, modules that move between host and GPU.

Expected values never come from the engine: the numpy oracle
(oracle/torch_order.py), the reference's own outputs (tests/golden/), or the
reference loop on CPU torch for keys small enough (N*M < 32768) that torch's
thread chunking cannot move a column to another order.  Comparison is bit for
bit.  Gap elements between keys are not asserted on: the chunk plans treat
them as padding and the download copies whole ranges."""
import copy
import importlib
import warnings
from functools import lru_cache

import numpy as np
import pytest
import torch

import hostlayouts as H
from conftest import load_manifest
from feddct_amd import synth
from feddct_amd.layout import KIND_I64, BucketLayout
from helpers import StateModule, bits_equal, buckets_to_state
from oracle import torch_order as O
from oracle.torch_mirror import reference_loop

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S32, S64 = 7.25, -3          # the sentinels: finite, and no input or mean produces them
ADV, REAL = synth.MODE_ADVERSARIAL, synth.MODE_REALISTIC


@pytest.fixture(scope="module", autouse=True)
def _device():
    torch.cuda.set_device(DEV)


def _man(name):
    return H.SWEEP if name == "sweep" else H.LAYOUTS[name]


# ---------------------------------------------------- inputs and oracles --
@lru_cache(maxsize=None)
def _state(name, seed, mode):
    """One client's state (shared, never written to)."""
    return synth.gen_state(_man(name), seed, mode)


def _states(name, r, n, mode=ADV):
    """Round r's clients: other values than any other round's."""
    return [_state(name, 1000 * r + i, mode) for i in range(n)]


def _weights(n):
    return O.weights_from_sizes(np.arange(1, n + 1) * 13 + 5)


def _oracle(states, w=None):
    """[(key, array)]: the reference's mean, or with weights the weighted sum
    of the fp32 keys (int64 keys keep the mean)."""
    if w is None:
        out = O.aggregate_state(states)
    else:
        out = []
        for j, (k, _) in enumerate(states[0]):
            x = np.stack([np.asarray(s[j][1]) for s in states], 0)
            out.append((k, O.mean_i64_trunc(x) if x.dtype == np.int64
                        else O.weighted_sum0(x, w)))
    for k, v in out:   # the sentinel must be able to tell "unwritten" from "right"
        assert not np.any(v == (S64 if v.dtype == np.int64 else np.float32(S32))), k
    return out


@lru_cache(maxsize=None)
def _want(name, r, n, mode=ADV, weighted=False):
    return _oracle(_states(name, r, n, mode), _weights(n) if weighted else None)


def _same(got, want, what):
    """Every key of ``got`` [(key, array)] has the oracle's bits and none of
    its elements still holds the sentinel."""
    got = dict(got)
    assert sorted(got) == sorted(k for k, _ in want), what
    for k, w in want:
        g = np.asarray(got[k])
        assert not np.any(g == (S64 if g.dtype == np.int64 else S32)), (what, k, "sentinel")
        assert bits_equal(g, np.asarray(w).reshape(g.shape)), (what, k)


# ------------------------------------------------------- A. HostPipeline --
class Rows:
    """Host buckets as the rows of ONE pinned [rows, numel] tensor per dtype
    (a large N costs one pinned allocation)."""

    def __init__(self, layout, rows):
        self.layout = layout
        self.b32 = torch.zeros(rows, max(layout.f32_numel, 64)).pin_memory()
        self.b64 = torch.zeros(rows, max(layout.i64_numel, 1), dtype=torch.int64).pin_memory()
        self.n32, self.n64 = self.b32.numpy(), self.b64.numpy()

    def put(self, row, state):
        for k, v in state:
            s = self.layout.by_key[k]
            dst = self.n64 if s.kind == KIND_I64 else self.n32
            dst[row, s.offset:s.offset + s.numel] = np.asarray(v).reshape(-1)

    def poison(self, rows):
        for r in rows:
            self.n32[r] = S32
            self.n64[r] = S64

    def r32(self, rows):
        return [self.b32[r] for r in rows]

    def r64(self, rows):
        return [self.b64[r] for r in rows]

    def state(self, row):
        return buckets_to_state(self.layout, self.b32[row], self.b64[row])

    def holds_sentinel(self, row):
        return all(np.all(v == (S64 if v.dtype == np.int64 else S32)) for _, v in self.state(row))


def _nonempty(ranges):
    """Non-empty ranges of a cut; a range has a plan iff it is non-empty."""
    for lo, hi, plan in ranges:
        assert (hi > lo) == (plan is not None), (lo, hi)
    return sum(hi > lo for lo, hi, _ in ranges)


def _round(pipe, rows, n, states, want, targets=(), weights=None, what=""):
    """One round: fresh inputs into rows 0..n-1, row n is the global, the
    rows ``targets`` receive the broadcast (rows < n: the clients' own input
    buckets).  Every row the round must write and that holds no input is
    poisoned first; afterwards the global and every target equal ``want``."""
    for i, st in enumerate(states):
        rows.put(i, st)
    targets = list(targets)
    rows.poison([n] + [t for t in targets if t > n])
    pipe.run(rows.r32(range(n)), rows.r64(range(n)), rows.b32[n], rows.b64[n],
             rows.r32(targets), rows.r64(targets), weights=weights)
    for t in [n] + targets:
        _same(rows.state(t), want, (what, "row", t))


def _three_fresh_rounds(pipe, rows, n, name="mid"):
    # round 1 without broadcast (ranges_nb), round 2 into two foreign buckets,
    # round 3 into the clients' own input buckets (the reference's broadcast)
    _round(pipe, rows, n, _states(name, 1, n), _want(name, 1, n), (), what="r1")
    _round(pipe, rows, n, _states(name, 2, n), _want(name, 2, n), (n + 1, n + 2), what="r2")
    _round(pipe, rows, n, _states(name, 3, n), _want(name, 3, n), range(n), what="r3")


@pytest.mark.parametrize("nchunks,fanout", [(0, "host"), (0, "dma"), (6, "host"), (6, "dma")])
def test_fresh_data_and_poison(nchunks, fanout):
    """A1.  mid, N = 20 (uploads long enough for a missing wait to show),
    three rounds per pipeline object, each on other inputs and into poisoned
    outputs."""
    from feddct_amd.pipeline import HostPipeline
    n = 20
    layout = BucketLayout.from_manifest(_man("mid"))
    pipe = HostPipeline(layout, n, DEV, nchunks=nchunks, fanout=fanout)
    if nchunks == 0:
        assert _nonempty(pipe.ranges) == 5 and _nonempty(pipe.ranges_nb) == 2
    else:
        assert _nonempty(pipe.ranges) == 6 and pipe.ranges_nb is pipe.ranges
    assert pipe.plan64 is not None
    _three_fresh_rounds(pipe, Rows(layout, n + 3), n)


def test_fresh_data_on_the_callers_stream():
    """A6.  The round is ordered on the caller's current stream: run inside a
    side stream with the inputs written on the host just before the call, then
    a round on the default stream with the same pipeline."""
    from feddct_amd.pipeline import HostPipeline
    n = 20
    layout = BucketLayout.from_manifest(_man("mid"))
    pipe = HostPipeline(layout, n, DEV)
    assert _nonempty(pipe.ranges) == 5 and _nonempty(pipe.ranges_nb) == 2
    rows = Rows(layout, n + 3)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        _three_fresh_rounds(pipe, rows, n)
    _round(pipe, rows, n, _states("mid", 4, n), _want("mid", 4, n), (n + 1, n + 2), what="r4")
    with torch.cuda.stream(side):
        _round(pipe, rows, n, _states("mid", 5, n), _want("mid", 5, n), (), what="r5")


@pytest.mark.parametrize("cut", ["1/16+15/16", "4x1/4", "even200"])
def test_custom_fractions_and_more_parts_than_tiles(cut):
    """A2.  ``fractions`` serves both cuts (broadcast or not); a cut with
    more parts than tiles has empty ranges and still gives the oracle's
    bits."""
    from feddct_amd.pipeline import HostPipeline
    n = 5
    layout = BucketLayout.from_manifest(_man("mid"))
    if cut == "even200":
        pipe = HostPipeline(layout, n, DEV, nchunks=200)
        assert len(pipe.ranges) == 200 and 60 <= _nonempty(pipe.ranges) <= 74
    else:
        fr = (0.0625, 0.9375) if cut == "1/16+15/16" else (0.25,) * 4
        pipe = HostPipeline(layout, n, DEV, fractions=fr)
        assert _nonempty(pipe.ranges) == len(fr) == _nonempty(pipe.ranges_nb)
        assert [(lo, hi) for lo, hi, _ in pipe.ranges] == \
            [(lo, hi) for lo, hi, _ in pipe.ranges_nb]
        if len(fr) == 2:   # the small chunk first
            lo, hi, _ = pipe.ranges[0]
            assert 0 < hi - lo < layout.f32_numel // 8
    _three_fresh_rounds(pipe, Rows(layout, n + 3), n)


@pytest.mark.parametrize("nchunks", [0, 6])
@pytest.mark.parametrize("n", [5, 20])
def test_weighted_rounds(n, nchunks):
    """A3.  fp32 keys: the weighted sum; int64 keys keep the mean."""
    from feddct_amd.pipeline import HostPipeline
    layout = BucketLayout.from_manifest(_man("mid"))
    pipe = HostPipeline(layout, n, DEV, nchunks=nchunks)
    assert _nonempty(pipe.ranges) == (6 if nchunks else 5)
    rows = Rows(layout, n + 3)
    w = _weights(n)
    assert len(set(w.tolist())) == n
    _round(pipe, rows, n, _states("mid", 1, n), _want("mid", 1, n, ADV, True), (n + 1, n + 2),
           weights=w, what="w1")
    # an unweighted round between two weighted ones, then into the clients' own
    _round(pipe, rows, n, _states("mid", 2, n), _want("mid", 2, n), (n + 1,), what="u2")
    _round(pipe, rows, n, _states("mid", 3, n), _want("mid", 3, n, ADV, True), range(n),
           weights=list(map(float, w)), what="w3")


SWEEP_N = [1, 2, 8, 9, 11, 12, 16, 17, 64, 128, 129, 255, 256, 300]


@pytest.mark.parametrize("n,weighted", [(n, False) for n in SWEEP_N]
                         + [(n, True) for n in (2, 12, 17, 129)])
def test_client_counts_where_the_launch_changes(n, weighted):
    """A4.  Tile-subset plans through every pointer path and batch size: 8-
    versus 16-client kernels (12), inline versus table pointers (128 / 129),
    the deep cascade (256), with and without weights, on a layout of 56 tiles
    of 1024 with unaligned key lengths and scalar tails, in five chunks."""
    from feddct_amd.pipeline import HostPipeline
    layout = BucketLayout.from_manifest(H.SWEEP)
    pipe = HostPipeline(layout, n, DEV, tile_elems=H.SWEEP_TILE)
    assert _nonempty(pipe.ranges) == 5 and pipe.plan64 is not None
    rows = Rows(layout, n + 3)
    assert rows.b32.numel() * 4 + rows.b64.numel() * 8 < 64 << 20
    _round(pipe, rows, n, _states("sweep", 1, n), _want("sweep", 1, n, ADV, weighted),
           (n + 1, n + 2), weights=_weights(n) if weighted else None, what=("sweep", n))


@pytest.mark.parametrize("fanout", ["host", "dma"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["tiny", "onetile", "noi64", "nof32"])
def test_edge_layouts(name, n, fanout):
    """A5.  One non-empty range and the rest ``hi == lo`` with no plan; no
    int64 plan; no fp32 range at all."""
    from feddct_amd.pipeline import HostPipeline
    layout = BucketLayout.from_manifest(_man(name))
    pipe = HostPipeline(layout, n, DEV, fanout=fanout)
    assert len(pipe.ranges) == 5 and len(pipe.ranges_nb) == 2
    assert _nonempty(pipe.ranges) == H.NONEMPTY[name]["taper"]
    assert (pipe.plan64 is None) == (name == "noi64")
    if name == "nof32":
        assert all((lo, hi, p) == (0, 0, None) for lo, hi, p in pipe.ranges)
    rows = Rows(layout, n + 3)
    _three_fresh_rounds(pipe, rows, n, name)
    if n == 3:
        _round(pipe, rows, n, _states(name, 4, n), _want(name, 4, n, ADV, True), (n + 1, n + 2),
               weights=_weights(n), what="w4")
    # an even cut of the same layout: 63 of the 64 ranges are empty (tiny, onetile)
    pipe = HostPipeline(layout, n, DEV, nchunks=64, fanout=fanout)
    assert len(pipe.ranges) == 64 and _nonempty(pipe.ranges) == H.NONEMPTY[name]["even64"]
    _round(pipe, rows, n, _states(name, 5, n), _want(name, 5, n), (n + 1, n + 2), what="e5")


def test_client_count_and_weights_length_are_checked():
    """A7.  Another client count, or a weights array that is not one weight
    per client (a ctypes array would zero-fill the missing ones: the last
    clients silently at weight 0), raises before anything is enqueued."""
    from feddct_amd.pipeline import HostPipeline
    n = 3
    layout = BucketLayout.from_manifest(_man("mid"))
    pipe = HostPipeline(layout, n, DEV)
    rows = Rows(layout, n + 3)
    for i, st in enumerate(_states("mid", 1, n)):
        rows.put(i, st)
    out = [n, n + 1, n + 2]
    rows.poison(out)

    def run(k, weights):
        pipe.run(rows.r32(range(k)), rows.r64(range(k)), rows.b32[n], rows.b64[n],
                 rows.r32(out[1:]), rows.r64(out[1:]), weights=weights)
    with pytest.raises(ValueError, match="built for 3 clients, got 2"):
        run(2, None)
    for bad in ([0.5, 0.25], [0.5, 0.25, 0.125, 0.125], np.float32([[0.5, 0.5]]), []):
        k = int(np.asarray(bad).size)
        with pytest.raises(ValueError, match=f"{k} weights for 3 clients"):
            run(n, bad)
    torch.cuda.synchronize()
    assert all(rows.holds_sentinel(r) for r in out)
    # a [n, 1] array is flattened; the round still works after the refusals
    w = _weights(n)
    run(n, w.reshape(n, 1))
    for t in out:
        _same(rows.state(t), _want("mid", 1, n, ADV, True), ("after", t))


# ------------------------------------- B. the drop-in on host modules --
def _mods(man, states, device=None):
    ms = [StateModule(man).load_numpy(s) for s in states]
    return ms if device is None else [m.to(device) for m in ms]


def _load(mods, states):
    """New values in place (the training step's stand-in)."""
    for m, s in zip(mods, states):
        m.load_numpy(s)


def _poison(*mods):
    with torch.no_grad():
        for m in mods:
            for v in m.state_dict().values():
                v.fill_(S32 if v.dtype.is_floating_point else S64)


def _sd(m):
    return [(k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items()]


def _bytes(m):
    return {k: v.tobytes() for k, v in _sd(m)}


def _on_host(*mods):
    return all(v.device.type == "cpu" for m in mods for v in m.state_dict().values())


@pytest.mark.parametrize("mode", [REAL, ADV])
@pytest.mark.parametrize("variant", ["fedavg", "fedprox"])
def test_host_modules_match_reference_goldens(golden, variant, mode):
    """B1.  The reference's own bits at every golden N, both synth modes,
    for the global and every client."""
    sa = importlib.import_module(f"feddct_amd.{variant}").server_aggregate
    man = golden["manifest"]["small"]
    gold = golden["gold"]
    for n in golden["manifest"]["ns"]:
        g = StateModule(man)
        clients = _mods(man, [synth.gen_state(man, i, mode) for i in range(n)])
        _poison(g)
        sa(g, clients)
        assert _on_host(g, *clients)
        want = [(e["key"], gold[f"{variant}/m{mode}/n{n}/{e['key']}"]) for e in man["keys"]]
        for j, m in enumerate([g] + clients):
            _same(_sd(m), want, (variant, mode, n, j))


def test_full_size_host_round_digest(golden):
    """B2.  wrn16_8_c10, N = 2, host-resident (the benchmark's
    cfg1_host_resident_n2 shape): the taper at real scale, against the
    reference's digest.  The only large case here."""
    from feddct_amd.fedavg import server_aggregate
    man = load_manifest("wrn16_8_c10")
    g = StateModule(man)
    clients = _mods(man, [synth.gen_state(man, i, REAL) for i in range(2)])
    _poison(g)
    server_aggregate(g, clients)
    assert _on_host(g, *clients)
    want = golden["digests"]["fedavg/wrn16_8_c10/n2"]
    order = [e["key"] for e in man["keys"]]
    for m in [g] + clients:
        sd = m.state_dict()
        assert O.state_digest([(k, sd[k].numpy()) for k in order]) == want


def test_fresh_rounds_on_host_modules_and_a_change_of_n():
    """B3.  Three rounds on the same mid-shaped host modules with fresh
    values each, then N = 4 (a subset of them; the pipe is cached per N) and
    N = 6 again.  The clients left out of the middle round keep their bytes."""
    from feddct_amd.fedavg import server_aggregate
    man = _man("mid")
    n = 6
    g = StateModule(man)
    clients = _mods(man, _states("mid", 1, n))
    for r in (1, 2, 3):
        if r > 1:
            _load(clients, _states("mid", r, n))
        _poison(g)
        server_aggregate(g, clients)
        for j, m in enumerate([g] + clients):
            _same(_sd(m), _want("mid", r, n), (r, j))
    sub = [0, 2, 3, 5]
    st = _states("mid", 4, n)
    _load(clients, st)
    _poison(g)
    kept = {i: _bytes(clients[i]) for i in (1, 4)}
    server_aggregate(g, [clients[i] for i in sub])
    want = _oracle([st[i] for i in sub])
    for j, m in enumerate([g] + [clients[i] for i in sub]):
        _same(_sd(m), want, ("n4", j))
    for i in (1, 4):
        assert _bytes(clients[i]) == kept[i], i
    _load(clients, _states("mid", 5, n))
    _poison(g)
    server_aggregate(g, clients)
    for j, m in enumerate([g] + clients):
        _same(_sd(m), _want("mid", 5, n), ("n6 again", j))
    assert _on_host(g, *clients)


def test_weighted_on_host_modules():
    """B4.  aggregate_weighted with and without the broadcast; equal weights
    take the mean path; sizes= and weights= agree; a weights array of another
    length than the client list raises with nothing written (the host path
    used to zero-fill the missing weights)."""
    from feddct_amd.aggregate import aggregate_weighted
    man = _man("mid")
    n = 5
    w = _weights(n)
    sizes = np.arange(1, n + 1) * 13 + 5
    assert bits_equal(w, O.weights_from_sizes(sizes))
    g = StateModule(man)
    clients = _mods(man, _states("mid", 1, n))
    # wrong lengths first, on modules no round has touched, then on bound ones
    for bound in (False, True):
        before = [_bytes(m) for m in [g] + clients]
        for bad in (w[:2], w[:4], np.concatenate([w, w[:1]])):
            for bc in (True, False):
                with pytest.raises(ValueError, match=f"{len(bad)} weights for {n} clients"):
                    aggregate_weighted(g, clients, weights=bad, broadcast=bc)
        assert [_bytes(m) for m in [g] + clients] == before
        if not bound:
            _poison(g)
            before = [_bytes(c) for c in clients]
            aggregate_weighted(g, clients, weights=w, broadcast=False)
            _same(_sd(g), _want("mid", 1, n, ADV, True), "no broadcast")
            assert [_bytes(c) for c in clients] == before
    # sizes= gives the same weights; broadcast
    _poison(g)
    aggregate_weighted(g, clients, sizes=sizes)
    for j, m in enumerate([g] + clients):
        _same(_sd(m), _want("mid", 1, n, ADV, True), ("sizes", j))
    _load(clients, _states("mid", 2, n))
    _poison(g)
    aggregate_weighted(g, clients, weights=w)
    for j, m in enumerate([g] + clients):
        _same(_sd(m), _want("mid", 2, n, ADV, True), ("weights", j))
    # equal weights: x * (1/N) is not x / N — the mean path's bits
    _load(clients, _states("mid", 3, n))
    _poison(g)
    before = [_bytes(c) for c in clients]
    aggregate_weighted(g, clients, sizes=[7] * n, broadcast=False)
    _same(_sd(g), _want("mid", 3, n), "equal, no broadcast")
    assert [_bytes(c) for c in clients] == before
    _poison(g)
    aggregate_weighted(g, clients, weights=[0.2] * n)
    for j, m in enumerate([g] + clients):
        _same(_sd(m), _want("mid", 3, n), ("equal", j))
    assert _on_host(g, *clients)


@pytest.mark.parametrize("variant", ["feddct", "splitfed"])
def test_split_call_on_host_modules(golden, variant):
    """B5.  All four model lists on host: the small split goldens, then a
    second round on fresh values against the oracle of each half."""
    sa = importlib.import_module(f"feddct_amd.{variant}").server_aggregate
    mm, pm = golden["manifest"]["main"], golden["manifest"]["proxy"]
    gold = golden["gold"]
    for n in (5, 24):
        sm = [synth.gen_state(mm, i, ADV) for i in range(n)]
        sp = [synth.gen_state(pm, 100 + i, ADV) for i in range(n)]
        ms, ps = _mods(mm, sm), _mods(pm, sp)
        gm, gp = StateModule(mm), StateModule(pm)
        _poison(gm, gp)
        sa(gm, gp, ms, ps)
        for part, man, g, cl, st in (("main", mm, gm, ms, sm), ("proxy", pm, gp, ps, sp)):
            want = [(e["key"], gold[f"{variant}/n{n}/{part}/{e['key']}"]) for e in man["keys"]]
            own = _oracle(st)
            for (k, a), (_, b) in zip(want, own):
                assert bits_equal(np.asarray(a), b), (part, k, "golden vs oracle")
            for j, m in enumerate([g] + cl):
                _same(_sd(m), want, (variant, n, part, j))
        sm = [synth.gen_state(mm, 2000 + i, ADV) for i in range(n)]
        sp = [synth.gen_state(pm, 2100 + i, ADV) for i in range(n)]
        _load(ms, sm)
        _load(ps, sp)
        _poison(gm, gp)
        sa(gm, gp, ms, ps)
        for part, g, cl, st in (("main", gm, ms, sm), ("proxy", gp, ps, sp)):
            want = _oracle(st)
            for j, m in enumerate([g] + cl):
                _same(_sd(m), want, (variant, n, part, "round 2", j))
        assert _on_host(gm, gp, *ms, *ps)


BASE = [("w", [100], "float32"), ("h", [70], "float16"), ("c", [3, 33], "float32"),
        ("n", [], "int64"), ("s", [], "float32")]
PACKED = [("h", [70], "float16"), ("d", [33], "float64"), ("b", [5], "bool"),
          ("i", [4], "int32"), ("f", [40], "float32")]


def _dman(base, overrides=None):
    o = overrides or {}
    return {"keys": [{"key": k, "shape": sh, "dtype": o.get(k, dt)} for k, sh, dt in base]}


def _filled(man, seed, scale=3.0):
    m = StateModule(man)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.dtype.is_floating_point:
                v.copy_(torch.randn(v.shape, generator=gen) * scale)
            elif v.dtype == torch.bool:
                v.copy_(torch.randint(0, 2, v.shape, generator=gen))
            else:
                v.copy_(torch.randint(-99, 1000, v.shape, generator=gen))
    return m


def _check_like(ours, ref, what):
    for k, v in ref.state_dict().items():
        o = ours.state_dict()[k]
        assert o.dtype == v.dtype and o.device.type == "cpu", (what, k)
        assert torch.equal(o.detach(), v.detach()), (what, k)


@pytest.mark.parametrize("case", ["client_dtypes", "packed", "half", "bfloat16"])
def test_staged_dtypes_on_host_modules(case):
    """B6.  Keys whose dtype is not the bucket's are staged per call, on
    host as on the device; an all-fp16 / all-bf16 host model set is laid out
    in fp32 and staged.  Against the reference loop on deep copies (keys of at
    most 100 elements, N = 9), two rounds."""
    from feddct_amd.fedavg import server_aggregate
    n = 9
    if case == "client_dtypes":
        variants = [{}, {"w": "float16", "h": "float32", "n": "int32"},
                    {"w": "float64", "h": "bfloat16", "c": "float16"},
                    {"s": "float64", "n": "int16", "h": "float64"}]
        g_ref = _filled(_dman(BASE), 1000)
        c_ref = [_filled(_dman(BASE, variants[i % 4]), i) for i in range(n)]
    elif case == "packed":
        g_ref = _filled(_dman(PACKED), 1000)
        c_ref = [_filled(_dman(PACKED), i) for i in range(n)]
    else:
        cast = (lambda m: m.half()) if case == "half" else (lambda m: m.bfloat16())
        man = _dman(BASE, {"h": "float32"})
        g_ref = cast(_filled(man, 1000))
        c_ref = [cast(_filled(man, i)) for i in range(n)]
        assert g_ref.w.dtype in (torch.float16, torch.bfloat16) and g_ref.n.dtype == torch.int64
    g, clients = copy.deepcopy(g_ref), [copy.deepcopy(c) for c in c_ref]
    for r in range(2):
        if r:
            with torch.no_grad():   # the same new values into both copies
                for i, (c, cr) in enumerate(zip(clients, c_ref)):
                    for v, w in zip(c.state_dict().values(), cr.state_dict().values()):
                        if w.dtype.is_floating_point:
                            w.mul_(1.0 + (i + 1) / 7)
                            v.copy_(w)
        reference_loop(g_ref, c_ref)
        server_aggregate(g, clients)
        _check_like(g, g_ref, (case, r, "global"))
        for i, (c, cr) in enumerate(zip(clients, c_ref)):
            _check_like(c, cr, (case, r, i))


@pytest.mark.parametrize("strict", [False, True])
def test_host_round_under_the_torch_gpu_order(strict):
    """B7.  Host-resident modules always take the CPU order — no fallback
    warning, no fallback count — whatever order device rounds reproduce."""
    from feddct_amd import aggregate as A
    man = _man("mid")
    n = 6
    e = A.engine()
    prev = (e.order, e.strict_gpu_order)
    g = StateModule(man)
    clients = _mods(man, _states("mid", 1, n))
    try:
        A.set_summation_order("torch_gpu", strict=strict)
        counts = dict(e.gpu_order_fallbacks)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for r in (1, 2):
                if r > 1:
                    _load(clients, _states("mid", r, n))
                _poison(g)
                A.server_aggregate(g, clients)
                for j, m in enumerate([g] + clients):
                    _same(_sd(m), _want("mid", r, n), (strict, r, j))
        assert not [w for w in rec if issubclass(w.category, RuntimeWarning)], \
            [str(w.message) for w in rec]
        assert e.gpu_order_fallbacks == counts
        assert A.summation_order() == "torch_gpu"
    finally:
        A.set_summation_order(prev[0], strict=prev[1])


def test_host_errors_like_the_reference():
    """B8.  What the reference raises, on host modules."""
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "w", "shape": [4097], "dtype": "float32"},
                    {"key": "n", "shape": [], "dtype": "int64"}]}
    st = [synth.gen_state(man, i, ADV) for i in range(3)]
    g = _mods(man, [synth.gen_state(man, 77, ADV)])[0]
    with pytest.raises(RuntimeError):
        server_aggregate(g, [])
    other = StateModule({"keys": [{"key": "v", "shape": [4097], "dtype": "float32"},
                                  {"key": "n", "shape": [], "dtype": "int64"}]})
    with pytest.raises(KeyError):
        server_aggregate(g, _mods(man, st[:1]) + [other])
    bad = StateModule({"keys": [{"key": "w", "shape": [4098], "dtype": "float32"},
                                {"key": "n", "shape": [], "dtype": "int64"}]})
    before = _bytes(g)
    with pytest.raises(RuntimeError, match="stack expects each tensor to be equal size"):
        server_aggregate(g, _mods(man, st[:1]) + [bad])
    assert _bytes(g) == before
    # an extra key: reduced, the global loaded, the broadcast in order up to
    # that client, which raises as load_state_dict(strict=True) does
    eman = {"keys": man["keys"] + [{"key": "z", "shape": [2], "dtype": "float32"}]}
    c0, c2 = _mods(man, [st[0], st[2]])
    extra = StateModule(eman).load_numpy(st[1])
    _poison(g)
    after = _bytes(c2)
    with pytest.raises(RuntimeError, match="Missing key"):
        server_aggregate(g, [c0, extra, c2])
    want = _oracle(st)
    _same(_sd(g), want, "global")
    _same(_sd(c0), want, "the client before")
    assert _bytes(c2) == after
    assert _on_host(g, c0, extra, c2)
    # a parameter replaced between rounds is seen (re-bind)
    clients = _mods(man, st)
    server_aggregate(g, clients)
    _same(_sd(g), want, "bound")
    st2 = [synth.gen_state(man, 500 + i, ADV) for i in range(3)]
    _load(clients, st2)
    new = torch.from_numpy(np.array(st2[1][0][1], copy=True)) * 3
    clients[1].w.data = new.clone()
    st2[1] = [("w", new.numpy()), st2[1][1]]
    _poison(g)
    server_aggregate(g, clients)
    want = _oracle(st2)
    for j, m in enumerate([g] + clients):
        _same(_sd(m), want, ("re-bound", j))


def test_modules_moving_between_host_and_gpu():
    """B9.  A host round, the same modules moved to the GPU and a device
    round, back to the host and a host round."""
    from feddct_amd.fedavg import server_aggregate
    man = _man("mid")
    n = 4
    g = StateModule(man)
    clients = _mods(man, _states("mid", 1, n))
    for r, where in ((1, "cpu"), (2, "cuda"), (3, "cpu"), (4, "cuda")):
        if r > 1:
            g = g.to(DEV if where == "cuda" else "cpu")
            clients = [c.to(DEV if where == "cuda" else "cpu") for c in clients]
            _load(clients, _states("mid", r, n))
        _poison(g)
        server_aggregate(g, clients)
        torch.cuda.synchronize()
        for j, m in enumerate([g] + clients):
            assert all(v.device.type == where for v in m.state_dict().values())
            _same(_sd(m), _want("mid", r, n), (r, where, j))


@pytest.mark.parametrize("where", ["global_gpu", "global_host"])
def test_global_and_clients_apart_on_mid(where):
    """B10.  The global on the GPU over host clients (the pipeline downloads
    into a device bucket) and the global on the host over GPU clients, on
    133k floats in five chunks, two fresh rounds each."""
    from feddct_amd.fedavg import server_aggregate
    man = _man("mid")
    n = 6
    g = StateModule(man)
    clients = _mods(man, _states("mid", 1, n))
    if where == "global_gpu":
        g = g.to(DEV)
    else:
        clients = [c.to(DEV) for c in clients]
    for r in (1, 2):
        if r > 1:
            _load(clients, _states("mid", r, n))
        _poison(g)
        server_aggregate(g, clients)
        torch.cuda.synchronize()
        assert next(g.parameters()).device.type == ("cuda" if where == "global_gpu" else "cpu")
        assert all(next(c.parameters()).device.type != next(g.parameters()).device.type
                   for c in clients)
        for j, m in enumerate([g] + clients):
            _same(_sd(m), _want("mid", r, n), (where, r, j))
