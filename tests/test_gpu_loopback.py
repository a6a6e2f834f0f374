"""GPU: the native multi-rank rounds of libfedagg_comm (fedcomm.hip, unchanged)
with W = 2..8 ranks on the one GPU of the box, over an in-process loopback of
the RCCL calls it makes (tests/loopback/loopccl.hip; RCCL itself refuses two
ranks on one device).  The C++ driver (tests/loopback/loop_round.cpp) builds
the clients with the portable synthetic state, runs one round per case — or a
script of several rounds on one plan per rank — and compares every result
rank of every round with one GPU's fa_reduce over all clients:
chained, striped and blocked bit for bit, sharded (e1) within the forward error bound
of two N-term sums; int64 keys bit for bit everywhere.

Both process models of fedcomm run: one thread + communicator per rank
(fa_comm_init_rank — the product's one-process-per-GPU model, ranks progress
independently) for every mode, and one thread driving every rank
(fa_comm_init) for the sharded and blocked rounds.  The chained and striped schedules
pair a send in one step with its receive in a later step of another rank;
RCCL matches those on the device, a host-side loopback driven by one thread
cannot (the receive would wait for a send the same thread has not issued),
so their single-thread form is left to tests/schedsim.py.  Cases cover
uneven counts, a rank without clients, every root (first, middle, last, all),
weighted rounds, 1..13 column chunks, N >= 256 (the deep cascade's four state
planes) and the layouts of BASELINE configs 3 and 5.

A plan lives for a whole federated run, and nearly all its staging is
allocated zero-filled, so a path that reads what its own round has not
written is right in round one and wrong in round two.  The scripted cases
(test_loopback_rounds_on_one_plan, test_loopback_rounds_deep_blocked) run two
to four rounds per plan with fresh client data written in place, other
weights, another root and a switch between mean and weighted every round,
without a host synchronisation in between, and check every round and that no
round wrote its inputs.  The rounds also run once on adversarial data
(exponents 2^-20..2^20, random signs: test_loopback_small_layout_adversarial)
and on the special values of tests/specials.py (inf, NaN, -0.0, subnormals,
overflow, inf - inf, weights 0 / subnormal / negative / inf:
test_loopback_special_values), there also against the oracle's arithmetic,
which does not depend on fa_reduce.  tests/test_schedule.py replays the same
schedules under the same special values on a CPU, so a difference here is the
executor's."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import load_manifest
from feddct_amd.layout import BucketLayout
from feddct_amd.workload import joint_manifest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "loopback", "loop_round")


def _write_layout(layout, path, params=None):
    """``params``: {offset: (key_index, mu, sigma)} per fp32 segment and
    {offset: key_index} per int64 one — the digest generator's inputs."""
    with open(path, "w") as f:
        f.write(f"{layout.f32_numel} {layout.i64_numel} {len(layout.segs32)} "
                f"{len(layout.segs64)}{' P' if params else ''}\n")
        for o, m in layout.segs32:
            extra = ""
            if params:
                k, mu, sg = params[0][int(o)]
                extra = f" {k} {float(np.float32(mu)):.9g} {float(np.float32(sg)):.9g}"
            f.write(f"{int(o)} {int(m)}{extra}\n")
        for o, m in layout.segs64:
            extra = f" {params[1][int(o)]}" if params else ""
            f.write(f"{int(o)} {int(m)}{extra}\n")


def _digest_params(layout, parts):
    """Per-segment generator parameters of a (joint) layout: key index = the
    key's position in its own manifest (feddct_amd/workload.py fill_client)."""
    from feddct_amd import synth
    p32, p64 = {}, {}
    for man, prefix in parts:
        for j, e in enumerate(man["keys"]):
            s = layout.by_key[prefix + e["key"]]
            if s.kind == "i64":
                p64[s.offset] = j
            else:
                mu, sg = synth.key_params(e["key"], tuple(e["shape"]), e["dtype"])
                p32[s.offset] = (j, mu, sg)
    return p32, p64


def _run(layout, cases, tmp_path, timeout=240, params=None, dump=None, profile=False,
         clients=None, weights=None, gate_ms=0):
    """``clients`` / ``weights``: files of round 0's fp32 client buckets and
    weights (FA_LOOP_CLIENTS / FA_LOOP_WEIGHTS) instead of the generator's;
    ``gate_ms``: FA_LOOP_GATE_MS, every later round issued behind a gate."""
    assert os.path.exists(DRIVER), "tests/loopback/loop_round is not built (run build())"
    lf = str(tmp_path / "layout.txt")
    _write_layout(layout, lf, params)
    env = dict(os.environ, FA_LOOP_TIMEOUT_S="30")
    if profile:
        env["FA_LOOP_PROFILE"] = "1"
    if gate_ms:
        env["FA_LOOP_GATE_MS"] = str(gate_ms)
    if dump:
        env["FA_LOOP_DUMP"] = dump
    if clients:
        env["FA_LOOP_CLIENTS"] = clients
    if weights:
        env["FA_LOOP_WEIGHTS"] = weights
    p = subprocess.run([DRIVER, lf, *cases], capture_output=True, text=True, timeout=timeout,
                       env=env)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    for r in rows:
        print(json.dumps(r))
    assert len(rows) == len(cases), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    bad = [r for r in rows if not r["ok"]]
    assert not bad, (bad, p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
    return rows


def _small_layout():
    """Every column class the schedules treat separately: vector runs, ILP-4
    tails, 0-d fp32 keys between vector keys, unaligned sizes, int64 keys."""
    return BucketLayout([("a", (37, 3), "float32"), ("s", (), "float32"),
                         ("b", (4101,), "float32"), ("t", (), "float32"),
                         ("c", (70000,), "float32"), ("d", (3,), "float32"),
                         ("e", (193,), "float32"), ("n1", (), "int64"),
                         ("f", (65, 65), "float32"), ("n2", (), "int64")])


@pytest.fixture(scope="module")
def cfg3_layout():
    mm, pm = load_manifest("wrnsl16_8_sf4_c10_main"), load_manifest("wrnsl16_8_sf4_c10_proxy")
    return BucketLayout.from_manifest(joint_manifest([mm, pm]))


SMALL_CASES = [
    "chained:2:3,2:-1:threads:0:1",
    "chained:3:2,0,3:0:threads:0:4",
    "chained:3:4,5,3:1:threads:1:3",
    "chained:5:4,4,4,4,4:4:threads:1:13",
    "chained:8:1,2,1,3,1,1,2,9:-1:threads:0:8",
    "chained:4:65,65,65,65:3:threads:0:4",          # N=260: four state planes
    "striped:2:3,2:0:threads:0:0",
    "striped:3:2,0,3:-1:threads:0:0",
    "striped:8:1,2,1,3,1,1,2,9:5:threads:0:0",
    "striped:4:65,65,65,65:-1:threads:0:0",          # N=260: device pointer tables
    # r06: every peer in one group per chunk; chunk counts; weighted
    "striped:8:3,3,3,3,3,3,3,3:7:threads:0:1",
    "striped:8:3,3,3,3,3,3,3,3:-1:threads:1:3",
    "striped:5:4,0,2,1,6:2:threads:1:8",
    "striped:3:2,5,1:-1:threads:1:2",
    "striped:4:65,65,65,65:0:threads:1:4",           # weighted, N=260
    "sharded:4:65,65,65,65:0:threads:1:4",
    "sharded:2:3,2:0:threads:0:8",
    "sharded:4:5,0,2,1:-1:threads:1:4",
    "sharded:3:4,5,3:2:single:0:1",
    "sharded_rs:2:3,2:0:threads:0:8",
    "sharded_rs:4:5,1,2,1:-1:threads:1:4",
    "sharded_rs:8:1,2,1,3,1,1,2,9:7:threads:0:13",
    "sharded_rs:3:4,5,3:-1:single:0:2",
    "blocked:1:20:0:threads:0:0",
    "blocked:2:10,10:1:threads:0:0",
    "blocked:3:7,0,13:-1:threads:1:0",
    "blocked:3:16,16,1:0:single:0:0",
    "blocked:8:20,20,20,20,20,20,20,20:0:threads:0:0",
    "blocked:8:20,20,20,20,20,20,20,20:-1:single:1:0",
    "blocked:6:12,9,30,0,14,8:4:threads:0:0",
    "blocked:3:100,156,44:-1:threads:0:0",            # N=300: the fold's level 2
    # r05: the default entry picks the exact form from the counts
    "multi:8:1,2,1,3,1,1,2,9:-1:threads:0:0",
    "multi:3:7,0,13:-1:threads:1:0",
    "multi:4:65,65,65,65:3:threads:1:0",               # N=260
    "multi_e1:4:5,0,2,1:-1:threads:1:4",               # opt-in e1: error bound
    "mean_multi:3:4,5,3:2:threads:0:0",                # stateless fp32 form
    "mean_multi:8:3,3,3,3,3,3,3,3:-1:threads:0:0",
]


def test_loopback_small_layout_all_modes(tmp_path):
    _run(_small_layout(), SMALL_CASES, tmp_path)


def _deep_layout():
    """_small_layout() with ``c`` cut to 6500 floats (~11 k floats in all):
    every column class still there, thousands of clients stay cheap."""
    return BucketLayout([("a", (37, 3), "float32"), ("s", (), "float32"),
                         ("b", (4101,), "float32"), ("t", (), "float32"),
                         ("c", (6500,), "float32"), ("d", (3,), "float32"),
                         ("e", (193,), "float32"), ("n1", (), "int64"),
                         ("f", (65, 65), "float32"), ("n2", (), "int64")])


DEEP_CASES = [
    "blocked:2:250,10:0:threads:0:0",          # the spanning block ends at 256: CONT plane 2
    "blocked:2:250,10:-1:single:1:0",
    "blocked:2:4090,10:0:threads:0:0",         # ... at 4096: CONT plane 3; 257 pieces, copied
    "blocked:2:4090,6:-1:threads:1:0",         # N = 4096: finishing continuation, 256 pieces
    "blocked:3:4090,4110,30:-1:threads:0:0",   # N = 8230: 515 pieces, l3 twice, three owners
    "chained:2:4096,5:1:threads:0:3",          # plane 3 alone crosses the hop
    "chained:3:4090,4110,30:-1:threads:1:4",
    "striped:2:4090,10:-1:threads:1:2",        # K_SCALE / the stacks in 64 launches of 64 rows
    "multi:3:4090,4110,30:0:threads:0:0",      # whatever the cost model picks stays exact
    # a one-rank communicator runs no fold (its round is one fa_reduce), so the
    # fold's piece counts around kFoldPtrs = 256 are all pinned here
    "blocked:2:4090,22:0:threads:0:0",         # N = 4112: 257 whole blocks, no remainder
    "blocked:2:4090,7:-1:threads:1:0",         # N = 4097 weighted: 257 pieces, a one-row remainder
    "blocked:2:4096,16:1:single:0:0",          # no spanning block: 257 local block sums
    "blocked:2:4090,310:-1:single:0:0",        # N = 4400: levels 1 and 2 open over one l3 promotion
]


@pytest.mark.parametrize("part", [0, 1, 2])
def test_loopback_deep_cascade(tmp_path, part):
    """N >= 4096 across ranks: the chain state's fourth plane over a hop, the
    blocked round's continuation planes 2 and 3, the owners' folds of 256
    pieces (read where they lie), of 257 (copied into the fold's rows, with
    and without a remainder) and of 515 (two level-3 promotions), the scale /
    stack kernels in 64 launches.  In three driver runs, so that none waits
    on thousands of client allocations for long."""
    _run(_deep_layout(), DEEP_CASES[part::3], tmp_path, timeout=300)


def test_loopback_cfg3_layout(cfg3_layout, tmp_path):
    """BASELINE config 3's joint FedDCT bucket (main + proxy, 11.0 M floats),
    5 client slots over 2..5 ranks."""
    cases = [
        "chained:2:3,2:-1:threads:0:8",
        "chained:5:1,1,1,1,1:4:threads:0:8",
        "chained:3:2,1,2:0:threads:1:4",
        "striped:2:3,2:1:threads:0:0",
        "striped:4:2,1,1,1:-1:threads:0:0",
        "striped:5:1,1,1,1,1:4:threads:0:4",
        "striped:5:1,1,1,1,1:-1:threads:1:2",
        "sharded:2:3,2:0:threads:0:8",
        "sharded_rs:4:2,1,1,1:-1:threads:1:8",
        "blocked:2:3,2:0:threads:0:0",
        "blocked:2:20,20:-1:threads:1:0",
    ]
    _run(cfg3_layout, cases, tmp_path)


def test_loopback_cfg5_sharded_chain(tmp_path):
    """BASELINE config 5's shape: 24 FedDCT slots (wrnsl16_8 sf4 C100) over
    8 ranks of 3 slots, chained to the last rank and to every rank, and
    striped (r06: every peer in one group per chunk) in 1 and 4 chunks,
    weighted too."""
    mm, pm = load_manifest("wrnsl16_8_sf4_c100_main"), load_manifest("wrnsl16_8_sf4_c100_proxy")
    lay = BucketLayout.from_manifest(joint_manifest([mm, pm]))
    cases = ["chained:8:3,3,3,3,3,3,3,3:7:threads:0:8",
             "chained:8:3,3,3,3,3,3,3,3:-1:threads:0:8",
             "striped:8:3,3,3,3,3,3,3,3:-1:threads:0:4",
             "striped:8:3,3,3,3,3,3,3,3:7:threads:1:1"]
    _run(lay, cases, tmp_path, timeout=300)


def test_loopback_blocked_bench_shape(tmp_path):
    """The bench's N>1 shape: 20 wrn16_8 clients per rank, 4 and 8 ranks
    (160 slots: 10 blocks, six of them cut by a shard boundary), the
    result on rank 0 and on every rank."""
    lay = BucketLayout.from_manifest(load_manifest("wrn16_8_c10"))
    cases = ["blocked:4:20,20,20,20:0:threads:0:0",
             "blocked:8:20,20,20,20,20,20,20,20:0:threads:0:0",
             "blocked:8:20,20,20,20,20,20,20,20:-1:threads:0:0"]
    _run(lay, cases, tmp_path, timeout=300)


def test_loopback_cfg5_default_entry_matches_reference_digest(tmp_path):
    """the DEFAULT multi-GPU entry (fa_multi_plan_create /
    fa_reduce_multi — no form named by the caller) on BASELINE config 5's
    shape, 24 FedDCT slots (wrnsl16_8 sf4 C100, main + proxy in one bucket)
    over 8 ranks of 3 slots, with the digest generator's inputs: the result
    rank's main and proxy halves hash to the digests the REFERENCE's own
    server_aggregate produced (tests/golden/digests.json, n24), and equal one
    GPU's reduction bit for bit.  With 3 slots per rank a 16-slot cascade
    block spans 6 ranks (no blocked round); r06: the cost model takes the
    link-parallel striped round (r05: chained)."""
    from feddct_amd import dist
    mm, pm = load_manifest("wrnsl16_8_sf4_c100_main"), load_manifest("wrnsl16_8_sf4_c100_proxy")
    lay = BucketLayout.from_manifest(joint_manifest([mm, pm]))
    assert dist.exact_form([3] * 8, lay) == "striped"
    params = _digest_params(lay, [(mm, "0."), (pm, "1.")])
    dump = str(tmp_path / "out.bin")
    rows = _run(lay, ["multi:8:3,3,3,3,3,3,3,3:7:threads:0:0"], tmp_path, timeout=300,
                params=params, dump=dump)
    assert rows[0]["check"] == "bit-exact"
    raw = open(dump, "rb").read()
    f32 = np.frombuffer(raw[:4 * lay.f32_numel], np.float32)
    i64 = np.frombuffer(raw[4 * lay.f32_numel:], np.int64)
    with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as f:
        want = json.load(f)
    for prefix, name in (("0.", "main"), ("1.", "proxy")):
        h = hashlib.sha256()
        for s in lay.slots:
            if not s.key.startswith(prefix):
                continue
            src = i64 if s.kind == "i64" else f32
            h.update(s.key[len(prefix):].encode())
            h.update(np.ascontiguousarray(src[s.offset:s.offset + s.numel]).tobytes())
        assert h.hexdigest() == want[f"feddct/wrnsl16_8_sf4_c100_{name}/n24"], name


def test_loopback_default_entry_random_shards(tmp_path):
    """The default entry over seeded random shard shapes (W = 2..8, 0..40
    slots per rank, empty ranks, every root, weighted and not): whatever form
    and chunk count the cost model picks, the result equals one GPU's
    reduction of all the slots bit for bit."""
    from feddct_amd import dist
    rng = np.random.default_rng(20260518)
    cases, forms = [], set()
    while len(cases) < 14:
        w = int(rng.integers(2, 9))
        counts = [int(c) for c in rng.integers(0, 41, size=w)]
        counts = [c if rng.random() > 0.15 else 0 for c in counts]
        if sum(counts) == 0:
            continue
        holders = [r for r, c in enumerate(counts) if c]
        root = int(rng.choice(holders + [-1]))
        forms.add(dist.exact_form(counts, _small_layout(), root_all=root < 0))
        cases.append(f"multi:{w}:{','.join(map(str, counts))}:{root}:threads:"
                     f"{int(rng.random() < 0.5)}:0")
    print("forms", sorted(forms))
    _run(_small_layout(), cases, tmp_path, timeout=300)


def test_loopback_default_entry_each_form(tmp_path):
    """The default entry's three exact forms each run at least once on the
    loopback: shapes the model sends to blocked, to chained and to striped
    (on a layout where a long chain of small hops loses to the stripes and
    the blocks win for many slots per rank)."""
    from feddct_amd import dist
    lay = BucketLayout([("a", (300000,), "float32"), ("s", (), "float32"),
                        ("b", (4101,), "float32"), ("n1", (), "int64")])
    shapes = {"striped": [3] * 8, "blocked": [20] * 4, "chained": [60, 60]}
    for form, counts in shapes.items():
        assert dist.exact_form(counts, lay) == form, (form, dist.exact_form(counts, lay))
    cases = [f"multi:{len(c)}:{','.join(map(str, c))}:{len(c) - 1}:threads:{i % 2}:0"
             for i, c in enumerate(shapes.values())]
    _run(lay, cases, tmp_path, timeout=300)


def test_loopback_round_profiles(tmp_path):
    """fa_comm_set_profile / fa_round_plan_profile (r06):
    a profiled round of each exact form reports its RCCL groups, its kernels
    and its wall time (rank 0 of the loopback), and stays bit-exact."""
    cases = ["striped:4:3,3,3,3:-1:threads:0:2", "chained:4:3,3,3,3:3:threads:0:4",
             "blocked:2:10,10:0:threads:1:0", "multi:8:3,3,3,3,3,3,3,3:7:threads:0:0"]
    rows = _run(_small_layout(), cases, tmp_path, profile=True)
    for r in rows:
        p = r["profile"]
        assert p is not None, r
        assert p["groups"] > 0 and p["kernels"] > 0 and p["wall_us"] > 0, r
        assert p["exchange_us"] > 0, r


# ---- several rounds on one plan ---------------------------------------------
# CASE:script — one entry per round, its root and m (mean) / w (weighted); `a`:
# adversarial data.  One plan and one communicator per rank for the whole
# script; fresh client data (in place), other weights every round.
E8 = "1,2,1,3,1,1,2,9"
ROUND_CASES = {
    "chained": [
        # back to the first schedule after two others have used the buffers
        "chained:3:4,5,3:1:threads:0:3:1m,-1w,0w,1m",
        "chained:4:65,65,65,65:3:threads:0:4:3m,0w,-1m",        # N=260: four state planes
        f"chained:8:{E8}:-1:threads:0:8:-1m,5w,-1m,a",
    ],
    "striped": [
        "striped:5:4,0,2,1,6:2:threads:0:8:2m,2w,-1w,0m",       # WSTAGE allocated by round 2
        "striped:4:65,65,65,65:-1:threads:0:0:-1m,0w,-1m",      # N=260: device pointer tables
        "striped:8:3,3,3,3,3,3,3,3:7:threads:1:3:7w,-1m,7w,a",
    ],
    "blocked": [
        "blocked:3:7,0,13:-1:threads:1:0:-1w,0m,2m",
        "blocked:8:20,20,20,20,20,20,20,20:0:threads:0:0:0m,-1w,0m",
        "blocked:3:100,156,44:-1:threads:0:0:-1m,1w,-1m",       # N=300: the fold's level 2
        "blocked:3:16,16,1:0:single:0:0:0m,2w,0m",
    ],
    "sharded": [                                                 # e1: the bound, per round
        "sharded:4:5,0,2,1:0:threads:0:4:0m,-1w,0m",            # a rank without clients: K_ZERO
        "sharded_rs:4:5,0,2,1:0:threads:0:4:0m,-1w,0m",
        "sharded:3:4,5,3:0:single:0:1:0m,-1w,0m",
        "sharded_rs:3:4,5,3:0:single:0:2:0m,-1w,0m",
    ],
    "multi": [
        f"multi:8:{E8}:-1:threads:0:0:-1m,3w,-1m",
        "multi:4:65,65,65,65:3:threads:1:0:3w,0m,a",
        "mean_multi:3:4,5,3:2:threads:0:0:2m,0m,-1m",           # the plan cached in the communicator
    ],
}


def _check_rounds(rows, cases):
    for r, c in zip(rows, cases):
        script = [e for e in c.split(":")[7].split(",") if e != "a"]
        assert r["rounds"] == len(script), r
        assert r["round_ok"] == [True] * len(script) and r["bad_round"] == 0, r
        assert r["bad_inputs"] == 0, r
        # the last round's result ranks
        assert r["result_ranks"] == (int(c.split(":")[1]) if script[-1][:-1] == "-1" else 1), r
        assert r["check"] == ("error bound" if c.startswith("sharded") else "bit-exact"), r


@pytest.mark.parametrize("form", sorted(ROUND_CASES))
def test_loopback_rounds_on_one_plan(tmp_path, form):
    """Two to four rounds on one plan per rank, every round with fresh client
    data (written in place on the rank's stream, no host synchronisation
    between rounds), other weights and, per the script, another root and mean
    or weighted: what a round leaves in the plan's staging (the zero-filled
    planes, PARTIAL, the receive rows, WSTAGE, the schedule cache) must not
    reach the next round's result.  Every round equals one GPU's reduction of
    that round's data (e1: within that round's bound), and the client buckets
    still hold the last round's data afterwards."""
    cases = ROUND_CASES[form]
    _check_rounds(_run(_small_layout(), cases, tmp_path), cases)


GATED_CASES = [c for form in sorted(ROUND_CASES) for c in ROUND_CASES[form][:1]] + [
    ROUND_CASES["sharded"][1], ROUND_CASES["multi"][2]]


def test_loopback_rounds_behind_a_gate(tmp_path):
    """Stream order of the executor (fedcomm.hip) with two and more ranks: one
    scripted case per round form, every rank's later rounds issued while a
    spin kernel still holds back, on the rank's own stream, the writes of that
    round's client data (FA_LOOP_GATE_MS, loop_round.cpp).  Whatever the
    executor queues for such a round — the exchanges, the /N finish and the
    int64 gather on its communication stream, the kernels on the caller's —
    runs in stream order behind those writes only through its entry join of
    the two streams; without it the communication stream reads the previous
    round's data and the round's result is wrong.  The driver fails a round
    whose call returned after its gate had ended."""
    assert all(":threads:" in c for c in GATED_CASES) and len(GATED_CASES) == 7
    _check_rounds(_run(_small_layout(), GATED_CASES, tmp_path, gate_ms=30), GATED_CASES)


def test_loopback_rounds_deep_blocked(tmp_path):
    """Two rounds (mean on rank 0, then weighted on every rank) on the blocked
    plans whose owner folds 256 pieces where they lie (bound in place) and 257
    (copied into the fold's rows)."""
    cases = ["blocked:2:4090,6:0:threads:0:0:0m,-1w",
             "blocked:2:4090,22:0:threads:0:0:0m,-1w"]
    _check_rounds(_run(_deep_layout(), cases, tmp_path, timeout=300), cases)


def test_loopback_small_layout_adversarial(tmp_path):
    """test_loopback_small_layout_all_modes' cases once more on adversarial
    data (fa_synth_fill_* mode 1: exponents 2^-20..2^20, random signs, int64
    values up to 2^25 in magnitude), where the order of every addition shows
    in the bits; the e1 cases keep their bound."""
    cases = [c + ":a" for c in SMALL_CASES]
    rows = _run(_small_layout(), cases, tmp_path)
    for r, c in zip(rows, cases):
        e1 = c.startswith("sharded") or c.startswith("multi_e1")
        assert r["check"] == ("error bound" if e1 else "bit-exact"), r
        assert r["rounds"] == 1 and r["bad_inputs"] == 0, r


# ---- special values -----------------------------------------------------------
def _special_layout():
    """_small_layout()'s column classes in about 10 k floats: vector runs that
    give each of 3 or 4 ranks a stripe, ILP-4 tails, 0-d fp32 keys between
    vector keys, unaligned sizes, int64 keys."""
    return BucketLayout([("a", (37, 3), "float32"), ("s", (), "float32"),
                         ("b", (2101,), "float32"), ("t", (), "float32"),
                         ("c", (6000,), "float32"), ("d", (3,), "float32"),
                         ("e", (193,), "float32"), ("n1", (), "int64"),
                         ("f", (33, 33), "float32"), ("n2", (), "int64")])


_SPECIAL = {}


def _special_inputs(n, mode):
    """Client buckets [n, f32_numel] with specials.pattern_matrix planted per
    fp32 key (phase = the key's index; the gaps ordinary normals, as
    specials.fill), the weights, and the oracle's result per key — computed
    once per (n, mode) and left unchanged."""
    import specials
    if (n, mode) not in _SPECIAL:
        lay = _special_layout()
        rng = np.random.default_rng(1000003 * n + 17)
        x = rng.standard_normal((n, lay.f32_numel)).astype(np.float32)
        f32 = [s for s in lay.slots if s.kind != "i64"]
        for j, s in enumerate(f32):
            x[:, s.offset:s.offset + s.numel] = specials.pattern_matrix(n, s.numel, j, rng)
        w = specials.mode_weights(n, mode)
        want = {s.key: specials.oracle(x[:, s.offset:s.offset + s.numel], mode, w) for s in f32}
        x.setflags(write=False)
        _SPECIAL[(n, mode)] = (x, w, want)
    return _SPECIAL[(n, mode)]


@pytest.mark.parametrize("mode", ["mean", "w1", "w2"])
@pytest.mark.parametrize("counts", ["3:7,0,13", "4:65,65,65,65"])
@pytest.mark.parametrize("form", ["chained", "striped", "blocked"])
def test_loopback_special_values(tmp_path, form, counts, mode):
    """inf, NaN, -0.0, subnormals, overflowing and cancelling columns in every
    column class, and weights that are 0, subnormal, negative (w1) and inf
    (w2: 0 * inf, inf - inf), through the executor's own kernels (the fold,
    the scale's vector and scalar arm, the stacks, the scatter, the chain
    state across a hop), result on every rank: every rank equals one GPU's
    fa_reduce (the driver; NaN where it has NaN), and the first result rank
    equals the oracle, an arithmetic that does not depend on fa_reduce."""
    import specials
    from feddct_amd import comm as C
    from helpers import bits_equal
    lay = _special_layout()
    W = int(counts.split(":")[0])
    cnt = [int(c) for c in counts.split(":")[1].split(",")]
    n = sum(cnt)
    for r in range(W):    # the layout gives every rank a stripe
        ops = C.describe(C.FA_MODE_STRIPED, lay, cnt, r, nchunks=2, root=-1)
        assert any(o["op"] == "K_STRIPE" and o["count"] > 0 for o in ops), r
    x, w, want = _special_inputs(n, mode)
    cf, wf, dump = (str(tmp_path / f) for f in ("clients.bin", "weights.bin", "out.bin"))
    x.tofile(cf)
    if w is not None:
        w.astype(np.float32).tofile(wf)
    case = f"{form}:{counts}:-1:threads:{int(w is not None)}:{0 if form == 'blocked' else 2}"
    rows = _run(lay, [case], tmp_path, clients=cf, weights=wf if w is not None else None,
                dump=dump)
    assert rows[0]["check"] == "bit-exact" and rows[0]["result_ranks"] == W, rows
    got = np.fromfile(dump, np.float32, count=lay.f32_numel)
    f32 = [s for s in lay.slots if s.kind != "i64"]
    for j, s in enumerate(f32):
        g = got[s.offset:s.offset + s.numel]
        assert bits_equal(g, want[s.key].reshape(-1)), (s.key, mode)
        if mode == "mean":
            # the all -0.0 columns: +0.0.  The driver holds every result rank
            # to the reference's bits wherever it is not NaN, so bits 0 on the
            # dumped rank are bits 0 on every rank
            neg0 = (np.arange(s.numel) + j) % specials.NPAT == 1
            assert not g[neg0].view(np.uint32).any(), s.key
