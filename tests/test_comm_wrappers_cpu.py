"""What feddct_amd/comm.py's native wrappers hand to the C ABI, call for
call, without a GPU and without the library: a recorder (tests/commrec.py)
stands in for ``comm.lib()`` and every case's log — the plan's create call,
what the multi plan reads back, fa_comm_info, each ``step``'s reduce call with
its FaShardIO, the destroy calls when the objects are collected — must be the
one the commit before the five plan classes and five aggregator classes were
folded into one base gave (tests/golden/comm_wrapper_calls.json, recorded from
that commit's comm.py by tests/golden/make_comm_wrapper_golden.py).  Worlds
1-3 at every rank: the only check of the wrappers' marshalling above one rank
(tests/test_gpu_comm.py runs them on RCCL at world size 1)."""
import json
import os
import sys

import pytest

from conftest import ROOT

import commrec

GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_comm_wrapper_golden as gold  # noqa: E402

from feddct_amd import comm as C  # noqa: E402


@pytest.fixture(scope="module")
def want():
    with open(gold.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    """name -> record of every case, run once against this tree's comm.py."""
    with pytest.MonkeyPatch.context() as mp:
        return commrec.record(C, lambda rec: mp.setattr(C, "_clib", rec))


def _cases(kind):
    return [c for c in commrec.cases() if c["kind"] == kind]


# a counts vector shorter than the world, at a rank beyond its end, in the
# three classes that do not compare len(counts) with the world: the recorded
# commit escaped with counts[rank]'s IndexError; a ValueError naming the
# unknown shard, NativeAggregator's text, may stand in its place
def _short_counts(c):
    return (c["kind"] == "agg" and c["cls"] in commrec.TAKES_COUNTS[:3]
            and c["kw"].get("counts") is not None and c["rank"] >= len(c["kw"]["counts"]))


def test_case_list_is_the_generators(want):
    """The recorded cases are the ones commrec.cases() enumerates (the names
    spell every parameter out), and they cover what they are meant to."""
    cs = commrec.cases()
    assert list(want["cases"]) == [c["name"] for c in cs]
    agg = _cases("agg")
    ok = [c for c in agg if want["cases"][c["name"]]["error"] is None]
    for cls in commrec.AGGREGATORS:
        mine = [c for c in ok if c["cls"] == cls]
        assert {(c["world"], c["rank"]) for c in mine} == set(commrec.WORLDS)
        assert {(c["layout"], c["weights"]) for c in mine} == {
            (lay, w) for lay in commrec.MANIFESTS for w in commrec.WEIGHTS}
        assert {(c["layout"], c["final"]) for c in mine} == {
            (lay, f) for lay in commrec.MANIFESTS for f in ("reduce", "allreduce")}
        assert {c["kw"].get("root") for c in mine} >= {None, 0, 2}
        if cls in commrec.TAKES_NCHUNKS:
            assert {c["kw"].get("nchunks") for c in mine} == {None, 0, 3}
        if cls in commrec.TAKES_COUNTS:
            given = [c for c in mine if "counts" in c["kw"] and c["nlocal"] is None]
            assert {len(c["kw"]["counts"]) for c in given} == {1, 2, 3}
            assert any(c["kw"]["counts"][c["rank"]] == 0 for c in given)
    assert {c["kw"].get("exchange") for c in ok if c["cls"] == commrec.AGGREGATORS[0]} == {None, 1}
    multi = [c for c in ok if c["cls"] == "NativeAggregator"]
    assert {c["kw"].get("exact") for c in multi} == {None, False}
    # a rank without slots moves NativeAggregator's default root off world - 1
    roots = {(c["world"], want["cases"][c["name"]]["attrs"]["root"]) for c in multi
             if c["final"] == "reduce" and "root" not in c["kw"]}
    assert {(2, 0), (3, 1), (2, 1), (3, 2)} <= roots
    assert {c["cls"] for c in _cases("plan")} == set(commrec.PLANS)


def test_aggregators_make_the_recorded_calls(want, got):
    bad = []
    for c in _cases("agg"):
        w, g = want["cases"][c["name"]], got[c["name"]]
        if _short_counts(c):
            assert w["error"] == "IndexError: list index out of range"
            n = c["nlocal"]
            assert g["error"] in (w["error"], f"ValueError: rank {c['rank']} holds {n} clients, "
                                              "shard is ?"), c["name"]
            g = dict(g, error=w["error"])
        if gold.dumps(g) != gold.dumps(w):
            bad.append(c["name"])
    assert not bad, (len(bad), bad[:5])
    assert sum(map(_short_counts, _cases("agg"))) == 3


def test_value_errors_keep_their_text(want, got):
    """A bad ``final``, a wrong shard length, a wrong sum(counts), and
    NativeAggregator's wrong len(counts): ValueError, the recorded text, and
    nothing created."""
    seen = set()
    for c in _cases("agg"):
        w, g = want["cases"][c["name"]], got[c["name"]]
        if (w["error"] or "").startswith("ValueError"):
            assert g["error"] == w["error"], c["name"]
            assert not [f for f, _ in g["calls"] if "_plan_create" in f], c["name"]
            seen.add((c["cls"], w["error"].split(",")[0].split(" not ")[0]))
    texts = {t for _, t in seen}
    assert texts == {"ValueError: final must be 'reduce' or 'allreduce'",
                     "ValueError: rank 0 holds 4 clients", "ValueError: rank 2 holds 0 clients",
                     "ValueError: rank 0 holds 3 clients", "ValueError: rank 1 holds 1 clients",
                     "ValueError: rank 0 holds 5 clients"}
    for cls in commrec.AGGREGATORS:
        assert len({t for k, t in seen if k == cls}) >= 3, cls
    # what constructs in the recorded commit still constructs: the e1 class
    # checks no more than it did, the three middle classes take a counts
    # vector of another length than the world where it names this rank
    for c in _cases("agg"):
        if want["cases"][c["name"]]["error"] is None:
            assert got[c["name"]]["error"] is None, c["name"]


def test_entry_point_labels(want, got):
    """FedaggError's text names the entry point by the label the wrappers
    always used (fa_shard_plan_create for fa_shard_plan_create_ex, ...)."""
    failing = [c for c in _cases("agg") if c["rec"].get("fail")]
    labels = {got[c["name"]]["error"] for c in failing}
    assert labels == {want["cases"][c["name"]]["error"] for c in failing}
    assert labels == {f"FedaggError: {f} failed ({rc})" for f, rc in (
        ("fa_shard_plan_create", -3), ("fa_stripe_plan_create", -3), ("fa_chain_plan_create", -3),
        ("fa_block_plan_create", -3), ("fa_multi_plan_create", -3), ("fa_reduce_sharded", -6),
        ("fa_reduce_striped", -6), ("fa_reduce_chained", -6), ("fa_reduce_blocked", -6),
        ("fa_reduce_multi", -6), ("fa_multi_plan_mode", -1), ("fa_multi_plan_chunks", -1))}


def test_plans_are_destroyed_once(want, got):
    """Collecting a plan calls its own destroy entry point once, with its
    handle; a second collection, or a second ``__del__``, calls nothing; a
    refused create leaves nothing to destroy; the communicator goes last."""
    for c in _cases("plan"):
        g = got[c["name"]]
        assert gold.dumps(g) == gold.dumps(want["cases"][c["name"]]), c["name"]
        destroy = commrec.DESTROY[c["cls"]]
        assert g["create"][0][0] == commrec.CREATE[c["cls"]]
        assert g["collected"] == [[destroy, [g["attrs"]["handle"]]]]
        assert g["collected_again"] == []
        assert [f for f, _ in g["finalised_twice"]] == [destroy]
        assert g["refused_calls"] == [commrec.CREATE[c["cls"]]]
        assert g["comm"] == [["fa_comm_destroy", [commrec.COMM_HANDLE]]]
    for c in _cases("agg"):          # and through an aggregator: plan, then communicator
        g = got[c["name"]]
        if g["error"] is None:
            tail = [f for f, _ in g["calls"][-2:]]
            assert tail == [commrec.DESTROY[commrec.PLANS[commrec.AGGREGATORS.index(c["cls"])]],
                            "fa_comm_destroy"], c["name"]


def test_host_helpers_marshal_as_recorded(want, got):
    """multi_select, round_model and describe: the layout's six arguments and
    the counts array as the recorded commit passed them."""
    for c in _cases("host"):
        assert gold.dumps(got[c["name"]]) == gold.dumps(want["cases"][c["name"]]), c["name"]


def test_signatures_and_class_relations(want):
    assert commrec.signatures(C) == want["signatures"]
    e1 = C.NativeShardedAggregator
    for cls in (C.NativeStripedAggregator, C.NativeChainedAggregator, C.NativeAggregator):
        assert cls.__bases__ == (e1,)
    assert C.NativeBlockedAggregator.__bases__ == (C.NativeChainedAggregator,)
    for n in commrec.PLANS + commrec.AGGREGATORS:
        assert getattr(C, n).__doc__


def test_the_real_library_is_back():
    """The recorder left ``comm._clib`` as it found it."""
    assert not isinstance(C._clib, commrec.Recorder)
