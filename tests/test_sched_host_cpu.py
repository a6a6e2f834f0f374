"""The multi-GPU schedules and cost model (feddct_amd/csrc/sched_host.cpp)
without HIP, without RCCL and without a device: tests/host/sched_host_check.cpp,
sched_host.cpp and plan_host.cpp compile with plain g++ and no ROCm include
path (the build succeeding shows the unit is HIP- and RCCL-free), and what
the program records — every rank's raw fa_xfer list of fa_describe_round, the
fa_round_cost bytes of fa_round_model, (mode, nchunks, model_us) of
fa_multi_select_layout — matches, byte for byte (the doubles as bits: both
sides compile without contraction), what the commit before the schedules
moved out of fedcomm.hip gave (tests/golden/sched_host_digests.json, recorded
from that commit's libfedagg_comm.so by tests/golden/make_sched_host_golden.py).
The program also checks every accepted round across its ranks by itself:
steps never decrease, sends and receives pair up per channel, the ranks post
the same collectives, every range lies inside its buffer.  The same program
runs once more built with the address and undefined-behaviour sanitizers, as
an ordinary child process.  No GPU."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_sched_host_golden as gold  # noqa: E402

SRCS = [os.path.join(ROOT, "tests", "host", "sched_host_check.cpp"),
        os.path.join(ROOT, "feddct_amd", "csrc", "sched_host.cpp"),
        os.path.join(ROOT, "feddct_amd", "csrc", "plan_host.cpp")]
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _env():
    """The child's environment: the model's constants are the header's."""
    return {k: v for k, v in os.environ.items() if not k.startswith("FA_MODEL_")}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, cases): the case file written once.  A case: the
    generator's parameters and the digests recorded under its name."""
    assert shutil.which("g++"), "g++ is needed to build the schedules' check program"
    tmp = tmp_path_factory.mktemp("sched_host")
    with open(os.path.join(GOLDEN, "sched_host_digests.json")) as f:
        rows = json.load(f)["cases"]
    # the recorded case list is the generator's enumeration
    assert [d["name"] for d in rows] == [c["name"] for c in gold.cases()]
    cases = [dict(c, **d) for c, d in zip(gold.cases(), rows)]
    (tmp / "cases.txt").write_text(gold.case_file(cases, gold.load_layouts()))
    return tmp, cases


@pytest.fixture(scope="module")
def run(work):
    """(cases, name -> blob): the check program built and run once over every case."""
    tmp, cases = work
    exe = str(tmp / "sched_host_check")
    subprocess.run([*CXX, "-o", exe, *SRCS], check=True)
    r = subprocess.run([exe, str(tmp / "cases.txt"), str(tmp / "out.bin")], capture_output=True,
                       text=True, env=_env())
    assert r.returncode == 0, r.stderr
    return cases, gold.read_records(str(tmp / "out.bin"))


def test_case_list_is_the_generators(run):
    """The recorded cases are the ones the generator enumerates (the `work`
    fixture compares the names, which spell every parameter out); its layouts
    and count vectors are tests/test_schedule.py's, and every count vector
    meets every mode, root kind, weighting and chunk count."""
    import test_schedule as S
    cases, _ = run
    assert gold.MAN == S.MAN and gold.COUNTS[:-1] == S.COUNTS and gold.COUNTS[-1] == [9]
    rounds = [c for c in cases if c["kind"] == "round"]
    assert len({c["name"] for c in cases}) == len(cases)
    for counts in gold.COUNTS:
        mine = [c for c in rounds if c["layout"] == "man" and c["counts"] == counts]
        W = len(counts)
        assert {c["mode"] for c in mine} == {0, 1, 2, 3}
        assert {c["xchg"] for c in mine if c["mode"] == gold.SHARDED} == {0, 1}
        assert {c["nchunks"] for c in mine} >= {0, 1, 5}
        assert {c["weighted"] for c in mine} == {0, 1}
        assert {c["root"] for c in mine} >= {0, -1, W - 1}
    assert any(c["root"] >= len(c["counts"]) for c in rounds)
    assert {c["layout"] for c in rounds} == {"man", "noi64", "wrnsl"}
    assert {len(c["counts"]) for c in rounds} == {1, 2, 3, 4, 5, 8}


def test_schedules_match_the_parent(run):
    cases, blobs = run
    bad = []
    for c in (c for c in cases if c["kind"] == "round"):
        blob = blobs[c["name"]]
        rcs, nops = gold.round_rcs(blob, len(c["counts"]))
        if (None if any(rcs) else nops) != c["nops"]:
            bad.append((c["name"], "ops", rcs, nops, c["nops"]))
        elif hashlib.sha256(blob).hexdigest() != c["sha256"]:
            bad.append((c["name"], "digest"))
    assert not bad, bad[:10]


def test_modelled_costs_match_the_parent(run):
    """fa_round_cost, its three doubles bit for bit."""
    cases, blobs = run
    rounds = [c for c in cases if c["kind"] == "round"]
    bad = [c["name"] for c in rounds
           if hashlib.sha256(blobs[c["name"] + "/model"]).hexdigest() != c["model_sha256"]]
    assert not bad, bad[:10]
    assert all(len(blobs[c["name"] + "/model"]) in (4, 4 + 32) for c in rounds)


def test_selection_matches_the_parent(run):
    """(mode, nchunks, model_us) of the default entry's choice, with
    FA_MULTI_ROOT_ALL set and unset, and FA_MULTI_REASSOCIATE."""
    cases, blobs = run
    sel = [c for c in cases if c["kind"] == "select"]
    assert {c["mflags"] for c in sel} == {0, gold.ROOT_ALL, gold.REASSOCIATE}
    bad = [c["name"] for c in sel
           if hashlib.sha256(blobs[c["name"]]).hexdigest() != c["sha256"]]
    assert not bad, bad[:10]
    assert all(blobs[c["name"]][:4] == b"\0\0\0\0" for c in sel)    # none refused


def test_refused_cases_are_exactly_the_expected(run):
    """A refusal may not hide a failure: refused are the rounds with
    root >= nranks (FA_E_INVAL) and the blocked rounds on counts that put a
    cascade block on more than two ranks (FA_E_RANGE, computed here from the
    counts), on every rank and in the model alike; nothing else."""
    import struct
    cases, blobs = run
    seen = set()
    for c in (c for c in cases if c["kind"] == "round"):
        want = gold.expected_refusal(c)
        rcs, _ = gold.round_rcs(blobs[c["name"]], len(c["counts"]))
        (mrc,) = struct.unpack_from("<i", blobs[c["name"] + "/model"])
        assert rcs == [want] * len(c["counts"]) and mrc == want, (c["name"], rcs, mrc, want)
        seen.add(want)
    assert seen == {0, gold.FA_E_INVAL, gold.FA_E_RANGE}


def test_sanitized_run(work, run):
    """The same program under AddressSanitizer and UBSan (a stand-alone
    executable, nothing preloaded): no report, and the same bytes."""
    tmp, _ = work
    probe = tmp / "empty.cpp"
    probe.write_text("int main() { return 0; }\n")
    trial = subprocess.run([*CXX, *SANITIZE, "-o", str(tmp / "empty"), str(probe)],
                           capture_output=True, text=True)
    if trial.returncode != 0:
        pytest.skip("g++ cannot link an empty main with " + " ".join(SANITIZE) + ": "
                    + trial.stderr.strip()[-200:])
    exe = str(tmp / "sched_host_check_san")
    subprocess.run([*CXX, "-g", *SANITIZE, "-o", exe, *SRCS], check=True)
    r = subprocess.run([exe, str(tmp / "cases.txt"), str(tmp / "out_san.bin")],
                       capture_output=True, text=True, env=_env())
    assert r.returncode == 0, r.stderr[-4000:]
    assert not r.stderr.strip(), r.stderr[-4000:]
    with open(tmp / "out.bin", "rb") as a, open(tmp / "out_san.bin", "rb") as b:
        assert a.read() == b.read()
