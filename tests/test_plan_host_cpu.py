"""The host planners (feddct_amd/csrc/plan_host.cpp) without HIP and without
a device: tests/host/plan_host_check.cpp and plan_host.cpp compile with plain
g++ and no ROCm include path (the build succeeding shows the unit is
HIP-free), and the tables the program cuts — build_tiles x pack_scalar x the
balanced tables, the launch rule's rows, the torch-GPU-order tables and its
refusals — match, byte for byte, what the commit before the planners moved
out of fedagg.hip cut (tests/golden/plan_host_digests.json, recorded from
that commit by tests/golden/make_plan_host_golden.py).  The program also
checks every table by itself: tiles disjoint and covering exactly the
segments, stride bits equal to fa_torch_gpu_config, lo[] monotone.  No GPU."""
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
import make_plan_host_golden as gold  # noqa: E402


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(cases, name -> blob): the check program built and run once over every case."""
    assert shutil.which("g++"), "g++ is needed to build the planners' check program"
    tmp = tmp_path_factory.mktemp("plan_host")
    exe = str(tmp / "plan_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "plan_host_check.cpp"),
                    os.path.join(ROOT, "feddct_amd", "csrc", "plan_host.cpp")], check=True)
    with open(os.path.join(GOLDEN, "plan_host_digests.json")) as f:
        cases = json.load(f)["cases"]
    (tmp / "cases.txt").write_text(gold.case_file(cases, gold.load_layouts()))
    r = subprocess.run([exe, str(tmp / "cases.txt"), str(tmp / "out.bin")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return cases, gold.read_records(str(tmp / "out.bin"))


def test_case_list_is_the_generators(run):
    """The recorded cases are the ones the generator enumerates (every layout,
    tile width, flag value, slot table and client count), with one refused
    torch-GPU-order configuration found with the parent."""
    cases, _ = run
    refused = [c for c in cases if c["kind"] == "tgpu" and c["ntiles"] is None]
    assert refused
    extra = {c["n"] for c in cases if c["kind"] == "tgpu"} - set(gold.TGPU_N)
    assert len(extra) == 1 and all(c["ntiles"] is None for c in cases if c.get("n") in extra)
    want = gold.cases(extra.pop())
    strip = lambda c: {k: v for k, v in c.items() if k not in ("sha256", "launch_sha256", "ntiles")}
    assert [strip(c) for c in cases] == want


@pytest.mark.parametrize("kind", ["default", "tgpu"])
def test_tables_match_the_parent(run, kind):
    cases, blobs = run
    bad = []
    for c in (c for c in cases if c["kind"] == kind):
        blob = blobs[c["name"]]
        if gold.ntiles(kind, blob) != c["ntiles"]:
            bad.append((c["name"], "tiles", gold.ntiles(kind, blob), c["ntiles"]))
        elif hashlib.sha256(blob).hexdigest() != c["sha256"]:
            bad.append((c["name"], "digest"))
    assert not bad, bad[:10]


def test_launch_rows_match_the_parent(run):
    """(table, nt, ns, vec_u, batch, slots, pipe) of a call of every N in
    LAUNCH_N, weighted and not, on every fp32 default-order plan."""
    cases, blobs = run
    rows = [c for c in cases if "launch_sha256" in c]
    assert len(rows) == 4 * 2 * 3 * 3
    bad = [c["name"] for c in rows
           if hashlib.sha256(blobs[c["name"] + "/launch"]).hexdigest() != c["launch_sha256"]]
    assert not bad, bad[:10]
    assert all(len(blobs[c["name"] + "/launch"]) == len(gold.LAUNCH_N) * 2 * 7 * 4 for c in rows)


def test_wrn16_8_tile_counts_of_the_planners_comment(run):
    """plan_tgpu's comment: wrn16_8 C10 at N = 32 / 48 / 64 cuts 5,372 tiles
    (5,369 when the gaps are declared padding), seven rounds of 768 slots.
    (The comment used to say 5,370 at N = 64; the planner of the commit the
    goldens were recorded from cuts 5,372 there too.)"""
    cases, blobs = run
    for flags, want in ((0, 5372), (gold.GAPS, 5369)):
        for n in (32, 48, 64):
            name = f"wrn16_8_c10/tgpu/n{n}/f{flags}/s768"
            assert gold.ntiles("tgpu", blobs[name]) == want, name
            assert -(-want // 768) == 7
