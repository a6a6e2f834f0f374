"""GPU: bench.py's command line — a plain run times its steps and prints the
headline line alone; --dump-outputs writes the global state of the last
timed step, and that state is the reference's (tests/golden/digests.json)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_manifest

pytestmark = pytest.mark.gpu

# what only --full measures (bench.py main): absent from a plain run's line
FULL_ONLY = ("gpu_state_idle", "copy_ceiling_GBps", "read_ceiling_GBps", "weighted_GBps",
             "headline_launch", "parity", "host_inclusive", "round", "dropin", "other_configs",
             "next_rows", "cfg1_host_resident_n2")


def test_plain_run_prints_the_headline_and_dumps_the_reference_state(tmp_path):
    from feddct_amd.layout import BucketLayout
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    nbytes = line["config"]["algorithmic_bytes_per_step"]
    assert abs(line["value"] - nbytes / (line["ms_per_step"] * 1e-3) / 1e9) < 0.01 * line["value"]
    assert line["cpu_baseline"] is None
    assert not [k for k in FULL_ONLY if k in line]
    # the dump: float32 / float64 arrays, at most 64 MB, the reference's bits
    assert sorted(os.listdir(out)) == ["global_f32.npy", "global_i64.npy"]
    f = np.load(out / "global_f32.npy")
    i = np.load(out / "global_i64.npy")
    assert f.dtype == np.float32 and i.dtype == np.float64
    assert f.nbytes + i.nbytes <= 64 * 1000 * 1000
    lay = BucketLayout.from_manifest(load_manifest("wrn16_8_c10"))
    h = hashlib.sha256()
    pf = pi = 0
    for s in lay.slots:
        h.update(s.key.encode())
        if s.kind == "i64":
            h.update(i[pi:pi + s.numel].astype(np.int64).tobytes())
            pi += s.numel
        else:
            h.update(f[pf:pf + s.numel].tobytes())
            pf += s.numel
    assert (pf, pi) == (f.size, i.size)
    with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as fh:
        assert h.hexdigest() == json.load(fh)["fedavg/wrn16_8_c10/n20"]
