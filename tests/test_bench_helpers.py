"""bench.py's reporting helpers (CPU): ULP distance and the ULP histogram the
N>1 bench line carries for the re-associated client-sharded sum."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_ulp_hist_counts_every_element():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(10000, generator=g)
    b = a.clone()
    # step b away from a by 0..40 ULP, in both directions and across zero
    steps = torch.randint(0, 41, (10000,), generator=g)
    bi = b.view(torch.int32)
    bi += torch.where(b >= 0, steps, -steps).to(torch.int32)
    h = bench.ulp_hist(a, b)
    assert sum(h.values()) == a.numel()
    assert h["0"] == int((steps == 0).sum())
    assert h["17+"] == int((steps >= 17).sum())
    assert bench.ulp_dist(a, b) == int(steps.max())


def test_ulp_across_signed_zero():
    a = torch.tensor([0.0, -0.0, 1.0e-45])
    b = torch.tensor([-0.0, 0.0, -1.0e-45])
    h = bench.ulp_hist(a, b)
    assert h["0"] == 2 and h["2"] == 1


def test_phase_deadline_exits_nonzero_with_the_flagged_line():
    """A phase that outlives its deadline prints the flagged line and ends
    the process with a non-zero status (it used to exit 0)."""
    import subprocess
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench.PhaseDeadline('xchg', 1.0, lambda p: print('{\"aborted\": \"%%s\"}' %% p)):\n"
            "    time.sleep(30)\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == bench.ABORT_RC != 0
    assert '{"aborted": "xchg"}' in r.stdout


def test_phase_deadline_cancelled_when_the_phase_finishes():
    with bench.PhaseDeadline("ok", 0.5, lambda p: None):
        pass
    import time
    time.sleep(0.8)   # the timer would have fired (and exited) by now


def test_build_line_keeps_the_bench_contract():
    """The one JSON line: every field the driver and the judge read, with
    value = world x per-rank bytes / step time and the roofline from the
    kernel time (bench contract, task ④)."""
    import argparse
    args = argparse.Namespace(steps=20, warmup=5)
    nb, t_step, t_kernel = 921663624, 150e-6, 141e-6
    line = bench.build_line(args, 2, nb, 43888744, t_step, t_kernel,
                            {"selected_mode": "blocked/native", "cpu_baseline": None})
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["metric"] == bench.METRIC and line["unit"] == "GB/s"
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["warmup"] == 5
    assert abs(line["value"] - 2 * nb / t_step / 1e9) < 0.01
    assert line["scaling"] == "weak" and line["higher_is_better"] is True
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == bench.HBM_PEAK_GBS
    assert abs(r["frac"] - nb / t_kernel / 1e9 / bench.HBM_PEAK_GBS) < 1e-3
    assert "blocked/native" in line["config"]["parallelism"]
    assert line["config"]["algorithmic_bytes_per_step"] == 2 * nb


def test_dump_outputs_writes_every_key_in_order(golden, tmp_path):
    """--dump-outputs: the keys' elements in state_dict order without the
    padding between them, fp32 keys as float32 and the int64 counters as
    float64, the same bytes on a second call."""
    import numpy as np
    from feddct_amd.layout import BucketLayout
    lay = BucketLayout.from_manifest(golden["manifest"]["small"])
    g = torch.Generator().manual_seed(3)
    o32 = torch.randn(max(64, lay.f32_numel), generator=g)
    o64 = torch.randint(0, 1 << 40, (max(1, lay.i64_numel),), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), lay, o32, o64)
    bench.dump_outputs(str(tmp_path / "b"), lay, o32, o64)
    assert sorted(os.listdir(tmp_path / "a")) == ["global_f32.npy", "global_i64.npy"]
    f = np.load(tmp_path / "a" / "global_f32.npy")
    i = np.load(tmp_path / "a" / "global_i64.npy")
    assert f.dtype == np.float32 and i.dtype == np.float64
    own = [s for s in lay.slots if s.alias_of is None]
    assert f.size == sum(s.numel for s in own if s.kind != "i64")
    assert i.size == sum(s.numel for s in own if s.kind == "i64")
    pf = pi = 0
    for s in own:
        if s.kind == "i64":
            want = o64[s.offset:s.offset + s.numel].numpy()
            assert np.array_equal(i[pi:pi + s.numel].astype(np.int64), want), s.key
            pi += s.numel
        else:
            want = o32[s.offset:s.offset + s.numel].numpy()
            assert f[pf:pf + s.numel].tobytes() == want.tobytes(), s.key
            pf += s.numel
    for name in ("global_f32.npy", "global_i64.npy"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()


def test_parse_smi_reads_clocks_power_and_temperatures():
    """bench.gpu_state_under_load's parser on rocm-smi --json text as the box
    prints it (a warning line first)."""
    import bench
    out = ('WARNING: AMD GPU device(s) is/are in a low-power state.\n'
           '{"card0": {"Temperature (Sensor junction) (C)": "46.0", '
           '"Temperature (Sensor memory) (C)": "33.0", "fclk clock speed:": "(1250Mhz)", '
           '"mclk clock speed:": "(2000Mhz)", "sclk clock speed:": "(2400Mhz)", '
           '"Current Socket Graphics Package Power (W)": "812.0", '
           '"GPU Memory Allocated (VRAM%)": "81", "Serial Number": "692533015330"}}')
    st = bench.parse_smi(out)
    assert st == {"sclk_mhz": 2400.0, "mclk_mhz": 2000.0, "fclk_mhz": 1250.0,
                  "socket_power_w": 812.0, "junction_c": 46.0, "memory_c": 33.0,
                  "vram_used_pct": 81.0, "serial": "692533015330"}
    assert "error" in bench.parse_smi("no json here")


def test_multi_env_fields(monkeypatch):
    """The N>1 line's environment block: the RCCL /
    NCCL / HSA / HIP variables of the process, the communicator's view, the
    peer-access matrix of the visible devices and the cost model's
    constants — what the first real multi-GPU run needs to be read."""
    class FakeComm:
        def info(self):
            return 8, 3, 3
    monkeypatch.setenv("NCCL_DEBUG", "WARN")
    monkeypatch.setenv("RCCL_MSCCL_ENABLE", "0")
    monkeypatch.setenv("UNRELATED_VAR", "x")
    e = bench.multi_env(FakeComm(), 8)
    assert e["env"]["NCCL_DEBUG"] == "WARN" and e["env"]["RCCL_MSCCL_ENABLE"] == "0"
    assert "UNRELATED_VAR" not in e["env"]
    assert (e["comm_count"], e["comm_rank"], e["comm_device"], e["world"]) == (8, 3, 3, 8)
    n = e["visible_devices"]
    assert len(e["peer_access"]) == n and all(len(row) == n for row in e["peer_access"])
    mc = e["model_constants"]
    assert mc["link_GBps"] > 0 and mc["hbm_GBps"] > 0 and mc["group_us"] >= 0
    # a rehearsal without a native communicator (gloo, --same-device) still
    # reports the environment and the peer matrix
    g = bench.multi_env(None, 2)
    assert g["comm_count"] is None and g["world"] == 2 and g["env"]["NCCL_DEBUG"] == "WARN"


def test_model_check():
    """The N>1 line's model check: measured over modelled per form, the
    model's pick against the measured best (the default entry's own line is
    left out: it duplicates its form)."""
    rep = {"blocked/native": {"ms_per_step": 1.0, "model_us": 800.0},
           "chained/native/c4": {"ms_per_step": 2.0, "model_us": 1500.0},
           "striped/native/c1": {"ms_per_step": 0.9, "model_us": 900.0},
           "default=blocked/native": {"ms_per_step": 0.5, "model_us": 800.0},
           "e1/torch.distributed": {"ms_per_step": 0.1},
           "broken": {"error": "x"}}
    mc = bench.model_check(rep)
    assert mc["model_pick"] == "blocked/native" and mc["measured_best"] == "striped/native/c1"
    assert mc["agree"] is False and mc["pick_over_best"] == round(1.0 / 0.9, 3)
    assert mc["measured_over_model"]["chained/native/c4"] == round(2000 / 1500, 3)
    assert "default=blocked/native" not in mc["measured_over_model"]
    assert bench.model_check({"a": {"ms_per_step": 1.0, "model_us": 5.0}}) is None
