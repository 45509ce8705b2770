"""GPU: the commands the driver will run.  `bench.py` under torch.distributed.run with ONE rank exercises everything the N-rank scaling
run does -- env rendezvous on 127.0.0.1, the RCCL process group, the r3d_comm communicator (its id shipped over the process group),
r3d_gather_frames behind the C ABI into the pre-allocated clip buffer, the uneven-tail arithmetic of --clip, MAX-over-ranks timing --
before an 8-GPU node ever sees it."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(args, torchrun):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable]
    if torchrun:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29533"]
    cmd += [os.path.join(ROOT, "bench.py")] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    return json.loads(lines[0])


def test_bench_weak_scaling_line_under_torchrun():
    d = _run(["--gpus", "1", "--steps", "6", "--warmup", "2", "--full", "--no-extras", "--no-cpu-baseline"], torchrun=True)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "repeats"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert d["config"]["frames_total"] == 6 and "workload" in d["config"]
    assert abs(d["value"] - 6 / (d["ms_per_step"] * 6e-3)) / d["value"] < 1e-3
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1 and d["repeats"]["n"] == 5
    assert d["value"] > 100
    # roofline.traffic is re-measured in the run (two rocprofv3 --pmc child passes) whenever the tool is there; else the committed figure, labelled
    import shutil
    r = d["roofline"]
    assert r["traffic"] and r["traffic_source"] and r["algorithmic_bytes_per_launch"] > 1e8
    if shutil.which("rocprofv3"):
        assert "child passes of this run" in r["traffic_source"], r["traffic_source"]
        assert 0.9 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.6, (r["traffic"], r["algorithmic_bytes_per_launch"])
    assert "f16mx" in d["dtype"] and r["precision"] == "f16mx"          # the precision of `value` is selected by name and spelled out
    # the clock the dominant kernel ran at is measured in the run (one wave per launch: s_memtime / s_memrealtime) and the fraction at that clock is
    # reported beside `frac`, never instead of it
    assert r["peak_clock_ghz"] == 2.4 and 0.8 < r["shader_clock_ghz"] <= 2.45, r["shader_clock_ghz"]
    assert abs(r["frac_at_measured_clock"] - r["frac"] * r["peak_clock_ghz"] / r["shader_clock_ghz"]) < 2e-3 and r["frac_at_measured_clock"] < 1
    assert set(r["shader_clock_ghz_other_kernels"]) == {"render_kernel", "upconv_fir"} and all(0.8 < v < 2.45 for v in r["shader_clock_ghz_other_kernels"].values())


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, reports the headline fields only, and --dump-outputs writes the frame of the last
    timed step: the same frame on every run with the same arguments."""
    import numpy as np
    frames = []
    for rep in range(2):
        out = tmp_path / ("run%d" % rep)
        d = _run(["--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(out)], torchrun=False)
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
            assert k in d, k
        for k in ("roofline", "repeats", "value_single_stream", "cpu_baseline", "cpu_baseline_reference", "torso_frame", "alt_f16x3"):
            assert k not in d, k
        assert d["steps"] == 5 and d["warmup"] == 2 and d["config"]["frames_total"] == 5 and d["higher_is_better"] is True
        assert abs(d["value"] - 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 1e-3 and d["value"] > 100
        f = np.load(out / "frames_last_step.npy")
        assert f.dtype == np.float32 and f.shape == (1, 512, 512, 3)
        assert f.min() >= 0 and f.max() <= 255 and np.array_equal(f, np.round(f)) and f.std() > 1.0
        frames.append(f)
    assert np.array_equal(frames[0], frames[1])


def test_profile_clock_is_zero_until_a_profiled_launch_and_plausible_after():
    import ctypes
    import numpy as np
    import torch
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.superresolution import Conv2d
    lib = _lib.load()
    g, cyc = ctypes.c_double(-1.0), ctypes.c_ulonglong(1)
    lib.r3d_profile_configure(0); lib.r3d_profile_reset()
    assert lib.r3d_profile_clock(1, ctypes.byref(g), ctypes.byref(cyc)) == 0 and g.value == 0.0 and cyc.value == 0
    assert lib.r3d_profile_clock(99, ctypes.byref(g), None) != 0                      # bad family id: error code, no crash
    c = Conv2d(128, 128, 3, 1, padding=1).cuda()
    x = torch.from_numpy(synth.hash_unitvar(3, (1, 128, 256, 256), stream=1)).cuda()
    y0 = c(x, out_format="cb8").clone()                                                # not profiled: nothing sampled
    torch.cuda.synchronize()
    assert lib.r3d_profile_clock(1, ctypes.byref(g), None) == 0 and g.value == 0.0
    lib.r3d_profile_configure(1 << 1); lib.r3d_profile_reset()
    for _ in range(20):
        y1 = c(x, out_format="cb8")
    torch.cuda.synchronize()
    assert lib.r3d_profile_clock(1, ctypes.byref(g), ctypes.byref(cyc)) == 0
    lib.r3d_profile_configure(0)
    assert 0.5 < g.value < 2.6 and cyc.value > 20 * 10000, (g.value, cyc.value)          # GHz of the sampled waves; 20 launches x >= 10 k cycles each
    assert torch.equal(y0, y1)                                                         # sampling does not touch the result


def test_bench_clip_mode_uneven_tail_under_torchrun():
    d = _run(["--gpus", "1", "--clip", "7", "--warmup", "2", "--no-extras", "--no-cpu-baseline"], torchrun=True)
    assert d["scaling"] == "strong" and d["config"]["frames_total"] == 7 and d["steps"] == 7
    assert d["value"] > 100


def test_sustained_mix_probe_and_power_probe_report_plausible_numbers():
    """bench.py's two board-level legs (extras): the f16mx MFMA mix sustained from registers / from LDS, and rocm-smi's power while frames render."""
    import shutil
    import time
    import torch
    sys.path.insert(0, ROOT)
    import bench
    r = bench.sustained_mix_probe(600.0, seconds=0.6)
    assert "skipped" not in r, r                                          # __graft_entry__.build() builds the probe
    for k in ("registers_constant", "registers_random", "lds_fed_random"):
        v = r[k]
        assert 100 < v["tflops"] < 1300 and 0.04 < v["frac_of_f16_peak"] < 0.52 and 0.8 < v["wave_clock_ghz"] < 2.45, (k, v)
    assert r["registers_constant"]["tflops"] >= r["lds_fed_random"]["tflops"]          # data that never toggles is the cheapest to multiply
    assert 0.3 < r["dominant_kernel_vs_lds_fed_mix"] < 1.5
    if shutil.which("rocm-smi"):
        x = torch.randn(4096, 4096, device="cuda")
        p = bench.power_probe(torch, lambda i: x @ x, torch.cuda.synchronize, 8, seconds=1.5)
        assert "skipped" in p or (50 < p["socket_power_w_mean"] < 1500 and 300 < p["sclk_mhz_mean"] < 2500 and p["samples"] >= 1), p
