"""bench.py's plain and --full runs and --dump-outputs (bench.py docstring).

CPU: dump_outputs writes float32 .npy files within its byte budget, a larger array as the same
seeded pixel sample on every call.  GPU: a plain run of the smallest configuration (C2, the Cornell
box at 64x36, 4 steps) prints the headline line without the legs that take runs of their own and
dumps exactly the radiance sums an in-process render of the same frames gives; the --full run adds
those legs and dumps the same sums.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_traversal", "kernel_lines", "traversal_stages", "cpu_baseline", "parity_vs_oracle")
W, H, STEPS = 64, 36, 4


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    b = _bench()
    assert b.DUMP_MAX_BYTES <= 64 * 1000 * 1000
    rng = np.random.default_rng(1)
    img = rng.random((9, 7, 3))                                  # float64 in, float32 out
    info = b.dump_outputs(str(tmp_path / "whole"), {"color": img})
    got = np.load(tmp_path / "whole" / "color.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img.astype(np.float32))
    assert info["color"] == {"shape": [9, 7, 3], "dtype": "float32", "sample": None}
    # C5's 4K frame (99.5 MB) at the real budget: the file, header included, stays within it
    b.dump_outputs(str(tmp_path / "uhd"), {"color": np.zeros((2160, 3840, 3), np.float32)})
    size = os.path.getsize(tmp_path / "uhd" / "color.npy")
    assert b.DUMP_MAX_BYTES - 2 * b.NPY_HEADER_MAX < size <= b.DUMP_MAX_BYTES
    os.remove(tmp_path / "uhd" / "color.npy")
    # a budget of 20 pixels: a sorted sample without replacement, the same on every call
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", b.NPY_HEADER_MAX + 20 * 3 * 4)
    info = b.dump_outputs(str(tmp_path / "s1"), {"color": img})
    b.dump_outputs(str(tmp_path / "s2"), {"color": img})
    s1, s2 = np.load(tmp_path / "s1" / "color.npy"), np.load(tmp_path / "s2" / "color.npy")
    assert s1.dtype == np.float32 and s1.shape == (20, 3)
    assert os.path.getsize(tmp_path / "s1" / "color.npy") <= b.DUMP_MAX_BYTES
    assert np.array_equal(s1, s2) and info["color"]["sample"]
    idx = np.sort(np.random.default_rng(0).choice(63, size=20, replace=False))
    assert np.array_equal(s1, img.astype(np.float32).reshape(-1, 3)[idx])


def _run(tmp_path, name, *extra):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--width", str(W),
           "--height", str(H), "--steps", str(STEPS), "--warmup", "1", "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), np.load(out / "color.npy")


@pytest.fixture(scope="module")
def rendered(cornell, luts):
    """The frames bench.py times for this command, rendered in-process."""
    import mpt
    from mpt import abi, scene
    b = _bench()
    opt = abi.KernelOptions.default()
    opt.direct_light_sampling = abi.LSS_MIS_LIGHT_BSDF
    cam = scene.make_camera(cornell.camera_info, W, H)
    frames = b.frames_for(cam, W, H, opt, (b.BAND_H, 0, 1), STEPS, bounces=3)
    with mpt.GPURenderer(0) as r:
        r.set_scene(cornell)
        r.set_luts(luts)
        r.render_samples(frames, max_batch=STEPS)
        r.synchronize_kernel()
        return r.framebuffer(abi.FB_COLOR)


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, rendered):
    line, color = _run(tmp_path, "plain")
    assert line["steps"] == STEPS and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = rays / elapsed and ms_per_step = elapsed / steps describe the same timed region
    rays = line["rays_per_sample"] * W * H * STEPS
    assert line["value"] == pytest.approx(rays / (line["ms_per_step"] * 1e-3 * STEPS) / 1e6, rel=1e-2)
    assert not [k for k in FULL_ONLY + ("configs", "batch1") if k in line]
    assert color.dtype == np.float32 and color.shape == (H, W, 3)
    assert np.array_equal(color, rendered)
    assert line["outputs"]["files"]["color"]["shape"] == [H, W, 3]


@pytest.mark.gpu
def test_full_run_adds_the_other_legs_and_dumps_the_same(tmp_path, rendered):
    line, color = _run(tmp_path, "full", "--full", "--configs", "none", "--cpu-seconds", "0.2", "--parity-spp", str(STEPS))
    assert line["full"] is True and line["steps"] == STEPS
    assert not [k for k in FULL_ONLY if line.get(k) is None]
    assert line["parity_vs_oracle"]["bit_exact"] is True and line["parity_vs_oracle"]["spp"] == STEPS
    assert line["traversal_stages"][0]["nodes_per_ray"] > 0          # the calibration pass ran instrumented
    assert np.array_equal(color, rendered)
