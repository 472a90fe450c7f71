"""Temporal accumulation of the C++ host side (hiprt-path-tracer_amd/host/gpu_renderer.*:
set_temporal / denoise_temporal / get_temporal / temporal_reset over mpt_set_temporal,
mpt_denoise_temporal, mpt_get_temporal and mpt_temporal_reset).  The driver
tests/cpp/temporal_move.cpp renders the blob of tests/test_host_cpp.py, moves the geometry twice
with update_vertices, calls denoise_temporal after each render and dumps the planes.  Checked: the
planes equal the Python route's (GPURenderer.denoise_temporal + temporal_planes) on the frames the
driver enqueued."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mpt import _build, abi, scene

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_cpp import H, W, _blob  # noqa: E402

KINDS = (abi.TEMPORAL_OUTPUT, abi.TEMPORAL_MOTION, abi.TEMPORAL_VISIBILITY, abi.TEMPORAL_HISTORY_A, abi.TEMPORAL_HISTORY_B)


def test_temporal_driver_built():
    """build() compiles the temporal driver next to the others (plain g++ against libmpt)."""
    assert _build.TEMPORAL_TEST.exists(), "temporal driver not built (run __graft_entry__.build())"
    assert os.access(_build.TEMPORAL_TEST, os.X_OK)
    assert len({_build.TEMPORAL_TEST, _build.DENOISE_TEST, _build.NORMALS_TEST, _build.HOST_TEST}) == 4
    assert "temporal.hip" in _build.SOURCES


def _read_out(path):
    raw = open(path, "rb").read()
    n_calls = struct.unpack_from("<i", raw)[0]
    off, fs, calls = 4, C.sizeof(abi.Frame), []
    for _ in range(n_calls):
        n = struct.unpack_from("<i", raw, off)[0]
        off += 4
        frames = [abi.Frame.from_buffer_copy(raw, off + i * fs) for i in range(n)]
        off += n * fs
        denoised_at = struct.unpack_from("<i", raw, off)[0]
        off += 4
        planes = []
        for ch in (3, 4, 4, 4, 4, 3):
            planes.append(np.frombuffer(raw, np.float32, W * H * ch, off).reshape(H, W, ch))
            off += W * H * ch * 4
        calls.append((frames, denoised_at, planes))
    assert off == len(raw)
    return calls


def _moved(sd, k):
    v = np.asarray(sd.vertices, np.float32).reshape(-1, 3)
    sphere = (np.asarray(sd.vertex_object) == 1)[:, None]
    return np.where(sphere, v + np.float32([0.05 * k, 0.02 * k, 0]), v).astype(np.float32)


@pytest.mark.gpu
def test_cpp_denoise_temporal_equals_python_route(cornell, luts, tmp_path):
    import mpt
    st = scene.parity_settings(3)
    st.samples_per_frame = 2
    opt = abi.KernelOptions.default()
    opt.direct_light_sampling = abi.LSS_MIS_LIGHT_BSDF
    cam = scene.make_camera(cornell.camera_info, W, H)
    blob, out = tmp_path / "in.blob", tmp_path / "out.bin"
    _blob(blob, cornell, luts, st, abi.WorldSettings.default(), opt, cam, 1, 0, [], 1)
    poses = [_moved(cornell, 1), _moved(cornell, 2)]
    with open(blob, "ab") as f:
        for p in poses:
            f.write(p.tobytes())
    r = subprocess.run([str(_build.TEMPORAL_TEST), str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    calls = _read_out(out)
    assert len(calls) == 3
    g = mpt.GPURenderer(0)
    try:
        g.set_scene(cornell)
        g.set_luts(luts)
        g.set_temporal(True)
        for k, (frames, denoised_at, planes) in enumerate(calls):
            assert len(frames) == 2 and denoised_at == 2 and frames[0].render_settings.sample_number == 0
            if k:
                g.update_vertices(poses[k - 1])
            g.render_samples(frames)
            den = g.denoise_temporal(camera=cam)
            for kind, got in zip(KINDS, planes[:5]):
                want = g.temporal_planes(kind)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"call {k}, plane {kind}"
            assert np.array_equal(planes[5].view(np.uint32), den.view(np.uint32)), f"call {k}: the denoised buffer"
            assert planes[4][..., 3].max() == k + 1
        assert not np.array_equal(calls[1][2][1][..., :2], calls[0][2][1][..., :2])          # the motion shows
    finally:
        g.close()
