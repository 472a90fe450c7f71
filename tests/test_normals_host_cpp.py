"""GPURenderer::set_normals / get_vertices of the C++ host side
(hiprt-path-tracer_amd/host/gpu_renderer.*) over 1 and 2 contexts.  The driver
tests/cpp/normals_move.cpp uploads the scene, sets the normal groups, moves the geometry with
update_vertices and downloads every context's arrays; then it removes the groups and updates again.
Checked: every context holds the bytes of the Python path (GPURenderer.set_normals, update_vertices,
get_vertices) and of mpt.normals_host; without the groups an update keeps the normals it finds."""
import struct
import subprocess

import numpy as np
import pytest

import mpt
from mpt import _build

from test_normals_host import poses, same_bytes
from test_refit_host import cornell_scene

F = np.float32


@pytest.mark.gpu
@pytest.mark.parametrize("split,with_flips", [(2, True), (1, False)], ids=["2ctx_flips", "1ctx"])
def test_cpp_set_normals_matches_the_python_path(luts, tmp_path, split, with_flips):
    sd = cornell_scene()
    v = poses("cornell")["jitter"]
    V, T = len(v), sd.num_triangles
    g, G = mpt.normal_groups(sd, only=np.arange(V) % 5 != 3)
    flips = (np.random.default_rng(9).random(G) < 0.4).astype(np.uint8) if with_flips else None
    blob, out = tmp_path / "in.blob", tmp_path / "out.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<I7i", 0x4D524E4D, T, V, len(sd.materials), len(sd.emissive), G, split, int(with_flips)))
        f.write(np.ascontiguousarray(sd.triangle_indices, np.int32).tobytes())
        for a, t in ((sd.vertices, F), (sd.normals, F), (sd.has_normals, np.uint8), (sd.texcoords, F), (sd.material_indices, np.int32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        f.write(b"".join(bytes(m) for m in sd.materials))
        f.write(np.ascontiguousarray(sd.emissive if len(sd.emissive) else np.zeros(1), np.int32).tobytes())
        f.write(g.tobytes())
        if with_flips:
            f.write(flips.tobytes())
        f.write(v.tobytes())
    r = subprocess.run([str(_build.NORMALS_TEST), str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"over {split} contexts" in r.stdout
    raw = open(out, "rb").read()
    assert struct.unpack_from("<i", raw)[0] == split and len(raw) == 4 + 2 * split * 2 * 12 * V
    arrays = np.frombuffer(raw, F, offset=4).reshape(2, split, 2, V, 3)
    py = mpt.GPURenderer(0)
    try:
        py.set_scene(sd)
        py.set_normals(g, flips, G)
        py.update_vertices(v)
        pv, pn = py.get_vertices()
    finally:
        py.close()
    want = mpt.normals_host(v, sd.triangle_indices, g, sd.normals, flips, G, sd.has_normals)
    assert same_bytes(pv, v) and same_bytes(pn, want)
    assert not same_bytes(want, sd.normals)
    for k in range(split):
        assert same_bytes(arrays[0, k, 0], v), f"context {k}: positions"
        assert same_bytes(arrays[0, k, 1], pn), f"context {k}: normals vs the Python path"
        assert same_bytes(arrays[1, k, 0], v) and same_bytes(arrays[1, k, 1], pn), f"context {k}: after set_normals(NULL)"
