"""mpt_rebuild_bvh_mode(MPT_BUILD_SAH): both BVH8s rebuilt on the GPU with the binary tree of
csrc/sah.h (csrc/sah.hip) between the keys and the collapse of csrc/lbvh.hip.

Bar: bit-exact, no tolerances, as in tests/test_ploc_rebuild.py and on its shapes.  After a mode-3
rebuild the device trees equal the host loop of the same definition (bvh_build_host(mode=3)) byte
for byte, flag lanes carried per primitive -- with one wave per node of at most 1024 triangles,
with every node on the grid path (MPT_SAH_TAIL=0) and across the hand-over between the two;
traversal equals the same context before the rebuild; renders equal the
oracle and an accumulation continues across the rebuild; later updates, material edits and mode
switches work on the new trees; a refused call changes nothing.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi

from raygen import grazing_rays
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_ploc_rebuild import assert_tree_equals_host, same_bytes, scene_of
from test_rebuild import SCENES, _restir_oracle, flags_of
from test_refit import fresh, in_plane_rays, moved_scene
from test_refit_host import EDITS, check_refit, cornell_scene, edit_jitter, edit_move, small_city
from test_shade_classes import _assert_modes_equal

pytestmark = pytest.mark.gpu

SAH = abi.BUILD_SAH


def scene_and_vertices(name):
    """The scene to upload and the vertices to move it to (None: as uploaded).  city_plane and
    tiny9_1e37 are reached by an update: a degenerate axis, and areas that overflow to inf."""
    if name == "city_plane":
        sd = small_city()
        return sd, EDITS["plane"](sd.vertices.astype(np.float32), sd.triangle_indices.reshape(-1, 3))
    if name == "tiny9_1e37":
        sd = scene_of("tiny9")
        return sd, (sd.vertices.astype(np.float32) * np.float32(1e37)).astype(np.float32)
    return scene_of(name), None


def rebuilt_trees(sd, luts, v=None):
    """Both trees before and after a mode-3 rebuild of a fresh context (moved to v first)."""
    r = fresh(sd, luts)
    try:
        if v is not None:
            r.update_vertices(v)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=SAH)
        after = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    return before, info, after


def check_against_host(name, sd, v, before, info, after):
    idx = sd.triangle_indices.reshape(-1, 3)
    light_prims = np.sort(before[1][1]["prim"]).astype(np.int32)
    assert_tree_equals_host(after[0], v, idx, None, flags_of(before[0][1], len(idx)), f"{name}: scene tree", mode=SAH)
    assert_tree_equals_host(after[1], v, idx, light_prims, flags_of(before[1][1], len(idx)), f"{name}: light tree", mode=SAH)
    assert (info.rebuilt, info.nodes, info.records, info.levels) == (1, len(after[0][0]), len(after[0][1]), after[0][2])
    has_light = int(len(light_prims) > 0)
    assert (info.light_rebuilt, info.light_nodes, info.light_records, info.light_levels) == \
        (has_light, len(after[1][0]), len(after[1][1]), after[1][2])
    return has_light


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["fresh", "moved"])
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_bytes_equal_host_build(luts, name, moved):
    """cornell: one wave per node from the root on; the small city (44,962 triangles): levels with
    nodes on the grid path (whole workgroups inside one node, workgroups across borders) first."""
    sd = SCENES[name]()
    v = sd.vertices.astype(np.float32)
    idx = sd.triangle_indices.reshape(-1, 3)
    r = fresh(sd, luts)
    try:
        if moved:
            v = EDITS["move"](v, idx)
            r.update_vertices(v)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=SAH)
        after = [r.get_bvh(w) for w in (0, 1)]
        # the rebuilt trees are their own refit: an identity update leaves every byte
        ri = r.update_vertices(v, info=True)
        again = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    has_light = check_against_host(name, sd, v, before, info, after)
    assert has_light
    if name == "city":
        assert after[0][1]["alpha_flag"].any() and after[0][1]["mat_class"].any()
    assert same_bytes(again, after), f"{name}: a tree changed under an identity update"
    assert ri.area_ratio == 1.0 and ri.light_area_ratio == 1.0
    assert (ri.nodes, ri.levels) == (info.nodes, info.levels)


@pytest.mark.parametrize("name", ["tiny4", "tiny9", "tiny257", "tiny1023", "tiny1024", "tiny1025", "tiny2049", "copies1000",
                                  "city_plane", "tiny9_1e37"])
def test_both_device_paths(monkeypatch, luts, name):
    """MPT_SAH_TAIL=0: every node on the grid path (atomics on the bins in global memory, privatised
    in LDS where a workgroup lies inside one node); the default: nodes above 1024 triangles there,
    the others one wave each -- 1025 and 2049 hand over between the two."""
    sd, nv = scene_and_vertices(name)
    v = sd.vertices.astype(np.float32) if nv is None else nv
    out = {}
    for tail in ("1", "0"):
        monkeypatch.setenv("MPT_SAH_TAIL", tail)
        out[tail] = rebuilt_trees(sd, luts, nv)
    monkeypatch.delenv("MPT_SAH_TAIL")
    check_against_host(name, sd, v, *out["1"])
    check_against_host(name, sd, v, *out["0"])
    assert same_bytes(out["0"][2], out["1"][2]), f"{name}: the two paths differ"


def test_depth_hook_on_both_paths(monkeypatch, luts):
    sd = cornell_scene()
    v = sd.vertices.astype(np.float32)
    default = rebuilt_trees(sd, luts)
    monkeypatch.setenv("MPT_SAH_DEPTH", "2")
    out = {}
    for tail in ("1", "0"):
        monkeypatch.setenv("MPT_SAH_TAIL", tail)
        out[tail] = rebuilt_trees(sd, luts)
        check_against_host(f"cornell at depth 2, tail {tail}", sd, v, *out[tail])   # (the host loop reads the hook too)
    assert same_bytes(out["0"][2], out["1"][2])
    assert not same_bytes(out["1"][2], default[2]), "MPT_SAH_DEPTH=2 changed nothing"


# ------------------------------------------------------------------------------------
# Traversal
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_traversal_after_rebuild_bit_exact(luts, name):
    sd0 = SCENES[name]()
    sd, nv, _ = moved_scene(name, "move")
    graze, glh = grazing_rays(sd, 20000, 21)
    plane, plh = in_plane_rays(sd, 5000, 22)
    sets = (("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh), ("in plane", plane, plh))
    r = fresh(sd0, luts)
    try:
        r.update_vertices(nv)
        res = []
        for phase in ("refitted", "rebuilt"):
            if phase == "rebuilt":
                r.rebuild_bvh(mode=SAH)
            out = []
            for what, rays, lh in sets:
                closest = r.trace_closest(rays, lh)
                t = closest[1]
                hit = closest[0] >= 0
                r3 = rays.copy()
                r3[:, 7] = np.where(hit, t * np.random.default_rng(2).choice(np.array([0.5, 1.0, 1.5], np.float32), len(rays)), rays[:, 7])
                out.append((closest, r3, r.trace_any(r3, lh)))
            res.append(out)
    finally:
        r.close()
    for k, (what, rays, lh) in enumerate(sets):
        (gp, gt, gu, gv), r3, occ = res[1][k]
        (bp, bt, bu, bv), _, bocc = res[0][k]
        assert_same(gp, bp, f"{name} {what} prim vs before the rebuild")
        hit = bp >= 0
        assert hit.mean() > 0.01
        for g, b, lane in ((gt, bt, "t"), (gu, bu, "u"), (gv, bv, "v")):
            assert_same(g[hit], b[hit], f"{name} {what} {lane} vs before the rebuild")
        assert_same(occ, bocc, f"{name} {what} occluded vs before the rebuild")


# ------------------------------------------------------------------------------------
# Renders
# ------------------------------------------------------------------------------------
def test_render_after_rebuild_mis(monkeypatch, luts):
    sd, nv, _ = moved_scene("cornell", "move")
    frs = frames(sd, 64, 36, 3, lss=STRATEGIES["mis"])
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(cornell_scene(), luts)
        try:
            r.update_vertices(nv)
            r.rebuild_bvh(mode=SAH)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    _assert_modes_equal(out, oracle_for(sd, luts).render(frs, aov=True), "SAH-rebuilt cornell mis")
    assert out[1][0].mean() > 0


def test_accumulation_continues_across_a_rebuild(luts):
    """2 samples, the mode-3 rebuild, 2 more samples -- no reset -- equal 4 uninterrupted samples of
    a second context bit for bit."""
    sd, nv, _ = moved_scene("cornell", "move")
    k = 2
    frs = frames(sd, 64, 36, 2 * k, lss=abi.LSS_MIS_LIGHT_BSDF)
    got = []
    for rebuild in (True, False):
        r = fresh(cornell_scene(), luts)
        try:
            r.update_vertices(nv)
            for f in frs[:k]:
                r.render(f)
            if rebuild:
                r.rebuild_bvh(mode=SAH)
            got.append(gpu_render(r, frs[k:]))
        finally:
            r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[0][j], got[1][j], f"{what} across a SAH rebuild")
    assert got[0][0].mean() > 0


# ------------------------------------------------------------------------------------
# Later work on the new trees
# ------------------------------------------------------------------------------------
def test_later_update_on_sah_trees(monkeypatch, luts):
    sd = small_city()
    v0 = sd.vertices.astype(np.float32)
    idx = sd.triangle_indices.reshape(-1, 3)
    vm = edit_move(v0, idx)
    vj = edit_jitter(vm, seed=9)
    got = {}
    for host in (0, 1):   # 1: later updates by the library's host loop (it must first take the new trees)
        monkeypatch.setenv("MPT_REFIT_HOST", str(host))
        r = fresh(sd, luts)
        try:
            r.update_vertices(vm)
            rb = r.rebuild_bvh(info=True, mode=SAH)
            built = [r.get_bvh(w) for w in (0, 1)]
            i1 = r.update_vertices(vm, info=True)
            assert i1.area_ratio == 1.0 and i1.light_area_ratio == 1.0
            i2 = r.update_vertices(vj, info=True)
            assert i2.area_ratio != 1.0 and (i2.nodes, i2.levels) == (rb.nodes, rb.levels)
            got[host] = [r.get_bvh(w) for w in (0, 1)]
        finally:
            r.close()
        for w in (0, 1):
            check_refit(built[w][0], built[w][1], got[host][w][0], got[host][w][1], vj, idx, f"jitter after a SAH rebuild, tree {w}")
    assert same_bytes(got[0], got[1]), "kernels vs host loop after a SAH rebuild"


def test_material_edit_then_second_rebuild(luts):
    """A wall turned emissive (the light set changes), then a second mode-3 rebuild: the light tree
    is rebuilt over the new set, renders equal the oracle."""
    sd0 = cornell_scene()
    sdB, nv, _ = moved_scene("cornell", "move")
    wall = int(sd0.material_indices[0])
    m1 = [abi.Material.from_buffer_copy(m) for m in sd0.materials]
    m1[wall].emission = abi.Color(0.3, 0.2, 0.1)
    m1[wall].emission_strength = 2.0
    frs = frames(sdB, 64, 36, 2, lss=abi.LSS_BSDF)
    s = copy.copy(sdB)
    s.materials = m1
    ref = _restir_oracle(s, luts, frs)
    r = fresh(sd0, luts)
    try:
        r.update_vertices(nv)
        r.rebuild_bvh(mode=SAH)
        n_light0 = len(r.get_bvh(1)[1])
        r.update_materials(m1)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=SAH)
        after = [r.get_bvh(w) for w in (0, 1)]
        got = gpu_render(r, frs)
    finally:
        r.close()
    assert len(after[1][1]) > n_light0
    check_against_host("cornell after a material edit", sd0, nv, before, info, after)
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[j], ref[j], f"second SAH rebuild after a material edit: {what}")


def test_mode_switches(luts):
    """Mode 0 -> 3 -> 1 -> 0 on the city: the mode-0 bytes of a context that only ever used mode 0."""
    sd = small_city()
    r = fresh(sd, luts)
    try:
        r.rebuild_bvh()
        first = [r.get_bvh(w) for w in (0, 1)]
        r.rebuild_bvh(mode=SAH)
        second = [r.get_bvh(w) for w in (0, 1)]
        r.rebuild_bvh(mode=abi.BUILD_PLOC)
        third = [r.get_bvh(w) for w in (0, 1)]
        r.rebuild_bvh(mode=abi.BUILD_LBVH)
        last = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    r = fresh(sd, luts)
    try:
        r.rebuild_bvh()
        only0 = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    assert same_bytes(last, only0) and same_bytes(first, only0)
    assert second[0][0].tobytes() != only0[0][0].tobytes() and third[0][0].tobytes() != second[0][0].tobytes()


# ------------------------------------------------------------------------------------
# Refusal
# ------------------------------------------------------------------------------------
def test_refused_rebuild_changes_nothing(monkeypatch, luts):
    sd = cornell_scene()
    v = sd.vertices.astype(np.float32)
    need = 2 * mpt.bvh_build_host(v, sd.triangle_indices.reshape(-1, 3), mode=SAH)[2] + 2
    r = mpt.GPURenderer(0)
    try:
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh(mode=SAH)
        assert e.value.code == -3                                   # MPT_ERR_NO_SCENE
        assert mpt.lib().mpt_rebuild_bvh_mode(None, SAH, None) == -1
        r.set_scene(sd)
        r.set_luts(luts)
        before = [r.get_bvh(w) for w in (0, 1)]
        for mode in (2, 4, -1):
            with pytest.raises(mpt.MptError) as e:
                r.rebuild_bvh(mode=mode)
            assert e.value.code == -1                               # MPT_ERR_INVALID_ARGUMENT
        unknown = [r.get_bvh(w) for w in (0, 1)]
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need - 1))
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh(mode=SAH)
        assert e.value.code == -4                                   # MPT_ERR_UNSUPPORTED
        after = [r.get_bvh(w) for w in (0, 1)]
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need))         # exactly enough: accepted
        assert r.rebuild_bvh(info=True, mode=SAH).rebuilt == 1
    finally:
        r.close()
    assert same_bytes(before, unknown) and same_bytes(before, after)
