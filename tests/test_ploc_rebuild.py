"""mpt_rebuild_bvh_mode(MPT_BUILD_PLOC): both BVH8s rebuilt on the GPU with the binary tree of
csrc/ploc.h (csrc/ploc.hip) between the keys and the collapse of csrc/lbvh.hip.

Bar: bit-exact, no tolerances, as in tests/test_rebuild.py and on its shapes.  After a mode-1
rebuild the device trees equal the host loop of the same definition (bvh_build_host(mode=1)) byte
for byte, flag lanes carried per primitive -- with the single-workgroup tail, without it
(MPT_PLOC_TAIL=0) and across the hand-over from the grid path to the tail; traversal equals a fresh
CPU oracle and the same context before the rebuild; renders equal the oracle and an accumulation
continues across the rebuild; later updates, material edits and mode switches work on the new
trees; a refused call changes nothing.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi, scene

from raygen import grazing_rays
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_ploc_host import chain
from test_rebuild import SCENES, _restir_oracle, flags_of, raw_scene
from test_refit import fresh, in_plane_rays, moved_scene
from test_refit_host import EDITS, check_refit, cornell_scene, edit_jitter, edit_move, small_city
from test_shade_classes import _assert_modes_equal

pytestmark = pytest.mark.gpu

PLOC = abi.BUILD_PLOC
_chain = {}


def chain_scene():
    """chain40 as a scene, the way test_rebuild.raw_scene makes one of loose triangles."""
    if not _chain:
        v, idx = chain(40)
        sd0 = cornell_scene()
        sd = scene.SceneData()
        sd.vertices = v
        sd.triangle_indices = idx.ravel().astype(np.int32)
        sd.normals = np.zeros_like(v)
        sd.has_normals = np.zeros(len(v), np.uint8)
        sd.texcoords = np.zeros((len(v), 2), np.float32)
        sd.materials = list(sd0.materials)
        sd.material_indices = (np.arange(len(idx)) % len(sd0.materials)).astype(np.int32)
        sd.textures = list(sd0.textures)
        sd.camera_info = sd0.camera_info
        sd.name = "chain40"
        _chain["sd"] = sd.finalize()
    return _chain["sd"]


def scene_of(name):
    if name == "chain40":
        return chain_scene()
    return SCENES[name]() if name in SCENES else raw_scene(name)


def assert_tree_equals_host(got, v, idx, prims, flags_by_prim, what, mode=PLOC):
    """got = get_bvh(w): the host loop's bytes of `mode`; the flag lanes per primitive as flags_by_prim."""
    gn, gt, gl = got
    if prims is not None and len(prims) == 0:
        assert len(gn) == 0 and len(gt) == 0
        return
    hn, ht, hl = mpt.bvh_build_host(v, idx, prims, mode=mode)
    assert gl == hl and len(gn) == len(hn) and len(gt) == len(ht), f"{what}: sizes {len(gn)} {len(gt)} {gl} vs {len(hn)} {len(ht)} {hl}"
    assert gn.tobytes() == hn.tobytes(), f"{what}: nodes"
    for f in ("a", "prim", "e1", "e2"):
        assert gt[f].tobytes() == ht[f].tobytes(), f"{what}: records {f}"
    for f in ("alpha_flag", "mat_class"):
        assert np.array_equal(gt[f], flags_by_prim[f][gt["prim"]]), f"{what}: flag lane {f}"


def same_bytes(a, b):
    return all(a[w][2] == b[w][2] and a[w][0].tobytes() == b[w][0].tobytes() and a[w][1].tobytes() == b[w][1].tobytes()
               for w in (0, 1))


def rebuilt_trees(sd, luts, v=None):
    """Both trees before and after a mode-1 rebuild of a fresh context (moved to v first)."""
    r = fresh(sd, luts)
    try:
        if v is not None:
            r.update_vertices(v)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=PLOC)
        after = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    return before, info, after


def check_against_host(name, sd, v, before, info, after):
    idx = sd.triangle_indices.reshape(-1, 3)
    light_prims = np.sort(before[1][1]["prim"]).astype(np.int32)
    assert_tree_equals_host(after[0], v, idx, None, flags_of(before[0][1], len(idx)), f"{name}: scene tree")
    assert_tree_equals_host(after[1], v, idx, light_prims, flags_of(before[1][1], len(idx)), f"{name}: light tree")
    assert (info.rebuilt, info.nodes, info.records, info.levels) == (1, len(after[0][0]), len(after[0][1]), after[0][2])
    has_light = int(len(light_prims) > 0)
    assert (info.light_rebuilt, info.light_nodes, info.light_records, info.light_levels) == \
        (has_light, len(after[1][0]), len(after[1][1]), after[1][2])
    return has_light


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["fresh", "moved"])
@pytest.mark.parametrize("name", list(SCENES))
def test_bytes_equal_host_build(luts, name, moved):
    sd = SCENES[name]()
    v = sd.vertices.astype(np.float32)
    idx = sd.triangle_indices.reshape(-1, 3)
    r = fresh(sd, luts)
    try:
        if moved:
            v = EDITS["move"](v, idx)
            r.update_vertices(v)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=PLOC)
        after = [r.get_bvh(w) for w in (0, 1)]
        # the rebuilt trees are their own refit: an identity update leaves every byte
        ri = r.update_vertices(v, info=True)
        again = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    has_light = check_against_host(name, sd, v, before, info, after)
    if name == "city":
        assert after[0][1]["alpha_flag"].any() and after[0][1]["mat_class"].any()
    if name in ("cornell", "city", "tiny257"):
        assert has_light
    assert same_bytes(again, after), f"{name}: a tree changed under an identity update"
    assert ri.area_ratio == 1.0 and (not has_light or ri.light_area_ratio == 1.0)
    assert (ri.nodes, ri.levels) == (info.nodes, info.levels)


@pytest.mark.parametrize("name", ["tiny9", "tiny257", "copies1000", "chain40", "cornell"])
def test_tail_off_gives_the_same_bytes(monkeypatch, luts, name):
    """MPT_PLOC_TAIL=0: every iteration on the grid path (the scan, the emit, the readback)."""
    sd = scene_of(name)
    v = sd.vertices.astype(np.float32)
    out = {}
    for tail in ("1", "0"):
        monkeypatch.setenv("MPT_PLOC_TAIL", tail)
        out[tail] = rebuilt_trees(sd, luts)
    monkeypatch.delenv("MPT_PLOC_TAIL")
    check_against_host(name, sd, v, *out["0"])
    assert same_bytes(out["0"][2], out["1"][2]), f"{name}: the tail changes the bytes"


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_grid_path_across_tile_borders(luts, n):
    """More than PLOC_TAIL clusters at first: the first iterations run on the grid path, over
    several workgroups' tiles and halos, and hand over to the tail."""
    sd = scene_of(f"tiny{n}")
    check_against_host(f"tiny{n}", sd, sd.vertices.astype(np.float32), *rebuilt_trees(sd, luts))


# ------------------------------------------------------------------------------------
# Traversal
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_traversal_after_rebuild_bit_exact(luts, name):
    sd0 = SCENES[name]()
    sd, nv, _ = moved_scene(name, "move")
    o = oracle_for(sd, luts)
    graze, glh = grazing_rays(sd, 20000, 21)
    plane, plh = in_plane_rays(sd, 5000, 22)
    sets = (("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh), ("in plane", plane, plh))
    r = fresh(sd0, luts)
    try:
        r.update_vertices(nv)
        res = []
        for phase in ("refitted", "rebuilt"):
            if phase == "rebuilt":
                r.rebuild_bvh(mode=PLOC)
            out = []
            for what, rays, lh in sets:
                closest = r.trace_closest(rays, lh)
                t = closest[1]
                hit = closest[0] >= 0
                r3 = rays.copy()
                r3[:, 7] = np.where(hit, t * np.random.default_rng(2).choice(np.array([0.5, 1.0, 1.5], np.float32), len(rays)), rays[:, 7])
                out.append((closest, r3, r.trace_any(r3, lh)))
            res.append(out)
        for k, (what, rays, lh) in enumerate(sets):
            (gp, gt, gu, gv), r3, occ = res[1][k]
            (bp, bt, bu, bv), _, bocc = res[0][k]
            op, ot, ou, ov = o.trace_closest(rays, lh)
            assert_same(gp, op, f"{name} {what} prim")
            assert_same(gp, bp, f"{name} {what} prim vs before the rebuild")
            hit = op >= 0
            assert hit.mean() > 0.01
            for g, b, c, lane in ((gt, bt, ot, "t"), (gu, bu, ou, "u"), (gv, bv, ov, "v")):
                assert_same(g[hit], c[hit], f"{name} {what} {lane}")
                assert_same(g[hit], b[hit], f"{name} {what} {lane} vs before the rebuild")
            op3, ot3, _, _ = o.trace_closest(r3, lh)
            assert_same(occ, (op3 >= 0) & (ot3 < r3[:, 7]), f"{name} {what} occluded")
            assert_same(occ, bocc, f"{name} {what} occluded vs before the rebuild")
    finally:
        r.close()


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
            r.rebuild_bvh(mode=PLOC)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    _assert_modes_equal(out, oracle_for(sd, luts).render(frs, aov=True), "PLOC-rebuilt cornell mis")
    assert out[1][0].mean() > 0


def test_render_restir_after_rebuild(luts):
    from test_restir import frames as restir_frames
    sd, nv, _ = moved_scene("cornell", "move")
    frs = restir_frames(sd, abi.LSS_RESTIR_DI, 3, w=64, h=36)
    r = fresh(cornell_scene(), luts)
    try:
        r.update_vertices(nv)
        r.rebuild_bvh(mode=PLOC)
        got = gpu_render(r, frs)
    finally:
        r.close()
    ref = _restir_oracle(sd, luts, frs)
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"restir after a PLOC rebuild: {what}")


def test_accumulation_continues_across_a_rebuild(luts):
    """2 samples, the mode-1 rebuild, 2 more samples -- no reset -- equal 4 uninterrupted samples of
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
                r.rebuild_bvh(mode=PLOC)
            got.append(gpu_render(r, frs[k:]))
        finally:
            r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[0][j], got[1][j], f"{what} across a PLOC rebuild")
    assert got[0][0].mean() > 0


# ------------------------------------------------------------------------------------
# Later work on the new trees
# ------------------------------------------------------------------------------------
def test_later_update_on_ploc_trees(monkeypatch, luts):
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
            rb = r.rebuild_bvh(info=True, mode=PLOC)
            built = [r.get_bvh(w) for w in (0, 1)]
            i2 = r.update_vertices(vj, info=True)
            assert i2.area_ratio != 1.0 and (i2.nodes, i2.levels) == (rb.nodes, rb.levels)
            got[host] = [r.get_bvh(w) for w in (0, 1)]
        finally:
            r.close()
        for w in (0, 1):
            check_refit(built[w][0], built[w][1], got[host][w][0], got[host][w][1], vj, idx, f"jitter after a PLOC rebuild, tree {w}")
    assert same_bytes(got[0], got[1]), "kernels vs host loop after a PLOC rebuild"


def test_material_edit_then_second_rebuild(luts):
    """A wall turned emissive (the light set changes), then a second mode-1 rebuild: the light tree
    is rebuilt over the new set, renders equal the oracle."""
    sd0 = cornell_scene()
    sdB, nv, _ = moved_scene("cornell", "move")
    idx = sd0.triangle_indices.reshape(-1, 3)
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
        r.rebuild_bvh(mode=PLOC)
        n_light0 = len(r.get_bvh(1)[1])
        r.update_materials(m1)
        before = [r.get_bvh(w) for w in (0, 1)]
        info = r.rebuild_bvh(info=True, mode=PLOC)
        after = [r.get_bvh(w) for w in (0, 1)]
        got = gpu_render(r, frs)
    finally:
        r.close()
    assert len(after[1][1]) > n_light0
    check_against_host("cornell after a material edit", sd0, nv, before, info, after)
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[j], ref[j], f"second PLOC rebuild after a material edit: {what}")


def test_mode_switches(luts):
    """Mode 0 -> 1 -> 0 on the city: the mode-0 bytes of a context that only ever used mode 0."""
    sd = small_city()
    r = fresh(sd, luts)
    try:
        r.rebuild_bvh()
        first = [r.get_bvh(w) for w in (0, 1)]
        r.rebuild_bvh(mode=PLOC)
        middle = [r.get_bvh(w) for w in (0, 1)]
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
    assert middle[0][0].tobytes() != only0[0][0].tobytes()


# ------------------------------------------------------------------------------------
# Refusal
# ------------------------------------------------------------------------------------
def test_refused_rebuild_changes_nothing(monkeypatch, luts):
    sd = cornell_scene()
    v = sd.vertices.astype(np.float32)
    need = 2 * mpt.bvh_build_host(v, sd.triangle_indices.reshape(-1, 3), mode=PLOC)[2] + 2
    r = mpt.GPURenderer(0)
    try:
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh(mode=PLOC)
        assert e.value.code == -3                                   # MPT_ERR_NO_SCENE
        assert mpt.lib().mpt_rebuild_bvh_mode(None, PLOC, None) == -1
        r.set_scene(sd)
        r.set_luts(luts)
        before = [r.get_bvh(w) for w in (0, 1)]
        for mode in (2, -1):
            with pytest.raises(mpt.MptError) as e:
                r.rebuild_bvh(mode=mode)
            assert e.value.code == -1                               # MPT_ERR_INVALID_ARGUMENT
        unknown = [r.get_bvh(w) for w in (0, 1)]
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need - 1))
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh(mode=PLOC)
        assert e.value.code == -4                                   # MPT_ERR_UNSUPPORTED
        after = [r.get_bvh(w) for w in (0, 1)]
        frs = frames(sd, 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        got = gpu_render(r, frs)
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need))         # exactly enough: accepted
        assert r.rebuild_bvh(info=True, mode=PLOC).rebuilt == 1
    finally:
        r.close()
    assert same_bytes(before, unknown) and same_bytes(before, after)
    assert_same(got[0], oracle_for(sd, luts).render(frs, aov=True)[0], "after a refused PLOC rebuild")
