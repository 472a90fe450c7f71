"""mpt_rebuild_bvh: both BVH8s rebuilt on the GPU (csrc/lbvh.hip) from the positions on the device.

Bar: bit-exact, no tolerances.  After a rebuild the device trees equal the host loop of the same
definition (mpt_bvh_build_host) byte for byte, flag lanes carried per primitive; traversal equals a
fresh CPU oracle of the moved scene and the results taken on the same context before the rebuild;
renders equal the oracle, and an accumulation continues across a rebuild without a reset; the
area ratios restart at 1; later updates and material edits work on the new trees; a refused call
changes nothing.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi, scene

from raygen import grazing_rays
from test_build_host import SORT_TILE, copies
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_refit import fresh, in_plane_rays, moved_scene
from test_refit_host import EDITS, check_refit, cornell_scene, edit_jitter, edit_move, moved_part, small_city, tiny
from test_shade_classes import _assert_modes_equal

pytestmark = pytest.mark.gpu

_raw = {}


def raw_scene(name):
    """Loose triangles as a scene: Cornell's materials dealt out in turn (some emissive, so that
    there is a light set), no normals."""
    if name not in _raw:
        v, idx = copies() if name == "copies1000" else tiny(int(name[4:]))
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
        sd.name = name
        _raw[name] = sd.finalize()
    return _raw[name]


SCENES = {f"tiny{n}": (lambda n=n: raw_scene(f"tiny{n}")) for n in (1, 3, 4, 9, 25, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1)}
SCENES.update({"copies1000": lambda: raw_scene("copies1000"), "cornell": cornell_scene, "city": small_city})


def assert_tree_equals_host(got, v, idx, prims, flags_by_prim, what):
    """got = get_bvh(w): the host loop's bytes; the flag lanes per primitive as flags_by_prim."""
    gn, gt, gl = got
    if prims is not None and len(prims) == 0:
        assert len(gn) == 0 and len(gt) == 0
        return
    hn, ht, hl = mpt.bvh_build_host(v, idx, prims)
    assert gl == hl and len(gn) == len(hn) and len(gt) == len(ht), f"{what}: sizes {len(gn)} {len(gt)} {gl} vs {len(hn)} {len(ht)} {hl}"
    assert gn.tobytes() == hn.tobytes(), f"{what}: nodes"
    for f in ("a", "prim", "e1", "e2"):
        assert gt[f].tobytes() == ht[f].tobytes(), f"{what}: records {f}"
    for f in ("alpha_flag", "mat_class"):
        assert np.array_equal(gt[f], flags_by_prim[f][gt["prim"]]), f"{what}: flag lane {f}"


def flags_of(tris, n_prims):
    out = {}
    for f in ("alpha_flag", "mat_class"):
        a = np.zeros(n_prims, np.uint32)
        a[tris["prim"]] = tris[f]
        out[f] = a
    return out


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
        info = r.rebuild_bvh(info=True)
        after = [r.get_bvh(w) for w in (0, 1)]
        # the rebuilt trees are their own refit: an identity update leaves every byte
        ri = r.update_vertices(v, info=True)
        again = [r.get_bvh(w) for w in (0, 1)]
    finally:
        r.close()
    light_prims = np.sort(before[1][1]["prim"]).astype(np.int32)
    assert_tree_equals_host(after[0], v, idx, None, flags_of(before[0][1], len(idx)), f"{name}: scene tree")
    assert_tree_equals_host(after[1], v, idx, light_prims, flags_of(before[1][1], len(idx)), f"{name}: light tree")
    if name == "city":
        assert after[0][1]["alpha_flag"].any() and after[0][1]["mat_class"].any()
    if name in ("cornell", "city", "tiny257"):
        assert len(light_prims) > 0
    assert (info.rebuilt, info.nodes, info.records, info.levels) == (1, len(after[0][0]), len(after[0][1]), after[0][2])
    has_light = int(len(light_prims) > 0)
    assert (info.light_rebuilt, info.light_nodes, info.light_records, info.light_levels) == \
        (has_light, len(after[1][0]), len(after[1][1]), after[1][2])
    for w in (0, 1):
        assert again[w][0].tobytes() == after[w][0].tobytes() and again[w][1].tobytes() == after[w][1].tobytes(), \
            f"{name}: tree {w} changed under an identity update"
    assert ri.area_ratio == 1.0 and (not has_light or ri.light_area_ratio == 1.0)
    assert (ri.nodes, ri.levels) == (info.nodes, info.levels)


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
                r.rebuild_bvh()
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
@pytest.mark.parametrize("strategy", ["mis", "ris"])
def test_render_after_rebuild(monkeypatch, luts, strategy):
    sd, nv, _ = moved_scene("cornell", "move")
    frs = frames(sd, 64, 36, 3, lss=STRATEGIES[strategy])
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(cornell_scene(), luts)
        try:
            r.update_vertices(nv)
            r.rebuild_bvh()
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    _assert_modes_equal(out, oracle_for(sd, luts).render(frs, aov=True), f"rebuilt cornell {strategy}")
    assert out[1][0].mean() > 0


def _restir_oracle(sd, luts, frs):
    from oracle import oracle as orc
    o = orc.Oracle(sd, luts)
    ref = o.render(frs, aov=True)
    o.close()
    return ref


@pytest.mark.parametrize("mode", [0, 1])
def test_render_restir_after_rebuild(monkeypatch, luts, mode):
    from test_restir import frames as restir_frames
    monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
    sd, nv, _ = moved_scene("cornell", "move")
    frs = restir_frames(sd, abi.LSS_RESTIR_DI, 3, w=64, h=36)
    r = fresh(cornell_scene(), luts)
    try:
        r.update_vertices(nv)
        r.rebuild_bvh()
        got = gpu_render(r, frs)
    finally:
        r.close()
    ref = _restir_oracle(sd, luts, frs)
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"restir after rebuild, light BVH {mode}: {what}")


@pytest.mark.parametrize("strategy", ["mis", "restir"])
def test_accumulation_continues_across_a_rebuild(luts, strategy):
    """k samples, the rebuild, k more samples -- no reset -- equal 2 k uninterrupted samples of a
    second context bit for bit."""
    sd, nv, _ = moved_scene("cornell", "move")
    k = 2
    if strategy == "restir":
        from test_restir import frames as restir_frames
        frs = restir_frames(sd, abi.LSS_RESTIR_DI, 2 * k, w=64, h=36)
    else:
        frs = frames(sd, 64, 36, 2 * k, lss=abi.LSS_MIS_LIGHT_BSDF)
    got = []
    for rebuild in (True, False):
        r = fresh(cornell_scene(), luts)
        try:
            r.update_vertices(nv)
            for f in frs[:k]:
                r.render(f)
            if rebuild:
                r.rebuild_bvh()
            got.append(gpu_render(r, frs[k:]))
        finally:
            r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[0][j], got[1][j], f"{strategy}: {what} across a rebuild")
    assert got[0][0].mean() > 0


# ------------------------------------------------------------------------------------
# area_ratio, later updates
# ------------------------------------------------------------------------------------
def test_area_ratio_and_later_update(monkeypatch, luts):
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
            assert r.update_vertices(vm, info=True).area_ratio > 1.0
            rb = r.rebuild_bvh(info=True)
            built = [r.get_bvh(w) for w in (0, 1)]
            i1 = r.update_vertices(vm, info=True)
            assert i1.area_ratio == 1.0 and i1.light_area_ratio == 1.0
            assert (i1.nodes, i1.levels, i1.light_nodes, i1.light_levels) == (rb.nodes, rb.levels, rb.light_nodes, rb.light_levels)
            same = [r.get_bvh(w) for w in (0, 1)]
            i2 = r.update_vertices(vj, info=True)
            assert i2.area_ratio != 1.0
            got[host] = [r.get_bvh(w) for w in (0, 1)]
        finally:
            r.close()
        for w in (0, 1):
            assert same[w][0].tobytes() == built[w][0].tobytes() and same[w][1].tobytes() == built[w][1].tobytes(), \
                f"host loop {host}: tree {w} is not its own refit"
            check_refit(built[w][0], built[w][1], got[host][w][0], got[host][w][1], vj, idx, f"jitter after rebuild, tree {w}")
    for w in (0, 1):
        assert got[0][w][0].tobytes() == got[1][w][0].tobytes() and got[0][w][1].tobytes() == got[1][w][1].tobytes(), \
            f"tree {w}: kernels vs host loop after a rebuild"


# ------------------------------------------------------------------------------------
# Mirrors: material edits after a rebuild
# ------------------------------------------------------------------------------------
def test_material_edits_after_rebuild(monkeypatch, luts):
    sd0 = cornell_scene()
    sdB, nv, _ = moved_scene("cornell", "move")
    wall = int(sd0.material_indices[0])
    m1 = [abi.Material.from_buffer_copy(m) for m in sd0.materials]   # a wall turned emissive: the light set changes
    m1[wall].emission = abi.Color(0.3, 0.2, 0.1)
    m1[wall].emission_strength = 2.0
    m2 = [abi.Material.from_buffer_copy(m) for m in m1]              # an alpha-tested material: flags re-stamped
    idx = sd0.triangle_indices.reshape(-1, 3)
    box_mat = int(sd0.material_indices[np.flatnonzero(moved_part(sd0.vertices, idx)[idx[:, 0]])[0]])
    m2[box_mat].alpha_opacity = 0.5
    edits = [m1, m2]
    frs = frames(sdB, 64, 36, 2, lss=abi.LSS_BSDF)
    for f in frs:
        f.render_settings.do_alpha_testing = True
    refs = []
    for mats in edits:
        s = copy.copy(sdB)
        s.materials = mats
        refs.append(_restir_oracle(s, luts, frs))
    assert not np.array_equal(refs[0][0], refs[1][0])
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.update_vertices(nv)
            r.rebuild_bvh()
            for k, mats in enumerate(edits):
                r.update_materials(mats)
                got = gpu_render(r, frs)
                for j, what in enumerate(["color", "albedo", "normals"]):
                    assert_same(got[j], refs[k][j], f"material edit {k} after the rebuild, light BVH {mode}: {what}")
                if k == 1:
                    tris = r.get_bvh(0)[1]
                    assert (tris["alpha_flag"][sd0.material_indices[tris["prim"]] == box_mat] != 0).all()
            # and a rebuild after the edits: the changed light set, the new flags
            r.rebuild_bvh()
            got = gpu_render(r, frs)
            assert_same(got[0], refs[-1][0], f"rebuild after the material edits, light BVH {mode}")
        finally:
            r.close()


# ------------------------------------------------------------------------------------
# Refusal
# ------------------------------------------------------------------------------------
def test_refused_rebuild_changes_nothing(monkeypatch, luts):
    sd = cornell_scene()
    v = sd.vertices.astype(np.float32)
    need = 2 * mpt.bvh_build_host(v, sd.triangle_indices.reshape(-1, 3))[2] + 2
    r = mpt.GPURenderer(0)
    try:
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh()
        assert e.value.code == -3                                   # MPT_ERR_NO_SCENE
        assert mpt.lib().mpt_rebuild_bvh(None, None) == -1
        r.set_scene(sd)
        r.set_luts(luts)
        before = [r.get_bvh(w) for w in (0, 1)]
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need - 1))
        with pytest.raises(mpt.MptError) as e:
            r.rebuild_bvh()
        assert e.value.code == -4                                   # MPT_ERR_UNSUPPORTED
        after = [r.get_bvh(w) for w in (0, 1)]
        frs = frames(sd, 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        got = gpu_render(r, frs)
        monkeypatch.setenv("MPT_BVH_MAX_STACK", str(need))         # exactly enough: accepted
        assert r.rebuild_bvh(info=True).rebuilt == 1
    finally:
        r.close()
    for w in (0, 1):
        assert before[w][2] == after[w][2]
        assert before[w][0].tobytes() == after[w][0].tobytes() and before[w][1].tobytes() == after[w][1].tobytes()
    assert_same(got[0], oracle_for(sd, luts).render(frs, aov=True)[0], "after a refused rebuild")
