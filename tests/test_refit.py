"""mpt_update_vertices: moved geometry with a GPU refit of both BVH8s (csrc/refit.hip).

Bar: bit-exact.  After an update the device trees equal the host loop's byte for byte; traversal
equals a fresh CPU oracle of the moved scene in (prim, t, u, v); renders (every light-sampling
strategy, MPT_LIGHT_BVH 0 and 1, with and without new vertex normals, ReSTIR DI, a used context,
adaptive sampling, later material edits, a too-deep light tree) equal the oracle of the moved
scene; refused calls change nothing.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi, scene

from raygen import grazing_rays
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_refit_host import (EDITS, check_refit, components, cornell_scene, edit_jitter, edit_move, moved_part, rot_y,
                             small_city)
from test_shade_classes import _assert_modes_equal

pytestmark = pytest.mark.gpu

SCENES = {"cornell": cornell_scene, "city": small_city}
_moved = {}


def moved_scene(name, edit, normals=False):
    """(scene with the edited vertices, new vertices, new normals or None), kept for the module
    (oracle_for caches by identity)."""
    key = (name, edit, normals)
    if key not in _moved:
        sd0 = SCENES[name]()
        v0 = sd0.vertices.astype(np.float32)
        idx = sd0.triangle_indices.reshape(-1, 3)
        nrm = None
        if edit == "render":
            nv, nrm = edit_render(sd0)
            if not normals:
                nrm = None
        else:
            nv = EDITS[edit](v0, idx)
        sd = copy.copy(sd0)
        sd.vertices = nv
        if nrm is not None:
            sd.normals = nrm
        _moved[key] = (sd, nv, nrm)
    return _moved[key]


def edit_render(sd):
    """The light's own triangles moved and one box turned and moved; the box's vertex normals
    turned with it."""
    v = sd.vertices.astype(np.float64).copy()
    idx = sd.triangle_indices.reshape(-1, 3)
    lab = components(idx, len(v))
    light = np.isin(lab, np.unique(lab[idx[sd.emissive].ravel()]))
    assert light.any() and not light.all()
    v[light] += np.array([0.3, -0.12, 0.15])
    box = moved_part(sd.vertices, idx) & ~light
    assert box.any()
    R = rot_y(30.0)
    c = v[box].mean(0)
    v[box] = (v[box] - c) @ R.T + c + np.array([-0.15, 0.25, 0.1])
    n = sd.normals.astype(np.float64).copy()
    n[box] = n[box] @ R.T
    return v.astype(np.float32), n.astype(np.float32)


def in_plane_rays(sd, n, seed):
    """raygen.grazing_rays for a scene without exactly axis-aligned faces (every vertex jittered):
    rays that start on a face and run inside its plane, whatever its orientation -- the direction
    is a combination of the face's edges.  Returns (rays[n, 8], last_hit[n])."""
    rng = np.random.default_rng(seed)
    V = sd.vertices.astype(np.float32)
    I = sd.triangle_indices.reshape(-1, 3)
    A, B, C = V[I[:, 0]], V[I[:, 1]], V[I[:, 2]]
    pick = rng.choice(np.flatnonzero(np.linalg.norm(np.cross(B - A, C - A), axis=1) > 0), n)
    r1, r2 = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    s = np.sqrt(r1)
    u, v = 1 - s, (1 - r2) * s
    e1, e2 = B[pick] - A[pick], C[pick] - A[pick]
    o = (A[pick] + e1 * u[:, None] + e2 * v[:, None]).astype(np.float32)
    w = rng.normal(size=(n, 2))
    d = e1 * w[:, :1] + e2 * w[:, 1:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, 1e35
    return rays, pick.astype(np.int32)


def fresh(sd, luts, env=None):
    r = mpt.GPURenderer(0)
    r.set_scene(sd)
    r.set_luts(luts)
    if env is not None:
        r.set_envmap(env)
    return r


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit", ["jitter", "move"])
@pytest.mark.parametrize("name", list(SCENES))
def test_bytes_equal_host_refit(monkeypatch, luts, name, edit):
    sd0 = SCENES[name]()
    sd, nv, _ = moved_scene(name, edit)
    idx = sd0.triangle_indices.reshape(-1, 3)
    got = {}
    for host in (0, 1):   # 1: the library's own host loop in place of the kernels (test hook)
        monkeypatch.setenv("MPT_REFIT_HOST", str(host))
        r = fresh(sd0, luts)
        try:
            before = [r.get_bvh(w) for w in (0, 1)]
            info = r.update_vertices(nv, info=True)
            got[host] = [r.get_bvh(w) for w in (0, 1)]
        finally:
            r.close()
        assert (info.nodes, info.levels) == (len(before[0][0]), before[0][2])
        assert (info.light_nodes, info.light_levels) == (len(before[1][0]), before[1][2])
    for w in (0, 1):
        assert got[0][w][0].tobytes() == got[1][w][0].tobytes(), f"{name} {edit}: nodes of tree {w}, kernels vs host loop"
        assert got[0][w][1].tobytes() == got[1][w][1].tobytes(), f"{name} {edit}: records of tree {w}, kernels vs host loop"
    # the scene tree against mpt_bvh_refit_host (which has no materials: flag lanes apart)
    hn, ht, hl = mpt.bvh_refit_host(sd0.vertices, idx, nv)
    gn, gt, gl = got[0][0]
    assert gl == hl and gn.tobytes() == hn.tobytes(), f"{name} {edit}: scene nodes vs mpt_bvh_refit_host"
    for f in ("a", "prim", "e1", "e2"):
        assert gt[f].tobytes() == ht[f].tobytes(), f"{name} {edit}: scene records {f}"
    for f in ("alpha_flag", "mat_class"):
        assert np.array_equal(gt[f], before[0][1][f]), f"{name} {edit}: flag lane {f} changed"
    if name == "city":
        assert gt["alpha_flag"].any() and gt["mat_class"].any()
    # the light tree: scene primitive ids, the scene's pad
    ln, lt, _ = got[0][1]
    assert len(ln) > 0 and len(lt) > 0
    check_refit(before[1][0], before[1][1], ln, lt, nv, idx, f"{name} {edit}: light tree")


@pytest.mark.parametrize("host", [0, 1])
def test_two_refits_in_a_row_equal_one(monkeypatch, luts, host):
    """The exact boxes are recomputed from the positions: a refit after a refit gives the bytes of
    one refit straight to the final positions (nothing inflates)."""
    monkeypatch.setenv("MPT_REFIT_HOST", str(host))
    sd0 = small_city()
    v0 = sd0.vertices.astype(np.float32)
    idx = sd0.triangle_indices.reshape(-1, 3)
    v1, v2 = edit_jitter(v0), edit_move(edit_jitter(v0, seed=5), idx)
    out = []
    for chain in ([v1, v2], [v2]):
        r = fresh(sd0, luts)
        try:
            for v in chain:
                r.update_vertices(v)
            out.append([r.get_bvh(w) for w in (0, 1)])
        finally:
            r.close()
    for w in (0, 1):
        assert out[0][w][0].tobytes() == out[1][w][0].tobytes() and out[0][w][1].tobytes() == out[1][w][1].tobytes()


# ------------------------------------------------------------------------------------
# Traversal
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,edit", [("cornell", "jitter"), ("cornell", "move"), ("cornell", "scale_down"),
                                       ("cornell", "plane"), ("city", "jitter"), ("city", "move")])
def test_traversal_after_update_bit_exact(luts, name, edit):
    sd0 = SCENES[name]()
    sd, nv, _ = moved_scene(name, edit)
    o = oracle_for(sd, luts)
    r = fresh(sd0, luts)
    try:
        r.update_vertices(nv)
        # (a jitter of every vertex leaves no exactly axis-aligned face for raygen.grazing_rays)
        graze, glh = in_plane_rays(sd, 20000, 21) if edit == "jitter" else grazing_rays(sd, 20000, 21)
        for what, rays, lh in (("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh)):
            gp, gt, gu, gv = r.trace_closest(rays, lh)
            op, ot, ou, ov = o.trace_closest(rays, lh)
            assert_same(gp, op, f"{name} {edit} {what} prim")
            hit = op >= 0
            if edit != "plane":
                assert hit.mean() > 0.01
            for g, c, k in ((gt, ot, "t"), (gu, ou, "u"), (gv, ov, "v")):
                assert_same(g[hit], c[hit], f"{name} {edit} {what} {k}")
            # from the hit points, the hit primitive excluded (last_hit of a first pass)
            r2 = rays.copy()
            r2[hit, 0:3] = rays[hit, 0:3] + ot[hit, None] * rays[hit, 4:7]
            lh2 = np.where(hit, op, -1).astype(np.int32)
            gp2, gt2, gu2, gv2 = r.trace_closest(r2, lh2)
            op2, ot2, ou2, ov2 = o.trace_closest(r2, lh2)
            assert_same(gp2, op2, f"{name} {edit} {what} prim after last-hit filter")
            h2 = op2 >= 0
            for g, c, k in ((gt2, ot2, "t"), (gu2, ou2, "u"), (gv2, ov2, "v")):
                assert_same(g[h2], c[h2], f"{name} {edit} {what} {k} after last-hit filter")
            rng = np.random.default_rng(2)
            r3 = rays.copy()
            r3[:, 7] = np.where(hit, ot * rng.choice(np.array([0.5, 1.0, 1.5], np.float32), len(rays)), rays[:, 7])
            op3, ot3, _, _ = o.trace_closest(r3, lh)
            assert_same(r.trace_any(r3, lh), (op3 >= 0) & (ot3 < r3[:, 7]), f"{name} {edit} {what} occluded")
    finally:
        r.close()


def test_city_render_alpha_testing_after_update(monkeypatch, luts):
    """The city's alpha-tested leaf cards and lamps after the rigid move, alpha testing on: the
    records keep their alpha-test flags and material classes through the refit."""
    sd0 = small_city()
    sd, nv, _ = moved_scene("city", "move")
    env = mpt.build_envmap(scene.procedural_sky(64, 32, seed=7))
    frs = frames(sd, 64, 36, 2, lss=abi.LSS_RIS_BSDF_AND_LIGHT, world=scene.envmap_world(1.0))
    for f in frs:
        f.render_settings.do_alpha_testing = True
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts, env)
        try:
            r.update_vertices(nv)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    _assert_modes_equal(out, oracle_for(sd, luts, env).render(frs, aov=True), "city alpha after move")


# ------------------------------------------------------------------------------------
# Renders
# ------------------------------------------------------------------------------------
def _render_after_update(monkeypatch, sd0, luts, nv, nrm, frs, modes=(0, 1)):
    out = {}
    for mode in modes:
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.update_vertices(nv, nrm)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    return out


@pytest.mark.parametrize("normals", [False, True], ids=["positions", "positions_normals"])
@pytest.mark.parametrize("strategy", ["uniform", "mis", "ris", "bsdf"])
def test_render_after_update(monkeypatch, luts, strategy, normals):
    """The light's triangles and one box moved: uniform-one-light reads the emissive-triangle
    table, MIS / RIS / BSDF the light BVH and its confirmation query."""
    sd, nv, nrm = moved_scene("cornell", "render", normals)
    frs = frames(sd, 40, 24, 3, lss=STRATEGIES[strategy])
    out = _render_after_update(monkeypatch, cornell_scene(), luts, nv, nrm, frs)
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal(out, ref, f"moved cornell {strategy}")
    assert out[1][0].mean() > 0
    # the move shows: the unmoved scene renders something else
    assert not np.array_equal(ref[0], oracle_for(cornell_scene(), luts).render(frs, aov=True)[0])


def test_render_restir_after_update(luts):
    """ReSTIR DI, fused, default settings: the context's first frame comes after the update."""
    from test_restir import frames as restir_frames
    sd, nv, nrm = moved_scene("cornell", "render", True)
    frs = restir_frames(sd, abi.LSS_RESTIR_DI, 3, w=40, h=24)
    r = fresh(cornell_scene(), luts)
    try:
        r.update_vertices(nv, nrm)
        got = gpu_render(r, frs)
    finally:
        r.close()
    from oracle import oracle as orc
    o = orc.Oracle(sd, luts)
    ref = o.render(frs, aov=True)
    o.close()
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"restir after update {what}")


@pytest.mark.parametrize("adaptive", [False, True], ids=["mis", "mis_adaptive"])
def test_used_context(luts, adaptive):
    """2 frames of scene A, the update, 2 frames of B (the first with need_to_reset and
    sample_number 0): a fresh oracle of B."""
    sd0 = cornell_scene()
    sd, nv, nrm = moved_scene("cornell", "render", True)

    def frs_for(s):
        frs = frames(s, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        for f in frs:
            if adaptive:
                f.render_settings.enable_adaptive_sampling = True
                f.render_settings.adaptive_sampling_min_samples = 1
                f.render_settings.adaptive_sampling_noise_threshold = 0.8
        return frs
    fa, fb = frs_for(sd0), frs_for(sd)
    assert fb[0].render_settings.need_to_reset and fb[0].render_settings.sample_number == 0
    r = fresh(sd0, luts)
    try:
        a = gpu_render(r, fa)
        assert_same(a[0], oracle_for(sd0, luts).render(fa, aov=True)[0], "scene A")
        info = r.update_vertices(nv, nrm, info=True)
        assert info.area_ratio > 1.0
        got = gpu_render(r, fb)
    finally:
        r.close()
    ref = oracle_for(sd, luts).render(fb, aov=True)
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"used context {what}")


# ------------------------------------------------------------------------------------
# Later material edits: the host copies the material paths read must hold the new positions
# ------------------------------------------------------------------------------------
def test_material_edits_after_update(monkeypatch, luts):
    sd0 = cornell_scene()
    sdB, nv, nrm = moved_scene("cornell", "render", True)
    wall = int(sd0.material_indices[0])
    edits = []
    m1 = [abi.Material.from_buffer_copy(m) for m in sd0.materials]   # a wall turned emissive: the light set is rebuilt
    m1[wall].emission = abi.Color(0.3, 0.2, 0.1)
    m1[wall].emission_strength = 2.0
    edits.append(m1)
    # the original emitter off -- by its colour: a strength of 0 makes the reference's
    # emission * strength / strength (intersection_material) a NaN, which is another test's subject
    m2 = [abi.Material.from_buffer_copy(m) for m in m1]
    for i, m in enumerate(m2):
        if i != wall:
            m.emission = abi.Color(0.0, 0.0, 0.0)
    edits.append(m2)
    m3 = [abi.Material.from_buffer_copy(m) for m in m2]              # an alpha-tested material
    idx = sd0.triangle_indices.reshape(-1, 3)
    box_mat = int(sd0.material_indices[np.flatnonzero(moved_part(sd0.vertices, idx)[idx[:, 0]])[0]])
    m3[box_mat].alpha_opacity = 0.5
    edits.append(m3)
    frs = frames(sdB, 40, 24, 2, lss=abi.LSS_BSDF)
    for f in frs:
        f.render_settings.do_alpha_testing = True
    refs = []
    for mats in edits:
        s = copy.copy(sdB)          # (the emissive list stays the uploaded one, as update_materials keeps it)
        s.materials = mats
        from oracle import oracle as orc
        o = orc.Oracle(s, luts)
        refs.append(o.render(frs, aov=True))
        o.close()
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[1][0], refs[2][0])
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.update_vertices(nv, nrm)
            for k, mats in enumerate(edits):
                r.update_materials(mats)
                got = gpu_render(r, frs)
                for j, what in enumerate(["color", "albedo", "normals"]):
                    assert_same(got[j], refs[k][j], f"material edit {k} after the update, light BVH {mode}: {what}")
            # and a further update after the edits: the rebuilt light tree is refitted as well
            r.update_vertices(sd0.vertices, sd0.normals)
            s = copy.copy(sd0)
            s.materials = edits[-1]
            got = gpu_render(r, frs)
        finally:
            r.close()
        from oracle import oracle as orc
        o = orc.Oracle(s, luts)
        ref = o.render(frs, aov=True)
        o.close()
        assert_same(got[0], ref[0], f"update after the material edits, light BVH {mode}")


def test_too_deep_light_tree(monkeypatch, luts):
    """MPT_LIGHT_BVH_MAX_STACK=2 drops the light tree: the update succeeds and light-hit queries
    take the whole-scene path."""
    monkeypatch.setenv("MPT_LIGHT_BVH_MAX_STACK", "2")
    sd, nv, nrm = moved_scene("cornell", "render", True)
    frs = frames(sd, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    r = fresh(cornell_scene(), luts)
    try:
        info = r.update_vertices(nv, nrm, info=True)
        assert info.light_nodes == 0 and len(r.get_bvh(1)[0]) == 0
        got = gpu_render(r, frs)
    finally:
        r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"too-deep light tree {what}")


# ------------------------------------------------------------------------------------
# Errors and info
# ------------------------------------------------------------------------------------
def test_errors_change_nothing(luts):
    sd = cornell_scene()
    v = sd.vertices.astype(np.float32)
    L = mpt.lib()
    r = mpt.GPURenderer(0)
    try:
        with pytest.raises(mpt.MptError) as e:
            r.update_vertices(v)
        assert e.value.code == -3                                   # MPT_ERR_NO_SCENE
        with pytest.raises(mpt.MptError) as e:
            r.get_bvh(0)
        assert e.value.code == -3
        r.set_scene(sd)
        r.set_luts(luts)
        assert L.mpt_update_vertices(r.h, None, None, len(v), None) == -1          # NULL
        assert L.mpt_update_vertices(None, v.ctypes.data, None, len(v), None) == -1
        for bad_n in (len(v) - 1, len(v) + 1, 0):
            assert L.mpt_update_vertices(r.h, v.ctypes.data, None, bad_n, None) == -1   # a wrong count
        for bad in (np.nan, np.inf, -np.inf):
            w = edit_jitter(v)
            w[len(w) // 2, 1] = bad
            with pytest.raises(mpt.MptError) as e:
                r.update_vertices(w)
            assert e.value.code == -1 and "finite" in str(e.value)
        frs = frames(sd, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        got = gpu_render(r, frs)
        nodes, tris, _ = r.get_bvh(0)
    finally:
        r.close()
    assert_same(got[0], oracle_for(sd, luts).render(frs, aov=True)[0], "after refused updates")
    hn, ht, _ = mpt.bvh_refit_host(v, sd.triangle_indices.reshape(-1, 3))
    assert nodes.tobytes() == hn.tobytes() and tris["a"].tobytes() == ht["a"].tobytes()


def test_info(luts):
    sd = small_city()
    v = sd.vertices.astype(np.float32)
    r = fresh(sd, luts)
    try:
        nodes, tris, levels = r.get_bvh(0)
        ln, lt, llevels = r.get_bvh(1)
        assert r.update_vertices(v) is None
        i0 = r.update_vertices(v, info=True)
        assert i0.area_ratio == 1.0 and i0.light_area_ratio == 1.0   # identical sums
        assert (i0.nodes, i0.levels, i0.light_nodes, i0.light_levels) == (len(nodes), levels, len(ln), llevels)
        i1 = r.update_vertices(edit_move(v, sd.triangle_indices.reshape(-1, 3)), info=True)
        assert i1.area_ratio > 1.0
        i2 = r.update_vertices(v, info=True)
        assert i2.area_ratio == 1.0                                   # back: nothing inflated
        counts = np.zeros(3, np.int32)
        assert mpt.lib().mpt_get_bvh(r.h, 0, None, 0, None, 0, counts.ctypes.data) == 0
        assert counts.tolist() == [len(nodes), len(tris), levels]
        assert mpt.lib().mpt_get_bvh(r.h, 2, None, 0, None, 0, counts.ctypes.data) == -1
    finally:
        r.close()
