"""mpt_upload_scene_mode: a scene upload with both BVH8s built on the GPU (csrc/upload.hip for the
flag words and the light set, csrc/lbvh.hip for the trees).

Bar: bit-exact, no tolerances.  After set_scene(sd, build=mode) the device trees equal the host
loop of the same definition (bvh_build_host(mode=mode)) byte for byte, over all primitives and over
the light set a host upload selects; the records' flag lanes equal those a host upload stamps;
traversal and renders equal a host-uploaded context's ("traversal results never depend on the
tree"); updates, rebuilds and material edits work afterwards as after a rebuild; a live context
changes topology; a refused call changes nothing, a failed one leaves no scene.

Every GPU test here goes through set_scene(..., build=mode) and so fails without the entry point.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi, scene, synthetic

from raygen import grazing_rays
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, random_rays
from test_ploc_rebuild import assert_tree_equals_host, same_bytes
from test_rebuild import SCENES, flags_of, raw_scene
from test_refit import fresh
from test_refit_host import EDITS, cornell_scene, moved_part, small_city

pytestmark = pytest.mark.gpu

MODES = [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH]
MODE_IDS = ["lbvh", "ploc", "sah"]

_made = {}


def _lit(m):
    k = m.emission_strength
    return m.emission_texture_index != -1 or m.emission.r * k > 0 or m.emission.g * k > 0 or m.emission.b * k > 0


def raw_variant(name):
    """raw_scene's recipe over tiny257 with materials that all cannot emit ("dark257": no light set)
    or all emit ("lit257": the light set is every primitive, the first and the last included)."""
    if name not in _made:
        sd = copy.copy(raw_scene("tiny257"))
        mats = [abi.Material.from_buffer_copy(m) for m in sd.materials]
        if name == "dark257":
            mats = [m for m in mats if not _lit(m)]
            assert len(mats) > 1
        else:
            for k, m in enumerate(mats):
                m.emission = abi.Color(0.5 + 0.1 * (k % 3), 0.4, 0.3)
                m.emission_strength = 1.0 + k
        sd.materials = mats
        sd.material_indices = (np.arange(len(sd.triangle_indices) // 3) % len(mats)).astype(np.int32)
        sd.name = name
        _made[name] = sd.finalize()
    return _made[name]


def scene_for(name):
    return raw_variant(name) if name in ("dark257", "lit257") else SCENES[name]()


def uploaded(sd, luts, mode, env=None):
    """A fresh context whose scene went through mpt_upload_scene_mode; (renderer, RebuildInfo)."""
    r = mpt.GPURenderer(0)
    try:
        info = r.set_scene(sd, build=mode, info=True)
        r.set_luts(luts)
        if env is not None:
            r.set_envmap(env)
    except BaseException:
        r.close()
        raise
    return r, info


def trees(r):
    return [r.get_bvh(w) for w in (0, 1)]


_host_trees = {}


def host_trees(name, luts):
    """Both trees of a context that uploaded the scene through mpt_upload_scene (kept per scene)."""
    if name not in _host_trees:
        r = fresh(scene_for(name), luts)
        try:
            _host_trees[name] = trees(r)
        finally:
            r.close()
    return _host_trees[name]


def check_trees(name, luts, sd, got, mode, v=None, host=None):
    """got against the host loop of `mode` over v (None: the scene's vertices); light set and flag
    lanes as in `host` (None: the host upload of the scene)."""
    host = host if host is not None else host_trees(name, luts)
    v = sd.vertices.astype(np.float32) if v is None else v
    idx = sd.triangle_indices.reshape(-1, 3)
    light_prims = np.sort(host[1][1]["prim"]).astype(np.int32)
    assert_tree_equals_host(got[0], v, idx, None, flags_of(host[0][1], len(idx)), f"{name}: scene tree", mode=mode)
    assert_tree_equals_host(got[1], v, idx, light_prims, flags_of(host[1][1], len(idx)), f"{name}: light tree", mode=mode)
    assert np.array_equal(np.sort(got[1][1]["prim"]), light_prims), f"{name}: light set"
    return light_prims


def check_info(info, got):
    assert (info.rebuilt, info.nodes, info.records, info.levels) == (1, len(got[0][0]), len(got[0][1]), got[0][2])
    has_light = int(len(got[1][1]) > 0)
    assert (info.light_rebuilt, info.light_nodes, info.light_records, info.light_levels) == \
        (has_light, len(got[1][0]), len(got[1][1]), got[1][2])


# ------------------------------------------------------------------------------------
# 1. Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(SCENES) + ["dark257", "lit257"])
def test_bytes_equal_host_build(luts, name, mode):
    sd = scene_for(name)
    n = len(sd.triangle_indices) // 3
    r, info = uploaded(sd, luts, mode)
    try:
        got = trees(r)
    finally:
        r.close()
    light_prims = check_trees(name, luts, sd, got, mode)
    check_info(info, got)
    if name == "city":
        assert got[0][1]["alpha_flag"].any() and got[0][1]["mat_class"].any()
    if name in ("cornell", "city", "tiny257"):
        assert 0 < len(light_prims) < n
    if name == "dark257":
        assert len(got[1][0]) == 0 and len(got[1][1]) == 0 and got[1][2] == 0 and info.light_rebuilt == 0
    if name == "lit257":
        assert np.array_equal(light_prims, np.arange(n)) and light_prims[0] == 0 and light_prims[-1] == n - 1


def test_too_deep_light_tree_is_dropped(monkeypatch, luts):
    """The light-hit tree past its stack bound is dropped as a host upload drops it: no light tree,
    the same image (the exact whole-scene closest-hit path)."""
    monkeypatch.setenv("MPT_LIGHT_BVH_MAX_STACK", "2")
    sd = cornell_scene()
    frs = frames(sd, 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    r = fresh(sd, luts)
    try:
        assert len(r.get_bvh(1)[0]) == 0
        ref = gpu_render(r, frs)
    finally:
        r.close()
    r, info = uploaded(sd, luts, abi.BUILD_SAH)
    try:
        assert len(r.get_bvh(1)[0]) == 0 and info.light_rebuilt == 0 and info.rebuilt == 1
        got = gpu_render(r, frs)
    finally:
        r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[j], ref[j], f"dropped light tree: {what}")
    assert got[0].mean() > 0


# ------------------------------------------------------------------------------------
# 2. Traversal
# ------------------------------------------------------------------------------------
_trav = {}


def trace_sets(r, sets):
    out = []
    for what, rays, lh, r3 in sets:
        out.append((r.trace_closest(rays, lh), r.trace_any(r3, lh) if r3 is not None else None))
    return out


def traversal_reference(name, luts):
    """Ray sets and the host-uploaded context's results; the any-hit rays end at 0.5 / 1 / 1.5 times
    the closest hit's distance."""
    if name not in _trav:
        sd = scene_for(name)
        graze, glh = grazing_rays(sd, 20000, 21)
        base = [("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh)]
        r = fresh(sd, luts)
        try:
            sets = []
            for what, rays, lh in base:
                prim, t, _, _ = r.trace_closest(rays, lh)
                r3 = rays.copy()
                f = np.random.default_rng(2).choice(np.array([0.5, 1.0, 1.5], np.float32), len(rays))
                r3[:, 7] = np.where(prim >= 0, t * f, rays[:, 7])
                sets.append((what, rays, lh, r3))
            _trav[name] = (sets, trace_sets(r, sets))
        finally:
            r.close()
    return _trav[name]


def assert_traversal_equal(got, ref, sets, what):
    for (kind, _, _, _), ((gp, gt, gu, gv), gocc), ((hp, ht, hu, hv), hocc) in zip(sets, got, ref):
        assert_same(gp, hp, f"{what} {kind} prim")
        hit = hp >= 0
        assert hit.mean() > 0.01
        for g, h, lane in ((gt, ht, "t"), (gu, hu, "u"), (gv, hv, "v")):
            assert_same(g[hit], h[hit], f"{what} {kind} {lane}")
        assert_same(gocc, hocc, f"{what} {kind} occluded")
        assert hocc.any() and not hocc.all()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_traversal_equals_host_upload(luts, name, mode):
    sets, ref = traversal_reference(name, luts)
    r, _ = uploaded(scene_for(name), luts, mode)
    try:
        got = trace_sets(r, sets)
    finally:
        r.close()
    assert_traversal_equal(got, ref, sets, f"{name} mode {mode}")


# ------------------------------------------------------------------------------------
# 3. Renders
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return scene.load_gltf(synthetic.write_textured_gltf(str(tmp_path_factory.mktemp("room"))))


_loaded = {}


def render_case(case, room):
    """(scene, frames) of a render case."""
    if case in STRATEGIES:
        sd = cornell_scene()
        return sd, frames(sd, 64, 64, 2, lss=STRATEGIES[case])
    if case == "restir":
        from test_restir import frames as restir_frames
        sd = cornell_scene()
        return sd, restir_frames(sd, abi.LSS_RESTIR_DI, 3, w=64, h=36)
    if case == "room_alpha":
        frs = frames(room, 48, 48, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        for f in frs:
            f.render_settings.do_alpha_testing = True
        return room, frs
    if case not in _loaded:
        _loaded[case] = scene.load_scene(case)
    return _loaded[case], frames(_loaded[case], 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF, bounces=8)


RENDER_CASES = list(STRATEGIES) + ["restir", "room_alpha", "multi-dispersion", "nested-dielectrics"]
_render_ref = {}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", RENDER_CASES)
def test_render_equals_host_upload(luts, room, case, mode):
    sd, frs = render_case(case, room)
    if case not in _render_ref:
        r = fresh(sd, luts)
        try:
            _render_ref[case] = gpu_render(r, frs)
        finally:
            r.close()
    ref = _render_ref[case]
    r, _ = uploaded(sd, luts, mode)
    try:
        got = gpu_render(r, frs)
    finally:
        r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[j], ref[j], f"{case} mode {mode}: {what}")
    assert ref[0].mean() > 0


# ------------------------------------------------------------------------------------
# 4. Life after the upload
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_updates_and_rebuild_after_upload(luts, name, mode):
    sd = scene_for(name)
    v0 = sd.vertices.astype(np.float32)
    idx = sd.triangle_indices.reshape(-1, 3)
    vm = EDITS["move"](v0, idx)
    r, info = uploaded(sd, luts, mode)
    try:
        built = trees(r)
        ri = r.update_vertices(v0, info=True)
        same = trees(r)
        r.update_vertices(vm)
        rb = r.rebuild_bvh(info=True, mode=mode)
        rebuilt = trees(r)
    finally:
        r.close()
    assert same_bytes(same, built), f"{name}: a tree changed under an identity update"
    assert ri.area_ratio == 1.0 and ri.light_area_ratio == 1.0
    assert (ri.nodes, ri.levels, ri.light_nodes, ri.light_levels) == (info.nodes, info.levels, info.light_nodes, info.light_levels)
    check_trees(name, luts, sd, rebuilt, mode, v=vm)
    check_info(rb, rebuilt)


def material_edit(sd, which):
    mats = [abi.Material.from_buffer_copy(m) for m in sd.materials]
    if which == "emissive":      # a wall turned emissive: the light set grows
        wall = int(sd.material_indices[0])
        assert not _lit(mats[wall])
        mats[wall].emission = abi.Color(0.3, 0.2, 0.1)
        mats[wall].emission_strength = 2.0
    else:                        # an alpha-tested box: the alpha lanes are re-stamped
        idx = sd.triangle_indices.reshape(-1, 3)
        box = int(sd.material_indices[np.flatnonzero(moved_part(sd.vertices, idx)[idx[:, 0]])[0]])
        mats[box].alpha_opacity = 0.5
    return mats


_edit_ref = {}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("which", ["emissive", "alpha"])
def test_material_edit_after_upload(luts, which, mode):
    sd = cornell_scene()
    n = len(sd.triangle_indices) // 3
    mats = material_edit(sd, which)
    frs = frames(sd, 64, 36, 2, lss=abi.LSS_BSDF)
    for f in frs:
        f.render_settings.do_alpha_testing = True

    def edited(r):
        r.update_materials(mats)
        t = trees(r)
        return t, gpu_render(r, frs)

    if which not in _edit_ref:
        r = fresh(sd, luts)
        try:
            _edit_ref[which] = edited(r)
        finally:
            r.close()
    ht, himg = _edit_ref[which]
    r, _ = uploaded(sd, luts, mode)
    try:
        before = trees(r)
        gt, gimg = edited(r)
    finally:
        r.close()
    assert np.array_equal(np.sort(gt[1][1]["prim"]), np.sort(ht[1][1]["prim"])), f"{which}: light set"
    for w in (0, 1):
        hf, gf = flags_of(ht[w][1], n), flags_of(gt[w][1], n)
        for lane in ("alpha_flag", "mat_class"):
            assert np.array_equal(gf[lane], hf[lane]), f"{which}: tree {w} {lane}"
    if which == "emissive":
        assert len(gt[1][1]) > len(before[1][1])
    else:
        assert gt[0][1]["alpha_flag"].sum() > before[0][1]["alpha_flag"].sum()
        assert gt[0][0].tobytes() == before[0][0].tobytes()       # the scene tree built on the device stays
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(gimg[j], himg[j], f"{which} edit after a mode {mode} upload: {what}")
    assert gimg[0].mean() > 0


# ------------------------------------------------------------------------------------
# 5. Topology change on a live context
# ------------------------------------------------------------------------------------
def snapshot(r, sd, rays):
    frs = frames(sd, 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    return trees(r), r.trace_closest(rays), r.trace_any(rays), gpu_render(r, frs)


def assert_snapshots_equal(a, b, what):
    assert same_bytes(a[0], b[0]), f"{what}: trees"
    for x, y, lane in zip(a[1], b[1], ("prim", "t", "u", "v")):
        hit = b[1][0] >= 0
        assert_same(x[hit], y[hit], f"{what}: closest {lane}")
    assert_same(a[1][0], b[1][0], f"{what}: closest prim")
    assert_same(a[2], b[2], f"{what}: occluded")
    for j, lane in enumerate(["color", "albedo", "normals"]):
        assert_same(a[3][j], b[3][j], f"{what}: {lane}")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_topology_change_on_a_live_context(luts, mode):
    first = cornell_scene()
    others = [small_city(), raw_scene("tiny9")]
    assert len({len(s.vertices) for s in others + [first]}) == 3 and len({len(s.materials) for s in [first, others[0]]}) == 2
    rays = {id(s): random_rays(s, 4000, 11) for s in others + [first]}
    live = fresh(first, luts)
    try:
        gpu_render(live, frames(first, 64, 36, 2, lss=abi.LSS_RIS_BSDF_AND_LIGHT))
        for sd in others:
            info = live.set_scene(sd, build=mode, info=True)
            got = snapshot(live, sd, rays[id(sd)])
            check_info(info, got[0])
            r, _ = uploaded(sd, luts, mode)
            try:
                ref = snapshot(r, sd, rays[id(sd)])
            finally:
                r.close()
            assert_snapshots_equal(got, ref, f"{sd.name} on a live context, mode {mode}")
        live.set_scene(first)                                   # and back, by the host builder
        got = snapshot(live, first, rays[id(first)])
        r = fresh(first, luts)
        try:
            ref = snapshot(r, first, rays[id(first)])
        finally:
            r.close()
        assert_snapshots_equal(got, ref, "back to a host upload")
        assert got[3][0].mean() > 0
    finally:
        live.close()


# ------------------------------------------------------------------------------------
# 6. Refusals
# ------------------------------------------------------------------------------------
def test_refused_upload_changes_nothing(luts):
    sd = cornell_scene()
    frs = frames(sd, 64, 36, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    bad = copy.copy(sd)
    bad.triangle_indices = sd.triangle_indices.copy()
    bad.triangle_indices[5] = len(sd.vertices)
    r, _ = uploaded(sd, luts, abi.BUILD_PLOC)
    try:
        before = trees(r)
        ref = gpu_render(r, frs)
        with pytest.raises(mpt.MptError) as e:
            r.set_scene(raw_scene("tiny9"), build=2)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and "unknown build mode" in str(e.value)
        with pytest.raises(mpt.MptError) as e:
            r.set_scene(bad, build=abi.BUILD_SAH)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and "triangle index out of range" in str(e.value)
        assert same_bytes(trees(r), before)
        got = gpu_render(r, frs)
    finally:
        r.close()
    for j, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[j], ref[j], f"after refused uploads: {what}")
    assert got[0].mean() > 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_too_deep_scene_tree_leaves_no_scene(monkeypatch, luts, mode):
    sd = raw_scene("tiny2049")
    frs = frames(sd, 64, 36, 1)
    r = fresh(cornell_scene(), luts)
    try:
        monkeypatch.setenv("MPT_BVH_MAX_STACK", "4")           # read at the call: one level only
        with pytest.raises(mpt.MptError) as e:
            r.set_scene(sd, build=mode)
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(mpt.MptError) as e:
            r.render(frs[0])
        assert e.value.code == abi.ERR_NO_SCENE
        monkeypatch.delenv("MPT_BVH_MAX_STACK")
        info = r.set_scene(sd, build=mode, info=True)           # the context is usable again
        got = trees(r)
    finally:
        r.close()
    check_info(info, got)
    check_trees("tiny2049", luts, sd, got, mode)
