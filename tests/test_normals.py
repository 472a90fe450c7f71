"""Recomputed vertex normals on the GPU (mpt_set_normals: csrc/normals.hip called by every geometry
update before the per-triangle attribute records are made).

The bar is the project's usual one, the same bytes on the GPU and on the host: a context that sets
the normal groups and then updates its geometry must hold -- positions, normals (mpt_get_vertices),
both trees and the refit report -- what a second context holds after update_vertices(v, n) with n =
mpt.normals_host of the pose the update itself produced.  mpt.normals_host is pinned to the
definition by tests/test_normals_host.py, which also caps the share of vertices that merely pass
through under the poses used here.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi

from test_anim_host import tube
from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for
from test_morph import W1, cornell_morph
from test_normals_host import PASS_CAP, poses, same_bytes
from test_refit import fresh
from test_refit_host import cornell_scene, small_city
from test_shade_classes import _assert_modes_equal
from test_skin import case as skin_case
from test_xform import assert_trees_equal, case as xform_case, edge_scene, info_tuple, soup_scene, trees

pytestmark = pytest.mark.gpu

F = np.float32


def pass_share(v, idx, g, G, has):
    """The share of grouped vertices with a normal flag whose group's face vectors sum to nothing
    (float64: a bound on what the fp32 loop passes through, exact for degenerate groups)."""
    I = np.asarray(idx).reshape(-1, 3)
    p = np.asarray(v, np.float64)
    f = np.cross(p[I[:, 1]] - p[I[:, 0]], p[I[:, 2]] - p[I[:, 0]])
    s = np.zeros((G, 3))
    for k in range(3):
        sel = g[I[:, k]] >= 0
        np.add.at(s, g[I[sel, k]], f[sel])
    grouped = (g >= 0) & (np.asarray(has) != 0)
    dead = ~((s * s).sum(1) > 0)
    return float(dead[g[grouped]].mean())


def state(r, info=None):
    v, n = r.get_vertices()
    return v, n, trees(r), None if info is None else info_tuple(info)


def assert_states_equal(a, b, what):
    assert same_bytes(a[0], b[0]), f"{what}: positions"
    assert same_bytes(a[1], b[1]), f"{what}: normals, {(a[1] != b[1]).any(1).sum()} vertices differ"
    assert_trees_equal(a[2], b[2], what)
    assert a[3] == b[3], f"{what}: report"


def host_state(luts, sd0, v, n, g, G, flips=None):
    """A context after update_vertices(v, normals_host of v over n); and those normals."""
    n2 = mpt.normals_host(v, sd0.triangle_indices, g, n, flips, G, sd0.has_normals)
    b = fresh(sd0, luts)
    try:
        return state(b, b.update_vertices(v, n2, info=True)), n2
    finally:
        b.close()


def welded(sd, only=None):
    g, G = mpt.normal_groups(sd, only=only)
    return g, G, mpt.normal_flips(sd, g, G)


def check_update(luts, sd0, setup, update, v, n, what, only=None):
    """setup(r), set_normals, update(r) -> info against the host path over the pose (v, n) that the
    update produces without the recompute."""
    g, G, flips = welded(sd0, only)
    share = pass_share(v, sd0.triangle_indices, g, G, sd0.has_normals)
    assert share <= PASS_CAP, f"{what}: {share:.3f} of the grouped vertices pass through"
    a = fresh(sd0, luts)
    try:
        setup(a)
        a.set_normals(g, flips, G)
        sa = state(a, update(a))
    finally:
        a.close()
    sb, n2 = host_state(luts, sd0, v, n, g, G, flips)
    assert_states_equal(sa, sb, what)
    grouped = (g >= 0) & (sd0.has_normals != 0)
    assert (n2[grouped] != np.asarray(n, F)[grouped]).any(1).mean() > 0.05, f"{what}: the recompute moved nothing"
    assert same_bytes(n2[~grouped], np.asarray(n, F)[~grouped])
    return sa


# ------------------------------------------------------------------------------------
# Bytes, once through every update call
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["positions", "positions_normals"])
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_update_vertices(luts, name, given):
    sd0 = {"cornell": cornell_scene, "city": small_city}[name]()
    v = poses(name)["jitter"]
    rng = np.random.default_rng(3)
    given_n = (sd0.normals * rng.uniform(0.5, 2.0, (len(v), 1))).astype(F)   # uploaded first, then overwritten
    n = given_n if given else sd0.normals
    check_update(luts, sd0, lambda r: None, lambda r: r.update_vertices(v, given_n if given else None, info=True), v, n,
                 f"{name}: update_vertices")


def test_update_vertices_device_tensor(luts):
    import torch
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    tv = torch.from_numpy(v).to(torch.device("cuda", 0))
    check_update(luts, sd0, lambda r: None, lambda r: r.update_vertices(tv, info=True), v, sd0.normals, "update_vertices of a tensor",
                 only=np.arange(len(v)) % 7 != 2)


def test_update_transforms(luts):
    sd0, ids, M, sd, nv, nn = xform_case("cornell_motion")
    check_update(luts, sd0, lambda r: r.set_objects(ids), lambda r: r.update_transforms(M, info=True), nv, nn, "update_transforms")


def test_update_skin(luts):
    sd0, J, W, M, sd, nv, nn = skin_case("cornell_pose")
    check_update(luts, sd0, lambda r: r.set_skin(J, W), lambda r: r.update_skin(M, info=True), nv, nn, "update_skin")


def plain_morph():
    """cornell_morph without its normal deltas: what most glTF files with blend shapes ship."""
    return [(t[0], t[1], None) for t in cornell_morph()]


def touched(targets, V):
    m = np.zeros(V, bool)
    for t in targets:
        m[t[0]] = True
    return m


def test_update_morph_without_normal_deltas(luts):
    sd0, targets = cornell_scene(), plain_morph()
    nv, nn = mpt.morph_host(sd0.vertices, sd0.normals, targets, W1)
    assert same_bytes(nn, sd0.normals)            # the rest normals pass through: what the feature is for
    check_update(luts, sd0, lambda r: r.set_morph(targets), lambda r: r.update_morph(W1, info=True), nv, nn,
                 "update_morph, no normal deltas", only=touched(targets, len(nv)))


def test_update_morph_skin(luts):
    sd0, J, W, M, _, _, _ = skin_case("cornell_pose")
    targets = plain_morph()
    nv, nn = mpt.skin_host(*mpt.morph_host(sd0.vertices, sd0.normals, targets, W1), J, W, M)

    def setup(r):
        r.set_skin(J, W)
        r.set_morph(targets)

    check_update(luts, sd0, setup, lambda r: r.update_morph_skin(W1, M, info=True), nv, nn, "update_morph_skin")


def test_update_animation(luts):
    _, sd0 = tube()
    t = 0.8
    w, m = mpt.animation_host(sd0, t, 0)
    nv, nn = mpt.skin_host(*mpt.morph_host(sd0.vertices, sd0.normals, sd0.morph, w), sd0.skin.joints, sd0.skin.weights, m)
    assert sd0.morph.touched.any() and len(sd0.morph.touched) == len(nv)

    def setup(r):
        r.set_skin(sd0.skin.joints, sd0.skin.weights, num_joints=sd0.skin.num_joints)
        r.set_morph(sd0.morph)
        r.set_animation(sd0, 0)

    check_update(luts, sd0, setup, lambda r: r.update_animation(t, info=True), nv, nn, "update_animation")


def test_refit_by_the_host_loop(monkeypatch, luts):
    """The MPT_REFIT_HOST branch of the updates' tail recomputes as well."""
    monkeypatch.setenv("MPT_REFIT_HOST", "1")
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    check_update(luts, sd0, lambda r: None, lambda r: r.update_vertices(v, info=True), v, sd0.normals, "MPT_REFIT_HOST")


# ------------------------------------------------------------------------------------
# Edges of the lane mapping; both kernel structures
# ------------------------------------------------------------------------------------
def both_structures(monkeypatch, luts, sd, v2, g, G, flips, what):
    """update_vertices(v2) after set_normals through the two kernels and through the one: the
    bytes of the host path, twice."""
    want = mpt.normals_host(v2, sd.triangle_indices, g, sd.normals, flips, G, sd.has_normals)
    r = fresh(sd, luts)
    try:
        r.set_normals(g, flips, G)
        for fused in ("0", "1"):
            monkeypatch.setenv("MPT_NORMALS_FUSED", fused)
            r.update_vertices(v2, sd.normals)
            gv, gn = r.get_vertices()
            assert same_bytes(gv, v2), f"{what}, fused={fused}: positions"
            assert same_bytes(gn, want), f"{what}, fused={fused}: {(gn != want).any(1).sum()} normals differ"
    finally:
        monkeypatch.delenv("MPT_NORMALS_FUSED")
        r.close()
    return want


@pytest.mark.parametrize("nv", [3, 63, 66, 129, 1027])
def test_soups(monkeypatch, luts, nv):
    v, idx = edge_scene(nv)
    assert len(v) == nv
    sd = soup_scene(v, idx)
    rng = np.random.default_rng(nv)
    v2 = (v + rng.normal(size=v.shape) * 0.05).astype(F)
    # every vertex its own group, the unused ones (counts that are no multiple of 3) included
    g, G = mpt.normal_groups(sd, weld=False)
    want = both_structures(monkeypatch, luts, sd, v2, g, G, None, f"soup {nv}, per vertex")
    used = np.zeros(nv, bool)
    used[idx.ravel()] = True
    assert not same_bytes(want[used], sd.normals[used]) and same_bytes(want[~used], sd.normals[~used])
    # random groups with flips, some vertices left out, the last vertex grouped
    G = max(1, nv // 4)
    g = rng.integers(-1, G, nv).astype(np.int32)
    g[-1] = G - 1
    both_structures(monkeypatch, luts, sd, v2, g, G, (rng.random(G) < 0.5).astype(np.uint8), f"soup {nv}, random groups")


def fan(valence, seed=0):
    """A centre (vertex 0) with `valence` triangles around it, not planar."""
    rng = np.random.default_rng(valence + seed)
    k = valence + 1
    a = np.linspace(0.0, 1.7 * np.pi, k)
    ring = np.stack([np.cos(a), rng.uniform(-0.3, 0.3, k), np.sin(a)], 1)
    v = np.concatenate([[[0.0, 0.4, 0.0]], ring]).astype(F)
    idx = np.array([[0, 2 + i, 1 + i] for i in range(valence)], np.int32)
    return v, idx


@pytest.mark.parametrize("valence", [1, 64, 65, 300])
def test_fan_valence(monkeypatch, luts, valence):
    v, idx = fan(valence)
    v = np.concatenate([v, np.array([[5.0, 5.0, 5.0]], F)])          # an unused vertex, grouped
    sd = soup_scene(v, idx)
    v2 = (v + np.random.default_rng(1).normal(size=v.shape) * 0.02).astype(F)
    g, G = mpt.normal_groups(sd, weld=False)
    want = both_structures(monkeypatch, luts, sd, v2, g, G, None, f"fan {valence}")
    assert same_bytes(want[-1], sd.normals[-1]) and not same_bytes(want[0], sd.normals[0])


@pytest.mark.parametrize("span", [2, 70])
def test_group_spanning_vertices(monkeypatch, luts, span):
    """One group over `span` ring vertices of a fan: neighbours in one group, so every triangle
    between them enters the group's row twice."""
    v, idx = fan(100)
    sd = soup_scene(v, idx)
    v2 = (v + np.random.default_rng(2).normal(size=v.shape) * 0.02).astype(F)
    g = np.arange(len(v), dtype=np.int32)
    g[1:1 + span] = 1
    G = len(v)                                # the ids 2 .. span stay empty groups
    want = both_structures(monkeypatch, luts, sd, v2, g, G, None, f"a group of {span} vertices")
    assert same_bytes(want[1:1 + span], np.tile(want[1], (span, 1)))
    assert not same_bytes(want[1], want[1 + span])


# ------------------------------------------------------------------------------------
# Render
# ------------------------------------------------------------------------------------
def test_render_after_update_morph_without_normal_deltas(luts):
    sd0, targets = cornell_scene(), plain_morph()
    g, G, flips = welded(sd0, touched(targets, len(sd0.vertices)))
    nv, nn = mpt.morph_host(sd0.vertices, sd0.normals, targets, W1)
    sd = copy.copy(sd0)
    sd.vertices, sd.normals = nv, mpt.normals_host(nv, sd0.triangle_indices, g, nn, flips, G, sd0.has_normals)
    frs = frames(sd, 40, 24, 3, lss=STRATEGIES["mis"])
    out = {}
    for recompute in (False, True):
        r = fresh(sd0, luts)
        try:
            r.set_morph(targets)
            if recompute:
                r.set_normals(g, flips, G)
            r.update_morph(W1)
            out[recompute] = gpu_render(r, frs)
        finally:
            r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal({1: out[True]}, ref, "morph without normal deltas, recomputed normals")
    assert out[True][0].mean() > 0
    assert not np.array_equal(out[True][2], out[False][2])           # the recompute shows in the normals AOV


# ------------------------------------------------------------------------------------
# State
# ------------------------------------------------------------------------------------
def test_set_normals_alone_changes_nothing_and_none_clears(luts):
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    g, G, flips = welded(sd0)
    frs = frames(sd0, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        before, img = state(a), gpu_render(a, frs)
        a.set_normals(g, flips, G)
        assert_states_equal(state(a), before, "set_normals alone")
        assert same_bytes(before[0], sd0.vertices) and same_bytes(before[1], sd0.normals)
        img2 = gpu_render(a, frs)   # (the frames start at sample 0: a new accumulation)
        for k in range(3):
            assert_same(img2[k], img[k], "set_normals alone: render")
        a.set_normals(None)
        sa, sb = state(a, a.update_vertices(v, info=True)), state(b, b.update_vertices(v, info=True))
        assert_states_equal(sa, sb, "set_normals(None), then an update")
        assert same_bytes(sa[1], sd0.normals)
        a.set_normals(None)                      # clearing twice is fine
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH], ids=["lbvh", "ploc", "sah"])
def test_state_survives_a_rebuild(luts, mode):
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    g, G, flips = welded(sd0)
    n2 = mpt.normals_host(v, sd0.triangle_indices, g, sd0.normals, flips, G, sd0.has_normals)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_normals(g, flips, G)
        a.rebuild_bvh(mode=mode)
        b.rebuild_bvh(mode=mode)
        sa, sb = state(a, a.update_vertices(v, info=True)), state(b, b.update_vertices(v, n2, info=True))
    finally:
        a.close()
        b.close()
    assert_states_equal(sa, sb, f"mode {mode}: an update after the rebuild")


def test_state_survives_a_material_edit_and_the_other_tables(luts):
    sd0, J, W, M, _, nv, nn = skin_case("cornell_pose")
    ids = xform_case("cornell_motion")[1]
    g, G, flips = welded(sd0)
    mats = [abi.Material.from_buffer_copy(m) for m in sd0.materials]
    mats[int(sd0.material_indices[0])].emission_strength = 2.0
    a = fresh(sd0, luts)
    try:
        a.set_normals(g, flips, G)
        a.update_materials(mats)
        a.set_objects(ids)
        a.set_morph(plain_morph())               # (drops the objects)
        a.set_skin(J, W)
        a.set_morph(None)
        sa = state(a, a.update_skin(M, info=True))
        # and it drops none of them: the skin is still posed from its rest pose
        a.set_normals(None)
        sa2 = state(a, a.update_skin(M, info=True))
    finally:
        a.close()
    b = fresh(sd0, luts)
    try:
        b.update_materials(mats)
        n2 = mpt.normals_host(nv, sd0.triangle_indices, g, nn, flips, G, sd0.has_normals)
        sb = state(b, b.update_vertices(nv, n2, info=True))
        sb2 = state(b, b.update_vertices(nv, nn, info=True))
    finally:
        b.close()
    assert_states_equal(sa, sb, "after a material edit, set_objects, set_morph and set_skin")
    assert_states_equal(sa2, sb2, "the skin after set_normals(None)")


def test_scene_uploads(luts):
    """Set and working after an upload with a build mode (the trees' host copies are stale there);
    every upload drops the state."""
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    g, G, flips = welded(sd0)
    n2 = mpt.normals_host(v, sd0.triangle_indices, g, sd0.normals, flips, G, sd0.has_normals)
    a, b = mpt.GPURenderer(0), mpt.GPURenderer(0)
    try:
        for r in (a, b):
            r.set_scene(sd0, build=abi.BUILD_SAH)
            r.set_luts(luts)
        a.set_normals(g, flips, G)
        sa, sb = state(a, a.update_vertices(v, info=True)), state(b, b.update_vertices(v, n2, info=True))
        assert_states_equal(sa, sb, "after set_scene(build=BUILD_SAH)")
        for build in (None, abi.BUILD_LBVH):
            a.set_normals(g, flips, G)
            a.set_scene(sd0, build=build)
            a.update_vertices(v)
            assert same_bytes(a.get_vertices()[1], sd0.normals), f"build={build}: set_scene dropped the state"
    finally:
        a.close()
        b.close()


def test_refusals_change_nothing(luts):
    sd0 = cornell_scene()
    v = poses("cornell")["jitter"]
    V = len(v)
    g, G, flips = welded(sd0)
    L = mpt.lib()
    r = mpt.GPURenderer(0)
    try:
        assert L.mpt_set_normals(r.h, mpt._p(g), None, V, G) == abi.ERR_NO_SCENE
        assert L.mpt_set_normals(r.h, None, None, 0, 0) == abi.ERR_NO_SCENE
        out = np.zeros((V, 3), F)
        assert L.mpt_get_vertices(r.h, mpt._p(out), None, V) == abi.ERR_NO_SCENE and not out.any()
        r.set_scene(sd0)
        r.set_luts(luts)
        r.set_normals(g, flips, G)
        bad = g.copy()
        bad[5] = G
        low = g.copy()
        low[7] = -2
        for args, msg in (((g[:-1], None, G), "vertex count"), ((g, None, 0), "group count"), ((bad, None, G), "group id"),
                          ((low, None, G), "group id")):
            with pytest.raises(mpt.MptError) as e:
                r.set_normals(*args)
            assert e.value.code == -1 and msg in str(e.value), str(e.value)
        assert L.mpt_set_normals(r.h, None, None, 0, 3) == -1          # NULL with a group count
        assert L.mpt_set_normals(None, mpt._p(g), None, V, G) == -1
        assert L.mpt_get_vertices(r.h, mpt._p(out), None, V - 1) == -1 and not out.any()
        assert L.mpt_get_vertices(r.h, mpt._p(out), None, V) == 0 and same_bytes(out, sd0.vertices)
        # the state set before the refusals is still the one that works
        sa = state(r, r.update_vertices(v, info=True))
    finally:
        r.close()
    sb, _ = host_state(luts, sd0, v, sd0.normals, g, G, flips)
    assert_states_equal(sa, sb, "after the refused calls")
