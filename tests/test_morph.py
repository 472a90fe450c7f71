"""mpt_set_morph / mpt_update_morph / mpt_update_morph_skin: morph targets applied on the GPU
(csrc/morph.hip), composed with the skin in one kernel, then the refit of both BVH8s.

Bar: bit-exact.  After an update the device trees and the report equal those of a second context
that got mpt_update_vertices of the host mirrors' output -- mpt_morph_host, followed by mpt_skin_host
when a skin is posed -- byte for byte, and pass the refit's own checks; traversal equals a fresh
upload of the morphed scene; renders equal the CPU oracle of the morphed scene; a morph composes with
a skin in every order of calls and excludes an object table; morph and skin share one rest pose;
refused calls change nothing, the retained weights and palette included; the kernel's lane groups,
waves and blocks are exercised at their edges and its variants (one vertex per lane, weights and
palette in LDS or gathered, sizes at and past the LDS budgets) give the same bytes.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi

from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_refit import fresh, in_plane_rays
from test_refit_host import check_refit, cornell_scene, edit_jitter, rot_y, small_city
from test_shade_classes import _assert_modes_equal
from test_skin import case as skin_case, cornell_pose, cornell_skin, random_pose, random_skin
from test_xform import IDENT, assert_trees_equal, cornell_objects, edge_scene, info_tuple, rigid, soup_scene, trees

pytestmark = pytest.mark.gpu

F = np.float32
_cases = {}
W1 = np.array([0.6, -0.8, 1.0, 0.0], F)
W2 = np.array([-0.3, 0.5, 0.4, 0.0], F)


def cornell_morph():
    """Four targets on cornell_skin's box and light: 0 moves every box vertex and has normal deltas,
    1 is sparse (every fifth box vertex, no normal deltas), 2 moves the light's own triangles, 3 is
    one box vertex with a delta of 4 (weight 0 in every accepted pose: the overflow's handle)."""
    sd = cornell_scene()
    _, light, box = cornell_objects()
    box, light = np.flatnonzero(box), np.flatnonzero(light)
    rng = np.random.default_rng(4)
    ext = float(np.ptp(sd.vertices[box], axis=0).max())
    t0 = (box, (rng.normal(size=(len(box), 3)) * 0.08 * ext).astype(F), (rng.normal(size=(len(box), 3)) * 0.4).astype(F))
    sp = box[::5]
    t1 = (sp, (rng.normal(size=(len(sp), 3)) * 0.1 * ext).astype(F), None)
    t2 = (light, np.tile(np.array([[0.1, -0.05, 0.08]], F) * F(ext), (len(light), 1)), None)
    t3 = (box[:1], np.array([[4.0, 0.0, 0.0]], F), None)
    return [t0, t1, t2, t3]


def case(name):
    """(rest scene, targets, weights, morphed scene, morphed vertices, morphed normals), kept for the
    module.  The morphed arrays are mpt.morph_host's."""
    if name in _cases:
        return _cases[name]
    if name.startswith("cornell"):
        sd0, targets = cornell_scene(), cornell_morph()
        w = W1 if name == "cornell" else W2
    else:
        assert name == "city"
        sd0 = small_city()
        V = len(sd0.vertices)
        rng = np.random.default_rng(23)
        ext = float(np.ptp(sd0.vertices, axis=0).max())
        free = np.arange(V) % 11 != 0                       # every 11th vertex without entries
        targets = []
        for t in range(6):
            ids = np.flatnonzero(free & (rng.random(V) < (0.1 if t == 4 else 0.7)))
            targets.append((ids, (rng.normal(size=(len(ids), 3)) * 0.01 * ext).astype(F),
                            (rng.normal(size=(len(ids), 3)) * 0.3).astype(F) if t < 3 else None))
        w = np.array([0.5, -0.7, 0.0, 1.2, 0.9, -0.2], F)
    nv, nn = mpt.morph_host(sd0.vertices, sd0.normals, targets, w)
    sd = copy.copy(sd0)
    sd.vertices, sd.normals = nv, nn
    _cases[name] = (sd0, targets, w, sd, nv, nn)
    return _cases[name]


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "city"])
def test_bytes_equal_host_path(luts, name):
    sd0, targets, w, sd, nv, nn = case(name)
    idx = sd0.triangle_indices.reshape(-1, 3)
    assert not np.array_equal(nv, sd0.vertices) and not np.array_equal(nn, sd0.normals)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        before = trees(a)
        a.set_morph(targets)
        ia = a.update_morph(w, info=True)
        ib = b.update_vertices(nv, nn, info=True)
        ta, tb = trees(a), trees(b)
    finally:
        a.close()
        b.close()
    assert_trees_equal(ta, tb, f"{name}: update_morph vs update_vertices of morph_host")
    assert info_tuple(ia) == info_tuple(ib) and ia.area_ratio != 1.0
    hn, ht, hl = mpt.bvh_refit_host(sd0.vertices, idx, nv)
    assert ta[0][2] == hl and ta[0][0].tobytes() == hn.tobytes(), f"{name}: scene nodes vs mpt_bvh_refit_host"
    for f in ("a", "prim", "e1", "e2"):
        assert ta[0][1][f].tobytes() == ht[f].tobytes(), f"{name}: scene records {f}"
    for k in (0, 1):
        assert len(ta[k][0]) > 0
        check_refit(before[k][0], before[k][1], ta[k][0], ta[k][1], nv, idx, f"{name}: tree {k}")


# ------------------------------------------------------------------------------------
# Traversal and renders
# ------------------------------------------------------------------------------------
def test_traversal_equals_fresh_upload(luts):
    sd0, targets, w, sd, nv, nn = case("cornell")
    a, b = fresh(sd0, luts), fresh(sd, luts)
    try:
        a.set_morph(targets)
        a.update_morph(w)
        graze, glh = in_plane_rays(sd, 20000, 21)
        for what, rays, lh in (("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh)):
            ga, gb = a.trace_closest(rays, lh), b.trace_closest(rays, lh)
            assert_same(ga[0], gb[0], f"{what} prim")
            hit = gb[0] >= 0
            assert hit.mean() > 0.01
            for k, q in enumerate("tuv"):
                assert_same(ga[k + 1][hit], gb[k + 1][hit], f"{what} {q}")
            r3 = rays.copy()
            rng = np.random.default_rng(2)
            r3[:, 7] = np.where(hit, gb[1] * rng.choice(np.array([0.5, 1.0, 1.5], F), len(rays)), rays[:, 7])
            assert_same(a.trace_any(r3, lh), b.trace_any(r3, lh), f"{what} occluded")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("strategy", ["mis", "ris"])
def test_render_after_update_morph(monkeypatch, luts, strategy):
    """The light's own triangles moved by a target and a box morphed with its vertex normals,
    MPT_LIGHT_BVH 0 and 1: the oracle of the morphed scene."""
    sd0, targets, w, sd, nv, nn = case("cornell")
    frs = frames(sd, 40, 24, 3, lss=STRATEGIES[strategy])
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.set_morph(targets)
            r.update_morph(w)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal(out, ref, f"cornell {strategy}")
    assert out[1][0].mean() > 0
    assert not np.array_equal(ref[0], oracle_for(sd0, luts).render(frs, aov=True)[0])   # the morph shows


# ------------------------------------------------------------------------------------
# Composition with the skin
# ------------------------------------------------------------------------------------
def test_morph_composes_with_the_skin(luts):
    sd0, targets, w, sd, nv, nn = case("cornell")
    J, W, _, _ = cornell_skin()
    M = cornell_pose(1)
    sv, sn = mpt.skin_host(nv, nn, J, W, M)                 # skin(morph(rest))
    assert not np.array_equal(sv, nv)
    plain = mpt.skin_host(sd0.vertices, sd0.normals, J, W, M)
    want = {}
    b = fresh(sd0, luts)
    try:
        for key, arrays in (("both", (sv, sn)), ("skin", plain), ("morph", (nv, nn))):
            b.update_vertices(*arrays)
            want[key] = trees(b)
    finally:
        b.close()
    orders = {
        "one call": lambda r: r.update_morph_skin(w, M),
        "morph, then skin": lambda r: (r.update_morph(w), r.update_skin(M)),
        "skin, then morph": lambda r: (r.update_skin(M), r.update_morph(w)),
    }
    for what, pose in orders.items():
        for first in ("morph", "skin"):                      # which of the two captured the rest pose
            r = fresh(sd0, luts)
            try:
                if first == "morph":
                    r.set_morph(targets)
                    r.set_skin(J, W)
                else:
                    r.set_skin(J, W)
                    r.set_morph(targets)
                pose(r)
                assert_trees_equal(trees(r), want["both"], f"{what} ({first} set first)")
            finally:
                r.close()
    r = fresh(sd0, luts)
    try:
        r.set_skin(J, W)
        r.set_morph(targets)
        r.update_morph(w)                                    # before any skin pose: the morph alone
        assert_trees_equal(trees(r), want["morph"], "update_morph before any skin pose")
        r.set_morph(targets)                                 # the weights start again at zero
        r.update_skin(M)                                     # retained weights all zero: today's update_skin
        assert_trees_equal(trees(r), want["skin"], "update_skin with the retained weights all zero")
        r.update_morph(w)                                    # and the palette is retained in turn
        assert_trees_equal(trees(r), want["both"], "update_morph with the retained palette")
    finally:
        r.close()


# ------------------------------------------------------------------------------------
# Edges: a partial last lane group, a partial wave, a partial block; rows of 0, 1 and T entries
# ------------------------------------------------------------------------------------
def rows_morph(nv, last_full, seed, T=3):
    """Per vertex 0, 1 or T entries in the pattern T 1 0 0 | T T 1 0: an empty row meets a full one at
    every lane group's boundary (3 | 4, 7 | 8); the last two vertices are empty, full or full, empty."""
    rng = np.random.default_rng(seed)
    counts = np.array([T, 1, 0, 0, T, T, 1, 0])[np.arange(nv) % 8]
    if nv >= 2:
        counts[-2:] = [0, T] if last_full else [T, 0]
    targets = []
    for t in range(T):
        ids = np.flatnonzero((counts == T) | ((counts == 1) & (np.arange(nv) % T == t)))
        targets.append((ids, rng.normal(size=(len(ids), 3)).astype(F) * F(0.3), rng.normal(size=(len(ids), 3)).astype(F) if t != 1 else None))
    return targets, counts


def both_paths(luts, sd, targets, w, skin=None):
    """(info, trees) through update_morph (update_morph_skin with skin = (J, W, M)) and through
    update_vertices of the host mirrors; either may be an MptError instead."""
    out = []
    for dev in (True, False):
        r = fresh(sd, luts)
        try:
            if dev:
                r.set_morph(targets)
                if skin:
                    r.set_skin(skin[0], skin[1], num_joints=len(skin[2]))
                    i = r.update_morph_skin(w, skin[2], info=True)
                else:
                    i = r.update_morph(w, info=True)
            else:
                hv, hn = mpt.morph_host(sd.vertices, sd.normals, targets, w)
                if skin:
                    hv, hn = mpt.skin_host(hv, hn, *skin)
                i = r.update_vertices(hv, hn, info=True)
            out.append((info_tuple(i), trees(r)))
        except mpt.MptError as e:
            out.append(e)
        finally:
            r.close()
    return out


@pytest.mark.parametrize("group", ["1", "4"])
@pytest.mark.parametrize("nv", [3, 63, 66, 129, 1027])
def test_edge_counts(monkeypatch, luts, nv, group):
    monkeypatch.setenv("MPT_MORPH_GROUP", group)
    monkeypatch.delenv("MPT_MORPH_LDS", raising=False)
    v, idx = edge_scene(nv)
    assert len(v) == nv
    w = np.array([0.9, -0.6, 0.4], F)
    for last_full in (True, False):
        targets, counts = rows_morph(nv, last_full, nv)
        assert counts[-1] == (3 if last_full else 0) and {0, 3} <= set(counts.tolist())
        dev, host = both_paths(luts, soup_scene(v, idx), targets, w)
        assert dev[0] == host[0]
        assert_trees_equal(dev[1], host[1], f"{nv} vertices, last row {'full' if last_full else 'empty'}")
        # the largest coordinate in the last vertex (it decides the pad): the last triangle's when the
        # count is a multiple of 3, else an unused vertex, which must not count
        v2 = v.copy()
        v2[-1] = [0.0, 900.0, 0.0]
        dev, host = both_paths(luts, soup_scene(v2, idx), targets, w)
        assert dev[0] == host[0]
        assert_trees_equal(dev[1], host[1], f"{nv} vertices, the maximum in the last")
    # the fused kernel at the same edges
    skin = random_skin(nv, 3, nv) + (np.stack([rigid(rot_y(25.0), [0, 0, 0], [0.5, 0, 0]), IDENT,
                                               rigid(np.diag([1.5, 0.5, 2.0]) @ rot_y(-70.0), [1, 0, 0], [0, 1, 0])]),)
    targets, _ = rows_morph(nv, True, nv)
    dev, host = both_paths(luts, soup_scene(v, idx), targets, w, skin)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nv} vertices, fused")
    # the only non-finite result in the last vertex (a full row): refused by both, used or not
    v3 = v.copy()
    v3[-1] = [3e38, 1.0, 1.0]
    ids, dp, dn = targets[0]
    assert ids[-1] == nv - 1
    dp = dp.copy()
    dp[-1] = [3e38, 0.0, 0.0]
    dev, host = both_paths(luts, soup_scene(v3, idx), [(ids, dp, dn)] + targets[1:], np.array([1.0, -0.6, 0.4], F))
    assert isinstance(dev, mpt.MptError) and dev.code == -1 and "finite" in str(dev)
    assert isinstance(host, mpt.MptError) and host.code == -1


def test_unused_vertex_does_not_set_the_pad(luts):
    """An appended unused vertex at 1e30 with an entry: the pad is the host path's (the maximum runs
    over the used vertices)."""
    from test_refit_host import tiny
    v, idx = tiny(21)
    v = np.concatenate([v, np.array([[1e30, 0, 0]], F)])
    sd = soup_scene(v, idx)
    ids = np.arange(len(v))
    targets = [(ids, np.tile(np.array([[0.0, 0.5, 0.1]], F), (len(v), 1)), None)]
    w = np.array([1.0], F)
    dev, host = both_paths(luts, sd, targets, w)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], "an unused vertex at 1e30")
    nv, _ = mpt.morph_host(sd.vertices, sd.normals, targets, w)
    pad = F(np.ldexp(max(F(np.abs(nv[:-1]).max()), F(1.0)), -20))
    rec = dev[1][0][1]
    lo = nv[idx[rec["prim"]]].min(1)
    assert ((lo - pad).astype(F).min(0) == dev[1][0][0]["p"][0]).all()


# ------------------------------------------------------------------------------------
# The kernel's variants give the same bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["morph", "fused"])
def test_one_vertex_per_lane_and_gather_give_the_same_bytes(monkeypatch, luts, fused):
    """MPT_MORPH_GROUP=1 (one vertex per lane, also the default) and 4 (four, 16-byte accesses) and
    MPT_MORPH_LDS=0 (weights, and the fused kernel's palette, gathered through the cache), alone and
    together, against the defaults."""
    sd0, targets, w, sd, nv, nn = case("city")
    _, J, W, M, _, _, _ = skin_case("city")
    out = []
    for group, lds in ((None, None), ("1", None), (None, "0"), ("1", "0"), ("4", None), ("4", "0")):
        for var, val in (("MPT_MORPH_GROUP", group), ("MPT_MORPH_LDS", lds)):
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)
        r = fresh(sd0, luts)
        try:
            r.set_morph(targets)
            if fused:
                r.set_skin(J, W, num_joints=len(M))
                out.append((info_tuple(r.update_morph_skin(w, M, info=True)), trees(r)))
            else:
                out.append((info_tuple(r.update_morph(w, info=True)), trees(r)))
        finally:
            r.close()
    for k in range(1, 6):
        assert out[0][0] == out[k][0]
        assert_trees_equal(out[0][1], out[k][1], f"kernel variant {k} vs the default")
    b = fresh(sd0, luts)
    try:
        b.update_vertices(*(mpt.skin_host(nv, nn, J, W, M) if fused else (nv, nn)))
        assert_trees_equal(out[0][1], trees(b), "the default vs the host mirrors")
    finally:
        b.close()


def many_targets(nv, T, seed):
    """T targets over nv vertices, most of them empty when T is large; the last one is used."""
    rng = np.random.default_rng(seed)
    owner = (np.arange(nv) * 7) % T
    second = (np.arange(nv) * 13 + 5) % T
    targets = []
    by_t = {}
    for vtx in range(nv):
        for t in {int(owner[vtx]), int(second[vtx])} | ({T - 1} if vtx % 50 == 0 or vtx == nv - 1 else set()):
            by_t.setdefault(t, []).append(vtx)
    for t in range(T):
        ids = np.array(by_t.get(t, []), np.int64)
        targets.append((ids, rng.normal(size=(len(ids), 3)).astype(F) * F(0.2), None))
    w = rng.uniform(-1, 1, T).astype(F)
    w[T // 3] = 0.0
    w[-1] = 0.75
    return targets, w


@pytest.mark.parametrize("group", ["1", "4"])
@pytest.mark.parametrize("T", [1, mpt.MORPH_LDS_TARGETS, mpt.MORPH_LDS_TARGETS + 1], ids=["one", "budget", "past"])
def test_target_counts_around_the_lds_budget(monkeypatch, luts, T, group):
    """One target, exactly the most weights staged in LDS and one more, which are gathered: the host
    path's bytes, and the gather's when they were staged."""
    nv = 1027
    v, idx = edge_scene(nv)
    sd = soup_scene(v, idx)
    targets, w = many_targets(nv, T, T)
    assert len(targets[-1][0]) > 0 and w[-1] != 0
    monkeypatch.delenv("MPT_MORPH_LDS", raising=False)
    monkeypatch.setenv("MPT_MORPH_GROUP", group)
    dev, host = both_paths(luts, sd, targets, w)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{T} targets")
    monkeypatch.setenv("MPT_MORPH_LDS", "0")
    gather = both_paths(luts, sd, targets, w)[0]
    assert gather[0] == dev[0]
    assert_trees_equal(gather[1], dev[1], f"{T} targets, gathered")


@pytest.mark.parametrize("group", ["1", "4"])
def test_fused_kernel_with_a_palette_past_its_budget(monkeypatch, luts, group):
    """J = SKIN_LDS_JOINTS + 1: the palette does not fit, so the fused kernel stages nothing, the
    weights neither."""
    monkeypatch.delenv("MPT_MORPH_LDS", raising=False)
    monkeypatch.setenv("MPT_MORPH_GROUP", group)
    nv, nj = 1027, mpt.SKIN_LDS_JOINTS + 1
    v, idx = edge_scene(nv)
    J, W = random_skin(nv, nj, 7)
    J[-1, 0], W[-1, 0] = nj - 1, 0.5
    targets, w = many_targets(nv, 5, 3)
    for joints, M in ((nj, random_pose(nj, nj)), (mpt.SKIN_LDS_JOINTS, random_pose(mpt.SKIN_LDS_JOINTS, 9))):
        Jk = np.minimum(J, joints - 1)
        dev, host = both_paths(luts, soup_scene(v, idx), targets, w, (Jk, W, M))
        assert dev[0] == host[0]
        assert_trees_equal(dev[1], host[1], f"fused, {joints} joints")


# ------------------------------------------------------------------------------------
# State: the rest pose, the retained weights
# ------------------------------------------------------------------------------------
def test_poses_start_from_the_rest_pose(luts):
    sd0, targets, w1, _, nv1, nn1 = case("cornell")
    _, _, w2, _, nv2, nn2 = case("cornell2")
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        b.update_vertices(nv2, nn2)
        want = trees(b)
        a.set_morph(targets)
        a.update_morph(w1)
        a.update_morph(w2)
        assert_trees_equal(trees(a), want, "the second of two poses")
        a.update_vertices(edit_jitter(sd0.vertices.astype(F)))               # leaves the rest pose as captured
        assert trees(a)[0][0].tobytes() != want[0][0].tobytes()
        a.update_morph(w2)
        assert_trees_equal(trees(a), want, "after an update_vertices in between")
        frs = frames(sd0, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        assert_same(gpu_render(a, frs)[2], gpu_render(b, frs)[2], "normals AOV: the normals come from the rest pose as well")
    finally:
        a.close()
        b.close()


def test_zero_weights_change_nothing(luts):
    sd0, targets, w, _, _, _ = case("cornell")
    frs = frames(sd0, 40, 24, 4, lss=abi.LSS_MIS_LIGHT_BSDF)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_morph(targets)
        before = trees(a)
        ga = gpu_render(a, frs[:2])
        z = np.zeros(4, F)
        z[1] = -0.0
        i = a.update_morph(z, info=True)
        assert i.area_ratio == 1.0 and i.light_area_ratio == 1.0
        assert_trees_equal(trees(a), before, "all-zero weights")
        ga = gpu_render(a, frs[2:])                                           # no reset: the accumulation continues
        gb = gpu_render(b, frs)
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(ga[k], gb[k], f"zero weights, {what}")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH], ids=["lbvh", "ploc", "sah"])
def test_rebuild_then_update_morph(luts, mode):
    sd0, targets, w1, _, nv1, nn1 = case("cornell")
    _, _, w2, _, nv2, nn2 = case("cornell2")
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_morph(targets)
        a.update_morph(w1)
        a.rebuild_bvh(mode=mode)
        ia = a.update_morph(w2, info=True)
        ta = trees(a)
        b.update_vertices(nv1, nn1)
        b.rebuild_bvh(mode=mode)
        ib = b.update_vertices(nv2, nn2, info=True)
        tb = trees(b)
    finally:
        a.close()
        b.close()
    assert_trees_equal(ta, tb, f"mode {mode}: update_morph vs update_vertices after the rebuild")
    assert info_tuple(ia) == info_tuple(ib)


def test_material_edit_after_update_morph(luts):
    from oracle import oracle as orc
    sd0, targets, w, sd, nv, nn = case("cornell")
    wall = int(sd0.material_indices[0])
    mats = [abi.Material.from_buffer_copy(m) for m in sd0.materials]
    mats[wall].emission = abi.Color(0.3, 0.2, 0.1)
    mats[wall].emission_strength = 2.0
    frs = frames(sd, 40, 24, 2, lss=abi.LSS_BSDF)
    s = copy.copy(sd)
    s.materials = mats
    o = orc.Oracle(s, luts)
    ref = o.render(frs, aov=True)
    o.close()
    r = fresh(sd0, luts)
    try:
        r.set_morph(targets)
        r.update_morph(w)
        r.update_materials(mats)
        got = gpu_render(r, frs)
    finally:
        r.close()
    for k, what in enumerate(["color", "albedo", "normals"]):
        assert_same(got[k], ref[k], f"material edit after update_morph: {what}")


def test_set_scene_drops_the_morph(luts):
    sd0, targets, w, _, _, _ = case("cornell")
    r = fresh(sd0, luts)
    try:
        r.set_morph(targets)
        r.update_morph(w)
        for build in (None, abi.BUILD_LBVH):
            r.set_scene(sd0, build=build)
            with pytest.raises(mpt.MptError) as e:
                r.update_morph(w)
            assert e.value.code == -1 and "no morph set" in str(e.value)
            r.set_morph(targets)
            r.update_morph(w)
        r.set_morph(None)
        with pytest.raises(mpt.MptError):
            r.update_morph(w)
    finally:
        r.close()


def test_morph_and_objects_exclude_each_other(luts):
    sd0, targets, w, _, nv, nn = case("cornell")
    ids, _, _ = cornell_objects()
    MO = np.stack([rigid(np.eye(3), 0, [0.3, -0.12, 0.15]), rigid(rot_y(30.0), [0, 0, 0], [0, 0.1, 0])])
    ov, on = mpt.transform_host(sd0.vertices, sd0.normals, ids, MO)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_morph(targets)
        a.set_objects(ids)                                   # drops the morph; the rest pose is the scene's
        with pytest.raises(mpt.MptError) as e:
            a.update_morph(w)
        assert e.value.code == -1 and "no morph set" in str(e.value)
        a.update_transforms(MO)
        b.update_vertices(ov, on)
        assert_trees_equal(trees(a), trees(b), "objects after a morph")
        a.set_morph(None)                                    # (not the morph's to free: the objects stay)
        a.update_transforms(MO)
        a.set_morph(targets)                                 # drops the objects; the rest pose is the moved scene
        with pytest.raises(mpt.MptError) as e:
            a.update_transforms(MO)
        assert e.value.code == -1 and "no objects set" in str(e.value)
        a.update_morph(w)
        b.update_vertices(*mpt.morph_host(ov, on, targets, w))
        assert_trees_equal(trees(a), trees(b), "a morph after objects")
        a.set_objects(None)                                  # (not the objects' to free: the morph stays)
        a.update_morph(w)
    finally:
        a.close()
        b.close()


def test_morph_and_skin_share_one_rest_pose(luts):
    sd0, targets, w, sd, nv, nn = case("cornell")
    J, W, _, _ = cornell_skin()
    M = cornell_pose(1)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        b.update_vertices(nv, nn)
        morphed = trees(b)
        b.update_vertices(*mpt.skin_host(nv, nn, J, W, M))
        both = trees(b)
        b.update_vertices(*mpt.skin_host(sd0.vertices, sd0.normals, J, W, M))
        skinned = trees(b)
        # a skin set after a morph does not capture again: the device holds a morphed pose by then
        a.set_morph(targets)
        a.update_morph(w)
        a.set_skin(J, W)
        a.update_skin(M)
        assert_trees_equal(trees(a), both, "the rest pose is still the scene's")
        # the skin removed: the rest pose stays, and the morph alone gives what it gave
        a.set_skin(None)
        with pytest.raises(mpt.MptError) as e:
            a.update_skin(M)
        assert "no skin set" in str(e.value)
        a.update_morph(w)
        assert_trees_equal(trees(a), morphed, "after set_skin(None)")
        # the two swapped
        a.set_skin(J, W)
        a.update_skin(M)
        a.set_morph(None)
        with pytest.raises(mpt.MptError) as e:
            a.update_morph(w)
        assert "no morph set" in str(e.value)
        a.update_skin(M)
        assert_trees_equal(trees(a), skinned, "after set_morph(None)")
        # a morph set after a skin does not capture again either
        a.set_morph(targets)
        a.update_morph(w)
        assert_trees_equal(trees(a), both, "a morph set after the skin")
        # both gone: the next one captures the device's pose
        a.set_morph(None)
        a.set_skin(None)
        a.set_morph(targets)
        a.update_morph(np.zeros(4, F))
        assert_trees_equal(trees(a), both, "a new capture")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# Refusals change nothing
# ------------------------------------------------------------------------------------
def test_refusals_change_nothing(luts):
    sd0, targets, w, sd, nv, nn = case("cornell")
    J, W, _, _ = cornell_skin()
    M1, M2 = cornell_pose(1), cornell_pose(2)
    frs = frames(sd, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    T, off, ids, dp, dn = mpt._morph_tables(targets, "test")
    L = mpt.lib()
    r = mpt.GPURenderer(0)
    try:
        assert L.mpt_set_morph(r.h, T, off.ctypes.data, ids.ctypes.data, dp.ctypes.data, dn.ctypes.data, len(sd0.vertices)) == -3
        assert L.mpt_update_morph(r.h, w.ctypes.data, T, None) == -3                  # MPT_ERR_NO_SCENE
        assert L.mpt_update_morph_skin(r.h, w.ctypes.data, T, M1.ctypes.data, 4, None) == -3
        r.set_scene(sd0)
        r.set_luts(luts)

        def state():
            return trees(r), gpu_render(r, frs)

        def unchanged(s0, what):
            s1 = state()
            assert_trees_equal(s0[0], s1[0], what)
            for k in range(3):
                assert_same(s0[1][k], s1[1][k], what)

        def refused(call, word, s0, what):
            with pytest.raises(mpt.MptError) as e:
                call()
            assert e.value.code == -1 and word in str(e.value), what
            unchanged(s0, what)

        s0 = state()
        refused(lambda: r.update_morph(w), "no morph set", s0, "no morph set")
        for bad in (dict(n=len(sd0.vertices) - 1), dict(T=0), dict(off=off + 1), dict(ids=np.where(ids == ids.max(), len(sd0.vertices), ids).astype(np.int32)),
                    dict(ids=ids[::-1].copy()), dict(dp=np.where(np.arange(dp.size).reshape(dp.shape) == 7, np.nan, dp).astype(F))):
            a = dict(T=T, off=off, ids=ids, dp=dp, dn=dn, n=len(sd0.vertices))
            a.update(bad)
            assert L.mpt_set_morph(r.h, a["T"], a["off"].ctypes.data, a["ids"].ctypes.data, a["dp"].ctypes.data, a["dn"].ctypes.data, a["n"]) == -1, bad
        refused(lambda: r.update_morph(w), "no morph set", s0, "still no morph")
        r.set_morph(targets)
        refused(lambda: r.update_morph_skin(w, M1), "no skin set", s0, "no skin set")
        r.set_skin(J, W, 4)
        r.update_morph_skin(w, M1)
        s0 = state()
        want = mpt.skin_host(nv, nn, J, W, M1)
        b = fresh(sd0, luts)
        try:
            b.update_vertices(*want)
            assert_trees_equal(s0[0], trees(b), "the accepted pose")
            for wbad in (np.append(W2, F(0)), W2[:3]):
                refused(lambda: r.update_morph(wbad), "count", s0, "a wrong T")
                refused(lambda: r.update_morph_skin(wbad, M2), "count", s0, "a wrong T, combined")
            refused(lambda: r.update_morph_skin(W2, M2[:3]), "count", s0, "a wrong J")
            nan = W2.copy()
            nan[1] = np.nan
            refused(lambda: r.update_morph(nan), "weight", s0, "a NaN weight")
            refused(lambda: r.update_morph_skin(nan, M2), "weight", s0, "a NaN weight, combined")
            over = np.array([0, 0, 0, 3e38], F)               # 3e38 * 4 overflows on the device
            with pytest.raises(mpt.MptError):
                mpt.morph_host(sd0.vertices, sd0.normals, targets, over)            # (the host mirror agrees)
            refused(lambda: r.update_morph(over), "vertex", s0, "an overflow on the device")
            big = M2.copy()                                                          # finite entries; the sums overflow on the device
            big[:3, :, :3], big[:3, :, 3] = np.eye(3) * 3e38, 3e38
            refused(lambda: r.update_morph_skin(W2, big), "vertex", s0, "overflowing matrices")
            # swap on acceptance: the refused call's weights and records were not kept
            r.update_morph(W2)
            b.update_vertices(*mpt.skin_host(*mpt.morph_host(sd0.vertices, sd0.normals, targets, W2), J, W, M1))
            assert_trees_equal(trees(r), trees(b), "update_morph after a refusal: the previous palette")
            refused(lambda: r.update_skin(big), "vertex", state(), "overflowing matrices, update_skin")
            r.update_skin(M2)
            b.update_vertices(*mpt.skin_host(*mpt.morph_host(sd0.vertices, sd0.normals, targets, W2), J, W, M2))
            assert_trees_equal(trees(r), trees(b), "update_skin after a refusal: the previous weights")
        finally:
            b.close()
    finally:
        r.close()
