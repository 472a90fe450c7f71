"""mpt_set_skin / mpt_update_skin: linear-blend skinning applied on the GPU (csrc/skin.hip), then the
refit of both BVH8s.

Bar: bit-exact.  After an update the device trees and the report equal those of a second context
that got mpt_update_vertices of mpt_skin_host's output (the host loop of csrc/skin.h), byte for
byte, and pass the refit's own checks; traversal equals a fresh upload of the skinned scene; renders
equal the CPU oracle of the skinned scene; every pose starts from the rest pose; a skin and an
object table exclude each other; refused calls change nothing; the kernel's lane groups, waves and
blocks are exercised at their edges and its variants (one vertex per lane, the palette in LDS or
gathered through the cache, palettes at and past the LDS budget) give the same bytes.

Every array of the context is the library's own allocation, so no call can hand the kernel a
misaligned array: the one-vertex-per-lane kernel is reached through MPT_SKIN_GROUP=1.
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
from test_xform import IDENT, assert_trees_equal, cornell_objects, edge_scene, info_tuple, rigid, soup_scene, trees

pytestmark = pytest.mark.gpu

_cases = {}


def cornell_skin():
    """One box on a chain of three joints, weights blended by height (a zero-weight slot on the
    light's joint as well); the light's own triangles on a fourth joint; the rest unskinned."""
    sd = cornell_scene()
    _, light, box = cornell_objects()
    v = sd.vertices.astype(np.float64)
    J = np.zeros((len(v), 4), np.int32)
    W = np.zeros((len(v), 4), np.float32)
    y = v[box, 1]
    s = 2.0 * (y - y.min()) / (y.max() - y.min())
    a = np.minimum(np.floor(s), 1.0)
    J[box] = np.stack([a, a + 1, np.full(len(a), 3), np.zeros(len(a))], 1).astype(np.int32)
    W[box, 1] = (s - a).astype(np.float32)
    W[box, 0] = np.float32(1.0) - W[box, 1]
    J[light, 0], W[light, 0] = 3, 1.0
    return J, W, light, box


def cornell_pose(k):
    sd = cornell_scene()
    _, _, light, box = cornell_skin()
    c = sd.vertices[box].astype(np.float64).mean(0)
    if k == 1:
        return np.stack([rigid(np.eye(3), 0, [0.02, 0.0, -0.03]), rigid(rot_y(20.0), c, [0.0, 0.05, 0.0]),
                         rigid(rot_y(45.0) @ np.diag([1.0, 1.2, 1.0]), c, [-0.1, 0.1, 0.05]),
                         rigid(np.eye(3), 0, [0.3, -0.12, 0.15])])
    lc = sd.vertices[light].astype(np.float64).mean(0)
    return np.stack([IDENT, rigid(rot_y(-30.0), c, [0.05, 0.0, 0.0]), rigid(rot_y(-60.0), c, [0.1, 0.15, 0.0]),
                     rigid(rot_y(-20.0), lc, [-0.2, -0.05, 0.1])])


def case(name):
    """(rest scene, joints, weights, matrices [J, 3, 4], skinned scene, skinned vertices, skinned
    normals), kept for the module.  The skinned arrays are mpt.skin_host's."""
    if name in _cases:
        return _cases[name]
    if name.startswith("cornell"):
        sd0 = cornell_scene()
        J, W, _, _ = cornell_skin()
        M = cornell_pose(1 if name == "cornell_pose" else 2)
    else:
        assert name == "city"
        sd0 = small_city()
        v = sd0.vertices.astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        g = np.stack(np.meshgrid(np.linspace(lo[0], hi[0], 8), np.linspace(lo[2], hi[2], 5), indexing="ij"), -1).reshape(-1, 2)
        centres = np.stack([g[:, 0], np.full(len(g), (lo[1] + hi[1]) / 2), g[:, 1]], 1)            # 40 joints
        d = np.linalg.norm(v[:, None, [0, 2]] - g[None], axis=2)
        J = np.argsort(d, axis=1)[:, :4].astype(np.int32)
        w = 1.0 / (np.take_along_axis(d, J.astype(np.int64), 1) + 0.05 * float((hi - lo).max()))
        W = (w / w.sum(1, keepdims=True)).astype(np.float32)
        W[::11] = 0.0                                                                           # unskinned vertices among them
        rng = np.random.default_rng(17)
        ext = float((hi - lo).max())
        M = np.stack([rigid(rot_y(rng.uniform(-25, 25)) @ np.diag(rng.uniform(0.8, 1.25, 3)), centres[k], rng.uniform(-0.02, 0.02, 3) * ext)
                      for k in range(len(centres))])
        M[5] = IDENT
    nv, nn = mpt.skin_host(sd0.vertices, sd0.normals, J, W, M)
    sd = copy.copy(sd0)
    sd.vertices, sd.normals = nv, nn
    _cases[name] = (sd0, J, W, M, sd, nv, nn)
    return _cases[name]


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_pose", "city"])
def test_bytes_equal_host_path(luts, name):
    sd0, J, W, M, sd, nv, nn = case(name)
    idx = sd0.triangle_indices.reshape(-1, 3)
    assert len(M) == (4 if name == "cornell_pose" else 40) and not np.array_equal(nv, sd0.vertices)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        before = trees(a)
        a.set_skin(J, W)
        ia = a.update_skin(M, info=True)
        ib = b.update_vertices(nv, nn, info=True)
        ta, tb = trees(a), trees(b)
    finally:
        a.close()
        b.close()
    assert_trees_equal(ta, tb, f"{name}: update_skin vs update_vertices of skin_host")
    assert info_tuple(ia) == info_tuple(ib) and ia.area_ratio != 1.0
    hn, ht, hl = mpt.bvh_refit_host(sd0.vertices, idx, nv)
    assert ta[0][2] == hl and ta[0][0].tobytes() == hn.tobytes(), f"{name}: scene nodes vs mpt_bvh_refit_host"
    for f in ("a", "prim", "e1", "e2"):
        assert ta[0][1][f].tobytes() == ht[f].tobytes(), f"{name}: scene records {f}"
    for w in (0, 1):
        assert len(ta[w][0]) > 0
        check_refit(before[w][0], before[w][1], ta[w][0], ta[w][1], nv, idx, f"{name}: tree {w}")


# ------------------------------------------------------------------------------------
# Traversal and renders
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_pose", "city"])
def test_traversal_equals_fresh_upload(luts, name):
    sd0, J, W, M, sd, nv, nn = case(name)
    a, b = fresh(sd0, luts), fresh(sd, luts)
    try:
        a.set_skin(J, W)
        a.update_skin(M)
        graze, glh = in_plane_rays(sd, 20000, 21)
        for what, rays, lh in (("random", random_rays(sd, 20000, 5), None), ("grazing", graze, glh)):
            ga, gb = a.trace_closest(rays, lh), b.trace_closest(rays, lh)
            assert_same(ga[0], gb[0], f"{name} {what} prim")
            hit = gb[0] >= 0
            assert hit.mean() > 0.01
            for k, q in enumerate("tuv"):
                assert_same(ga[k + 1][hit], gb[k + 1][hit], f"{name} {what} {q}")
            r3 = rays.copy()
            rng = np.random.default_rng(2)
            r3[:, 7] = np.where(hit, gb[1] * rng.choice(np.array([0.5, 1.0, 1.5], np.float32), len(rays)), rays[:, 7])
            assert_same(a.trace_any(r3, lh), b.trace_any(r3, lh), f"{name} {what} occluded")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("strategy", ["mis", "ris"])
def test_render_after_update_skin(monkeypatch, luts, strategy):
    """The light's own triangles moved on their joint and a box bent with its vertex normals,
    MPT_LIGHT_BVH 0 and 1: the oracle of the skinned scene."""
    sd0, J, W, M, sd, nv, nn = case("cornell_pose")
    frs = frames(sd, 40, 24, 3, lss=STRATEGIES[strategy])
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.set_skin(J, W)
            r.update_skin(M)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal(out, ref, f"cornell_pose {strategy}")
    assert out[1][0].mean() > 0
    assert not np.array_equal(ref[0], oracle_for(sd0, luts).render(frs, aov=True)[0])   # the pose shows


# ------------------------------------------------------------------------------------
# Edges: a partial last lane group, a partial wave, a partial block
# ------------------------------------------------------------------------------------
def both_paths(luts, sd, J, W, M):
    """(info, trees) through update_skin and through update_vertices of the host mirror; either may
    be an MptError instead."""
    out = []
    for dev in (True, False):
        r = fresh(sd, luts)
        try:
            if dev:
                r.set_skin(J, W, num_joints=len(M))
                i = r.update_skin(M, info=True)
            else:
                i = r.update_vertices(*mpt.skin_host(sd.vertices, sd.normals, J, W, M), info=True)
            out.append((info_tuple(i), trees(r)))
        except mpt.MptError as e:
            out.append(e)
        finally:
            r.close()
    return out


def random_skin(nv, nj, seed):
    rng = np.random.default_rng(seed)
    J = rng.integers(0, nj, (nv, 4)).astype(np.int32)
    W = rng.random((nv, 4)).astype(np.float32)
    W[rng.random((nv, 4)) < 0.3] = 0.0
    W /= np.maximum(W.sum(1, keepdims=True), np.float32(1e-3))
    W[::5] = 0.0
    return J, W


def random_pose(nj, seed):
    rng = np.random.default_rng(seed)
    M = np.stack([rigid(rot_y(rng.uniform(-40, 40)) @ np.diag(rng.uniform(0.6, 1.6, 3)), rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5, 3))
                  for _ in range(nj)])
    M[nj // 2] = IDENT
    return M


@pytest.mark.parametrize("nv", [3, 63, 66, 129, 1027])
def test_edge_counts(luts, nv):
    v, idx = edge_scene(nv)
    assert len(v) == nv
    sd = soup_scene(v, idx)
    J, W = random_skin(nv, 3, nv)
    J[-1], W[-1] = [2, 0, 1, 2], [0.5, 0.25, 0.0, 0.25]
    M = np.stack([rigid(rot_y(25.0), [0, 0, 0], [0.5, 0, 0]), IDENT, rigid(np.diag([1.5, 0.5, 2.0]) @ rot_y(-70.0), [1, 0, 0], [0, 1, 0])])
    dev, host = both_paths(luts, sd, J, W, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nv} vertices")
    # the largest coordinate in the last vertex (it decides the pad): the last triangle's when the
    # count is a multiple of 3, else an unused vertex, which must not count
    v2 = v.copy()
    v2[-1] = [0.0, 900.0, 0.0]
    dev, host = both_paths(luts, soup_scene(v2, idx), J, W, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nv} vertices, the maximum in the last")
    # the only non-finite result in the last vertex: refused by both, used or not
    big = M.copy()
    big[2, :, :3] = np.diag([3e38, 1, 1])
    J3 = np.where(J == 2, 0, J).astype(np.int32)
    J3[-1], W3 = [2, 2, 2, 2], W.copy()
    W3[-1] = [1.0, 0.0, 0.0, 0.0]
    v3 = v.copy()
    v3[-1] = [5.0, 1.0, 1.0]                      # 5 * 3e38 overflows
    dev, host = both_paths(luts, soup_scene(v3, idx), J3, W3, big)
    assert isinstance(dev, mpt.MptError) and dev.code == -1 and "finite" in str(dev)
    assert isinstance(host, mpt.MptError) and host.code == -1


def test_unused_vertex_does_not_set_the_pad(luts):
    """An appended unused vertex at 1e30 on a joint: the pad is the host path's (the maximum runs
    over the used vertices)."""
    from test_refit_host import tiny
    v, idx = tiny(21)
    v = np.concatenate([v, np.array([[1e30, 0, 0]], np.float32)])
    sd = soup_scene(v, idx)
    J = np.zeros((len(v), 4), np.int32)
    W = np.tile(np.array([1, 0, 0, 0], np.float32), (len(v), 1))
    M = rigid(rot_y(10.0), [0, 0, 0], [0, 0.5, 0])[None]
    dev, host = both_paths(luts, sd, J, W, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], "an unused vertex at 1e30")
    nv, _ = mpt.skin_host(sd.vertices, sd.normals, J, W, M)
    pad = np.float32(np.ldexp(max(np.float32(np.abs(nv[:-1]).max()), np.float32(1.0)), -20))
    rec = dev[1][0][1]
    lo = nv[idx[rec["prim"]]].min(1)
    assert ((lo - pad).astype(np.float32).min(0) == dev[1][0][0]["p"][0]).all()


# ------------------------------------------------------------------------------------
# The kernel's variants give the same bytes
# ------------------------------------------------------------------------------------
def test_one_vertex_per_lane_and_gather_give_the_same_bytes(monkeypatch, luts):
    """MPT_SKIN_GROUP=1 (one vertex per lane) and MPT_SKIN_LDS=0 (the palette gathered through the
    cache), alone and together, against the defaults; [J, 4, 4] matrices lose their bottom row."""
    sd0, J, W, M, sd, nv, nn = case("city")
    M4 = np.zeros((len(M), 4, 4), np.float32)
    M4[:, :3], M4[:, 3, 3] = M, 1.0
    out = []
    for group, lds, m in ((None, None, M), ("1", None, M4), (None, "0", M), ("1", "0", M)):
        for var, val in (("MPT_SKIN_GROUP", group), ("MPT_SKIN_LDS", lds)):
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)
        r = fresh(sd0, luts)
        try:
            r.set_skin(J, W, num_joints=len(M))
            out.append((info_tuple(r.update_skin(m, info=True)), trees(r)))
        finally:
            r.close()
    for k in range(1, 4):
        assert out[0][0] == out[k][0]
        assert_trees_equal(out[0][1], out[k][1], f"kernel variant {k} vs the default")


@pytest.mark.parametrize("nj", [1, mpt.SKIN_LDS_JOINTS, mpt.SKIN_LDS_JOINTS + 1], ids=["one", "budget", "past"])
def test_palette_sizes_around_the_lds_budget(monkeypatch, luts, nj):
    """One joint, exactly the largest palette staged in LDS (mpt.SKIN_LDS_JOINTS, the library's
    MPT_SKIN_LDS_JOINTS) and one joint more, which is gathered: the host path's bytes, and the
    gather's when the palette was staged."""
    nv = 1027
    v, idx = edge_scene(nv)
    sd = soup_scene(v, idx)
    J, W = random_skin(nv, nj, 100 + nj)
    J[-1, 0], W[-1, 0] = nj - 1, 0.5              # the last joint is used
    M = random_pose(nj, nj)
    if nj == 1:
        M[0] = rigid(rot_y(33.0), [0.2, 0, 0], [0, 0.1, 0])
    monkeypatch.delenv("MPT_SKIN_LDS", raising=False)
    monkeypatch.delenv("MPT_SKIN_GROUP", raising=False)
    dev, host = both_paths(luts, sd, J, W, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nj} joints")
    monkeypatch.setenv("MPT_SKIN_LDS", "0")
    gather = both_paths(luts, sd, J, W, M)[0]
    assert gather[0] == dev[0]
    assert_trees_equal(gather[1], dev[1], f"{nj} joints, gathered")


# ------------------------------------------------------------------------------------
# Rest-pose semantics
# ------------------------------------------------------------------------------------
def test_poses_start_from_the_rest_pose(luts):
    sd0, J, W, M1, _, nv1, nn1 = case("cornell_pose")
    _, _, _, M2, _, nv2, nn2 = case("cornell_pose2")
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        b.update_vertices(nv2, nn2)
        want = trees(b)
        a.set_skin(J, W)
        a.update_skin(M1)
        a.update_skin(M2)
        assert_trees_equal(trees(a), want, "the second of two poses")
        a.update_vertices(edit_jitter(sd0.vertices.astype(np.float32)))      # leaves the rest pose as captured
        assert trees(a)[0][0].tobytes() != want[0][0].tobytes()
        a.update_skin(M2)
        assert_trees_equal(trees(a), want, "after an update_vertices in between")
        frs = frames(sd0, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        assert_same(gpu_render(a, frs)[2], gpu_render(b, frs)[2], "normals AOV: the normals come from the rest pose as well")
    finally:
        a.close()
        b.close()


def test_identity_pose_changes_nothing(luts):
    """Weights that do not sum to 1 under an all-identity pose: no byte changes, the ratio is 1."""
    sd0, J, W, M, _, _, _ = case("cornell_pose")
    W2 = (W * np.float32(0.7)).astype(np.float32)
    frs = frames(sd0, 40, 24, 4, lss=abi.LSS_MIS_LIGHT_BSDF)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_skin(J, W2)
        before = trees(a)
        ga = gpu_render(a, frs[:2])
        i = a.update_skin(np.stack([IDENT] * 4), info=True)
        assert i.area_ratio == 1.0 and i.light_area_ratio == 1.0
        assert_trees_equal(trees(a), before, "an identity pose")
        ga = gpu_render(a, frs[2:])                                           # no reset: the accumulation continues
        gb = gpu_render(b, frs)
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(ga[k], gb[k], f"identity pose, {what}")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# Interplay
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH], ids=["lbvh", "ploc", "sah"])
def test_rebuild_then_update_skin(luts, mode):
    sd0, J, W, M1, _, nv1, nn1 = case("cornell_pose")
    _, _, _, M2, _, nv2, nn2 = case("cornell_pose2")
    idx = sd0.triangle_indices.reshape(-1, 3)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_skin(J, W)
        a.update_skin(M1)
        a.rebuild_bvh(mode=mode)
        built = trees(a)
        ia = a.update_skin(M2, info=True)
        ta = trees(a)
        b.update_vertices(nv1, nn1)
        b.rebuild_bvh(mode=mode)
        ib = b.update_vertices(nv2, nn2, info=True)
        tb = trees(b)
    finally:
        a.close()
        b.close()
    light_prims = np.sort(built[1][1]["prim"]).astype(np.int32)
    for w, prims in ((0, None), (1, light_prims)):
        hn, ht, hl = mpt.bvh_build_host(nv1, idx, prims, mode=mode)
        assert built[w][2] == hl and built[w][0].tobytes() == hn.tobytes(), f"tree {w} after the rebuild vs the host build"
        check_refit(hn, built[w][1], ta[w][0], ta[w][1], nv2, idx, f"mode {mode}: tree {w} refitted")
    assert_trees_equal(ta, tb, f"mode {mode}: update_skin vs update_vertices after the rebuild")
    assert info_tuple(ia) == info_tuple(ib)


def test_material_edit_after_update_skin(monkeypatch, luts):
    from oracle import oracle as orc
    sd0, J, W, M, sd, nv, nn = case("cornell_pose")
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
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.set_skin(J, W)
            r.update_skin(M)
            r.update_materials(mats)
            got = gpu_render(r, frs)
        finally:
            r.close()
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(got[k], ref[k], f"material edit after update_skin, light BVH {mode}: {what}")


def test_set_scene_drops_the_skin(luts):
    sd0, J, W, M, _, _, _ = case("cornell_pose")
    r = fresh(sd0, luts)
    try:
        r.set_skin(J, W)
        r.update_skin(M)
        for build in (None, abi.BUILD_LBVH):
            r.set_scene(sd0, build=build)
            with pytest.raises(mpt.MptError) as e:
                r.update_skin(M)
            assert e.value.code == -1 and "no skin set" in str(e.value)
            r.set_skin(J, W)
            r.update_skin(M)
        r.set_skin(None)
        with pytest.raises(mpt.MptError):
            r.update_skin(M)
    finally:
        r.close()


def test_skin_and_objects_exclude_each_other(luts):
    """A rigid object is a one-joint skin: the two tables share the rest pose, and setting one drops
    the other."""
    sd0, J, W, M, _, nv, nn = case("cornell_pose")
    ids, _, _ = cornell_objects()
    MO = np.stack([rigid(np.eye(3), 0, [0.3, -0.12, 0.15]), rigid(rot_y(30.0), [0, 0, 0], [0, 0.1, 0])])
    ov, on = mpt.transform_host(sd0.vertices, sd0.normals, ids, MO)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_skin(J, W)
        a.set_objects(ids)                                   # drops the skin; the rest pose is the scene's
        with pytest.raises(mpt.MptError) as e:
            a.update_skin(M)
        assert e.value.code == -1 and "no skin set" in str(e.value)
        a.update_transforms(MO)
        b.update_vertices(ov, on)
        assert_trees_equal(trees(a), trees(b), "objects after a skin")
        a.set_skin(None)                                     # (not the skin's to free: the objects stay)
        a.update_transforms(MO)
        a.set_skin(J, W)                                     # drops the objects; the rest pose is the moved scene
        with pytest.raises(mpt.MptError) as e:
            a.update_transforms(MO)
        assert e.value.code == -1 and "no objects set" in str(e.value)
        a.update_skin(M)
        b.update_vertices(*mpt.skin_host(ov, on, J, W, M))
        assert_trees_equal(trees(a), trees(b), "a skin after objects")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# Refusals change nothing
# ------------------------------------------------------------------------------------
def test_refusals_change_nothing(luts):
    sd0, J, W, M, sd, nv, nn = case("cornell_pose")
    frs = frames(sd, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    L = mpt.lib()
    r = mpt.GPURenderer(0)
    try:
        assert L.mpt_set_skin(r.h, J.ctypes.data, W.ctypes.data, len(J), 4) == -3           # MPT_ERR_NO_SCENE
        assert L.mpt_update_skin(r.h, M.ctypes.data, 4, None) == -3
        r.set_scene(sd0)
        r.set_luts(luts)

        def state():
            return trees(r), gpu_render(r, frs)

        def unchanged(s0, what):
            s1 = state()
            assert_trees_equal(s0[0], s1[0], what)
            for k in range(3):
                assert_same(s0[1][k], s1[1][k], what)

        s0 = state()
        with pytest.raises(mpt.MptError) as e:
            r.update_skin(M)
        assert e.value.code == -1 and "no skin set" in str(e.value)
        unchanged(s0, "no skin set")
        static = np.flatnonzero(~W.any(1))[0]
        bad_j, neg_j, bad_w = J.copy(), J.copy(), W.copy()
        bad_j[static, 2] = 4                                                         # in a zero-weight slot
        neg_j[static, 0] = -1
        bad_w[3, 1] = np.inf
        for args in ((J[:-1], W[:-1], 4), (bad_j, W, 4), (neg_j, W, 4), (J, bad_w, 4), (J, W, 0), (J, W, 3)):
            with pytest.raises(mpt.MptError) as e:
                r.set_skin(*args)
            assert e.value.code == -1
        with pytest.raises(mpt.MptError):
            r.update_skin(M)                                                         # (still no skin)
        r.set_skin(J, W, 4)
        r.update_skin(M)
        s0 = state()
        assert_same(s0[1][0], oracle_for(sd, luts).render(frs, aov=True)[0], "the accepted pose")
        M2 = case("cornell_pose2")[3]
        for m in (np.concatenate([M2, M2[:1]]), M2[:3]):
            with pytest.raises(mpt.MptError) as e:
                r.update_skin(m)
            assert e.value.code == -1 and "count" in str(e.value)
            unchanged(s0, "a wrong count")
        nan = M2.copy()
        nan[1, 2, 0] = np.nan
        with pytest.raises(mpt.MptError) as e:
            r.update_skin(nan)
        assert e.value.code == -1 and "matrix" in str(e.value)
        unchanged(s0, "a NaN entry")
        big = M2.copy()                                                              # finite entries; the sums overflow on the device
        big[:3, :, :3], big[:3, :, 3] = np.eye(3) * 3e38, 3e38                        # the whole chain: the box's weights sum to 1
        assert np.isfinite(big).all()
        with pytest.raises(mpt.MptError):
            mpt.skin_host(sd0.vertices, sd0.normals, J, W, big)                      # (the host mirror agrees that it overflows)
        with pytest.raises(mpt.MptError) as e:
            r.update_skin(big)
        assert e.value.code == -1 and "vertex" in str(e.value)
        unchanged(s0, "an overflow on the device")
        r.update_skin(M2)                                                            # and the context still works
        assert_same(gpu_render(r, frs)[0], oracle_for(case("cornell_pose2")[4], luts).render(frs, aov=True)[0], "after the refusals")
    finally:
        r.close()
