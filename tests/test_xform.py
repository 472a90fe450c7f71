"""mpt_set_objects / mpt_update_transforms / mpt_update_vertices_device: per-object motion applied on
the GPU (csrc/xform.hip), then the refit of both BVH8s.

Bar: bit-exact.  After an update the device trees and the report equal those of a second context
that got mpt_update_vertices of mpt_transform_host's output (the host loop of csrc/xform.h), byte
for byte, and pass the refit's own checks; traversal equals a fresh upload of the moved scene;
renders equal the CPU oracle of the moved scene; the rest pose is what every update starts from;
refused calls change nothing; the kernel's lane groups, waves and blocks are exercised at their
edges.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi, scene

from test_gpu_parity import STRATEGIES, assert_same, frames, gpu_render, oracle_for, random_rays
from test_refit import fresh, in_plane_rays
from test_refit_host import check_refit, components, cornell_scene, edit_jitter, moved_part, rot_y, small_city, tiny
from test_shade_classes import _assert_modes_equal

pytestmark = pytest.mark.gpu

IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)


def rigid(R, centre, t):
    """[3, 4]: x -> R (x - centre) + centre + t."""
    R, centre, t = np.asarray(R, np.float64), np.broadcast_to(np.asarray(centre, np.float64), (3,)), np.asarray(t, np.float64)
    return np.concatenate([R, (centre - R @ centre + t)[:, None]], 1).astype(np.float32)


_cases = {}


def cornell_objects():
    """Object 0: the light's own triangles; object 1: one box with its vertex normals; the rest static."""
    sd = cornell_scene()
    idx = sd.triangle_indices.reshape(-1, 3)
    lab = components(idx, len(sd.vertices))
    light = np.isin(lab, np.unique(lab[idx[sd.emissive].ravel()]))
    box = moved_part(sd.vertices, idx) & ~light
    assert light.any() and box.any() and not (light | box).all()
    ids = np.full(len(sd.vertices), -1, np.int32)
    ids[light], ids[box] = 0, 1
    return ids, light, box


def case(name):
    """(rest scene, ids, matrices [K, 3, 4], moved scene, moved vertices, moved normals), kept for the
    module (oracle_for caches by identity).  The moved arrays are mpt.transform_host's."""
    if name in _cases:
        return _cases[name]
    if name.startswith("cornell"):
        sd0 = cornell_scene()
        ids, light, box = cornell_objects()
        v = sd0.vertices.astype(np.float64)
        M = np.zeros((2, 3, 4), np.float32)
        if name == "cornell_motion":          # as test_refit.edit_render: the light moved, a box turned and moved
            M[0] = rigid(np.eye(3), 0, [0.3, -0.12, 0.15])
        elif name == "cornell_motion2":
            M[0] = rigid(rot_y(-20.0), v[light].mean(0), [-0.2, -0.05, 0.1])
        else:                                  # cornell_light_scale: a non-uniform scale changes the light's area
            assert name == "cornell_light_scale"
            M[0] = rigid(np.diag([1.6, 1.0, 0.55]), v[light].mean(0), [0.1, -0.1, 0.0])
        M[1] = rigid(rot_y(-50.0 if name == "cornell_motion2" else 30.0), v[box].mean(0), [-0.15, 0.25, 0.1])
    else:
        assert name == "city"
        sd0 = small_city()
        idx = sd0.triangle_indices.reshape(-1, 3)
        lab = components(idx, len(sd0.vertices))
        size = np.bincount(lab)
        parts = np.flatnonzero(size <= len(lab) // 10)[::3]      # every third small part is an object
        ids = np.full(len(lab), -1, np.int32)
        remap = np.full(lab.max() + 1, -1, np.int32)
        remap[parts] = np.arange(len(parts))
        ids = remap[lab]
        assert len(parts) > 20 and (ids < 0).any()
        rng = np.random.default_rng(11)
        v = sd0.vertices.astype(np.float64)
        ext = float((v.max(0) - v.min(0)).max())
        M = np.stack([rigid(rot_y(rng.uniform(-60, 60)), v[ids == k].mean(0), rng.uniform(-0.02, 0.02, 3) * ext)
                      for k in range(len(parts))])
        M[3] = IDENT                                               # an identity object among them
    nv, nn = mpt.transform_host(sd0.vertices, sd0.normals, ids, M)
    sd = copy.copy(sd0)
    sd.vertices, sd.normals = nv, nn
    _cases[name] = (sd0, ids, M, sd, nv, nn)
    return _cases[name]


def trees(r):
    return [r.get_bvh(w) for w in (0, 1)]


def assert_trees_equal(a, b, what):
    for w in (0, 1):
        assert a[w][2] == b[w][2], f"{what}: levels of tree {w}"
        assert a[w][0].tobytes() == b[w][0].tobytes(), f"{what}: nodes of tree {w}"
        assert a[w][1].tobytes() == b[w][1].tobytes(), f"{what}: records of tree {w}"


def info_tuple(i):
    return (i.nodes, i.levels, i.light_nodes, i.light_levels, i.area_ratio, i.light_area_ratio)


# ------------------------------------------------------------------------------------
# Bytes
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_motion", "cornell_light_scale", "city"])
def test_bytes_equal_host_path(luts, name):
    sd0, ids, M, sd, nv, nn = case(name)
    idx = sd0.triangle_indices.reshape(-1, 3)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        before = trees(a)
        a.set_objects(ids)
        ia = a.update_transforms(M, info=True)
        ib = b.update_vertices(nv, nn, info=True)
        ta, tb = trees(a), trees(b)
    finally:
        a.close()
        b.close()
    # 1. against the host path, byte for byte
    assert_trees_equal(ta, tb, f"{name}: update_transforms vs update_vertices of transform_host")
    assert info_tuple(ia) == info_tuple(ib) and ia.area_ratio != 1.0
    # 2. against mpt_bvh_refit_host of those vertices, through check_refit
    hn, ht, hl = mpt.bvh_refit_host(sd0.vertices, idx, nv)
    assert ta[0][2] == hl and ta[0][0].tobytes() == hn.tobytes(), f"{name}: scene nodes vs mpt_bvh_refit_host"
    for f in ("a", "prim", "e1", "e2"):
        assert ta[0][1][f].tobytes() == ht[f].tobytes(), f"{name}: scene records {f}"
    for w in (0, 1):
        assert len(ta[w][0]) > 0
        check_refit(before[w][0], before[w][1], ta[w][0], ta[w][1], nv, idx, f"{name}: tree {w}")


def test_four_by_four_and_one_vertex_per_lane(monkeypatch, luts):
    """[K, 4, 4] matrices lose their bottom row; MPT_XFORM_GROUP=1 (one vertex per lane) gives the bytes
    of the default grouping."""
    sd0, ids, M, sd, nv, nn = case("city")
    M4 = np.zeros((len(M), 4, 4), np.float32)
    M4[:, :3], M4[:, 3, 3] = M, 1.0
    out = []
    for group, m in (("4", M4), ("1", M)):
        monkeypatch.setenv("MPT_XFORM_GROUP", group)
        r = fresh(sd0, luts)
        try:
            r.set_objects(ids, num_objects=len(M))
            out.append((info_tuple(r.update_transforms(m, info=True)), trees(r)))
        finally:
            r.close()
    assert out[0][0] == out[1][0]
    assert_trees_equal(out[0][1], out[1][1], "one vertex per lane vs four")


# ------------------------------------------------------------------------------------
# Traversal and renders
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_motion", "city"])
def test_traversal_equals_fresh_upload(luts, name):
    sd0, ids, M, sd, nv, nn = case(name)
    a, b = fresh(sd0, luts), fresh(sd, luts)
    try:
        a.set_objects(ids)
        a.update_transforms(M)
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


@pytest.mark.parametrize("name,strategy", [("cornell_motion", "mis"), ("cornell_motion", "ris"), ("cornell_light_scale", "mis")])
def test_render_after_update_transforms(monkeypatch, luts, name, strategy):
    """The light's own triangles moved (or scaled: its area changes) and a box turned with its vertex
    normals, MPT_LIGHT_BVH 0 and 1: the oracle of the moved scene."""
    sd0, ids, M, sd, nv, nn = case(name)
    frs = frames(sd, 40, 24, 3, lss=STRATEGIES[strategy])
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("MPT_LIGHT_BVH", str(mode))
        r = fresh(sd0, luts)
        try:
            r.set_objects(ids)
            r.update_transforms(M)
            out[mode] = gpu_render(r, frs)
        finally:
            r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal(out, ref, f"{name} {strategy}")
    assert out[1][0].mean() > 0
    assert not np.array_equal(ref[0], oracle_for(sd0, luts).render(frs, aov=True)[0])   # the motion shows


# ------------------------------------------------------------------------------------
# Rest-pose semantics
# ------------------------------------------------------------------------------------
def test_updates_start_from_the_rest_pose(luts):
    """Two updates in a row, then an update_vertices in between: every update_transforms gives the
    bytes of the host mirror of its own matrices alone."""
    sd0, ids, M1, _, nv1, nn1 = case("cornell_motion")
    _, _, M2, _, nv2, nn2 = case("cornell_motion2")
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        b.update_vertices(nv2, nn2)
        want = trees(b)
        a.set_objects(ids)
        a.update_transforms(M1)
        a.update_transforms(M2)
        assert_trees_equal(trees(a), want, "the second of two updates")
        a.update_vertices(edit_jitter(sd0.vertices.astype(np.float32)))      # leaves the rest pose as captured
        assert trees(a)[0][0].tobytes() != want[0][0].tobytes()
        a.update_transforms(M2)
        assert_trees_equal(trees(a), want, "after an update_vertices in between")
        frs = frames(sd0, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        assert_same(gpu_render(a, frs)[2], gpu_render(b, frs)[2], "normals AOV: the normals come from the rest pose as well")
    finally:
        a.close()
        b.close()


def test_identity_update_changes_nothing(luts):
    sd0, ids, M, _, _, _ = case("cornell_motion")
    frs = frames(sd0, 40, 24, 4, lss=abi.LSS_MIS_LIGHT_BSDF)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_objects(ids)
        ga = gpu_render(a, frs[:2])
        i = a.update_transforms(np.stack([IDENT, IDENT]), info=True)
        assert i.area_ratio == 1.0 and i.light_area_ratio == 1.0
        ga = gpu_render(a, frs[2:])                                           # no reset: the accumulation continues
        gb = gpu_render(b, frs)
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(ga[k], gb[k], f"identity update, {what}")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# Interplay
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH], ids=["lbvh", "ploc", "sah"])
def test_rebuild_then_update_transforms(luts, mode):
    """update_transforms, rebuild_bvh(mode), update_transforms: the rebuilt trees are
    mpt_bvh_build_host_mode's, and the second update refits them -- the bytes of a context that went
    the same way through update_vertices, and check_refit on the host-built trees."""
    sd0, ids, M1, _, nv1, nn1 = case("cornell_motion")
    _, _, M2, _, nv2, nn2 = case("cornell_motion2")
    idx = sd0.triangle_indices.reshape(-1, 3)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        a.set_objects(ids)
        a.update_transforms(M1)
        a.rebuild_bvh(mode=mode)
        built = trees(a)
        ia = a.update_transforms(M2, info=True)
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
        for f in ("a", "prim", "e1", "e2"):
            assert built[w][1][f].tobytes() == ht[f].tobytes()
        check_refit(hn, built[w][1], ta[w][0], ta[w][1], nv2, idx, f"mode {mode}: tree {w} refitted")
    assert_trees_equal(ta, tb, f"mode {mode}: update_transforms vs update_vertices after the rebuild")
    assert info_tuple(ia) == info_tuple(ib)


def test_material_edit_after_update_transforms(monkeypatch, luts):
    """The material paths read the host copies, which an update leaves stale: a wall turned
    emissive (the light set changes and its tree is rebuilt from downloaded positions)."""
    from oracle import oracle as orc
    sd0, ids, M, sd, nv, nn = case("cornell_motion")
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
            r.set_objects(ids)
            r.update_transforms(M)
            r.update_materials(mats)
            got = gpu_render(r, frs)
        finally:
            r.close()
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(got[k], ref[k], f"material edit after update_transforms, light BVH {mode}: {what}")


def test_set_scene_drops_the_objects(luts):
    sd0, ids, M, _, _, _ = case("cornell_motion")
    r = fresh(sd0, luts)
    try:
        r.set_objects(ids)
        r.update_transforms(M)
        for build in (None, abi.BUILD_LBVH):
            r.set_scene(sd0, build=build)
            with pytest.raises(mpt.MptError) as e:
                r.update_transforms(M)
            assert e.value.code == -1 and "no objects" in str(e.value)
            r.set_objects(ids)
            r.update_transforms(M)
        r.set_objects(None)
        with pytest.raises(mpt.MptError):
            r.update_transforms(M)
    finally:
        r.close()


# ------------------------------------------------------------------------------------
# Refusals change nothing
# ------------------------------------------------------------------------------------
def test_refusals_change_nothing(luts):
    sd0, ids, M, sd, nv, nn = case("cornell_motion")
    frs = frames(sd, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
    L = mpt.lib()
    r = mpt.GPURenderer(0)
    try:
        assert L.mpt_set_objects(r.h, ids.ctypes.data, len(ids), 2) == -3           # MPT_ERR_NO_SCENE
        assert L.mpt_update_transforms(r.h, M.ctypes.data, 2, None) == -3
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
        with pytest.raises(mpt.MptError) as e:                                       # no objects set
            r.update_transforms(M)
        assert e.value.code == -1
        unchanged(s0, "no objects set")
        bad_ids = ids.copy()
        bad_ids[7] = 2
        for args in ((ids[:-1], 2), (bad_ids, 2), (np.where(ids == 1, -2, ids), 2)):
            with pytest.raises(mpt.MptError) as e:                                   # a wrong vertex count, ids out of range
                r.set_objects(*args)
            assert e.value.code == -1
        with pytest.raises(mpt.MptError):
            r.update_transforms(M)                                                   # (still no objects)
        r.set_objects(ids, 2)
        r.update_transforms(M)
        s0 = state()
        assert_same(s0[1][0], oracle_for(sd, luts).render(frs, aov=True)[0], "the accepted update")
        M2 = case("cornell_motion2")[2]
        for what, m in (("a wrong count", np.concatenate([M2, M2[:1]])), ("a wrong count", M2[:1])):
            with pytest.raises(mpt.MptError) as e:
                r.update_transforms(m)
            assert e.value.code == -1 and "count" in str(e.value)
            unchanged(s0, what)
        nan = M2.copy()
        nan[1, 2, 0] = np.nan
        with pytest.raises(mpt.MptError) as e:
            r.update_transforms(nan)
        assert e.value.code == -1 and "matrix" in str(e.value)
        unchanged(s0, "a NaN entry")
        big = M2.copy()                                                              # finite entries; the sums overflow on the device
        big[1, :, :3], big[1, :, 3] = np.eye(3) * 3e38, 3e38
        assert np.isfinite(big).all()
        with pytest.raises(mpt.MptError):
            mpt.transform_host(sd0.vertices, sd0.normals, ids, big)                  # (the host mirror agrees that it overflows)
        with pytest.raises(mpt.MptError) as e:
            r.update_transforms(big)
        assert e.value.code == -1 and "vertex" in str(e.value)
        unchanged(s0, "an overflow on the device")
        r.update_transforms(M2)                                                      # and the context still works
        assert_same(gpu_render(r, frs)[0], oracle_for(case("cornell_motion2")[3], luts).render(frs, aov=True)[0], "after the refusals")
    finally:
        r.close()


# ------------------------------------------------------------------------------------
# Edges: a partial last lane group, a partial wave, a partial block
# ------------------------------------------------------------------------------------
def soup_scene(v, idx):
    sd0 = cornell_scene()
    sd = scene.SceneData()
    sd.vertices = v
    sd.triangle_indices = idx.ravel().astype(np.int32)
    rng = np.random.default_rng(len(v))
    n = rng.normal(size=v.shape)
    sd.normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    sd.has_normals = np.ones(len(v), np.uint8)
    sd.texcoords = np.zeros((len(v), 2), np.float32)
    sd.materials = list(sd0.materials)
    sd.material_indices = (np.arange(len(idx)) % len(sd0.materials)).astype(np.int32)
    sd.textures = list(sd0.textures)
    sd.camera_info = sd0.camera_info
    sd.name = f"soup{len(v)}"
    return sd.finalize()


def edge_scene(n_vertices):
    """tiny() triangles, with unused vertices appended up to n_vertices (3, 63, 66, 129, 1027: the
    counts are not all multiples of 3)."""
    v, idx = tiny(n_vertices // 3)
    extra = n_vertices - len(v)
    if extra:
        v = np.concatenate([v, np.random.default_rng(1).random((extra, 3)).astype(np.float32)])
    return v, idx


def both_paths(luts, sd, ids, M):
    """(info, trees) through update_transforms and through update_vertices of the host mirror;
    either may be an MptError instead."""
    out = []
    for dev in (True, False):
        r = fresh(sd, luts)
        try:
            if dev:
                r.set_objects(ids, num_objects=len(M))
                i = r.update_transforms(M, info=True)
            else:
                i = r.update_vertices(*mpt.transform_host(sd.vertices, sd.normals, ids, M), info=True)
            out.append((info_tuple(i), trees(r)))
        except mpt.MptError as e:
            out.append(e)
        finally:
            r.close()
    return out


@pytest.mark.parametrize("nv", [3, 63, 66, 129, 1027])
def test_edge_counts(luts, nv):
    v, idx = edge_scene(nv)
    assert len(v) == nv
    sd = soup_scene(v, idx)
    rng = np.random.default_rng(nv)
    ids = rng.integers(-1, 3, nv).astype(np.int32)
    ids[-1] = 2
    M = np.stack([rigid(rot_y(25.0), [0, 0, 0], [0.5, 0, 0]), IDENT, rigid(np.diag([1.5, 0.5, 2.0]) @ rot_y(-70.0), [1, 0, 0], [0, 1, 0])])
    dev, host = both_paths(luts, sd, ids, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nv} vertices")
    # the largest coordinate in the last vertex (it decides the pad): the last triangle's when the
    # count is a multiple of 3, else an unused vertex, which must not count
    v2 = v.copy()
    v2[-1] = [0.0, 900.0, 0.0]
    sd2 = soup_scene(v2, idx)
    dev, host = both_paths(luts, sd2, ids, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], f"{nv} vertices, the maximum in the last")
    # the only non-finite result in the last vertex: refused by both, used or not
    big = M.copy()
    big[2, :, :3] = np.diag([3e38, 1, 1])
    ids3 = np.where(ids == 2, 0, ids).astype(np.int32)
    ids3[-1] = 2
    v3 = v.copy()
    v3[-1] = [5.0, 1.0, 1.0]                      # 5 * 3e38 overflows
    dev, host = both_paths(luts, soup_scene(v3, idx), ids3, big)
    assert isinstance(dev, mpt.MptError) and dev.code == -1 and "finite" in str(dev)
    assert isinstance(host, mpt.MptError) and host.code == -1


def test_unused_vertex_does_not_set_the_pad(luts):
    """An appended unused vertex at 1e30 inside an object: the pad is the host path's (the maximum
    runs over the used vertices)."""
    v, idx = tiny(21)
    v = np.concatenate([v, np.array([[1e30, 0, 0]], np.float32)])
    sd = soup_scene(v, idx)
    ids = np.zeros(len(v), np.int32)
    M = rigid(rot_y(10.0), [0, 0, 0], [0, 0.5, 0])[None]
    dev, host = both_paths(luts, sd, ids, M)
    assert dev[0] == host[0]
    assert_trees_equal(dev[1], host[1], "an unused vertex at 1e30")
    nv, _ = mpt.transform_host(sd.vertices, sd.normals, ids, M)
    pad = np.float32(np.ldexp(max(np.float32(np.abs(nv[:-1]).max()), np.float32(1.0)), -20))
    rec = dev[1][0][1]
    lo = nv[idx[rec["prim"]]].min(1)
    assert ((lo - pad).astype(np.float32).min(0) == dev[1][0][0]["p"][0]).all()      # the root's origin: the pad of the used vertices


# ------------------------------------------------------------------------------------
# update_vertices with device tensors
# ------------------------------------------------------------------------------------
def test_update_vertices_device(luts):
    import torch
    sd0, ids, M, sd, nv, nn = case("cornell_motion")
    dev = torch.device("cuda", 0)
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        tv = torch.from_numpy(nv).to(dev)
        tn = torch.from_numpy(nn).to(dev)
        ia, ib = a.update_vertices(tv, info=True), b.update_vertices(nv, info=True)
        assert info_tuple(ia) == info_tuple(ib)
        assert_trees_equal(trees(a), trees(b), "positions only, from a tensor")
        nv2, nn2 = case("cornell_motion2")[4:6]
        # an odd offset into a larger tensor: not 16-byte aligned
        pool = torch.zeros(3 * len(nv2) + 1, dtype=torch.float32, device=dev)
        pool[1:] = torch.from_numpy(nv2).reshape(-1).to(dev)
        ia = a.update_vertices(pool[1:].reshape(-1, 3), torch.from_numpy(nn2).to(dev), info=True)
        ib = b.update_vertices(nv2, nn2, info=True)
        assert info_tuple(ia) == info_tuple(ib)
        ta = trees(a)
        assert_trees_equal(ta, trees(b), "positions and normals, from tensors")
        frs = frames(sd0, 40, 24, 2, lss=abi.LSS_MIS_LIGHT_BSDF)
        ra = gpu_render(a, frs)
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(ra[k], gpu_render(b, frs)[k], f"render after the device update: {what}")
        # a NaN in the tensor: refused, nothing changed
        bad = tv.clone()
        bad[len(bad) // 2, 1] = float("nan")
        with pytest.raises(mpt.MptError) as e:
            a.update_vertices(bad, tn)
        assert e.value.code == -1 and "finite" in str(e.value)
        assert_trees_equal(trees(a), ta, "after a refused device update")
        for k in range(3):
            assert_same(gpu_render(a, frs)[k], ra[k], "a frame after a refused device update")
        with pytest.raises(mpt.MptError) as e:
            a.update_vertices(tv[:-1])
        assert e.value.code == -1
        # a mix of host and device arrays
        with pytest.raises(TypeError):
            a.update_vertices(tv, nn)
        with pytest.raises(TypeError):
            a.update_vertices(nv, tn)
        # a CPU tensor takes the host path
        a.update_vertices(torch.from_numpy(nv), torch.from_numpy(nn))
        b.update_vertices(nv, nn)
        assert_trees_equal(trees(a), trees(b), "a CPU tensor")
        # a host pointer handed to the device entry point is refused before any kernel reads it
        assert mpt.lib().mpt_update_vertices_device(a.h, nv.ctypes.data, None, len(nv), None) == -1
    finally:
        a.close()
        b.close()
