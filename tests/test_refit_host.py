"""The BVH8 refit on the host (mpt_bvh_refit_host: the builder, then the host loop of
csrc/refit.h -- the arithmetic the kernels of mpt_update_vertices share), no GPU.

Checked in numpy on the returned bytes, for every scene and vertex edit below: the tree keeps
its topology and record order; every record holds the fp32 A / B - A / C - A of the new vertices
and its w lanes; every de-quantised slot box contains what it must (a leaf slot its triangles'
padded boxes, an internal slot every slot box of the child node); every bound is within one
quantisation step of the exact box and the exponents are the smallest that fit (a refit does not
quietly widen boxes).  Comparisons are made in float64: an exactly conservative bound stays
conservative under its rounding (a representable value never crosses a rounded one).

The entry point is stateless (it builds, then refits once), so "two refits in a row" cannot be
expressed through it; tests/test_refit.py chains two updates on a context, through the kernels
and through the host loop.
"""
import numpy as np
import pytest

import mpt
from mpt import scene


# ------------------------------------------------------------------------------------
# Scenes and vertex edits (shared with tests/test_refit.py)
# ------------------------------------------------------------------------------------
_scenes = {}


def small_city():
    if "city" not in _scenes:
        from mpt import synthetic
        _scenes["city"] = synthetic.procedural_city(1234, blocks=2, leaf_cards=2)
    return _scenes["city"]


def cornell_scene():
    if "cornell" not in _scenes:
        _scenes["cornell"] = scene.load_scene("cornell_pbr")
    return _scenes["cornell"]


def tiny(n_tris):
    """n_tris separate triangles: the root is one leaf, the tree one level."""
    rng = np.random.default_rng(n_tris)
    v = rng.random((3 * n_tris, 3)).astype(np.float32) * 4 - 2
    return v, np.arange(3 * n_tris, dtype=np.int32).reshape(-1, 3)


def components(indices, nv):
    """Connected-component label of every vertex."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    I = np.asarray(indices).reshape(-1, 3)
    a = np.concatenate([I[:, 0], I[:, 1]])
    b = np.concatenate([I[:, 1], I[:, 2]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(nv, nv))
    return connected_components(g, directed=False)[1]


def extent(v):
    return float((v.max(0) - v.min(0)).max())


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def edit_jitter(v, indices=None, seed=3):
    rng = np.random.default_rng(seed)
    return (v + (2 * rng.random(v.shape) - 1) * 0.01 * extent(v)).astype(np.float32)


def moved_part(v, indices):
    """The vertices of one connected part: the one of the most vertices that is at most a tenth
    of the scene (an object, not the room or the ground)."""
    lab = components(indices, len(v))
    size = np.bincount(lab)
    ok = np.flatnonzero(size <= max(3, len(v) // 10))
    part = ok[np.argmax(size[ok])] if len(ok) else int(np.argmin(size))
    return lab == part


def edit_move(v, indices, deg=30.0):
    """One connected part turned about its centroid and moved far across the scene: the tree
    built around its old place is left badly stale."""
    sel = moved_part(v, indices)
    out = v.astype(np.float64).copy()
    c = out[sel].mean(0)
    out[sel] = (out[sel] - c) @ rot_y(deg).T + c + np.array([0.8, 0.35, -0.6]) * extent(v)
    return out.astype(np.float32)


def edit_plane(v, indices=None):
    out = v.copy()
    out[:, 1] = np.float32(0.25)
    return out


EDITS = {
    "identity": lambda v, i: v.copy(),
    "jitter": edit_jitter,
    "move": edit_move,
    "scale_up": lambda v, i: (v * np.float32(1000.0)).astype(np.float32),
    "scale_down": lambda v, i: (v * np.float32(0.001)).astype(np.float32),
    "plane": edit_plane,
}


# ------------------------------------------------------------------------------------
# The checks
# ------------------------------------------------------------------------------------
def box_pad(v, indices):
    used = v[np.unique(indices)]
    return np.float32(np.ldexp(max(np.float32(np.abs(used).max()), np.float32(1.0)), -20))


def level_ranges(nodes):
    """[begin, end) of each breadth-first level: a level's internal slots are the next level."""
    out, begin, end = [], 0, 1
    while begin < end:
        out.append((begin, end))
        n_int = int(np.unpackbits(nodes["imask"][begin:end]).sum())
        begin, end = end, end + n_int
    assert end == len(nodes)
    return out


def slot_kinds(nodes):
    internal = ((nodes["imask"][:, None] >> np.arange(8)) & 1).astype(bool)
    leaf = ~internal & (nodes["meta"] != 0)
    return internal, leaf


def exact_boxes(nodes, tris, v, indices):
    """Padded triangle boxes per record, exact slot boxes [N, 8, 3] and node boxes [N, 3], fp32."""
    I = np.asarray(indices).reshape(-1, 3)
    P = v[I[tris["prim"]]]                                   # [R, 3 vertices, 3]
    pad = box_pad(v, indices)
    tlo, thi = (P.min(1) - pad).astype(np.float32), (P.max(1) + pad).astype(np.float32)
    internal, leaf = slot_kinds(nodes)
    N = len(nodes)
    slo = np.full((N, 8, 3), np.inf, np.float32)
    shi = np.full((N, 8, 3), -np.inf, np.float32)
    cnt, off = nodes["meta"] >> 5, nodes["meta"] & 31
    for k in range(int(cnt[leaf].max()) if leaf.any() else 0):
        m = leaf & (cnt > k)
        rec = (nodes["tri_base"][:, None] + off + k)[m]
        slo[m] = np.minimum(slo[m], tlo[rec])
        shi[m] = np.maximum(shi[m], thi[rec])
    nlo, nhi = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    for begin, end in reversed(level_ranges(nodes)):
        s = slice(begin, end)
        m = internal[s]
        child = (nodes["child_base"][s, None] + nodes["meta"][s])[m]
        slo[s][m] = nlo[child]
        shi[s][m] = nhi[child]
        nlo[s], nhi[s] = slo[s].min(1), shi[s].max(1)
    return tlo, thi, slo, shi, nlo, nhi


def dequantised(nodes):
    """Slot boxes [N, 8, 3] as the kernels decode them, in float64."""
    sc = np.ldexp(1.0, nodes["e"].astype(np.int64) - 127)    # [N, 3]
    p = nodes["p"].astype(np.float64)
    lo = p[:, None, :] + nodes["qlo"].transpose(0, 2, 1) * sc[:, None, :]
    hi = p[:, None, :] + nodes["qhi"].transpose(0, 2, 1) * sc[:, None, :]
    return lo, hi, sc


def check_refit(nodes0, tris0, nodes, tris, v, indices, what):
    I = np.asarray(indices).reshape(-1, 3)
    for f in ("imask", "meta", "child_base", "tri_base"):
        assert np.array_equal(nodes[f], nodes0[f]), f"{what}: {f} changed"
    for f in ("prim", "alpha_flag", "mat_class"):
        assert np.array_equal(tris[f], tris0[f]), f"{what}: record lane {f} changed"
    A, B, C = (v[I[tris["prim"], k]] for k in range(3))
    assert np.array_equal(tris["a"], A), f"{what}: A"
    assert np.array_equal(tris["e1"], B - A), f"{what}: e1"
    assert np.array_equal(tris["e2"], C - A), f"{what}: e2"

    tlo, thi, slo, shi, nlo, nhi = exact_boxes(nodes, tris, v, indices)
    internal, leaf = slot_kinds(nodes)
    used = internal | leaf
    dlo, dhi, sc = dequantised(nodes)
    # empty slots keep their (zero) bytes
    assert not nodes["qlo"].transpose(0, 2, 1)[~used].any() and not nodes["qhi"].transpose(0, 2, 1)[~used].any(), what
    # the origin is the exact node box's lo; the exponents are the smallest that fit
    assert np.array_equal(nodes["p"], nlo), f"{what}: node origin"
    ext = nhi.astype(np.float64) - nlo.astype(np.float64)
    e = nodes["e"].astype(np.int64) - 127
    assert (e >= -126).all() and (e <= 127).all(), what
    assert (255.0 * sc >= ext).all(), f"{what}: an exponent too small for its node box"
    assert ((e == -126) | (255.0 * sc / 2 <= ext)).all(), f"{what}: an exponent larger than needed"
    # containment of the exact slot boxes (leaf: its triangles' padded boxes; internal: the child's exact box)
    assert (dlo[used] <= slo[used]).all() and (dhi[used] >= shi[used]).all(), f"{what}: a slot box misses its content"
    # tightness: within one quantisation step
    step = np.broadcast_to(sc[:, None, :], dlo.shape)
    assert (slo[used] - dlo[used] <= step[used]).all(), f"{what}: a low bound more than a step below"
    assert (dhi[used] - shi[used] <= step[used]).all(), f"{what}: a high bound more than a step above"
    # an internal slot's de-quantised box contains every (exact) slot box of the child node.  (The
    # child's own de-quantised boxes sit on the child's grid and may reach past the parent's by
    # less than a child step, in the builder's trees as well: traversal only needs the content.)
    pn, ps = np.nonzero(internal)
    child = nodes["child_base"][pn] + nodes["meta"][pn, ps]
    clo = np.where(used[child][:, :, None], slo[child], np.inf).min(1)
    chi = np.where(used[child][:, :, None], shi[child], -np.inf).max(1)
    assert (dlo[pn, ps] <= clo).all() and (dhi[pn, ps] >= chi).all(), f"{what}: a child's slot box leaves its parent's"
    return nlo, nhi


CASES = {"cornell": lambda: (cornell_scene().vertices.astype(np.float32), cornell_scene().triangle_indices.reshape(-1, 3)),
         "city": lambda: (small_city().vertices.astype(np.float32), small_city().triangle_indices.reshape(-1, 3)),
         "tri1": lambda: tiny(1), "tri3": lambda: tiny(3)}
_built = {}


def built(name):
    if name not in _built:
        v, idx = CASES[name]()
        _built[name] = (v, idx) + mpt.bvh_refit_host(v, idx)
    return _built[name]


def test_scene_sizes():
    assert cornell_scene().num_triangles == 8096
    c = small_city()
    assert c.num_triangles == 44962 and len(c.vertices) == 86100
    for name, n in (("tri1", 1), ("tri3", 3)):
        v, idx, nodes, tris, levels = built(name)
        assert len(nodes) == 1 and len(tris) == n and levels == 1 and nodes["imask"][0] == 0


@pytest.mark.parametrize("edit", list(EDITS))
@pytest.mark.parametrize("name", list(CASES))
def test_refit_host(name, edit):
    v, idx, nodes0, tris0, levels0 = built(name)
    nv = EDITS[edit](v, idx)
    nodes, tris, levels = mpt.bvh_refit_host(v, idx, nv)
    assert levels == levels0 and len(level_ranges(nodes)) == levels
    nlo, nhi = check_refit(nodes0, tris0, nodes, tris, nv, idx, f"{name} {edit}")
    if edit == "identity":
        # the root box equals the builder's (byte equality of the whole tree is not asked for:
        # the builder takes its exponents from an fp32 extent)
        assert np.array_equal(nodes["p"][0], nodes0["p"][0]) and np.array_equal(nodes["e"][0], nodes0["e"][0])
        assert np.array_equal(nodes["qhi"][0], nodes0["qhi"][0]) and np.array_equal(nodes["qlo"][0], nodes0["qlo"][0])
    if edit == "plane":
        pad = box_pad(nv, idx)                           # a zero-extent axis: only the pad is left
        assert (nhi[:, 1].astype(np.float64) - nlo[:, 1] <= 2.01 * pad).all()
    if edit in ("scale_up", "scale_down") and name in ("cornell", "city"):
        k = 10 if edit == "scale_up" else -10             # 1000 = 2^9.97: pad and exponents move with the scale
        d = nodes["e"][0].astype(int) - nodes0["e"][0].astype(int)
        assert ((d == k) | (d == k - np.sign(k))).all(), d


def test_builder_output_is_its_own_refit_input():
    """new_vertices NULL returns the builder's output, and the builder's own boxes pass the same
    containment checks (the reference point of the tightness bound)."""
    v, idx, nodes0, tris0, _ = built("city")
    tlo, thi, slo, shi, nlo, nhi = exact_boxes(nodes0, tris0, v, idx)
    internal, leaf = slot_kinds(nodes0)
    used = internal | leaf
    dlo, dhi, _ = dequantised(nodes0)
    assert (dlo[used] <= slo[used]).all() and (dhi[used] >= shi[used]).all()


def test_refit_host_errors():
    v, idx = tiny(3)
    L = mpt.lib()
    bad = v.copy()
    bad[4, 1] = np.nan
    with pytest.raises(mpt.MptError) as e:
        mpt.bvh_refit_host(v, idx, bad)
    assert e.value.code == -1
    bad[4, 1] = np.inf
    with pytest.raises(mpt.MptError):
        mpt.bvh_refit_host(v, idx, bad)
    with pytest.raises(mpt.MptError):
        mpt.bvh_refit_host(v, idx + 7)                    # an index past the vertices
    counts = np.zeros(3, np.int32)
    assert L.mpt_bvh_refit_host(v.ctypes.data, None, len(v), idx.ctypes.data, len(idx), None, 0, None, 0, counts.ctypes.data) == 0
    assert counts.tolist() == [1, 3, 1]
    small = np.zeros(10, np.uint8)
    assert L.mpt_bvh_refit_host(v.ctypes.data, None, len(v), idx.ctypes.data, len(idx), small.ctypes.data, 10,
                                small.ctypes.data, 10, None) == -1
