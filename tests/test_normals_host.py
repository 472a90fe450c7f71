"""Recomputed vertex normals on the host (mpt_normals_host: the table builder and the host loop of
csrc/normals.h -- the arithmetic the kernels behind mpt_set_normals share), no GPU.

mpt.normals_host is compared byte for byte with restate() below, an independent float32 numpy
restatement of the definition: elementwise, the same operation order, the row sum looped in table
order.  Then exact known answers (a planar grid, an axis-aligned box whose cross products are exact),
the pass-through cases, the table order and the refusals.

Coverage condition: poses() gives the poses that tests/test_normals.py runs on the GPU; on them the
share of grouped vertices that take the pass-through branch (their group's sum has no positive finite
length) is asserted to stay under PASS_CAP, so that a byte comparison there compares recomputed
normals and not copies.
"""
import numpy as np
import pytest

import mpt

from test_refit_host import cornell_scene, edit_jitter, small_city

F = np.float32
PASS_CAP = 0.02   # at most 2 % of the grouped vertices may pass through under a pose of poses()


# ------------------------------------------------------------------------------------
# The restatement
# ------------------------------------------------------------------------------------
def table(idx, group, G):
    """rows[g]: the triangle ids of the corners in group g, in memory order of the corners."""
    rows = [[] for _ in range(G)]
    for c, v in enumerate(np.asarray(idx).reshape(-1)):
        if group[v] >= 0:
            rows[group[v]].append(c // 3)
    return rows


def face_vectors(v, idx):
    I = np.asarray(idx).reshape(-1, 3)
    v = np.asarray(v, F)
    a, b, c = v[I[:, 0]], v[I[:, 1]], v[I[:, 2]]
    e1, e2 = (b - a).astype(F), (c - a).astype(F)
    m = lambda x, y: (x * y).astype(F)
    return np.stack([(m(e1[:, 1], e2[:, 2]) - m(e1[:, 2], e2[:, 1])).astype(F),
                     (m(e1[:, 2], e2[:, 0]) - m(e1[:, 0], e2[:, 2])).astype(F),
                     (m(e1[:, 0], e2[:, 1]) - m(e1[:, 1], e2[:, 0])).astype(F)], 1)


def restate(v, idx, group, normals, flips=None, G=None, has=None):
    """(normals, passed): the definition in float32 numpy; passed marks the grouped vertices with a
    normal flag whose group's sum had no positive finite length."""
    group = np.asarray(group)
    G = int(group.max()) + 1 if G is None else G
    f = face_vectors(v, idx)
    rows = table(idx, group, G)
    out = np.array(normals, F).reshape(-1, 3)
    passed = np.zeros(len(out), bool)
    unit = np.zeros((G, 3), F)
    ok = np.zeros(G, bool)
    with np.errstate(all="ignore"):
        for g in range(G):
            s = np.zeros(3, F)
            for p in rows[g]:
                s = (s + f[p]).astype(F)
            if flips is not None and flips[g]:
                s = -s
            l2 = F(F(F(s[0] * s[0]) + F(s[1] * s[1])) + F(s[2] * s[2]))
            if l2 > 0 and l2 <= np.finfo(F).max:
                ok[g] = True
                unit[g] = s / np.sqrt(l2, dtype=F)
    for i in range(len(out)):
        g = group[i]
        if g < 0 or (has is not None and not has[i]):
            continue
        if ok[g]:
            out[i] = unit[g]
        else:
            passed[i] = True
    return out, passed


def same_bytes(a, b):
    return np.ascontiguousarray(a, F).tobytes() == np.ascontiguousarray(b, F).tobytes()


# ------------------------------------------------------------------------------------
# Poses (shared with tests/test_normals.py)
# ------------------------------------------------------------------------------------
SCENES = {"cornell": cornell_scene, "city": small_city}


def poses(name):
    """The positions that the GPU tests move a scene to: a jitter of 1 % of the extent."""
    sd = SCENES[name]()
    return {"jitter": edit_jitter(sd.vertices.astype(F))}


def groupings(sd):
    V = len(sd.vertices)
    only = np.arange(V) % 3 != 1
    return {"welded": mpt.normal_groups(sd), "per_vertex": mpt.normal_groups(sd, weld=False),
            "only": mpt.normal_groups(sd, only=only)}


def wild_normals(sd, seed=7):
    """Normals as an update might leave them: non-unit, with -0 among them."""
    rng = np.random.default_rng(seed)
    n = (sd.normals * rng.uniform(0.5, 2.0, (len(sd.normals), 1))).astype(F)
    n[::5, 1] = F(-0.0)
    return n


@pytest.mark.parametrize("grouping", ["welded", "per_vertex", "only"])
@pytest.mark.parametrize("name", list(SCENES))
def test_equals_the_restatement(name, grouping):
    sd = SCENES[name]()
    idx = sd.triangle_indices
    g, G = groupings(sd)[grouping]
    assert G > 1 and g.max() == G - 1
    if grouping == "welded":
        assert G < len(g), "nothing welded"
    if grouping == "only":
        assert (g == -1).sum() == (np.arange(len(g)) % 3 == 1).sum()
    n0 = wild_normals(sd)
    rng = np.random.default_rng(1)
    flips = (rng.random(G) < 0.3).astype(np.uint8)
    for pose, v in [("rest", sd.vertices.astype(F))] + list(poses(name).items()):
        for fl in (None, flips):
            got = mpt.normals_host(v, idx, g, n0, fl, G, sd.has_normals)
            ref, passed = restate(v, idx, g, n0, fl, G, sd.has_normals)
            assert same_bytes(got, ref), f"{name} {grouping} {pose}: {(got != ref).any(1).sum()} vertices differ"
            grouped = (g >= 0) & (np.asarray(sd.has_normals) != 0)
            share = passed.sum() / grouped.sum()
            print(f"{name} {grouping} {pose}: {grouped.sum()} grouped vertices, pass-through share {share:.4f}")
            assert share <= PASS_CAP, f"{name} {grouping} {pose}: {share:.3f} of the grouped vertices pass through"
            assert not same_bytes(got[grouped], n0[grouped])
            assert same_bytes(got[~grouped], n0[~grouped])


# ------------------------------------------------------------------------------------
# Exact known answers
# ------------------------------------------------------------------------------------
def grid(nx, nz):
    xs, zs = np.meshgrid(np.arange(nx, dtype=F), np.arange(nz, dtype=F), indexing="ij")
    v = np.stack([xs.ravel(), np.full(nx * nz, 0.5, F), zs.ravel()], 1).astype(F)
    tri = []
    for i in range(nx - 1):
        for j in range(nz - 1):
            a, b, c, d = i * nz + j, (i + 1) * nz + j, i * nz + j + 1, (i + 1) * nz + j + 1
            tri += [[a, c, b], [b, c, d]]   # counter-clockwise seen from +y
    return v, np.array(tri, np.int32)


def box(reverse=False):
    """An axis-aligned box, four vertices per face with the face's authored normal."""
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 2.5, 2.75])
    v, n, tri = [], [], []
    for ax in range(3):
        for sg in (-1, 1):
            u, w = (ax + 1) % 3, (ax + 2) % 3
            base = len(v)
            for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = np.zeros(3)
                p[ax] = hi[ax] if sg > 0 else lo[ax]
                p[u] = hi[u] if du else lo[u]
                p[w] = hi[w] if dw else lo[w]
                v.append(p)
                nn = np.zeros(3)
                nn[ax] = sg
                n.append(nn)
            q = [[base, base + 1, base + 2], [base, base + 2, base + 3]]
            if sg < 0:
                q = [t[::-1] for t in q]
            tri += q
    tri = np.array(tri, np.int32)
    if reverse:
        tri = tri[:, ::-1].copy()
    return np.array(v, F), np.array(n, F), tri


def test_planar_grid_is_exactly_up():
    v, tri = grid(7, 5)
    n0 = np.tile(np.array([[0.6, 0.0, 0.8]], F), (len(v), 1))
    for weld in (True, False):
        g, G = mpt.normal_groups(v, n0, weld=weld)
        got = mpt.normals_host(v, tri, g, n0)
        assert same_bytes(got, np.tile(np.array([[0.0, 1.0, 0.0]], F), (len(v), 1)))


def test_box_keeps_its_hard_edges():
    v, n, tri = box()
    g, G = mpt.normal_groups(v, n)
    assert G == 24                           # a corner's three vertices differ in their normals
    junk = np.tile(np.array([[0.3, 0.3, 0.3]], F), (len(v), 1))
    assert same_bytes(mpt.normals_host(v, tri, g, junk), n)
    # welded by position alone the corners would be smoothed: the normals are what keeps them apart
    gp, Gp = mpt.normal_groups(v, np.zeros_like(n))
    assert Gp == 8 and not same_bytes(mpt.normals_host(v, tri, gp, junk), n)


def test_reversed_winding_needs_the_flips():
    v, n, tri = box(reverse=True)
    g, G = mpt.normal_groups(v, n)
    junk = np.tile(np.array([[0.3, 0.3, 0.3]], F), (len(v), 1))
    assert np.array_equal(mpt.normals_host(v, tri, g, junk), -n)   # (by value: the zeros' signs differ)
    flips = mpt.normal_flips((v, n, tri), g, G)
    assert flips.dtype == np.uint8 and flips.all()
    # (equal by value and in every non-zero component's bits: the definition negates the sum, whose
    # zero components are +0 -- the sum starts at +0 -- so the flipped normal's zeros are -0)
    got = mpt.normals_host(v, tri, g, junk, flips)
    assert np.array_equal(got, n) and same_bytes(got[n != 0], n[n != 0])
    assert np.signbit(got[n == 0]).all()
    # a box wound the right way needs none
    v2, n2, tri2 = box()
    assert not mpt.normal_flips((v2, n2, tri2), g, G).any()


def test_normal_groups_and_flips_take_a_scene():
    sd = cornell_scene()
    g, G = mpt.normal_groups(sd)
    g2, G2 = mpt.normal_groups(sd.vertices, sd.normals)
    assert G == G2 and np.array_equal(g, g2) and g.dtype == np.int32
    # numbered in the order of the groups' first vertices
    first = np.array([np.flatnonzero(g == k)[0] for k in range(G)])
    assert (np.diff(first) > 0).all()
    f = mpt.normal_flips(sd, g, G)
    f2 = mpt.normal_flips((sd.vertices, sd.normals, sd.triangle_indices, sd.has_normals), g, G)
    assert np.array_equal(f, f2) and len(f) == G


# ------------------------------------------------------------------------------------
# Pass-through
# ------------------------------------------------------------------------------------
def test_pass_through_keeps_the_bytes():
    v, tri = grid(4, 4)
    V = len(v)
    v = np.concatenate([v, np.array([[9, 9, 9], [9, 9, 9], [9, 9, 9], [5, 5, 5]], F)])   # a point triangle, an unused vertex
    tri = np.concatenate([tri, np.array([[V, V + 1, V + 2]], np.int32)])
    g = np.arange(len(v), dtype=np.int32)
    g[3] = -1                                # untouched by its group id
    G = len(v) + 1                           # the last group is empty
    has = np.ones(len(v), np.uint8)
    has[6] = 0                               # no vertex normal: shaded with the geometric normal
    n0 = np.tile(np.array([[-0.0, 3.0, 0.25]], F), (len(v), 1))
    got = mpt.normals_host(v, tri, g, n0, None, G, has)
    keep = [3, 6, V, V + 1, V + 2, V + 3]    # group -1, no flag, the degenerate group (3), no triangle
    assert same_bytes(got[keep], n0[keep])
    rest = np.setdiff1d(np.arange(len(v)), keep)
    assert same_bytes(got[rest], np.tile(np.array([[0.0, 1.0, 0.0]], F), (len(rest), 1)))
    ref, passed = restate(v, tri, g, n0, None, G, has)
    assert same_bytes(got, ref) and sorted(np.flatnonzero(passed)) == [V, V + 1, V + 2, V + 3]
    # an overflowing cross product passes through as well
    big = v.copy()
    big[:V] *= F(3e19)
    got = mpt.normals_host(big, tri, g, n0, None, G, has)
    assert same_bytes(got[[0, 5, 10]], n0[[0, 5, 10]])


# ------------------------------------------------------------------------------------
# Table order
# ------------------------------------------------------------------------------------
def test_triangle_order_may_matter_group_numbers_do_not():
    sd = small_city()
    v = poses("city")["jitter"]
    idx = sd.triangle_indices.reshape(-1, 3)
    g, G = mpt.normal_groups(sd)
    n0 = sd.normals.astype(F)
    a = mpt.normals_host(v, idx, g, n0, None, G, sd.has_normals)
    rng = np.random.default_rng(5)
    # renumbered groups: the same bytes
    perm = rng.permutation(G).astype(np.int32)
    g2 = np.where(g >= 0, perm[np.maximum(g, 0)], -1).astype(np.int32)
    assert same_bytes(mpt.normals_host(v, idx, g2, n0, None, G, sd.has_normals), a)
    # permuted triangles: another order of additions -- equal to ITS restatement, and close
    idx2 = idx[rng.permutation(len(idx))]
    b = mpt.normals_host(v, idx2, g, n0, None, G, sd.has_normals)
    assert same_bytes(b, restate(v, idx2, g, n0, None, G, sd.has_normals)[0])
    assert np.abs(a - b).max() < 1e-5
    print("vertices whose bytes depend on the triangle order:", int((a != b).any(1).sum()), "of", len(a))


def test_a_triangle_with_two_corners_in_one_group_counts_twice():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 0, -1], [0, 1, 0]], F)
    tri = np.array([[0, 1, 2], [0, 1, 3]], np.int32)     # normals +y (area 1/2) and +z (area 1/2)
    n0 = np.zeros((4, 3), F)
    g = np.array([0, 0, 1, 2], np.int32)                   # vertices 0 and 1 welded: both triangles twice
    got = mpt.normals_host(v, tri, g, n0)
    assert same_bytes(got, restate(v, tri, g, n0)[0])
    assert table(tri, g, 3) == [[0, 0, 1, 1], [0], [1]]
    r = F(2.0) / np.sqrt(F(8.0), dtype=F)
    assert same_bytes(got[0], np.array([0, r, r], F)) and same_bytes(got[0], got[1])


# ------------------------------------------------------------------------------------
# Refusals
# ------------------------------------------------------------------------------------
def test_refusals_leave_the_arrays():
    v, tri = grid(3, 3)
    g = np.arange(len(v), dtype=np.int32)
    n0 = np.tile(np.array([[0.6, 0.0, 0.8]], F), (len(v), 1))
    keep = n0.copy()

    def refused(vv, ii, gg, G, msg):
        with pytest.raises(mpt.MptError) as e:
            mpt.normals_host(vv, ii, gg, n0, None, G)
        assert e.value.code == -1 and msg in str(e.value), str(e.value)
        assert same_bytes(n0, keep)

    refused(v, tri, g, 0, "group count")
    refused(v, tri, g, len(v) - 1, "group id")
    bad = g.copy()
    bad[2] = -2
    refused(v, tri, bad, len(v), "group id")
    bad_tri = tri.copy()
    bad_tri[1, 1] = len(v)
    refused(v, bad_tri, g, len(v), "vertex index")
    bad_tri[1, 1] = -1
    refused(v, bad_tri, g, len(v), "vertex index")
    L = mpt.lib()
    assert L.mpt_normals_host(None, len(v), mpt._p(tri), len(tri), mpt._p(g), None, len(v), None, mpt._p(n0)) == -1
    assert L.mpt_normals_host(mpt._p(v), 0, mpt._p(tri), len(tri), mpt._p(g), None, len(v), None, mpt._p(n0)) == -1
    assert L.mpt_normals_host(mpt._p(v), len(v), mpt._p(tri), -1, mpt._p(g), None, len(v), None, mpt._p(n0)) == -1
    assert same_bytes(n0, keep)
    with pytest.raises(ValueError):
        mpt.normals_host(v, tri, g[:-1], n0)
    with pytest.raises(ValueError):
        mpt.normals_host(v, tri, g, n0, np.zeros(2, np.uint8))
    with pytest.raises(ValueError):
        mpt.normal_groups(v, n0, only=np.ones(3, bool))
    # a returned array is new: the caller's normals are never written
    out = mpt.normals_host(v, tri, g, n0)
    assert same_bytes(n0, keep) and not same_bytes(out, keep)


def test_morph_data_touched():
    from mpt import scene
    md = scene.MorphData()
    md.vertex_ids = np.array([4, 1, 4], np.int32)
    with pytest.raises(ValueError):
        md.touched
    md.num_vertices = 6
    assert md.touched.tolist() == [False, True, False, False, True, False]
