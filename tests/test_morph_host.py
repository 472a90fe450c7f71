"""mpt_morph_host: the host loop of csrc/morph.h, which mpt_update_morph's kernel shares byte for
byte (tests/test_morph.py compares the two on the GPU); the by-target tables' checks and their
transposition by vertex; the glTF loader's SceneData.morph; synthetic.write_morphed_gltf.  No GPU.

The arithmetic is restated here in numpy float32, one explicit rounding per operation in the
definition's order (numpy's float32 sqrt and division are IEEE-correctly rounded): the library's
output equals it byte for byte.  Against float64 the bound comes from counting roundings.
"""
import itertools
import json
import os

import numpy as np
import pytest

import mpt
from mpt import _build, scene, synthetic

from test_skin_host import U, blend64, gamma, gltf_skinning, position_terms
from test_xform_host import angle

F = np.float32


def tables(targets):
    """[(ids, dpos, dnrm or None)] -> the C ABI's arrays (offsets, ids, dpos, dnrm or None)."""
    return mpt._morph_tables(targets, "test")[1:]


def restate(v, n, targets, w, order=None):
    """morph.h in explicit float32 steps.  targets: [(ids, dpos, dnrm or None)] with sorted ids;
    order: the order in which a vertex's targets are visited (None: ascending target index)."""
    has_n = any(t[2] is not None for t in targets)
    ov, on = v.copy(), None if n is None else n.copy()
    rows = {}
    for t in (range(len(targets)) if order is None else order):
        ids, dp, dn = targets[t]
        for k, vi in enumerate(ids):
            rows.setdefault(int(vi), []).append((t, F(dp[k]), None if dn is None else F(dn[k])))
    with np.errstate(over="ignore", invalid="ignore"):
        for vi, es in rows.items():
            acc = [F(x) for x in v[vi]]
            tt = [F(0)] * 3 if n is None else [F(x) for x in n[vi]]
            applied = False
            for t, dp, dn in es:
                wk = F(w[t])
                if wk == 0:
                    continue
                applied = True
                for r in range(3):
                    acc[r] = F(acc[r] + F(wk * dp[r]))
                    if has_n:
                        tt[r] = F(tt[r] + F(wk * (F(0) if dn is None else dn[r])))
            if not applied:
                continue
            ov[vi] = acc
            if has_n and n is not None:
                l2 = F(F(F(tt[0] * tt[0]) + F(tt[1] * tt[1])) + F(tt[2] * tt[2]))
                if l2 > 0 and np.isfinite(l2):
                    l = np.sqrt(l2)
                    assert l.dtype == np.float32
                    on[vi] = [F(x / l) for x in tt]
    return ov, on


def soup(V, T, seed, with_normals=True, skip_every=7):
    rng = np.random.default_rng(seed)
    v = (rng.random((V, 3)) * 8 - 4).astype(F)
    n = rng.normal(size=(V, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    targets = []
    for t in range(T):
        ids = np.flatnonzero((rng.random(V) < rng.uniform(0.1, 0.9)) & (np.arange(V) % skip_every != 0))
        if t == 1:
            ids = ids[:0]                                   # an empty target
        dp = rng.normal(size=(len(ids), 3)).astype(F)
        dn = (0.5 * rng.normal(size=(len(ids), 3))).astype(F) if with_normals and t % 3 != 2 else None
        targets.append((ids, dp, dn))
    w = rng.uniform(-1.5, 1.5, T).astype(F)
    w[T // 2] = 0.0
    return v, n, targets, w


# ------------------------------------------------------------------------------------
# The arithmetic
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals", [True, False])
def test_equals_the_float32_restatement(with_normals):
    v, n, targets, w = soup(700, 7, 3, with_normals)
    ov, on = mpt.morph_host(v, n, targets, w)
    rv, rn = restate(v, n, targets, w)
    assert ov.tobytes() == rv.tobytes() and on.tobytes() == rn.tobytes()
    assert not np.array_equal(ov, v)
    assert np.array_equal(on, n) == (not with_normals)
    pv, pn = mpt.morph_host(v, None, targets, w)            # positions only
    assert pn is None and pv.tobytes() == rv.tobytes()


def test_positions_agree_with_float64():
    """acc = p; acc = fl(acc + fl(w d)) per applied entry: with k applied entries the first term and
    p pass through k sums, every product is rounded once and passes through at most k sums, so every
    term of S = |p| + sum |w d| carries at most k + 1 <= 2k roundings: |acc - exact| <= g_2k S (k >= 1;
    k = 0 is exact).  The float64 evaluation of the fp32 inputs adds at most 2^-40 S."""
    v, n, targets, w = soup(4000, 9, 5)
    ov, _ = mpt.morph_host(v, None, targets, w)
    exact = v.astype(np.float64)
    S = np.abs(exact)
    k = np.zeros(len(v))
    for t, (ids, dp, _) in enumerate(targets):
        if w[t] != 0:
            term = np.float64(w[t]) * dp.astype(np.float64)
            exact[ids] += term
            S[ids] += np.abs(term)
            k[ids] += 1
    err = np.abs(ov.astype(np.float64) - exact)
    bound = (gamma(2 * k) + 2.0 ** -40)[:, None] * S
    print(f"positions: max error / (2^-24 S) = {(err / (U * S)).max():.3f}, most applied entries {int(k.max())}")
    assert k.max() >= 5 and (err <= bound).all()
    assert np.array_equal(ov[k == 0], v[k == 0])


def test_pass_through_is_byte_exact():
    v, n, targets, w = soup(300, 5, 11)
    v[0] = [-0.0, 1.0, -0.0]                                # vertex 0 has no entries (skip_every)
    n[0] = [0.0, 3.0, 4.0]
    v[1], n[1] = [-0.0, -0.0, 2.0], [0.3, 0.0, 0.0]         # vertex 1: entries of a zero-weight target only
    only = (np.array([1]), np.array([[1.0, 2.0, 3.0]], F), np.array([[0.5, 0.5, 0.5]], F))
    targets = [(ids[ids != 1], dp[ids != 1], None if dn is None else dn[ids != 1]) for ids, dp, dn in targets] + [only]
    w = np.append(w, F(0.0))
    assert any(len(t[0]) and t[2] is not None for t in targets)
    ov, on = mpt.morph_host(v, n, targets, w)
    for vi in (0, 1):
        assert ov[vi].tobytes() == v[vi].tobytes() and on[vi].tobytes() == n[vi].tobytes(), vi
    assert ov.tobytes() == restate(v, n, targets, w)[0].tobytes()
    # all-zero weights (a -0 among them): nothing changes, a -0 coordinate and a non-unit normal included
    z = np.zeros(len(w), F)
    z[2] = -0.0
    vz, nz = v.copy(), n * F(1.7)
    vz[int(targets[0][0][0])] = [-0.0, 0.0, -0.0]            # (a vertex with entries)
    ov, on = mpt.morph_host(vz, nz, targets, z)
    assert ov.tobytes() == vz.tobytes() and on.tobytes() == nz.tobytes()
    # a weight that is not zero does move a vertex with entries, and renormalises its normal
    ov, on = mpt.morph_host(vz, nz, targets, w)
    moved = np.flatnonzero((ov != vz).any(1))
    assert len(moved) > 100 and np.abs(np.linalg.norm(on[moved].astype(np.float64), axis=1) - 1).max() < 4 * U


def test_entry_order_is_the_target_order():
    """Vertex 4 appears in targets 0, 2 and 5, whose sizes differ (2 is the largest, 0 the smallest):
    its deltas are added in target order, whatever the sizes.  The values make the order visible:
    3 + 1e8 rounds to 1e8 (the spacing there is 8) but (3 + 3) + 1e8 to 1e8 + 8."""
    V = 12
    v = np.zeros((V, 3), F)
    n = np.zeros((V, 3), F)
    small = F(0.001)
    mine = {0: [3, 1e8, 3], 2: [1e8, 3, 3], 5: [3, 3, 1e8]}
    others = {0: [1], 2: [0, 1, 2, 3, 5, 6, 7], 5: [3, 6, 9], 1: [], 3: [7, 8], 4: [0]}
    targets = []
    for t in range(6):
        ids = sorted(others[t] + ([4] if t in mine else []))
        dp = np.array([mine[t] if i == 4 else [small, small, small] for i in ids], F).reshape(-1, 3)
        targets.append((np.array(ids, np.int64), dp, None))
    w = np.ones(6, F)
    ov, _ = mpt.morph_host(v, None, targets, w)
    want = restate(v, None, targets, w)[0]
    assert ov.tobytes() == want.tobytes()
    assert ov[4].tolist() == [1e8, 1e8, 1e8 + 8]
    sizes = [len(t[0]) for t in targets]
    by_size = sorted(range(6), key=lambda t: sizes[t])
    assert [t for t in by_size if t in mine] == [0, 5, 2]
    differ = [p for p in itertools.permutations([0, 2, 5])
              if restate(v, None, targets, w, order=[1, 3, 4] + list(p))[0][4].tobytes() != want[4].tobytes()]
    assert (0, 5, 2) in differ and (2, 5, 0) in differ and len(differ) == 4       # ascending and descending size among them
    # the caller's arrays in another layout (targets' entries given unsorted): the wrapper sorts, same bytes
    shuffled = [(ids[::-1], dp[::-1], None) for ids, dp, _ in targets]
    assert mpt.morph_host(v, None, shuffled, w)[0].tobytes() == want.tobytes()


def test_normal_falls_back_to_the_rest_normal():
    v = np.zeros((3, 3), F)
    n = np.array([[0, 0, 1], [0, 0, 1], [0, 2, 0]], F)
    targets = [(np.array([0, 1, 2]), np.ones((3, 3), F), np.array([[0, 0, -1], [3e38, 3e38, 0], [0, 1, 0]], F))]
    ov, on = mpt.morph_host(v, n, targets, np.ones(1, F))
    assert on[0].tolist() == [0, 0, 1] and on[1].tolist() == [0, 0, 1]       # zero length; overflowing squared length
    assert on[2].tolist() == [0, 1, 0] and ov.tolist() == [[1, 1, 1]] * 3
    assert on.tobytes() == restate(v, n, targets, np.ones(1, F))[1].tobytes()


# ------------------------------------------------------------------------------------
# Refusals
# ------------------------------------------------------------------------------------
def call(v, n, T, off, ids, dp, dn, w):
    ov, on = np.empty_like(v), np.empty_like(v)
    p = lambda a: None if a is None else a.ctypes.data
    return mpt.lib().mpt_morph_host(p(v), p(n), len(v), T, p(off), p(ids), p(dp), p(dn), p(w), p(ov), p(on)), ov


def test_refusals():
    v, n, targets, w = soup(50, 4, 21)
    off, ids, dp, dn = tables(targets)
    T = 4
    assert call(v, n, T, off, ids, dp, dn, w)[0] == 0
    k2 = int(off[2])                                        # the first entry of target 2
    assert off[3] - off[2] >= 2

    def edited(a, where, value):
        b = a.copy()
        b[where] = value
        return b

    swapped = ids.copy()
    swapped[[k2, k2 + 1]] = swapped[[k2 + 1, k2]]
    cases = {
        "offsets not starting at 0": dict(off=edited(off, 0, 1)),
        "offsets decreasing": dict(off=edited(off, 2, off[3] + 1)),
        "id too large": dict(ids=edited(ids, k2, 50)),
        "id negative": dict(ids=edited(ids, 0, -1)),
        "ids out of order": dict(ids=swapped),
        "a duplicate id": dict(ids=edited(ids, k2 + 1, ids[k2])),
        "NaN position delta": dict(dp=edited(dp, (3, 1), np.nan)),
        "infinite normal delta": dict(dn=edited(dn, (len(dn) - 1, 0), np.inf)),
        "NaN weight": dict(w=edited(w, 1, np.nan)),
        "infinite weight": dict(w=edited(w, 3, -np.inf)),
        "no targets": dict(T=0),
        "negative target count": dict(T=-1),
    }
    for what, change in cases.items():
        a = dict(v=v, n=n, T=T, off=off, ids=ids, dp=dp, dn=dn, w=w)
        a.update(change)
        keep = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in a.items()}
        assert call(**a)[0] == -1, what
        assert mpt.lib().mpt_last_error()
        for k, x in a.items():
            if isinstance(x, np.ndarray):
                assert x.tobytes() == keep[k].tobytes(), f"{what}: {k} touched"
    # an overflowing output: finite inputs
    big = v.copy()
    big[int(ids[0])] = [3e38, 0, 0]
    dbig = edited(dp, (0, 0), 3e38)
    assert w[0] != 0
    rc, _ = call(big, n, T, off, ids, dbig, dn, edited(w, 0, 1.0))
    assert rc == -1 and b"finite" in mpt.lib().mpt_last_error()
    with pytest.raises(mpt.MptError) as e:
        mpt.morph_host(big, n, [(ids[:off[1]], dbig[:off[1]], None)], [1.0])
    assert e.value.code == -1
    # NULL arrays and a vertex count of 0
    assert call(v[:0], n[:0], T, off, ids, dp, dn, w)[0] == -1
    assert mpt.lib().mpt_morph_host(None, None, 50, T, off.ctypes.data, ids.ctypes.data, dp.ctypes.data, None, w.ctypes.data,
                                    v.ctypes.data, None) == -1


def test_empty_tables_are_accepted():
    """Every target empty (N = 0): nothing moves; the arrays of entries may then be NULL."""
    v, n, _, _ = soup(20, 3, 2)
    off = np.zeros(4, np.int32)
    ov = np.empty_like(v)
    w = np.ones(3, F)
    assert mpt.lib().mpt_morph_host(v.ctypes.data, None, 20, 3, off.ctypes.data, None, None, None, w.ctypes.data, ov.ctypes.data,
                                    None) == 0
    assert ov.tobytes() == v.tobytes()
    assert mpt.morph_host(v, n, [([], np.zeros((0, 3)), None)] * 3, w)[1].tobytes() == n.tobytes()


def test_wrapper_rejects_duplicates_before_any_library_call(monkeypatch):
    v, n, targets, w = soup(30, 2, 8)
    ids, dp, dn = targets[0]
    assert len(ids) >= 2
    dup = (np.append(ids, ids[0]), np.concatenate([dp, dp[:1]]), np.concatenate([dn, dn[:1]]))

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(mpt, "lib", no_library)
    with pytest.raises(ValueError, match="more than once"):
        mpt.morph_host(v, n, [dup, targets[1]], w)
    with pytest.raises(ValueError, match="more than once"):
        mpt.GPURenderer.set_morph(object(), [dup, targets[1]])
    with pytest.raises(ValueError, match="position deltas"):
        mpt.morph_host(v, n, [(ids, dp[:-1], None), targets[1]], w)
    with pytest.raises(ValueError, match="weights for"):
        mpt.morph_host(v, n, targets, w[:1])


def test_constants_and_symbols():
    assert mpt.MORPH_LDS_TARGETS == 4096
    with open(os.path.join(str(_build.INCLUDE), "mpt.h")) as f:
        assert "#define MPT_MORPH_LDS_TARGETS 4096" in f.read()
    for s in ("mpt_set_morph", "mpt_update_morph", "mpt_update_morph_skin", "mpt_morph_host"):
        assert s in mpt.SYMBOLS and hasattr(mpt.lib(), s)


# ------------------------------------------------------------------------------------
# The glTF loader
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[True, False], ids=["skinned", "unskinned"])
def morphed(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("morphed") / "tube.gltf")
    synthetic.write_morphed_gltf(path, skinned=request.param)
    return path, scene.load_gltf(path), request.param


def raw_morph(path):
    """The file, the tube's own positions, normals and per-target (POSITION, NORMAL or None) deltas
    in float64 (sparse accessors expanded)."""
    with open(path) as f:
        g = json.load(f)
    bins = [scene._uri_bytes(os.path.dirname(path), b["uri"]) for b in g["buffers"]]
    prim = g["meshes"][0]["primitives"][0]
    get = lambda i: scene._accessor(g, bins, i).astype(np.float64)
    tg = [(get(t["POSITION"]), get(t["NORMAL"]) if "NORMAL" in t else None) for t in prim["targets"]]
    return g, bins, get(prim["attributes"]["POSITION"]), get(prim["attributes"]["NORMAL"]), tg


def test_loader_morph_shapes(morphed):
    path, sd, skinned = morphed
    m = sd.morph
    g, bins, p, nl, tg = raw_morph(path)
    assert (sd.skin is not None) == skinned
    assert m is not None and m.num_targets == 2
    assert m.target_offsets.dtype == np.int32 and m.target_offsets.tolist() == [0, 56, 64]
    assert m.vertex_ids.dtype == np.int32 and m.vertex_ids.shape == (64,)
    assert m.pos_deltas.dtype == np.float32 and m.pos_deltas.shape == (64, 3) and m.nrm_deltas.shape == (64, 3)
    assert m.target_node.tolist() == [0, 0] and m.target_index.tolist() == [0, 1]
    assert m.default_weights.dtype == np.float32 and m.default_weights.tolist() == [0.25, 0.5]
    assert g["meshes"][0]["weights"] == [0.25, 0.5] and "sparse" in g["accessors"][g["meshes"][0]["primitives"][0]["targets"][1]["POSITION"]]
    tube = np.flatnonzero(sd.vertex_object == 0)
    assert len(tube) == 56 and set(m.vertex_ids.tolist()) <= set(tube.tolist())     # the floor has no targets
    sparse = m.vertex_ids[56:]
    assert len(sparse) == 8 and (np.diff(sparse) > 0).all() and (np.diff(m.vertex_ids[:56]) > 0).all()
    assert np.array_equal(sparse - tube[0], np.flatnonzero(np.any(tg[1][0] != 0, axis=1)))     # the middle ring
    assert not m.nrm_deltas[56:].any() and m.nrm_deltas[:56].any()                   # target 1 has no NORMAL
    # the node's rotation is in the deltas: R d, not d
    R = scene._node_matrix(g["nodes"][0])[:3, :3]
    assert not np.allclose(R, np.eye(3))
    assert np.abs(m.pos_deltas[:56] - tg[0][0] @ R.T).max() <= 4 * U and np.abs(m.pos_deltas[:56] - tg[0][0]).max() > 0.01
    # node.weights override mesh.weights
    g["nodes"][0]["weights"] = [0.5, -1.0]
    p2 = os.path.join(os.path.dirname(path), "node_weights.gltf")
    with open(p2, "w") as f:
        json.dump(g, f)
    assert scene.load_gltf(p2).morph.default_weights.tolist() == [0.5, -1.0]


def test_loader_world_morph_then_skin_is_gltfs_mesh_space_order(morphed):
    """skin_host(morph_host(rest)) on the loader's world-space arrays against glTF's order in
    float64: morph in mesh space, p + sum w d, then the skin (skinned) or the node's transform M.

    Bound, per coordinate.  The loader rounds M p and R d to fp32: u A_p and u |w| A_d, with A_p =
    |R| |p| + |t| and A_d = |R| |d| (the float64 evaluations themselves: 2^-40 of the same terms).
    morph_host adds g_2k S_m, S_m = |v| + sum |w d| over its k <= 2 applied entries
    (test_positions_agree_with_float64).  That is E_m, the whole bound without a skin.  The skin
    maps E_m through |B| (test_skin_host.blend64's Bs) and adds its own g_8 S plus one rounding of
    every matrix entry, u S (test_skin_host.skin_bound)."""
    path, sd, skinned = morphed
    m = sd.morph
    g, bins, p, nl, tg = raw_morph(path)
    tube = sd.vertex_object == 0
    w = np.array([0.7, -0.4], F)
    w64 = w.astype(np.float64)
    M = scene._node_matrix(g["nodes"][0])
    R, t = M[:3, :3], M[:3, 3]
    local = p + sum(w64[k] * tg[k][0] for k in range(2))
    mv, mn = mpt.morph_host(sd.vertices, sd.normals, m, w)
    A_p = np.abs(p) @ np.abs(R).T + np.abs(t)
    A_d = sum(abs(w64[k]) * (np.abs(tg[k][0]) @ np.abs(R).T) for k in range(2))
    S_m = np.abs(sd.vertices[tube].astype(np.float64)) + A_d
    E_m = (U + 2.0 ** -40) * (A_p + A_d) + gamma(4) * S_m
    assert mv[~tube].tobytes() == sd.vertices[~tube].tobytes() and mn[~tube].tobytes() == sd.normals[~tube].tobytes()
    if not skinned:
        ref = local @ R.T + t
        got, bound = mv[tube], E_m
        # normals: RIT (n + sum w dn), normalised; the loader's division by |RIT n| keeps the sum parallel to it
        RIT = np.linalg.inv(R).T
        nref = (nl + w64[0] * tg[0][1]) @ RIT.T
        assert (angle(mn[tube], nref / np.linalg.norm(nref, axis=1, keepdims=True)) < 1e-5).all()
        assert (angle(mn[tube], sd.normals[tube]) > 1e-3).any()
    else:
        from test_skin_host import raw_tube
        _, _, j, wt, ibm = raw_tube(path)
        bend = np.eye(4)
        bend[:3, 3] = sd.skin.node_locals[2][:3, 3] + [0.05, 0.0, -0.02]
        c, s = np.cos(0.6), np.sin(0.6)
        bend[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        over = {2: bend}
        ref = gltf_skinning(g, local, j, wt, ibm, lambda ni: over.get(ni, scene._node_matrix(g["nodes"][ni])))
        SM = scene.skin_matrices(sd, over)
        got, _ = mpt.skin_host(mv, mn, sd.skin.joints, sd.skin.weights, SM)
        got = got[tube]
        B, Bs = blend64(SM, sd.skin.joints[tube], sd.skin.weights[tube])
        S = position_terms(B, Bs, mv[tube])[1]
        bound = np.einsum("vrc,vc->vr", Bs[:, :, :3], E_m) + S * (gamma(8) + U + 2.0 ** -40)
        assert np.abs(ref - (local @ R.T + t)).max() > 0.1          # the pose bends the tube
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{'skinned' if skinned else 'unskinned'}: max error {err.max():.3e}, max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all() and bound.max() < 1e-5
    assert np.abs(ref - (p @ R.T + t)).max() > 0.05                 # the morph shows


def test_files_without_targets_have_no_morph(tmp_path):
    assert scene.load_scene("cornell_pbr").morph is None
    assert scene.load_gltf(synthetic.write_skinned_gltf(str(tmp_path / "tube.gltf"))).morph is None


def test_morph_driver_built():
    """build() compiles the driver next to the others (plain g++ against libmpt)."""
    assert _build.MORPH_TEST.exists(), "morph driver not built (run __graft_entry__.build())"
    assert os.access(_build.MORPH_TEST, os.X_OK)
