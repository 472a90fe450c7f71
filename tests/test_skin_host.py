"""Linear-blend skinning on the host (mpt_skin_host: the host loop of csrc/skin.h -- the arithmetic
the kernel of mpt_update_skin shares), no GPU.

Checked against a numpy float64 restatement: positions and normals within bounds derived from the
roundings of the definition, the side of a mirrored normal, byte-exact pass-through of unskinned
vertices and of identity joints, the one-joint case against mpt_transform_host, the refusals; the
glTF loader's SceneData.skin and scene.skin_matrices on synthetic.write_skinned_gltf's file; the C++
driver of tests/test_skin_host_cpp.py.  tests/test_skin.py runs the kernel against this loop byte
for byte.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import mpt
from mpt import _build, scene, synthetic

from test_xform_host import angle, rot

U = 2.0 ** -24   # the unit roundoff of fp32


def gamma(k):
    """k roundings compounded: (1 + u)^k - 1 <= k u / (1 - k u)."""
    return k * U / (1 - k * U)


def joint_matrices(k, seed, mirror=False, spread=25.0):
    """[k, 3, 4] float32: rotations within `spread` degrees of one common rotation (so that no blend
    of them collapses) times scales in [0.5, 2], a translation; mirror: every joint mirrored in x."""
    rng = np.random.default_rng(seed)
    base = rot(rng.normal(size=3), rng.uniform(0, 360))
    out = np.zeros((k, 3, 4), np.float32)
    for i in range(k):
        A = rot(rng.normal(size=3), rng.uniform(-spread, spread)) @ base @ np.diag(rng.uniform(0.5, 2.0, 3))
        if mirror:
            A = A @ np.diag([-1.0, 1.0, 1.0])
        out[i, :, :3] = A
        out[i, :, 3] = rng.uniform(-5, 5, 3)
    return out


def soup(v_count, k, seed, unskinned_every=7):
    rng = np.random.default_rng(seed)
    v = (rng.random((v_count, 3)) * 8 - 4).astype(np.float32)
    n = rng.normal(size=(v_count, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    J = rng.integers(0, k, (v_count, 4)).astype(np.int32)
    W = rng.random((v_count, 4)).astype(np.float32)
    W[rng.random((v_count, 4)) < 0.25] = 0.0          # fewer than four influences
    W[W.sum(1) == 0, 0] = 1.0
    W /= W.sum(1, keepdims=True)
    W[::unskinned_every] = 0.0
    return v, n, J, W


def blend64(M, J, W):
    """(B, Bs): the float64 blend sum_i w_i M_i per vertex, [V, 3, 4], and sum_i |w_i M_i|."""
    m = M.astype(np.float64)[J]                       # [V, 4, 3, 4]
    w = W.astype(np.float64)[:, :, None, None]
    return (w * m).sum(1), np.abs(w * m).sum(1)


def position_terms(B, Bs, v):
    """(x*, S): the float64 position and sum_c Bs[r][c] |x_c| + Bs[r][3]."""
    x = v.astype(np.float64)
    return np.einsum("vrc,vc->vr", B[:, :, :3], x) + B[:, :, 3], np.einsum("vrc,vc->vr", Bs[:, :, :3], np.abs(x)) + Bs[:, :, 3]


def cofactor_abs(As):
    """P_rc = As As + As As over the index pairs of cofactor (r, c), for [V, 3, 3] magnitudes."""
    i1, i2 = [1, 2, 0], [2, 0, 1]
    P = np.zeros_like(As)
    for r in range(3):
        for c in range(3):
            P[:, r, c] = As[:, i1[r], i1[c]] * As[:, i2[r], i2[c]] + As[:, i1[r], i2[c]] * As[:, i2[r], i1[c]]
    return P


def test_positions_agree_with_float64():
    """B[e] = ((w0 m0 + w1 m1) + w2 m2) + w3 m3 in fp32: one product and at most three sums on every
    term, so |B^[e] - B[e]| <= g4 Bs[e], Bs[e] = sum_i |w_i m_i[e]|, g_k = k u / (1 - k u).  Then
    ((B0 x + B1 y) + B2 z) + B3: again one product and at most three sums on every term, on top of B's
    own four: |p' - p*| <= g8 S, S = Bs0 |x| + Bs1 |y| + Bs2 |z| + Bs3."""
    M = joint_matrices(9, 1, spread=180.0)
    v, n, J, W = soup(5000, 9, 2)
    ov, _ = mpt.skin_host(v, None, J, W, M)
    sk = W.any(1)
    B, Bs = blend64(M, J[sk], W[sk])
    ref, S = position_terms(B, Bs, v[sk])
    err = np.abs(ov[sk].astype(np.float64) - ref)
    print(f"positions: max error / (2^-24 S) = {(err / (U * S)).max():.3f} (bound 8)")
    assert (err <= gamma(8) * S).all()
    assert np.array_equal(ov[~sk], v[~sk])


@pytest.mark.parametrize("mirror", [False, True], ids=["proper", "mirrored"])
def test_normals_agree_with_float64(mirror):
    """The exact result is the direction of C n, C the cofactor matrix of A, the linear part of the
    exact blend (times the sign of det A).  Roundings of the definition, u = 2^-24, first order:
      a^ = fl32 blend              |a^_rc - A_rc| <= 4u Bs_rc (positions' docstring), and |A_rc| <= Bs_rc
      co^ = fl(fl(a b) - fl(c d))  each factor carries 4u of its Bs, each product rounds once and the
                                   difference once (u |ab - cd| <= u (|ab| + |cd|)):
                                   |co^_rc - C_rc| <= 10u P_rc,  P_rc = Bs Bs + Bs Bs over the same index
                                   pairs as the cofactor, and |C_rc| <= P_rc
      t_r = (N_r0 nx + N_r1 ny) + N_r2 nz   one product and at most two sums on every term:
                                   |t_r - (C n)_r| <= sum_j (10u P_rj + 3u |C_rj|) |n_j| <= 13u sum_j P_rj |n_j|
                                   so |t - C n| <= 13u |P|_F |n|
      |C n| >= s3(C) |n|, s3(C) = s2(A) s3(A)   (C's singular values are A's in pairs), so the direction of
                                   t is within 13u |P|_F / (s2(A) s3(A)) of C n's
      t_r / l, the reference's own normalisation, second-order terms: another 2u, as test_xform_host
    Bound per vertex: (13 |P|_F / (s2(A) s3(A)) + 2) * 2^-24 radians, A's singular values from numpy.
    The sign is that of det in fp32, whose error the same P bounds: |det^ - det| <= 13u sum_j Bs_0j P_0j;
    the test asserts that |det A| stays far above it, so no vertex is left out."""
    M = joint_matrices(12, 3, mirror)
    v, n, J, W = soup(6000, 12, 4)
    _, on = mpt.skin_host(v, n, J, W, M)
    sk = W.any(1)
    B, Bs = blend64(M, J[sk], W[sk])
    A, As = B[:, :, :3], Bs[:, :, :3]
    det = np.linalg.det(A)
    assert (np.sign(det) == (-1 if mirror else 1)).all()
    P = cofactor_abs(As)
    det_err = 13 * U * (As[:, 0, :] * P[:, 0, :]).sum(1)
    print(f"normals: min |det A| = {np.abs(det).min():.3f}, max det error bound {det_err.max():.2e}")
    assert (np.abs(det) > 0.05).all() and (np.abs(det) > 1000 * det_err).all()
    ref = np.einsum("vrc,vc->vr", np.linalg.inv(A).transpose(0, 2, 1), n[sk].astype(np.float64))
    ref /= np.linalg.norm(ref, axis=1, keepdims=True)
    sv = np.linalg.svd(A, compute_uv=False)
    bound = (13 * np.linalg.norm(P.reshape(len(P), -1), axis=1) / (sv[:, 1] * sv[:, 2]) + 2) * U
    got = angle(on[sk], ref)
    print(f"normals ({'mirrored' if mirror else 'proper'}): max angle {got.max():.3e} rad, bound there "
          f"{bound[got.argmax()]:.3e}, max angle / bound {(got / bound).max():.3f}")
    assert (got <= bound).all()
    assert (np.abs(np.linalg.norm(on[sk].astype(np.float64), axis=1) - 1) <= 4 * U).all()
    assert np.array_equal(on[~sk], n[~sk])


def test_negative_determinant_keeps_the_side():
    """A joint that mirrors in x, blended with a second mirroring joint: the plain cofactor matrix
    would flip the normal to the other side."""
    M = np.zeros((2, 3, 4), np.float32)
    M[0, :, :3] = np.diag([-1.0, 1.0, 1.0]) @ rot([0.2, 1.0, -0.4], 40.0)
    M[1, :, :3] = np.diag([-1.0, 1.0, 1.0]) @ rot([0.2, 1.0, -0.4], 55.0)
    v = np.zeros((4, 3), np.float32)
    n = np.array([[0, 0, 1], [1, 0, 0], [0.6, 0.8, 0], [0, -1, 0]], np.float32)
    J = np.tile(np.array([0, 1, 0, 0], np.int32), (4, 1))
    W = np.tile(np.array([0.75, 0.25, 0, 0], np.float32), (4, 1))
    _, on = mpt.skin_host(v, n, J, W, M)
    A = 0.75 * M[0, :, :3].astype(np.float64) + 0.25 * M[1, :, :3].astype(np.float64)
    assert np.linalg.det(A) < 0
    ref = n.astype(np.float64) @ np.linalg.inv(A)     # rows of (inverse(A)^T n)
    assert ((on.astype(np.float64) * ref).sum(1) > 0.99 * np.linalg.norm(ref, axis=1)).all()


def test_pass_through_is_byte_exact():
    v, n, J, W = soup(999, 3, 5)
    v[5] = [-0.0, 1.5, -0.0]
    v[7] = [-0.0, -0.0, 2.5]
    n[:, :] *= np.linspace(0.1, 3.0, len(n), dtype=np.float32)[:, None]      # non-unit normals
    n[11] = 0.0
    M = joint_matrices(3, 6)
    ident = np.zeros((3, 4), np.float32)
    ident[:, :3] = np.eye(3)
    M[1] = ident
    # 1. zero weights, +0 and -0, whatever the joints
    W[7] = [0.0, -0.0, 0.0, -0.0]
    zero = ~W.any(1)
    assert zero.sum() > 100 and zero[7]
    # 2. identity joints only, the weights not normalised
    only1 = np.arange(len(v)) % 7 == 5
    J[only1] = 1
    W[only1] = [0.3, 0.9, 0.0, 2.5]
    # 3. a non-identity joint with weight 0 next to identity joints
    mix = np.arange(len(v)) % 7 == 3
    J[mix] = [1, 0, 1, 2]
    W[mix] = [0.5, 0.0, 0.25, -0.0]
    assert only1[5] and not zero[5]
    ov, on = mpt.skin_host(v, n, J, W, M)
    keep = zero | only1 | mix
    assert ov[keep].tobytes() == v[keep].tobytes() and on[keep].tobytes() == n[keep].tobytes()
    assert np.signbit(ov[5, 0]) and np.signbit(ov[5, 2]) and np.signbit(ov[7, 0]) and np.signbit(ov[7, 1])
    moved = ~keep & (W[:, :] * (J != 1)).any(1)
    assert moved.sum() > 300 and (ov[moved] != v[moved]).any(1).all()
    # an all-identity pose: nothing changes, whatever the weights sum to
    W2 = (W * np.float32(1.7)).astype(np.float32)
    ov2, on2 = mpt.skin_host(v, n, J, W2, np.stack([ident] * 3))
    assert ov2.tobytes() == v.tobytes() and on2.tobytes() == n.tobytes()
    # a 4x4 is a 3x4 with its bottom row dropped
    M4 = np.zeros((3, 4, 4), np.float32)
    M4[:, :3] = M
    M4[:, 3] = [0, 0, 0, 1]
    ov4, on4 = mpt.skin_host(v, n, J, W, M4)
    assert ov4.tobytes() == ov.tobytes() and on4.tobytes() == on.tobytes()
    # a zero normal under a real blend passes through as well (l2 is 0)
    J[11], W[11] = [0, 2, 0, 0], [0.5, 0.5, 0, 0]
    assert np.array_equal(mpt.skin_host(v, n, J, W, M)[1][11], [0, 0, 0])
    # -0 in the matrix is not the identity: the vertex takes the arithmetic path, and -0 + 0 is +0
    M[1, 0, 1] = -0.0
    ov3, _ = mpt.skin_host(v, n, J, W, M)
    assert not np.signbit(ov3[5, 0])


def test_one_joint_equals_transform_host():
    """One joint with weight 1 in slot 0: B = ((1 m + 0 m') + 0 m'') + 0 m''' = m entry for entry when m
    has no -0 (x + 0 keeps every x but -0), so the positions are mpt_transform_host's bytes.  The
    normals differ by design (the cofactors here are fp32, there rounded from double): each within
    its own bound of the exact direction (test_normals_agree_with_float64 here and in
    test_xform_host), so within the sum of the two of each other."""
    M = joint_matrices(5, 8, spread=180.0)
    assert not (np.signbit(M) & (M == 0)).any()
    rng = np.random.default_rng(9)
    v, n, _, _ = soup(3000, 5, 10)
    ids = rng.integers(-1, 5, len(v)).astype(np.int32)
    J = rng.integers(0, 5, (len(v), 4)).astype(np.int32)
    J[:, 0] = np.maximum(ids, 0)
    W = np.zeros((len(v), 4), np.float32)
    W[ids >= 0, 0] = 1.0
    ov, on = mpt.skin_host(v, n, J, W, M)
    tv, tn = mpt.transform_host(v, n, ids, M)
    assert ov.tobytes() == tv.tobytes()
    assert np.array_equal(on[ids < 0], tn[ids < 0])
    A = M[:, :, :3].astype(np.float64)
    sv = np.linalg.svd(A, compute_uv=False)
    P = np.stack([cofactor_abs(np.abs(a)[None])[0] for a in A])
    skin_b = 13 * np.linalg.norm(P.reshape(len(P), -1), axis=1) / (sv[:, 1] * sv[:, 2]) + 2
    xform_b = 4 * np.sqrt(3) * sv[:, 0] / sv[:, -1] + 2
    mv = ids >= 0
    assert (angle(on, tn)[mv] <= ((skin_b + xform_b) * U)[ids[mv]]).all()


def test_refusals():
    v, n, J, W = soup(64, 2, 7)
    M = joint_matrices(2, 8)
    v0, n0 = v.copy(), n.copy()
    bad = M.copy()
    bad[1, 2, 1] = np.nan
    with pytest.raises(mpt.MptError) as e:
        mpt.skin_host(v, n, J, W, bad)
    assert e.value.code == -1 and "matrix" in str(e.value)
    bad = M.copy()
    bad[0, :, :3] = np.eye(3) * 3e38
    J2, W2 = J.copy(), W.copy()
    J2[1], W2[1] = 0, [1.0, 0.5, 0.5, 0.5]
    with pytest.raises(mpt.MptError) as e:
        mpt.skin_host(v, n, J2, W2, bad)
    assert e.value.code == -1 and "vertex" in str(e.value)
    assert not W[0].any()                         # an unskinned vertex: its slots are checked all the same
    for wrong in (2, -1):
        j2 = J.copy()
        j2[0, 3] = wrong
        with pytest.raises(mpt.MptError) as e:
            mpt.skin_host(v, n, j2, W, M)
        assert e.value.code == -1 and "joint index" in str(e.value)
    for wrong in (np.nan, np.inf):
        w2 = W.copy()
        w2[5, 2] = wrong
        with pytest.raises(mpt.MptError) as e:
            mpt.skin_host(v, n, J, w2, M)
        assert e.value.code == -1 and "weight" in str(e.value)
    assert np.array_equal(v, v0) and np.array_equal(n, n0)
    with pytest.raises(ValueError):
        mpt.skin_host(v, n, J, W, M[:, :2])
    with pytest.raises(ValueError):
        mpt.skin_host(v, n, J[:, :3], W[:, :3], M)
    with pytest.raises(ValueError):
        mpt.skin_host(v, n, J[:-1], W[:-1], M)
    L = mpt.lib()
    out = np.zeros_like(v)
    assert L.mpt_skin_host(None, None, J.ctypes.data, W.ctypes.data, len(v), M.ctypes.data, 2, out.ctypes.data, None) == -1
    assert L.mpt_skin_host(v.ctypes.data, None, J.ctypes.data, W.ctypes.data, 0, M.ctypes.data, 2, out.ctypes.data, None) == -1
    assert L.mpt_skin_host(v.ctypes.data, None, J.ctypes.data, W.ctypes.data, len(v), M.ctypes.data, 0, out.ctypes.data, None) == -1
    assert L.mpt_skin_host(v.ctypes.data, None, J.ctypes.data, W.ctypes.data, len(v), M.ctypes.data, 2, out.ctypes.data,
                           out.ctypes.data) == -1   # normals out without normals in


# ------------------------------------------------------------------------------------
# The glTF loader
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[3, 2], ids=["3joints_u16", "2joints_f32"])
def skinned(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("skinned") / "tube.gltf")
    synthetic.write_skinned_gltf(path, joints=request.param, normalized_weights=request.param == 3)
    return path, scene.load_gltf(path), request.param


def raw_tube(path):
    """The tube's own accessors and the file's nodes, float64."""
    with open(path) as f:
        g = json.load(f)
    bins = [scene._uri_bytes(os.path.dirname(path), b["uri"]) for b in g["buffers"]]
    att = g["meshes"][0]["primitives"][0]["attributes"]
    p = scene._accessor(g, bins, att["POSITION"]).astype(np.float64)
    j = scene._accessor(g, bins, att["JOINTS_0"]).astype(np.int64)
    w = scene._accessor(g, bins, att["WEIGHTS_0"]).astype(np.float64)
    ibm = scene._accessor(g, bins, g["skins"][0]["inverseBindMatrices"]).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    return g, p, j, w, ibm


def gltf_skinning(g, p, j, w, ibm, locals_):
    """glTF 2.0 §3.7.3.3 in float64: sum_i w_i global(joint_i) inverse_bind_i p, the skinned node's
    own transform ignored."""
    def world(ni):
        for pi, nd in enumerate(g["nodes"]):
            if ni in nd.get("children", []):
                return world(pi) @ locals_(ni)
        return locals_(ni)
    jm = np.stack([world(ni) @ ibm[k] for k, ni in enumerate(g["skins"][0]["joints"])])
    ph = np.concatenate([p, np.ones((len(p), 1))], 1)
    return np.einsum("vi,virc,vc->vr", w, jm[j], ph)[:, :3]


def test_loader_skin_shapes(skinned):
    path, sd, nj = skinned
    sk = sd.skin
    V = len(sd.vertices)
    assert sk is not None and sk.num_joints == nj
    assert sk.joints.dtype == np.int32 and sk.joints.shape == (V, 4) and sk.weights.dtype == np.float32 and sk.weights.shape == (V, 4)
    assert sk.joints.min() >= 0 and sk.joints.max() == nj - 1
    assert sk.joint_nodes.tolist() == list(range(1, nj + 1)) and sk.bind.shape == (nj, 4, 4) and sk.bind.dtype == np.float64
    assert sk.node_parents.tolist()[:nj + 1] == [-1, -1] + list(range(1, nj)) and sk.node_locals.shape == (len(sk.node_parents), 4, 4)
    tube = sd.vertex_object == 0
    assert tube.sum() == 56 and (~tube).sum() == 16
    assert not sk.weights[~tube].any() and (np.abs(sk.weights[tube].sum(1) - 1) <= 2 * U).all()
    assert ((sk.weights[tube] > 0).sum(1) == 2).any()               # blended vertices at the joints
    g, p, j, w, ibm = raw_tube(path)
    assert np.array_equal(sk.joints[tube], j) and np.array_equal(sk.weights[tube], w.astype(np.float32))
    # the mesh node's own transform is not the identity, and the rest pose has it
    W0 = sk.node_locals[0]
    assert not np.allclose(W0, np.eye(4))
    assert np.abs(sd.vertices[tube] - (p @ W0[:3, :3].T + W0[:3, 3])).max() <= 4 * U * 4


def skin_bound(sd, M64, tube):
    """|skin_host(fl32 M, fl32 v) - sum_i w_i M_i v| <= (g8 + 2u) S: the positions' bound, plus one
    rounding of every matrix entry and of every rest coordinate to fp32 (each u of its term of S);
    2^-40 S on top for the float64 evaluations themselves."""
    B, Bs = blend64(M64, sd.skin.joints[tube], sd.skin.weights[tube])
    return B, position_terms(B, Bs, sd.vertices[tube])[1] * (gamma(8) + 2 * U + 2.0 ** -40)


def test_loader_file_pose_reproduces_the_vertices(skinned):
    """skin_host of skin_matrices(sd) against sd.vertices.  Exactly, sum_i w_i M_i v = v + D v with D =
    sum_i w_i M_i - I (the inverse bind matrices are stored as fp32 and the weights need not sum to 1
    to the last bit, so D is not 0): the bound is skin_bound's plus |D| (|v|, 1) evaluated in float64."""
    path, sd, nj = skinned
    sk = sd.skin
    tube = sd.vertex_object == 0
    M = scene.skin_matrices(sd)
    assert M.dtype == np.float32 and M.shape == (nj, 3, 4)
    ov, on = mpt.skin_host(sd.vertices, sd.normals, sk.joints, sk.weights, M)
    B, bound = skin_bound(sd, M, tube)
    D = B - np.eye(4)[:3]
    x = np.abs(sd.vertices[tube].astype(np.float64))
    bound = bound + np.einsum("vrc,vc->vr", np.abs(D[:, :, :3]), x) + np.abs(D[:, :, 3])
    err = np.abs(ov[tube].astype(np.float64) - sd.vertices[tube])
    print(f"file pose: max error {err.max():.3e}, max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all() and bound.max() < 1e-5
    assert ov[~tube].tobytes() == sd.vertices[~tube].tobytes() and on[~tube].tobytes() == sd.normals[~tube].tobytes()
    assert (angle(on[tube], sd.normals[tube]) < 1e-5).all()


def test_loader_bent_pose_matches_the_gltf_equation(skinned):
    path, sd, nj = skinned
    sk = sd.skin
    tube = sd.vertex_object == 0
    g, p, j, w, ibm = raw_tube(path)
    bend = np.eye(4)
    bend[:3, :3] = rot([0.0, 0.3, 1.0], 50.0)
    bend[:3, 3] = sk.node_locals[2][:3, 3] + [0.05, 0.0, -0.02]
    root = sk.node_locals[1].copy()
    root[:3, :3] = root[:3, :3] @ rot([1.0, 0.0, 0.0], -15.0)
    over = {1: root, 2: bend}
    ref = gltf_skinning(g, p, j, w, ibm, lambda ni: over.get(ni, scene._node_matrix(g["nodes"][ni])))
    M = scene.skin_matrices(sd, over)
    ov, _ = mpt.skin_host(sd.vertices, sd.normals, sk.joints, sk.weights, M)
    # the exact value sum_i w_i M64_i v64 is the glTF equation's (M_i = global_i bind_i inverse(world), v = world p);
    # fl32 of M64 and of v64 are skin_bound's two input roundings
    _, bound = skin_bound(sd, M, tube)
    err = np.abs(ov[tube].astype(np.float64) - ref)
    print(f"bent pose: max error {err.max():.3e}, max error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.abs(ref - sd.vertices[tube]).max() > 0.2              # the pose bends the tube
    assert ov[~tube].tobytes() == sd.vertices[~tube].tobytes()
    # the file's pose through the same equation is the rest pose
    same = gltf_skinning(g, p, j, w, ibm, lambda ni: scene._node_matrix(g["nodes"][ni]))
    assert np.abs(same - sd.vertices[tube]).max() < 1e-5


def test_loader_refuses_a_second_influence_set(tmp_path):
    path = synthetic.write_skinned_gltf(str(tmp_path / "tube.gltf"))
    with open(path) as f:
        g = json.load(f)
    att = g["meshes"][0]["primitives"][0]["attributes"]
    att["JOINTS_1"], att["WEIGHTS_1"] = att["JOINTS_0"], att["WEIGHTS_0"]
    with open(path, "w") as f:
        json.dump(g, f)
    with pytest.raises(ValueError, match="JOINTS_1"):
        scene.load_gltf(path)


# sha256 of SceneData.vertices and SceneData.vertex_object as the loader gave them before it read skins
SHIPPED = {
    "cornell_pbr": (4287, "4502fe04ee2d5be7e8133428ee6258c0e8eb9521365931c25e478b9d0eaa8792",
                    "df13220e27a9123d25f9e7ccc6260844b09a8de04472b60258622f3f605f8db9"),
    "nested-dielectrics": (1150, "4dee5755527c7cf216fb936069a87be24d3a0412525834ac65d9d318569aafb5",
                           "7e0f4a2cbb60c831b80dc9f6883da543c7d8fe04e0e8c6b530cb09cceed0e279"),
    "nested-dielectrics-complex": (1787, "15d26990cb04463e7a5a8c7c2b9ff686c97799186d787de88810954353c87001",
                                   "610766d61b01320173a1220707a255d614a42b75cc23e5fe78e3280f51aee726"),
    "multi-dispersion": (27004, "b8688ee309cad4c540fad325289bd96d1bae44a1bc24d98f7c48e89d2330dfaf",
                         "c1ffe45b6087c6ac1cba039b10235e2f610b9e05b3e639c7bd7f1226dda66bba"),
}


@pytest.mark.parametrize("name", list(SHIPPED))
def test_shipped_scenes_are_unchanged_and_unskinned(name):
    sd = scene.load_scene(name)
    count, hv, ho = SHIPPED[name]
    assert sd.skin is None
    assert len(sd.vertices) == count
    assert hashlib.sha256(sd.vertices.tobytes()).hexdigest() == hv
    assert hashlib.sha256(sd.vertex_object.tobytes()).hexdigest() == ho
    with pytest.raises(ValueError):
        scene.skin_matrices(sd)


def test_skin_driver_built():
    """build() compiles the driver next to the others (plain g++ against libmpt)."""
    assert _build.SKIN_TEST.exists(), "skin driver not built (run __graft_entry__.build())"
    assert os.access(_build.SKIN_TEST, os.X_OK)
