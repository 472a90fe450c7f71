"""Per-object motion on the host (mpt_transform_host: the host loop of csrc/xform.h -- the
arithmetic the kernel of mpt_update_transforms shares), no GPU.

Checked against a numpy float64 restatement: positions and normals within bounds derived from the
roundings of the definition, the side of a mirrored normal, byte-exact pass-through of identity
objects and static vertices, the refusals; the glTF loader's SceneData.vertex_object; the C++
driver of tests/test_xform_host_cpp.py.  tests/test_xform.py runs the kernel against this loop
byte for byte.
"""
import os

import numpy as np
import pytest

import mpt
from mpt import _build, scene

U = 2.0 ** -24   # the unit roundoff of fp32


def rot(axis, deg):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) * c + s * K + (1 - c) * np.outer(axis, axis)


def random_matrices(k, seed, mirror=False):
    """[k, 3, 4] float32: rotations times scales in [0.5, 2] times shears up to 0.5, a translation."""
    rng = np.random.default_rng(seed)
    out = np.zeros((k, 3, 4), np.float32)
    for i in range(k):
        sc = np.diag(rng.uniform(0.5, 2.0, 3))
        if mirror:
            sc[i % 3, i % 3] *= -1.0
        sh = np.eye(3)
        sh[0, 1], sh[0, 2], sh[1, 2] = rng.uniform(-0.5, 0.5, 3)
        out[i, :, :3] = rot(rng.normal(size=3), rng.uniform(0, 360)) @ sc @ sh
        out[i, :, 3] = rng.uniform(-5, 5, 3)
    return out


def soup(v_count, k, seed, static_every=7):
    rng = np.random.default_rng(seed)
    v = (rng.random((v_count, 3)) * 8 - 4).astype(np.float32)
    n = rng.normal(size=(v_count, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    ids = rng.integers(0, k, v_count).astype(np.int32)
    ids[::static_every] = -1
    return v, n, ids


def angle(a, b):
    """Angle between rows of a and b, float64, accurate for small angles."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def test_positions_agree_with_float64():
    """Per component ((m0 x + m1 y) + m2 z) + m3 in fp32: three products and three sums, each result
    within one relative rounding; every partial sum is bounded by S = |m0 x| + |m1 y| + |m2 z| + |m3|
    up to the same roundings, so the error stays within 4 * 2^-24 * S (three roundings of the sums
    that carry a term to the end, plus the term's own product rounding, first order)."""
    M = random_matrices(9, 1)
    v, n, ids = soup(5000, 9, 2)
    ov, _ = mpt.transform_host(v, None, ids, M)
    mv = ids >= 0
    m = M[ids[mv]].astype(np.float64)
    x = v[mv].astype(np.float64)
    ref = np.einsum("vrc,vc->vr", m[:, :, :3], x) + m[:, :, 3]
    S = np.abs(m[:, :, :3] * x[:, None, :]).sum(2) + np.abs(m[:, :, 3])
    err = np.abs(ov[mv].astype(np.float64) - ref)
    print(f"positions: max error / (2^-24 S) = {(err / (U * S)).max():.3f} (bound 4)")
    assert (err <= 4 * U * S).all()
    assert np.array_equal(ov[~mv], v[~mv])


@pytest.mark.parametrize("mirror", [False, True], ids=["proper", "mirrored"])
def test_normals_agree_with_float64(mirror):
    """The exact result is the direction of C n, C the cofactor matrix of the linear part A (times the
    sign of det A: the direction of inverse(A)^T n).  Roundings of the definition, u = 2^-24:
      N = fl(C)                      one relative rounding per entry (C itself is made in double)
      t_r = (N_r0 nx + N_r1 ny) + N_r2 nz   three products and two sums: with N's own rounding at
                                     most four roundings on any term, |t_r - (C n)_r| <= 4u sum_j |C_rj| |n_j|
                                     <= 4u |C_r| |n| (Cauchy-Schwarz), so |t - C n| <= 4u |C|_F |n| <= 4 sqrt(3) u s1(C) |n|
      |C n| >= s3(C) |n|             so the direction of t is within 4 sqrt(3) u cond(C) of C n's,
                                     and cond(C) = cond(A) (C's singular values are A's in pairs)
      t_r / l                        one l for the three components: its own error scales the vector
                                     and turns nothing; the three divisions round once each, u
      the float64 reference's own normalisation and the second-order terms: another u is ample
    Bound: (4 sqrt(3) cond(A) + 2) * 2^-24 radians, cond(A) from numpy's SVD of each matrix."""
    M = random_matrices(12, 3, mirror)
    v, n, ids = soup(6000, 12, 4)
    _, on = mpt.transform_host(v, n, ids, M)
    mv = ids >= 0
    A = M[:, :, :3].astype(np.float64)
    assert (np.sign(np.linalg.det(A)) == (-1 if mirror else 1)).all()
    ref = np.einsum("vrc,vc->vr", np.linalg.inv(A).transpose(0, 2, 1)[ids[mv]], n[mv].astype(np.float64))
    ref /= np.linalg.norm(ref, axis=1, keepdims=True)
    sv = np.linalg.svd(A, compute_uv=False)
    bound = ((4 * np.sqrt(3) * sv[:, 0] / sv[:, -1] + 2) * U)[ids[mv]]
    got = angle(on[mv], ref)
    print(f"normals ({'mirrored' if mirror else 'proper'}): max angle {got.max():.3e} rad, bound there "
          f"{bound[got.argmax()]:.3e}, max angle / bound {(got / bound).max():.3f}")
    assert (got <= bound).all()
    assert (np.abs(np.linalg.norm(on[mv].astype(np.float64), axis=1) - 1) <= 4 * U).all()
    assert np.array_equal(on[~mv], n[~mv])


def test_negative_determinant_keeps_the_side():
    """A mirror in x: the plain cofactor matrix would flip the normal to the other side."""
    M = np.zeros((1, 3, 4), np.float32)
    M[0, :, :3] = np.diag([-1.0, 1.0, 1.0]) @ rot([0.2, 1.0, -0.4], 40.0)
    v = np.zeros((4, 3), np.float32)
    n = np.array([[0, 0, 1], [1, 0, 0], [0.6, 0.8, 0], [0, -1, 0]], np.float32)
    _, on = mpt.transform_host(v, n, np.zeros(4, np.int32), M)
    A = M[0, :, :3].astype(np.float64)
    assert np.linalg.det(A) < 0
    ref = n.astype(np.float64) @ np.linalg.inv(A)     # rows of (inverse(A)^T n)
    assert ((on.astype(np.float64) * ref).sum(1) > 0.99 * np.linalg.norm(ref, axis=1)).all()


def test_identity_and_static_pass_bytes_through():
    v, n, ids = soup(999, 3, 5)
    v[5] = [-0.0, 1.5, -0.0]
    n[:, :] *= np.linspace(0.1, 3.0, len(n), dtype=np.float32)[:, None]      # non-unit normals
    n[11] = 0.0
    M = random_matrices(3, 6)
    ident = np.zeros((3, 4), np.float32)
    ident[:, :3] = np.eye(3)
    M[1] = ident
    ids[5] = 1
    ov, on = mpt.transform_host(v, n, ids, M)
    keep = (ids == 1) | (ids == -1)
    assert keep.sum() > 300
    assert ov[keep].tobytes() == v[keep].tobytes() and on[keep].tobytes() == n[keep].tobytes()
    assert np.signbit(ov[5, 0]) and np.signbit(ov[5, 2])
    assert not np.array_equal(ov[~keep], v[~keep])
    # a 4x4 is a 3x4 with its bottom row dropped
    M4 = np.zeros((3, 4, 4), np.float32)
    M4[:, :3] = M
    M4[:, 3] = [0, 0, 0, 1]
    ov4, on4 = mpt.transform_host(v, n, ids, M4)
    assert ov4.tobytes() == ov.tobytes() and on4.tobytes() == on.tobytes()
    # a zero normal under a real transform passes through as well (l2 is 0)
    ids[11] = 0
    assert np.array_equal(mpt.transform_host(v, n, ids, M)[1][11], [0, 0, 0])
    # -0 in the matrix is not the identity: x + (-0)*y is still x here, but the call takes the arithmetic path
    M[1, 0, 1] = -0.0
    ov2, _ = mpt.transform_host(v, n, ids, M)
    assert not np.signbit(ov2[5, 0])


def test_refusals():
    v, n, ids = soup(64, 2, 7)
    M = random_matrices(2, 8)
    v0, n0 = v.copy(), n.copy()
    bad = M.copy()
    bad[1, 2, 1] = np.nan
    with pytest.raises(mpt.MptError) as e:
        mpt.transform_host(v, n, ids, bad)
    assert e.value.code == -1 and "matrix" in str(e.value)
    bad = M.copy()
    bad[0, :, :3] = np.eye(3) * 3e38
    with pytest.raises(mpt.MptError) as e:
        mpt.transform_host(v, n, ids, bad)
    assert e.value.code == -1 and "vertex" in str(e.value)
    for wrong in (2, -2):
        i2 = ids.copy()
        i2[3] = wrong
        with pytest.raises(mpt.MptError) as e:
            mpt.transform_host(v, n, i2, M)
        assert e.value.code == -1
    assert np.array_equal(v, v0) and np.array_equal(n, n0)
    with pytest.raises(ValueError):
        mpt.transform_host(v, n, ids, M[:, :2])
    L = mpt.lib()
    out = np.zeros_like(v)
    assert L.mpt_transform_host(None, None, ids.ctypes.data, len(v), M.ctypes.data, 2, out.ctypes.data, None) == -1
    assert L.mpt_transform_host(v.ctypes.data, None, ids.ctypes.data, 0, M.ctypes.data, 2, out.ctypes.data, None) == -1


def test_scene_loader_vertex_object():
    sd = scene.load_scene("cornell_pbr")
    vo = sd.vertex_object
    assert vo is not None and vo.dtype == np.int32 and vo.shape == (len(sd.vertices),)
    assert vo.min() == 0 and len(np.unique(vo)) == vo.max() + 1 and vo.max() >= 1   # two mesh nodes
    t = vo[sd.triangle_indices.reshape(-1, 3)]
    assert (t == t[:, :1]).all()


def test_xform_driver_built():
    """build() compiles the driver next to the others (plain g++ against libmpt)."""
    assert _build.XFORM_TEST.exists(), "xform driver not built (run __graft_entry__.build())"
    assert os.access(_build.XFORM_TEST, os.X_OK)
