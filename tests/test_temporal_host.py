"""Temporal accumulation on the host (mpt_primary_rays_host, mpt_temporal_host: csrc/temporal.h in a
host loop, no GPU) -- the definition of DESIGN.md §2 that k_primary_rays and k_temporal share bit
for bit (tests/test_temporal.py compares the kernels with this path).  The visibility comes from
the oracle's trace_closest on primary_rays_host's rays.

* restatement: temporal_host against a numpy restatement of the definition written here, run in
  float32 and in float64, over a chain of three calls (rotating camera, a quad moving before a wall,
  misses beside the wall, piecewise-constant normals).  Measure and method are test_denoise.py's:
  max |x - y| / (|y| + 1e-6) on per-sample means; the host path may differ from the float64 run by
  at most 8x the deviation between the two numpy runs.  The inputs keep every decision away from
  its threshold, asserted in float64 over every pixel first: fractional parts of (fx, fy) in [0.1,
  0.9], depth differences within half the tolerance or beyond twice it, 1 - cosine likewise.
  Measured here: the two numpy runs differ by 1.49e-07 on the first call and by 1.23e-04 and 8.06e-05
  on the next two (the measure is relative and the blend cancels), the host path differs from float64
  by 1.44e-07, 1.23e-04 and 8.06e-05: on these frames it equals the float32 run bit for bit.
* motion in closed form: a quad parallel to the image plane translated in its plane, and the camera
  translated; (fx, fy) against the float64 evaluation of the projection.  Measured: the largest
  error is 28.2 ulps of the pixel coordinate (geometry moved) and 29.3 ulps (camera moved) -- the
  coordinate is W / 2 times a clip-space value near 1, so a coordinate near 1 carries 20 times that
  value's rounding --; asserted: 4x the larger, rounded up to 30: 120 ulps, because float32 matrix
  products of this size vary by a few ulps with operand values.
* exact properties, bit for bit: first call and reset, alpha = 1, the cap, disocclusion, misses under
  a camera rotation, a point behind the previous camera, 1x1 and 2x1 frames, non-finite colours,
  every settings refusal.
* quality: 8 poses of the cornell box's sphere moving slowly, 1 spp each, 48x36 by the oracle;
  temporal + denoise_host against denoise_host alone on the last pose, MSE after the display
  tonemap against a 256-spp oracle image of that pose.  Measured with the default settings:
  MSE(temporal + denoise) / MSE(denoise) = 0.804 (0.00501 against 0.00624; the noisy frame: 0.02604),
  asserted: strictly lower, for the seeds used (cpu_seed_schedule's first eight)."""
import ctypes as C
import math

import numpy as np
import pytest

import mpt
from mpt import abi, scene

f32 = np.float32


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def settings(n=1, **kw):
    s = abi.TemporalSettings.default()
    s.sample_number = n
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def camera(position=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), w=40, h=30):
    info = dict(position=np.asarray(position, np.float64), lookat=np.asarray(lookat, np.float64), up=np.array([0.0, 1.0, 0.0]),
                hfov=0.6, aspect=w / h, znear=0.1, zfar=100.0)
    return scene.make_camera(info, w, h, jitter=False)


def mat(m, dt):
    return np.array([[m.m[i][j] for j in range(4)] for i in range(4)], f32).astype(dt)


def quad(x0, x1, y0, y1, z):
    return np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], f32)


def soup(quads, cornell):
    """A SceneData of quads (two triangles each) with the cornell box's materials."""
    v = np.concatenate(quads).astype(f32)
    idx = np.concatenate([4 * k + np.array([[0, 1, 2], [0, 2, 3]]) for k in range(len(quads))]).astype(np.int32)
    sd = scene.SceneData()
    sd.vertices = v
    sd.triangle_indices = idx.ravel()
    sd.normals = np.zeros_like(v)
    sd.has_normals = np.zeros(len(v), np.uint8)
    sd.texcoords = np.zeros((len(v), 2), f32)
    sd.materials = list(cornell.materials)
    sd.material_indices = np.zeros(len(idx), np.int32)
    sd.textures = list(cornell.textures)
    sd.camera_info = cornell.camera_info
    sd.name = "temporal quads"
    return sd.finalize()


def moved(sd, v):
    out = scene.SceneData()
    out.__dict__.update(sd.__dict__)
    out.vertices = np.ascontiguousarray(v, f32)
    return out


def visibility(oracle_lib, luts, sd, cam, w, h):
    """float32 [h, w, 4] {t, u, v, prim bits} of the centre rays, by the oracle's traversal."""
    o = oracle_lib.Oracle(sd, luts)
    prim, t, u, v = o.trace_closest(mpt.primary_rays_host(cam, w, h))
    o.close()
    return np.stack([t, u, v, prim.view(f32)], -1).reshape(h, w, 4)


def planes(w, h, n, seed, normal_regions=True):
    """Random colour sums up to 2 n, albedo in [0.05, 0.95], unit normals constant per region: any
    two regions' normals are equal or at least 60 degrees apart."""
    rng = np.random.default_rng(seed)
    color = (rng.uniform(0, 2 * n, size=(h, w, 3)) * rng.uniform(0, 1, size=(h, w, 1)) ** 2).astype(f32)
    albedo = rng.uniform(0.05, 0.95, size=(h, w, 3)).astype(f32)
    axes = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]], f32)
    ys, xs = np.mgrid[0:h, 0:w]
    region = ((xs * 2) // max(w, 1) + 2 * ((ys * 2) // max(h, 1))) if normal_regions else np.zeros((h, w), int)
    return color, albedo, axes[region]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def no_history(s, color, albedo):
    """output(prepare(color)) of csrc/denoise.h in float32: what a pixel without history shows."""
    n = f32(s.sample_number)
    with np.errstate(all="ignore"):
        m = color.astype(f32) / n
        m = np.where(np.isnan(m), f32(0), np.minimum(np.maximum(m, f32(0)), f32(1.0e35))).astype(f32)
        a = np.where(np.isfinite(albedo), albedo, 0).astype(f32)
        d = np.maximum(a, f32(0.01)) if s.use_albedo else np.ones_like(a)
        return (m / d) * d * n


# ------------------------------------------------------------------------------------------
# numpy restatement of the definition, in dtype dt
# ------------------------------------------------------------------------------------------
def mat_point(m, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    xt = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2] * z) + m[0, 3]
    yt = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2] * z) + m[1, 3]
    zt = ((m[2, 0] * x + m[2, 1] * y) + m[2, 2] * z) + m[2, 3]
    wt = ((m[3, 0] * x + m[3, 1] * y) + m[3, 2] * z) + m[3, 3]
    one = np.ones_like(wt)
    iw = np.where(np.abs(wt) < 1.0e-10, one, one / np.where(wt == 0, one, wt))
    return np.stack([xt * iw, yt * iw, zt * iw], -1), wt


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def restate(s, cam, prev_cam, vis, idx, pos, prev_pos, color, albedo, normals, history, dt, margins=None):
    """One call of DESIGN.md §2 on [H, W, .] arrays in dtype dt -> (output, motion[..., :3], history
    A, history B).  margins (a dict, float64 runs): what the decisions' distances from their
    thresholds were."""
    H, W = vis.shape[:2]
    n = dt(s.sample_number)
    with np.errstate(all="ignore"):
        m = color.astype(dt) / n
        m = np.where(np.isnan(m), dt(0), np.minimum(np.maximum(m, dt(0)), dt(f32(1.0e35))))
        a = np.where(np.isfinite(albedo), albedo, 0).astype(dt)
        nr = np.where(np.isfinite(normals), normals, 0).astype(dt)
        d = np.maximum(a, dt(f32(0.01))) if s.use_albedo else np.ones_like(a)
        e = m / d
        iv, ip, ivp = mat(cam.inverse_view, dt), mat(cam.inverse_projection, dt), mat(prev_cam.inverse_view, dt)
        vp = mat(prev_cam.view_projection, dt)
        ys, xs = np.mgrid[0:H, 0:W]
        xn = (xs.astype(dt) + dt(0.5)) / dt(W) * dt(2) - dt(1)
        yn = (ys.astype(dt) + dt(0.5)) / dt(H) * dt(2) - dt(1)
        zero = np.zeros((1, 3), dt)
        o = mat_point(iv, zero)[0][0]
        o_prev = mat_point(ivp, zero)[0][0]
        pvs = mat_point(ip, np.stack([xn, yn, -np.ones_like(xn)], -1))[0]
        pws = mat_point(iv, pvs)[0]
        t = pws - o
        dirs = t / np.sqrt(dot(t, t))[..., None]
        prim = np.ascontiguousarray(vis[..., 3]).view(np.int32)
        hit = prim >= 0
        tri = idx.reshape(-1, 3)[np.where(hit, prim, 0)]
        u, v = vis[..., 1].astype(dt), vis[..., 2].astype(dt)
        u, v = np.where(hit, u, dt(0)), np.where(hit, v, dt(0))
        w = dt(1) - u - v

        def bary(p):
            p = p.reshape(-1, 3).astype(dt)
            return (w[..., None] * p[tri[..., 0]] + u[..., None] * p[tri[..., 1]]) + v[..., None] * p[tri[..., 2]]

        P, Qh = bary(pos), bary(prev_pos)
        Q = np.where(hit[..., None], Qh, o_prev + dirs)
        dP, dQ = P - o, Qh - o_prev
        depth_cur = np.where(hit, np.sqrt(dot(dP, dP)), dt(-1))
        depth_exp = np.where(hit, np.sqrt(dot(dQ, dQ)), dt(-1))
        ss, wc = mat_point(vp, Q)
        ok = wc > 0
        fx = ((ss[..., 0] + dt(1)) * dt(0.5)) * dt(W) - dt(0.5)
        fy = ((ss[..., 1] + dt(1)) * dt(0.5)) * dt(H) - dt(0.5)
        fx, fy = np.where(ok, fx, dt(-1)), np.where(ok, fy, dt(-1))
        have = ok & (history is not None) & (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
        e_h, len_h, wsum = np.zeros_like(e), np.zeros((H, W), dt), np.zeros((H, W), dt)
        anyv = np.zeros((H, W), bool)
        if history is not None:
            ha, hb = (np.asarray(p).astype(dt) for p in history)
            flx, fly = np.floor(np.where(have, fx, 0)), np.floor(np.where(have, fy, 0))
            x0, y0 = flx.astype(int), fly.astype(int)
            tx, ty = fx - flx, fy - fly
            if margins is not None:
                margins["frac"] = np.concatenate([(fx - np.floor(fx))[ok], (fy - np.floor(fy))[ok]])
                margins["depth"], margins["cos"] = [], []
            wx, wy = [dt(1) - tx, tx], [dt(1) - ty, ty]
            num = np.zeros_like(e)
            for j in range(2):
                for i in range(2):
                    qx, qy = x0 + i, y0 + j
                    inside = have & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    qa, qb = ha[cy, cx], hb[cy, cx]
                    len_q, depth_q = qb[..., 3], qa[..., 3]
                    cand = inside & (len_q >= 1)
                    dd = np.abs(depth_q - depth_exp)
                    c = dot(nr, qb[..., :3])
                    both = cand & hit & (depth_q >= 0)
                    valid = np.where(hit, both & (dd <= dt(f32(s.depth_tolerance)) * depth_exp) & (c >= dt(f32(s.normal_threshold))),
                                     cand & (depth_q < 0))
                    if margins is not None:
                        margins["depth"].append((dd / (dt(f32(s.depth_tolerance)) * depth_exp))[both])
                        margins["cos"].append(((1 - c) / (1 - dt(f32(s.normal_threshold))))[both])
                    wq = wx[i] * wy[j]
                    num = np.where(valid[..., None], num + wq[..., None] * qa[..., :3], num)
                    wsum = np.where(valid, wsum + wq, wsum)
                    len_h = np.where(valid, np.where(anyv, np.minimum(len_h, len_q), len_q), len_h)
                    anyv |= valid
            have = anyv & (wsum > 0)
            e_h = num / np.where(have, wsum, dt(1))[..., None]
        else:
            have = np.zeros((H, W), bool)
        al = np.maximum(dt(f32(s.alpha)), dt(1) / (len_h + dt(1)))
        blend = np.where((al < 1)[..., None], e_h + al[..., None] * (e - e_h), e)
        e_new = np.where(have[..., None], blend, e)
        len_new = np.where(have, np.minimum(len_h + dt(1), dt(s.max_history)), dt(1))
        out = e_new * d * n
        return (out, np.stack([fx, fy, depth_exp], -1), np.concatenate([e_new, depth_cur[..., None]], -1),
                np.concatenate([nr, len_new[..., None]], -1))


def rel(x, y):
    """max |x - y| / (|y| + 1e-6)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y) / (np.abs(y) + 1e-6))) if x.size else 0.0


# ------------------------------------------------------------------------------------------
# The scene of the restatement, closed-form and disocclusion tests: a wall at z = -6 that leaves
# the right of the view empty, a quad at z = -3 before it
# ------------------------------------------------------------------------------------------
W0, H0 = 40, 30
WALL = quad(-30.0, 0.9, -30.0, 30.0, -6.0)
FRONT = quad(-0.35, -0.05, -0.25, 0.2, -3.0)


def px_per_unit(cam, w, z):
    """Pixels per world unit at view depth z (a camera looking down -z)."""
    m = mat(cam.view_projection, np.float64)
    p = mat_point(m, np.array([[0.0, 0.0, -z], [1.0, 0.0, -z]]))[0]
    return abs(p[1, 0] - p[0, 0]) * w / 2


@pytest.fixture(scope="module")
def chain(cornell, luts, oracle_lib):
    """Three calls: the camera turns a little further before each (0.31 / 0.27 pixels of yaw and
    pitch per call at the image centre), the front quad moves 0.2 pixels to the right per call."""
    w, h = W0, H0
    cam0 = camera(w=w, h=h)
    step = 0.2 / px_per_unit(cam0, w, 3.0)
    per_px = 1.0 / px_per_unit(cam0, w, 1.0)          # the tangent of one pixel's angle
    calls = []
    for k in range(3):
        cam = camera(lookat=(math.tan(0.31 * per_px * k), math.tan(-0.27 * per_px * k), -1.0), w=w, h=h)
        v = np.concatenate([WALL, FRONT + f32([step * k, 0, 0])]).astype(f32)
        sd = soup([v[:4], v[4:]], cornell)
        vis = visibility(oracle_lib, luts, sd, cam, w, h)
        calls.append(dict(cam=cam, pos=v, idx=np.asarray(sd.triangle_indices, np.int32), vis=vis, planes=planes(w, h, 3, 20 + k)))
    for c in calls:
        c["vis"].setflags(write=False)
    return calls


def run_chain(chain, s, how):
    """The three calls through `how` (temporal_host or a restatement): a list of (out, motion, A, B)."""
    res, hist = [], None
    for k, c in enumerate(chain):
        p = chain[max(k - 1, 0)]
        r = how(s, c["cam"], p["cam"], c["vis"], c["idx"], c["pos"], p["pos"], *c["planes"], hist)
        hist = (r[2], r[3])
        res.append(r)
    return res


def test_host_path_matches_restatement(chain):
    s = settings(3, depth_tolerance=0.1, normal_threshold=0.9, alpha=0.2)
    n = s.sample_number
    prims = np.concatenate([np.unique(c["vis"][..., 3].view(np.int32)) for c in chain])
    assert set(prims.tolist()) >= {-1, 0, 2}, "wall, front quad and misses are all seen"
    margins = [dict() for _ in chain]
    it = iter(margins)
    r64 = run_chain(chain, s, lambda *a: restate(*a, np.float64, next(it)))
    # no decision sits near its threshold, over every pixel and tap (float64)
    for k, mg in enumerate(margins[1:], 1):
        fr = mg["frac"]
        assert fr.size == 2 * W0 * H0 and fr.min() >= 0.1 and fr.max() <= 0.9, (k, fr.min(), fr.max())
        dr, cr = np.concatenate(mg["depth"]), np.concatenate(mg["cos"])
        assert dr.size and ((dr <= 0.5) | (dr >= 2.0)).all(), (k, dr[(dr > 0.5) & (dr < 2.0)])
        assert (dr <= 0.5).any() and (dr >= 2.0).any(), "both sides of the depth test are taken"
        assert ((cr <= 0.5) | (cr >= 2.0)).all(), (k, cr[(cr > 0.5) & (cr < 2.0)])
        assert (cr <= 0.5).any() and (cr >= 2.0).any(), "both sides of the normal test are taken"
    r32 = run_chain(chain, s, lambda *a: restate(*a, np.float32))
    got = run_chain(chain, s, mpt.temporal_host)
    for k in range(3):
        lens = got[k][3][..., 3]
        assert lens.max() == k + 1 and set(np.unique(lens).tolist()) <= set(range(1, k + 2))
        dev = max(rel(r32[k][0] / n, r64[k][0] / n), rel(r64[k][0] / n, r32[k][0].astype(np.float64) / n))
        err = rel(got[k][0].astype(np.float64) / n, r64[k][0] / n)
        print(f"call {k}: float32 vs float64 restatement {dev:.3g}, host path vs float64 {err:.3g}, "
              f"host path == float32 run: {same(got[k][0], r32[k][0])}")
        assert np.isfinite(got[k][0]).all()
        assert err <= 8 * dev, f"call {k}: host path {err:.3g} from float64, the numpy runs {dev:.3g} apart"
        # the planes that carry decisions agree exactly: lengths, primitive ids, depth signs
        assert np.array_equal(got[k][3][..., 3], r64[k][3][..., 3])
        assert same(got[k][1][..., 3], chain[k]["vis"][..., 3])
        assert np.abs(got[k][1][..., :3] - r64[k][1]).max() <= 1e-4 and rel(got[k][2], r64[k][2]) <= 8 * dev + 1e-5


# ------------------------------------------------------------------------------------------
# Motion in closed form
# ------------------------------------------------------------------------------------------
def ulps(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), 1.0).astype(f32)).astype(np.float64)))


MEASURED_ULPS = 30   # the largest of the two cases below, as measured; asserted: 4x


@pytest.mark.parametrize("what", ["geometry", "camera"])
def test_motion_in_closed_form(cornell, luts, oracle_lib, what):
    w, h = W0, H0
    cam1 = camera(w=w, h=h)
    ppu = px_per_unit(cam1, w, 3.0)
    dx, dy = 2.3 / ppu, -1.6 / ppu                # the quad moves 2.3 pixels right and 1.6 down the rows
    front = quad(-0.4, 0.2, -0.3, 0.25, -3.0)
    if what == "geometry":
        cam0, prev = cam1, front - f32([dx, dy, 0])
    else:                                          # the camera moved the other way: the same image motion
        cam0, prev = camera(position=(dx, dy, 0.0), lookat=(dx, dy, -1.0), w=w, h=h), front
    sd = soup([front], cornell)
    vis = visibility(oracle_lib, luts, sd, cam1, w, h)
    hit = vis[..., 3].view(np.int32) >= 0
    assert 100 < hit.sum() < w * h
    idx = np.asarray(sd.triangle_indices, np.int32)
    pl = planes(w, h, 1, 3)
    out, motion, ha, hb = mpt.temporal_host(settings(1), cam1, cam0, vis, idx, front, prev, *pl)
    r64 = restate(settings(1), cam1, cam0, vis, idx, front, prev, *pl, None, np.float64)[1]
    worst = max(ulps(motion[..., 0], r64[..., 0]), ulps(motion[..., 1], r64[..., 1]))
    print(f"{what} moved: largest error of (fx, fy) {worst:.2f} ulps of the pixel coordinate")
    assert worst <= 4 * MEASURED_ULPS
    # and the float64 evaluation is the closed form: every pixel of the quad came from 2.3 pixels to
    # the left, 1.6 rows further on
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.abs(r64[..., 0][hit] - (xs[hit] - 2.3)).max() < 2e-3
    assert mat(cam1.view_projection, np.float64)[1, 1] > 0          # world +y is the next row
    assert np.abs(r64[..., 1][hit] - (ys[hit] + 1.6)).max() < 2e-3
    assert np.abs(r64[..., 2][hit] - motion[..., 2][hit]).max() < 1e-5      # the expected depth
    assert (motion[..., 2][~hit] == -1).all()


# ------------------------------------------------------------------------------------------
# Exact properties
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def still(cornell, luts, oracle_lib):
    """Wall and quad, nothing moves: (camera, vertices, indices, visibility)."""
    cam = camera(w=W0, h=H0)
    v = np.concatenate([WALL, FRONT]).astype(f32)
    sd = soup([WALL, FRONT], cornell)
    vis = visibility(oracle_lib, luts, sd, cam, W0, H0)
    vis.setflags(write=False)
    return cam, v, np.asarray(sd.triangle_indices, np.int32), vis


def test_settings_default():
    s = abi.TemporalSettings()
    assert mpt.lib().mpt_temporal_settings_default(C.byref(s)) == abi.OK
    assert bytes(s) == bytes(abi.TemporalSettings.default()) and C.sizeof(s) == 24
    assert (s.sample_number, s.max_history, s.use_albedo) == (1, 32, 1)
    assert (s.alpha, s.depth_tolerance, s.normal_threshold) == (float(f32(0.1)), float(f32(0.02)), float(f32(0.9)))
    for n in ("mpt_temporal_settings_default", "mpt_set_temporal", "mpt_temporal_accumulate", "mpt_temporal_reset",
              "mpt_get_temporal", "mpt_denoise_temporal", "mpt_primary_rays_host", "mpt_temporal_host"):
        assert n in mpt.SYMBOLS and hasattr(mpt.lib(), n)


def test_primary_rays_are_the_camera_rays_without_jitter(still):
    cam = still[0]
    rays = mpt.primary_rays_host(cam, W0, H0).reshape(H0, W0, 8)
    iv, ip = mat(cam.inverse_view, f32), mat(cam.inverse_projection, f32)
    ys, xs = np.mgrid[0:H0, 0:W0]
    xn = (xs.astype(f32) + f32(0.5)) / f32(W0) * f32(2) - f32(1)
    yn = (ys.astype(f32) + f32(0.5)) / f32(H0) * f32(2) - f32(1)
    o = mat_point(iv, np.zeros((1, 3), f32))[0][0]
    t = mat_point(iv, mat_point(ip, np.stack([xn, yn, -np.ones_like(xn)], -1))[0])[0] - o
    d = t / np.sqrt(dot(t, t))[..., None]
    assert same(rays[..., 0:3], np.broadcast_to(o, (H0, W0, 3))) and same(rays[..., 4:7], d)
    assert (rays[..., 3] == 0).all() and np.isposinf(rays[..., 7]).all()


def test_first_call_reset_alpha_one_and_the_cap(still):
    cam, v, idx, vis = still
    pl = [planes(W0, H0, 2, k) for k in range(4)]
    s = settings(2)
    first = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *pl[0])
    assert same(first[0], no_history(s, pl[0][0], pl[0][1])) and (first[3][..., 3] == 1).all()
    assert same(first[3][..., :3], pl[0][2]) and same(first[2][..., 3], first[1][..., 2])    # normals; depth = expected depth
    hist = (first[2], first[3])
    # a second call with the same normals: every pixel finds itself, length 2
    c1 = (pl[1][0], pl[1][1], pl[0][2])
    second = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *c1, hist)
    assert (second[3][..., 3] == 2).all() and not same(second[0], no_history(s, c1[0], c1[1]))
    # alpha = 1: the current frame alone, whatever the history holds
    one = mpt.temporal_host(settings(2, alpha=1.0), cam, cam, vis, idx, v, v, *c1, hist)
    assert same(one[0], no_history(s, c1[0], c1[1])) and (one[3][..., 3] == 2).all()
    # the call after a reset is a first call
    again = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *c1)
    assert same(again[0], no_history(s, c1[0], c1[1])) and (again[3][..., 3] == 1).all()
    # max_history caps the length
    sc, h = settings(2, max_history=3), None
    lens = []
    for k in range(5):
        r = mpt.temporal_host(sc, cam, cam, vis, idx, v, v, pl[k % 4][0], pl[k % 4][1], pl[0][2], h)
        h = (r[2], r[3])
        lens.append(float(r[3][..., 3].max()))
        assert (r[3][..., 3] == lens[-1]).all()
    assert lens == [1, 2, 3, 3, 3]
    assert np.array_equal(mpt.temporal_host(settings(2, max_history=1), cam, cam, vis, idx, v, v, *c1, hist)[3][..., 3],
                          np.ones((H0, W0), f32))


def test_disocclusion(cornell, luts, oracle_lib):
    """A bright quad moves 6 pixels sideways before a wall: what it uncovers has no history, what
    it covers follows it."""
    w, h = W0, H0
    cam = camera(w=w, h=h)
    shift = 6.0 / px_per_unit(cam, w, 3.0)
    before, after = FRONT, FRONT + f32([shift, 0, 0])
    vis0 = visibility(oracle_lib, luts, soup([WALL, before], cornell), cam, w, h)
    vis1 = visibility(oracle_lib, luts, soup([WALL, after], cornell), cam, w, h)
    idx = np.asarray(soup([WALL, before], cornell).triangle_indices, np.int32)
    v0, v1 = np.concatenate([WALL, before]).astype(f32), np.concatenate([WALL, after]).astype(f32)
    on0, on1 = vis0[..., 3].view(np.int32) >= 2, vis1[..., 3].view(np.int32) >= 2
    s = settings(1)
    nrm = np.broadcast_to(f32([0, 0, 1]), (h, w, 3))
    c0 = np.where(on0[..., None], f32(5.0), f32(0.25)) * np.ones((h, w, 3), f32)
    c1 = np.where(on1[..., None], f32(5.0), f32(0.25)) * np.ones((h, w, 3), f32)
    alb = np.full((h, w, 3), 0.5, f32)
    r0 = mpt.temporal_host(s, cam, cam, vis0, idx, v0, v0, c0, alb, nrm)
    r1 = mpt.temporal_host(s, cam, cam, vis1, idx, v1, v0, c1, alb, nrm, (r0[2], r0[3]))
    lens = r1[3][..., 3]
    wall1 = vis1[..., 3].view(np.int32) >= 0
    # (a reprojected position is an integer up to rounding, so a neighbour's history may come in
    # with a weight near zero: "uncovered" are the pixels whose whole 3 x 3 neighbourhood was quad)
    inner = on0.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(on0, (dy, dx), (0, 1))
    uncovered = inner & ~on1
    assert uncovered.sum() >= 20 and on1.sum() >= 50
    assert (lens[uncovered] == 1).all() and same(r1[0][uncovered], no_history(s, c1, alb)[uncovered])
    assert (lens[on1] == 2).all(), "every pixel of the quad finds the quad"
    assert np.abs(r1[1][..., 0][on1] - (np.mgrid[0:h, 0:w][1][on1] - 6.0)).max() < 1e-3     # it came from 6 pixels to the left
    assert rel(r1[0][on1], c1[on1]) <= 1e-6, "the quad's history is the quad's colour, not the wall's"
    rest = wall1 & ~on1 & ~on0
    assert (lens[rest] == 2).all() and rel(r1[0][rest], c1[rest]) <= 1e-6


def test_misses_reproject_by_direction_and_do_not_mix_with_hits(cornell, luts, oracle_lib):
    w, h = W0, H0
    cam0 = camera(w=w, h=h)
    per_px = 1.0 / px_per_unit(cam0, w, 1.0)
    cam1 = camera(lookat=(math.tan(3.0 * per_px), 0.0, -1.0), w=w, h=h)      # the view turns: the image moves ~3 pixels
    sd = soup([WALL], cornell)
    v, idx = WALL.astype(f32), np.asarray(sd.triangle_indices, np.int32)
    vis0, vis1 = visibility(oracle_lib, luts, sd, cam0, w, h), visibility(oracle_lib, luts, sd, cam1, w, h)
    miss0, miss1 = vis0[..., 3].view(np.int32) < 0, vis1[..., 3].view(np.int32) < 0
    assert miss0.sum() > 50 and miss1.sum() > 50 and (~miss1).sum() > 50
    s = settings(1)
    alb, nrm = np.full((h, w, 3), 0.5, f32), np.broadcast_to(f32([0, 0, 1]), (h, w, 3))
    c0 = np.where(miss0[..., None], f32(0.125), f32(3.0)) * np.ones((h, w, 3), f32)
    c1 = np.where(miss1[..., None], f32(0.125), f32(3.0)) * np.ones((h, w, 3), f32)
    r0 = mpt.temporal_host(s, cam0, cam0, vis0, idx, v, v, c0, alb, nrm)
    assert (r0[2][..., 3][miss0] == -1).all() and (r0[2][..., 3][~miss0] > 0).all()
    r1 = mpt.temporal_host(s, cam1, cam0, vis1, idx, v, v, c1, alb, nrm, (r0[2], r0[3]))
    fx, lens = r1[1][..., 0], r1[3][..., 3]
    xs = np.mgrid[0:h, 0:w][1]
    shift = (fx - xs)[miss1]
    assert 2.0 < np.abs(shift).min() and np.abs(shift).max() < 6.0 and (r1[1][..., 2][miss1] == -1).all()
    # a miss blends only with misses and a hit only with hits: both colours stay pure
    assert rel(r1[0][miss1], c1[miss1]) <= 1e-6 and rel(r1[0][~miss1], c1[~miss1]) <= 1e-6
    inside = (fx >= 0) & (fx <= w - 1)
    assert (lens[miss1 & inside] == 2).any() and (lens[~miss1 & inside] == 2).any()
    assert set(np.unique(lens).tolist()) <= {1.0, 2.0}


def test_a_point_behind_the_previous_camera_has_no_history(still):
    cam, v, idx, vis = still
    behind = camera(position=(0.0, 0.0, -20.0), lookat=(0.0, 0.0, -21.0), w=W0, h=H0)    # past the wall, looking away
    pl = planes(W0, H0, 1, 4, normal_regions=False)
    s = settings(1)
    r0 = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *pl)
    r1 = mpt.temporal_host(s, cam, behind, vis, idx, v, v, *pl, (r0[2], r0[3]))
    hit = vis[..., 3].view(np.int32) >= 0
    assert hit.sum() > 100
    assert (r1[1][..., 0][hit] == -1).all() and (r1[1][..., 1][hit] == -1).all()
    assert (r1[3][..., 3][hit] == 1).all() and same(r1[0][hit], no_history(s, pl[0], pl[1])[hit])


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1)])
def test_smallest_frames(cornell, luts, oracle_lib, w, h):
    cam = camera(w=w, h=h)
    sd = soup([quad(-30, 30, -30, 30, -6.0)], cornell)
    v, idx = np.asarray(sd.vertices, f32), np.asarray(sd.triangle_indices, np.int32)
    vis = visibility(oracle_lib, luts, sd, cam, w, h)
    assert (vis[..., 3].view(np.int32) >= 0).all()
    pl0, pl1 = planes(w, h, 2, 1, False), planes(w, h, 2, 2, False)
    s = settings(2)
    r0 = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *pl0)
    r1 = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *pl1, (r0[2], r0[3]))
    assert r1[0].shape == (h, w, 3) and (r1[3][..., 3] == 2).all()
    want = restate(s, cam, cam, vis, idx, v, v, *pl1, (r0[2], r0[3]), np.float64)[0]
    assert rel(r1[0], want) <= 1e-5
    assert np.abs(r1[1][..., 0] - np.arange(w)).max() < 1e-4 and np.abs(r1[1][..., 1]).max() < 1e-4


def test_non_finite_colours_are_sanitised_as_in_the_denoiser(still):
    cam, v, idx, vis = still
    color, albedo, normals = planes(W0, H0, 4, 6, False)
    clean = [color.copy(), albedo.copy(), normals.copy()]
    color[10, 10, 0], clean[0][10, 10, 0] = np.nan, 0.0
    color[12, 30, 1], clean[0][12, 30, 1] = np.inf, f32(1.0e35) * f32(4)
    color[20, 7, 2], clean[0][20, 7, 2] = -3.0, 0.0
    albedo[5, 5, 1], clean[1][5, 5, 1] = np.nan, 0.0
    albedo[25, 33, 0], clean[1][25, 33, 0] = np.inf, 0.0
    normals[15, 20, 2], clean[2][15, 20, 2] = -np.inf, 0.0
    s = settings(4)
    hist = None
    for _ in range(2):
        a = mpt.temporal_host(s, cam, cam, vis, idx, v, v, color, albedo, normals, hist)
        b = mpt.temporal_host(s, cam, cam, vis, idx, v, v, *clean, hist)
        assert all(np.isfinite(p).all() for p in (a[0], a[1][..., :3], a[2], a[3])) and all(same(x, y) for x, y in zip(a, b))
        hist = (a[2], a[3])


BAD = [dict(sample_number=0), dict(sample_number=-3), dict(max_history=0), dict(max_history=1025), dict(alpha=0.0), dict(alpha=-0.5),
       dict(alpha=1.5), dict(alpha=float("nan")), dict(depth_tolerance=0.0), dict(depth_tolerance=-1.0),
       dict(depth_tolerance=float("inf")), dict(depth_tolerance=float("nan")), dict(normal_threshold=-1.5),
       dict(normal_threshold=1.5), dict(normal_threshold=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_settings_validation(still, bad):
    cam, v, idx, vis = still
    with pytest.raises(mpt.MptError) as e:
        mpt.temporal_host(settings(1, **bad), cam, cam, vis, idx, v, v, *planes(W0, H0, 1, 1))
    assert e.value.code == abi.ERR_INVALID_ARGUMENT and list(bad)[0] in str(e.value)


def test_host_arguments_are_checked(still):
    cam, v, idx, vis = still
    pl = planes(W0, H0, 1, 1)
    far = vis.copy()
    far[0, 0, 3] = np.int32(7).view(f32)
    with pytest.raises(mpt.MptError, match="primitive id"):
        mpt.temporal_host(settings(1), cam, cam, far, idx, v, v, *pl)
    with pytest.raises(mpt.MptError, match="vertex index"):
        mpt.temporal_host(settings(1), cam, cam, vis, idx + 5, v, v, *pl)
    a = abi.TemporalHostArgs()
    assert mpt.lib().mpt_temporal_host(C.byref(a)) == abi.ERR_INVALID_ARGUMENT
    assert mpt.lib().mpt_temporal_host(None) == abi.ERR_INVALID_ARGUMENT
    assert mpt.lib().mpt_primary_rays_host(C.byref(cam), 0, 3, pl[0].ctypes.data) == abi.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------
# Quality
# ------------------------------------------------------------------------------------------
def tonemapped(mean):
    return (1.0 - np.exp(-np.maximum(np.asarray(mean, np.float64), 0.0) * 1.8)) ** (1 / 2.2)


QW, QH, POSES = 48, 36, 8


def quality_poses(cornell):
    """The cornell box with its sphere (the glTF's second mesh) 0.015 further along x in every pose."""
    v = np.asarray(cornell.vertices, f32).reshape(-1, 3)
    sphere = np.asarray(cornell.vertex_object) == 1
    assert 1000 < sphere.sum() < len(v)
    return [np.where(sphere[:, None], v + f32([0.015 * k, 0, 0]), v).astype(f32) for k in range(POSES)]


def test_temporal_then_denoise_beats_denoise_alone(cornell, luts, oracle_lib):
    cam = scene.make_camera(cornell.camera_info, QW, QH)
    seeds = [seed for _, seed in scene.cpu_seed_schedule(POSES)]
    poses = quality_poses(cornell)
    idx = np.asarray(cornell.triangle_indices, np.int32)
    s, d = abi.TemporalSettings.default(), abi.DenoiseSettings.default()
    hist, out = None, None
    for k, v in enumerate(poses):
        sd = moved(cornell, v)
        o = oracle_lib.Oracle(sd, luts)
        fr = scene.make_frame(cam, QW, QH, settings=scene.parity_settings(3), sample_number=0, random_seed=seeds[k])
        color, albedo, normals = o.render([fr], aov=True)
        prim, t, uu, vv = o.trace_closest(mpt.primary_rays_host(cam, QW, QH))
        vis = np.stack([t, uu, vv, prim.view(f32)], -1).reshape(QH, QW, 4)
        out, _, ha, hb = mpt.temporal_host(s, cam, cam, vis, idx, v, poses[max(k - 1, 0)], color, albedo, normals, hist)
        hist = (ha, hb)
        if k == POSES - 1:
            frames = []
            for j, seed in scene.cpu_seed_schedule(256):
                frames.append(scene.make_frame(cam, QW, QH, settings=scene.parity_settings(3), sample_number=j, random_seed=seed + 977))
            ref = tonemapped(o.render(frames).astype(np.float64) / 256)
        o.close()
    assert hist[1][..., 3].max() == POSES and np.median(hist[1][..., 3]) >= POSES - 1
    alone = np.mean((tonemapped(mpt.denoise_host(d, color, albedo, normals)) - ref) ** 2)
    both = np.mean((tonemapped(mpt.denoise_host(d, out, albedo, normals)) - ref) ** 2)
    noisy = np.mean((tonemapped(color) - ref) ** 2)
    print(f"last pose: noisy MSE {noisy:.5f}, denoise alone {alone:.5f}, temporal + denoise {both:.5f} (ratio {both / alone:.3f})")
    assert both < alone
