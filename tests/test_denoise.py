"""The denoiser (mpt_denoise / mpt_denoise_device / mpt_denoise_host): an edge-avoiding a-trous
filter on albedo-demodulated radiance, guided by the albedo and normals AOVs, on
the GPU as k_denoise_prepare + k_atrous_* (csrc/denoise.hip) and on the host from the same pixel
functions (csrc/denoise.h).

CPU part (mpt_denoise_host, no GPU):
* the host path against a numpy restatement of the definition written here, run once in float32
  and once in float64.  Measure: max |x - y| / (|y| + 1e-6) on per-sample means.  The host path
  may differ from the float64 run by at most 8x the deviation between the two numpy runs (taken
  in both directions, the larger): the factor covers tmath's 1-ulp exp and the different rounding
  of the normal power.  Measured here: the two numpy runs differ by 0.44e-6..4.4e-6 on the oracle
  frame, 0.36e-6..2.2e-6 on the synthetic one and 0.1e-6..0.4e-6 on the shapes smaller than the
  stencil; the host path differs from float64 by 0.4e-6..4.4e-6, 0.4e-6..2.2e-6 and 0.1e-6..0.6e-6.
* exact properties: scaling, non-finite and negative inputs, normal edges, miss pixels, shapes
  smaller than the stencil; settings validation.
* the filter denoises: MSE against a 512-spp oracle render after the display tonemap.

GPU part (-m gpu): the kernels equal the host path bit for bit -- the context's own buffers and
caller-owned planes, every iteration count and guide combination, host and device destinations,
stream ordering without a synchronise, the errors, the gather route of a row partition."""
import ctypes as C

import numpy as np
import pytest

import mpt
from mpt import abi, scene

f32 = np.float32


# ------------------------------------------------------------------------------------------
# numpy restatement of the definition, in dtype dt
# ------------------------------------------------------------------------------------------
def restate(color, albedo, normals, s, dt):
    """The filter of DESIGN.md §2 on [H, W, 3] arrays in dtype dt; the constants are the fp32
    constants' values."""
    K = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dt)
    n = dt(s.sample_number)
    H, W = color.shape[:2]
    with np.errstate(all="ignore"):
        m = color.astype(dt) / n
        m = np.where(np.isnan(m), dt(0), np.minimum(np.maximum(m, dt(0)), dt(f32(1.0e35))))
        a = np.where(np.isfinite(albedo), albedo, 0).astype(dt)
        nr = np.where(np.isfinite(normals), normals, 0).astype(dt)
        d = np.maximum(a, dt(f32(0.01))) if s.use_albedo else np.ones_like(a)
        e = m / d
        inv_a = dt(1) / (dt(f32(s.sigma_albedo)) * dt(f32(s.sigma_albedo)))
        for it in range(s.iterations):
            st = 1 << it
            sc = dt(f32(s.sigma_color)) * dt(2.0 ** -it)
            inv_c = dt(1) / (sc * sc)
            num, den = np.zeros_like(e), np.zeros((H, W), dt)
            lum = (e[..., 0] + e[..., 1]) + e[..., 2]
            for dy in range(-2, 3):
                oy = dy * st
                if abs(oy) >= H:
                    continue
                py, qy = slice(max(0, -oy), H - max(0, oy)), slice(max(0, oy), H - max(0, -oy))
                for dx in range(-2, 3):
                    ox = dx * st
                    if abs(ox) >= W:
                        continue
                    px, qx = slice(max(0, -ox), W - max(0, ox)), slice(max(0, ox), W - max(0, -ox))
                    h = K[dy + 2] * K[dx + 2]
                    ep, eq = e[py, px], e[qy, qx]
                    if dx == 0 and dy == 0:
                        w = np.full(ep.shape[:2], h, dt)
                    else:
                        df = ep - eq
                        dc = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
                        mm = (lum[py, px] + lum[qy, qx]) / dt(6)
                        xx = dc / (mm * mm + dt(f32(1.0e-4))) * inv_c
                        if s.use_albedo:
                            da = a[py, px] - a[qy, qx]
                            xx = xx + ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * inv_a
                        keep = xx <= dt(80)
                        w = h * np.exp(-np.where(keep, xx, dt(0)))
                        if s.use_normals:
                            t = (nr[py, px, 0] * nr[qy, qx, 0] + nr[py, px, 1] * nr[qy, qx, 1]) + nr[py, px, 2] * nr[qy, qx, 2]
                            keep &= t > 0
                            t = np.minimum(np.where(keep, t, dt(0)), dt(1))
                            for _ in range(s.normal_power_log2):
                                t = t * t
                            w = w * t
                        w = np.where(keep, w, dt(0))   # a skipped tap adds nothing
                    num[py, px] = num[py, px] + w[..., None] * np.where(w[..., None] != 0, eq, dt(0))
                    den[py, px] = den[py, px] + w
            e = num / den[..., None]
        return e * d * n


def rel(x, y):
    """max |x - y| / (|y| + 1e-6)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y) / (np.abs(y) + 1e-6))) if x.size else 0.0


def settings(n=1, **kw):
    s = abi.DenoiseSettings.default()
    s.sample_number = n
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def synthetic(w, h, n, seed):
    """Random colour sums up to 2 n, unit normals in a few flat regions, piecewise-constant albedo,
    a block of miss pixels (albedo 0, normal 0, colour kept)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = ((xs * 3) // max(w, 1) + 3 * ((ys * 2) // max(h, 1))) % 5
    normals_of = rng.normal(size=(5, 3))
    normals_of /= np.linalg.norm(normals_of, axis=1, keepdims=True)
    normals_of[1] = normals_of[0]            # two regions that differ in albedo only
    albedo_of = rng.uniform(0.05, 0.95, size=(5, 3))
    color = (rng.uniform(0, 2 * n, size=(h, w, 3)) * rng.uniform(0, 1, size=(h, w, 1)) ** 2).astype(f32)
    albedo, normals = albedo_of[region].astype(f32), normals_of[region].astype(f32)
    miss = (xs >= w // 2) & (xs < w // 2 + 4) & (ys < max(1, h // 3))
    albedo[miss] = 0
    normals[miss] = 0
    return color, albedo, normals


def check_against_restatement(color, albedo, normals, s, what):
    r32, r64 = restate(color, albedo, normals, s, np.float32), restate(color, albedo, normals, s, np.float64)
    n = s.sample_number
    dev = max(rel(r32 / n, r64 / n), rel(r64 / n, r32.astype(np.float64) / n))
    got = mpt.denoise_host(s, color, albedo, normals)
    assert np.isfinite(got).all(), what
    err = rel(got.astype(np.float64) / n, r64 / n)
    print(f"{what}: float32 vs float64 restatement {dev:.3g}, host path vs float64 {err:.3g}")
    assert err <= 8 * dev, f"{what}: host path {err:.3g} from float64, the numpy runs {dev:.3g} apart"
    return got


W0, H0 = 64, 48


def oracle_frames(sd, n, w=W0, h=H0, band=(1, 0, 1)):
    cam = scene.make_camera(sd.camera_info, w, h)
    out = []
    for k, seed in scene.cpu_seed_schedule(n):
        st = scene.parity_settings(3)
        st.denoiser_AOV_accumulation_counter = k
        st.do_update_status_buffers = k == n - 1
        out.append(scene.make_frame(cam, w, h, settings=st, sample_number=k, random_seed=seed, band=band))
    return out


@pytest.fixture(scope="module")
def oracle_renders(cornell, luts, oracle_lib):
    """Cornell 64x48 by the oracle: (colour sums, albedo, normals) at 1 and 4 spp, the 512-spp mean."""
    o = oracle_lib.Oracle(cornell, luts)
    out = {n: o.render(oracle_frames(cornell, n), aov=True) for n in (1, 4)}
    out["ref"] = o.render(oracle_frames(cornell, 512)).astype(np.float64) / 512
    o.close()
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return out


GUIDES = [(1, 1), (1, 0), (0, 1), (0, 0)]


# ------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("use_albedo,use_normals", GUIDES)
def test_host_path_matches_restatement_on_an_oracle_render(oracle_renders, use_albedo, use_normals, iterations):
    color, albedo, normals = oracle_renders[4]
    s = settings(4, iterations=iterations, use_albedo=use_albedo, use_normals=use_normals)
    check_against_restatement(color, albedo, normals, s, f"oracle 64x48 a{use_albedo} n{use_normals} it{iterations}")


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("use_albedo,use_normals", GUIDES)
def test_host_path_matches_restatement_on_synthetic_planes(use_albedo, use_normals, iterations):
    color, albedo, normals = synthetic(47, 33, 7, 11)
    s = settings(7, iterations=iterations, use_albedo=use_albedo, use_normals=use_normals)
    check_against_restatement(color, albedo, normals, s, f"synthetic 47x33 a{use_albedo} n{use_normals} it{iterations}")


def test_settings_default():
    s = abi.DenoiseSettings()
    assert mpt.lib().mpt_denoise_settings_default(C.byref(s)) == abi.OK
    d = abi.DenoiseSettings.default()
    assert bytes(s) == bytes(d) and C.sizeof(s) == 28
    assert (s.sample_number, s.iterations, s.use_albedo, s.use_normals, s.normal_power_log2) == (1, 5, 1, 1, 6)
    assert (s.sigma_color, s.sigma_albedo) == (4.0, float(f32(0.1)))


def test_scaling_is_exact():
    color, albedo, normals = synthetic(47, 33, 3, 5)
    one = mpt.denoise_host(settings(3), color, albedo, normals)
    two = mpt.denoise_host(settings(6), color * f32(2), albedo, normals)
    assert np.array_equal(two, one * f32(2))


def test_non_finite_and_negative_inputs_do_not_spread():
    color, albedo, normals = synthetic(47, 33, 4, 6)
    clean = [color.copy(), albedo.copy(), normals.copy()]
    color[10, 10, 0], clean[0][10, 10, 0] = np.nan, 0.0
    color[12, 30, 1], clean[0][12, 30, 1] = np.inf, f32(1.0e35) * f32(4)      # clamp(inf / 4, 0, 1e35) = 1e35
    color[20, 7, 2], clean[0][20, 7, 2] = -3.0, 0.0
    albedo[5, 5, 1], clean[1][5, 5, 1] = np.nan, 0.0
    albedo[25, 40, 0], clean[1][25, 40, 0] = np.inf, 0.0
    normals[15, 20, 2], clean[2][15, 20, 2] = -np.inf, 0.0
    for ua, un in GUIDES:
        s = settings(4, use_albedo=ua, use_normals=un)
        got = mpt.denoise_host(s, color, albedo, normals)
        assert np.isfinite(got).all()
        assert np.array_equal(got, mpt.denoise_host(s, *clean))


def test_orthogonal_half_planes_do_not_leak():
    w, h, n = 40, 24, 4
    left, right = np.array([0.8, 0.3, 0.1], f32) * n, np.array([0.05, 0.6, 1.7], f32) * n
    color = np.where(np.arange(w)[None, :, None] < 19, left, right).astype(f32) * np.ones((h, 1, 1), f32)
    normals = np.where(np.arange(w)[None, :, None] < 19, f32([1, 0, 0]), f32([0, 1, 0])).astype(f32) * np.ones((h, 1, 1), f32)
    albedo = np.full((h, w, 3), 0.5, f32)
    got = mpt.denoise_host(settings(n), color, albedo, normals)
    assert rel(got[:, :19], np.broadcast_to(left, (h, 19, 3))) <= 1e-6
    assert rel(got[:, 19:], np.broadcast_to(right, (h, w - 19, 3))) <= 1e-6
    # without the normal guide (and with one albedo) the two sides do mix
    mixed = mpt.denoise_host(settings(n, use_normals=0, sigma_color=1.0e3), color, albedo, normals)
    assert rel(mixed[:, 17:21], color[:, 17:21]) > 1e-2


def test_miss_pixels_keep_their_value():
    color, albedo, normals = synthetic(47, 33, 4, 8)
    miss = (normals == 0).all(-1)
    assert miss.sum() >= 8
    for ua in (0, 1):
        got = mpt.denoise_host(settings(4, use_albedo=ua), color, albedo, normals)
        assert rel(got[miss], color[miss]) <= 1e-6
        assert rel(got[~miss], color[~miss]) > 1e-2


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (1, 70), (64, 1)])
def test_shapes_smaller_than_the_stencil(w, h):
    color, albedo, normals = synthetic(w, h, 2, 9)
    got = check_against_restatement(color, albedo, normals, settings(2, iterations=5), f"{w}x{h}")
    assert got.shape == (h, w, 3)


BAD = [dict(sample_number=0), dict(sample_number=-3), dict(iterations=0), dict(iterations=9), dict(normal_power_log2=-1),
       dict(normal_power_log2=11), dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=float("inf")),
       dict(sigma_color=float("nan")), dict(sigma_albedo=0.0), dict(sigma_albedo=float("inf")), dict(sigma_albedo=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_settings_validation(bad):
    color, albedo, normals = synthetic(5, 3, 1, 1)
    s = settings(1, **bad)
    out = np.zeros_like(color)
    rc = mpt.lib().mpt_denoise_host(C.byref(s), color.ctypes.data, albedo.ctypes.data, normals.ctypes.data, 5, 3, out.ctypes.data)
    assert rc == abi.ERR_INVALID_ARGUMENT
    assert list(bad)[0].encode() in mpt.lib().mpt_last_error()
    assert not out.any()
    assert mpt.lib().mpt_denoise_host(C.byref(settings(1)), color.ctypes.data, None, normals.ctypes.data, 5, 3,
                                      out.ctypes.data) == abi.ERR_INVALID_ARGUMENT


def tonemapped(mean):
    return (1.0 - np.exp(-np.maximum(np.asarray(mean, np.float64), 0.0) * 1.8)) ** (1 / 2.2)


# MSE_denoised / MSE_noisy of the float64 restatement on these frames was 0.215 at 1 spp and 0.441
# at 4 spp (the issue's prototype: 0.21 and 0.44), so the issue's thresholds stand.
@pytest.mark.parametrize("spp,threshold", [(4, 0.6), (1, 0.3)])
def test_the_filter_denoises(oracle_renders, spp, threshold):
    color, albedo, normals = oracle_renders[spp]
    ref = tonemapped(oracle_renders["ref"])
    s = settings(spp)
    noisy = np.mean((tonemapped(color / spp) - ref) ** 2)
    r64 = np.mean((tonemapped(restate(color, albedo, normals, s, np.float64) / spp) - ref) ** 2)
    got = np.mean((tonemapped(mpt.denoise_host(s, color, albedo, normals).astype(np.float64) / spp) - ref) ** 2)
    print(f"{spp} spp: noisy MSE {noisy:.5f}, denoised {got:.5f} (ratio {got / noisy:.3f}), restatement ratio {r64 / noisy:.3f}")
    assert got <= threshold * noisy


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
W, H = 47, 33


def _renderer(sd, luts):
    r = mpt.GPURenderer(0)
    r.set_scene(sd)
    r.set_luts(luts)
    return r


def _planes(r):
    return r.framebuffer(abi.FB_COLOR), r.framebuffer(abi.FB_ALBEDO), r.framebuffer(abi.FB_NORMALS)


@pytest.fixture(scope="module")
def rendered(cornell, luts):
    """Cornell, 47x33, 4 samples, rendered once: (renderer, its three planes on the host)."""
    r = _renderer(cornell, luts)
    r.render_samples(oracle_frames(cornell, 4, W, H))
    r.synchronize_kernel()
    yield r, _planes(r)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_albedo,use_normals", GUIDES)
def test_gpu_denoise_of_own_buffers_equals_host_path(rendered, use_albedo, use_normals):
    import torch
    r, planes = rendered
    assert r.denoise_settings().sample_number == 4
    dst = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for iterations in range(1, 6):
        s = r.denoise_settings(settings(iterations=iterations, use_albedo=use_albedo, use_normals=use_normals))
        want = mpt.denoise_host(s, *planes)
        got = r.denoise(s)
        assert got.shape == (H, W, 3)
        assert np.array_equal(got, want), f"it {iterations}: {(got != want).sum()} values differ"
        s.sample_number = 5     # another result, so that the device destination shows its own run
        want5 = mpt.denoise_host(s, *planes)
        r.denoise_to_device(dst.data_ptr(), s)
        ptr, n = r.denoised()
        assert n == 5 and ptr != 0
        r.synchronize_kernel()
        assert np.array_equal(dst.cpu().numpy().reshape(H, W, 3), want5)
        assert np.array_equal(device_array(ptr, H * W * 3).cpu().numpy().reshape(H, W, 3), want5)   # the kept buffer
    assert np.array_equal(r.framebuffer(abi.FB_COLOR), planes[0])   # the sums are read in place, not changed
    if use_albedo and use_normals:
        assert np.array_equal(r.denoise(), mpt.denoise_host(settings(4), *planes))   # the defaults


class _DevicePointer:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def device_array(ptr, n):
    """n floats at a raw device pointer as a torch tensor (no copy)."""
    import torch
    return torch.as_tensor(_DevicePointer(ptr, n), device="cuda")


SHAPES = [(1, 1, 5), (5, 3, 5), (1, 70, 5), (64, 1, 5), (131, 67, 5), (257, 40, 5), (131, 67, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,iterations", SHAPES)
def test_gpu_denoise_of_caller_owned_planes_equals_host_path(rendered, w, h, iterations):
    import torch
    r, _ = rendered
    color, albedo, normals = synthetic(w, h, 3, 100 + w)
    color[h // 2, w // 2, 0] = np.nan
    normals[0, 0, 1] = np.inf
    dev = [torch.from_numpy(a).cuda() for a in (color, albedo, normals)]
    dst = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for ua, un in GUIDES[:1] + (GUIDES[1:] if (w, h) == (131, 67) else []):
        s = settings(3, iterations=iterations, use_albedo=ua, use_normals=un)
        want = mpt.denoise_host(s, color, albedo, normals)
        r.denoise_device(s, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), w, h, dst.data_ptr())
        r.synchronize_kernel()
        got = dst.cpu().numpy().reshape(h, w, 3)
        assert np.array_equal(got, want), f"{w}x{h} a{ua} n{un}: {(got != want).sum()} values differ"
    for a, b in zip(dev, (color, albedo, normals)):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)   # the inputs are left alone


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["0", "0xff"], ids=["gather", "tiled"])
def test_gpu_either_kernel_at_every_step_equals_host_path(rendered, monkeypatch, mask):
    """The library picks the gather or the tiled kernel per step from a table; MPT_DENOISE_TILED (read
    at every call) forces one of them at every step, 128 included: larger than the image."""
    import torch
    r, _ = rendered
    w, h = 131, 67
    color, albedo, normals = synthetic(w, h, 3, 77)
    dev = [torch.from_numpy(a).cuda() for a in (color, albedo, normals)]
    dst = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = settings(3, iterations=8)
    want = mpt.denoise_host(s, color, albedo, normals)
    monkeypatch.setenv("MPT_DENOISE_TILED", mask)
    r.denoise_device(s, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), w, h, dst.data_ptr())
    r.synchronize_kernel()
    got = dst.cpu().numpy().reshape(h, w, 3)
    assert np.array_equal(got, want), f"{(got != want).sum()} values differ"


@pytest.mark.gpu
def test_gpu_denoise_is_ordered_on_the_stream(cornell, luts):
    import torch
    frs = oracle_frames(cornell, 4, W, H)
    r = _renderer(cornell, luts)
    den = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    out = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_samples(frs)
    r.denoise_to_device(den.data_ptr())                      # straight after the frames: no synchronise
    ptr, n = r.denoised()
    st = r.display_settings(abi.VIEW_BLEND)
    st.sample_number_2 = n
    st.blend_factor = 0.7
    r.display_to_device(out.data_ptr(), settings=st, second_dev_ptr=ptr)
    r.synchronize_kernel()                                   # the one synchronise
    planes = _planes(r)
    want_den = mpt.denoise_host(settings(4), *planes)
    assert n == 4
    assert np.array_equal(den.cpu().numpy().reshape(H, W, 3), want_den)
    want = mpt.display_host(st, planes[0], want_den)
    assert np.array_equal(out.cpu().numpy().reshape(H, W, 4), want)
    assert np.array_equal(r.display_denoised(0.7), want)
    st.blend_factor = 1.0
    assert np.array_equal(r.display_denoised(), mpt.display_host(st, planes[0], want_den))
    assert not np.array_equal(r.display_denoised(), r.display())     # the filtered image is another image
    r.close()


@pytest.mark.gpu
def test_gpu_denoise_errors(cornell, luts):
    r = _renderer(cornell, luts)
    s = settings(1)
    assert mpt.lib().mpt_denoise(r.h, C.byref(s), None, 1) == abi.ERR_INVALID_ARGUMENT
    assert b"no frame rendered" in mpt.lib().mpt_last_error()
    with pytest.raises(mpt.MptError, match="nothing denoised"):
        r.denoised()
    r.render_samples(oracle_frames(cornell, 2, W, H))
    with pytest.raises(mpt.MptError, match="nothing denoised"):
        r.denoised()
    with pytest.raises(mpt.MptError, match="iterations"):
        r.denoise(settings(2, iterations=9))
    assert r.denoise().shape == (H, W, 3)
    assert r.denoised()[1] == 2
    r.resize(W, H)
    with pytest.raises(mpt.MptError, match="nothing denoised") as e:
        r.denoised()
    assert e.value.code == abi.ERR_INVALID_ARGUMENT
    r.close()
    b = _renderer(cornell, luts)
    b.render_samples(oracle_frames(cornell, 2, W, H, band=(8, 0, 2)))
    with pytest.raises(mpt.MptError, match="gather") as e:
        b.denoise()
    assert e.value.code == abi.ERR_UNSUPPORTED
    b.close()


@pytest.mark.gpu
def test_gpu_denoise_of_gathered_partition_equals_single_context(rendered, cornell, luts):
    import torch
    single, _ = rendered
    want = single.denoise()
    rs = []
    for k in range(2):
        r = _renderer(cornell, luts)
        r.render_samples(oracle_frames(cornell, 4, W, H, band=(8, k, 2)))
        rs.append(r)
    dev = [torch.from_numpy(mpt.gather(rs, 0, kind)).cuda() for kind in (abi.FB_COLOR, abi.FB_ALBEDO, abi.FB_NORMALS)]
    dst = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rs[0].denoise_device(rs[0].denoise_settings(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), W, H, dst.data_ptr())
    rs[0].synchronize_kernel()
    got = dst.cpu().numpy().reshape(H, W, 3)
    for r in rs:
        r.close()
    assert np.array_equal(got, want), f"{(got != want).sum()} values differ"
