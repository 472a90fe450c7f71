"""The display step (mpt_display / mpt_display_host / mpt_write_png): the reference's display
shaders (src/Shaders/*.frag as Screenshoter::write_to_png runs them) restated in fp32, on the
GPU as k_display (csrc/display.hip) and on the host from the same pixel functions (csrc/display.h).

CPU part (mpt_display_host, no GPU):
* every view against a numpy float64 restatement written here.  fp32 error can move a value
  across a byte boundary, so the restatement yields a lowest and a highest admissible code per
  channel: the `1 - exp` term moved by +-2^-22 absolute and the final value by (1 +- 2^-20)
  relative (tests/test_tmath.py bounds exp and pow to 1 ulp; the rest covers the roundings of the
  multiplies and divides).  Channels the shader sets to a constant without arithmetic (alpha,
  the white-furnace colours without tonemapping, the converged map, a heat-map value exactly on
  a stop) carry no fp32 error and are compared exactly.  The inputs must be sharp: high - low
  <= 1 everywhere and at most 1 % of the channels may have two admissible codes.
* hand-derived exact cases, mpt_display_uniforms against a table, the PNG writer's round trip.

GPU part (-m gpu): mpt_display equals mpt_display_host of the context's own buffers bit for
bit -- every view, host and device destinations and second buffers, low-resolution upscaling,
row partitions, stream ordering without a synchronise, row tails."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import mpt
from mpt import abi, image, partition, scene

RGB_VIEWS = (abi.VIEW_DEFAULT, abi.VIEW_BLEND, abi.VIEW_NORMALS, abi.VIEW_ALBEDO, abi.VIEW_WHITE_FURNACE_THRESHOLD)
COUNT_VIEWS = (abi.VIEW_PIXEL_CONVERGENCE_HEATMAP, abi.VIEW_PIXEL_CONVERGED_MAP)
D_REL, D_EXP = 2.0 ** -20, 2.0 ** -22
f32 = np.float32


# ------------------------------------------------------------------------------------------
# float64 restatement: (lowest value, highest value, exact mask) per channel -> code bounds
# ------------------------------------------------------------------------------------------
def _byte(v):
    p = np.asarray(v, np.float64) * 255.0
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, np.minimum(np.floor(np.where(p > 0, p, 0.0)), 255.0), 0.0).astype(np.int64)


def _codes(vlo, vhi, exact):
    a, b = _byte(vlo * (1 - D_REL)), _byte(vlo * (1 + D_REL))
    c, d = _byte(vhi * (1 - D_REL)), _byte(vhi * (1 + D_REL))
    lo, hi = np.minimum(np.minimum(a, b), np.minimum(c, d)), np.maximum(np.maximum(a, b), np.maximum(c, d))
    e = _byte(vlo)
    return np.where(exact, e, lo), np.where(exact, e, hi)


def _tonemap64(c, s):
    exposure, inv_gamma = float(f32(s.exposure)), float(f32(1) / f32(s.gamma))
    t = 1.0 - np.exp(-c * exposure)
    return np.maximum(t - D_EXP, 0.0) ** inv_gamma, (t + D_EXP) ** inv_gamma


def _upscale(a, s):
    h, w = a.shape[:2]
    return a[np.ix_(np.arange(h) // s, np.arange(w) // s)]


def reference_bounds(s, src, src2=None):
    """(low, high) uint8-range codes [H, W, 4] of view s.view, float64."""
    sc = s.resolution_scaling
    h, w = src.shape[:2]
    one = np.ones((h, w, 1))
    if s.view in COUNT_VIEWS:
        cnt = _upscale(src, sc).astype(np.float64)
        if s.view == abi.VIEW_PIXEL_CONVERGED_MAP:
            v = np.where((cnt < float(f32(s.threshold_val))) & (cnt != -1.0), 1.0, 0.0)[..., None] * np.ones(4)
            return _codes(v, v, np.ones_like(v, bool))
        stops = np.array([[c.r, c.g, c.b] for c in s.color_stops[:s.nb_stops]], np.float64)
        lo_v, hi_v = float(f32(s.min_val)), float(f32(s.max_val))
        if lo_v == hi_v:
            v = np.concatenate([np.broadcast_to(stops[-1], (h, w, 3)), one], -1)
            return _codes(v, v, np.ones_like(v, bool))
        x = np.clip(np.where(cnt == -1.0, hi_v, cnt), lo_v, hi_v)
        stop = (x - lo_v) / (hi_v - lo_v) * (s.nb_stops - 1)
        lo_i, hi_i = np.floor(stop).astype(int), np.ceil(stop).astype(int)
        f = (stop - lo_i)[..., None]
        v = np.concatenate([stops[lo_i] * (1 - f) + stops[hi_i] * f, one], -1)
        exact = np.concatenate([np.broadcast_to(f == 0, (h, w, 3)), one > 0], -1)
        return _codes(v, v, exact)
    c = _upscale(src, sc).astype(np.float64)
    exact = np.zeros((h, w, 3), bool)
    tone = s.do_tonemapping == 1
    if s.view == abi.VIEW_ALBEDO:
        lo = hi = c
    elif s.view == abi.VIEW_BLEND:
        c1 = c / max(1, s.sample_number)
        c2 = _upscale(src2, sc).astype(np.float64) / max(1, s.sample_number_2)
        (l1, h1), (l2, h2) = (_tonemap64(c1, s), _tonemap64(c2, s)) if tone else ((c1, c1), (c2, c2))
        f = float(f32(s.blend_factor))
        lo, hi = l1 * (1 - f) + l2 * f, h1 * (1 - f) + h2 * f
        # the alpha is 1 (1 - f) + 1 f in fp32: IEEE operations numpy's float32 repeats exactly
        alpha = float(f32(1) * (f32(1) - f32(s.blend_factor)) + f32(1) * f32(s.blend_factor))
        lo, hi = _codes(lo, hi, exact)
        a = np.full((h, w, 1), _byte(alpha))
        return np.concatenate([lo, a], -1), np.concatenate([hi, a], -1)
    else:
        if s.view == abi.VIEW_NORMALS:
            c = (c + 1.0) * 0.5
        else:
            c = c / s.sample_number
            if s.view == abi.VIEW_DEFAULT:
                c = np.clip(c, 0.0, 1.0e35)
            else:
                red = (c > float(f32(0.51))).any(-1) & bool(s.use_high_threshold)
                green = ~red & (c < float(f32(0.49))).any(-1) & bool(s.use_low_threshold)
                c = np.where(red[..., None], [1.0, 0.0, 0.0], np.where(green[..., None], [0.0, 1.0, 0.0], c))
                exact = np.broadcast_to(((red | green) & (not tone))[..., None], (h, w, 3))
        lo, hi = _tonemap64(c, s) if tone else (c, c)
    lo, hi = _codes(lo, hi, exact)
    a = np.full((h, w, 1), 255)
    return np.concatenate([lo, a], -1), np.concatenate([hi, a], -1)


def _inputs(w, h, n, seed):
    rng = np.random.default_rng(seed)
    color = (rng.random((h, w, 3)) * 2 * n).astype(f32)
    # the white-furnace view compares the mean with 0.49 / 0.51: no input within fp32 error of them
    mean = color.astype(np.float64) / n
    color[(np.abs(mean - 0.51) < 1e-4) | (np.abs(mean - 0.49) < 1e-4)] = 0.0
    nrm = rng.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(f32)
    albedo = rng.random((h, w, 3)).astype(f32)
    second = (rng.random((h, w, 3)) * 2 * 3).astype(f32)
    # heat map over [n, n + 11]: eleven steps put no interior count on a byte boundary
    counts = rng.integers(n, n + 12, (h, w)).astype(np.int32)
    counts[rng.random((h, w)) < 0.25] = -1
    return color, nrm, albedo, second, counts


def _settings(view, n, s, tone):
    st = mpt.display_settings(view=view)
    st.sample_number, st.sample_number_2, st.resolution_scaling, st.do_tonemapping = n, 3, s, int(tone)
    st.blend_factor = 0.3
    st.use_low_threshold = 1
    st.min_val, st.max_val, st.threshold_val = n, n + 11, n + 6
    return st


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("tone", [True, False], ids=["tonemap", "linear"])
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("w,h", [(47, 33), (1, 1)])
def test_host_views_match_float64_restatement(w, h, s, tone, n):
    color, nrm, albedo, second, counts = _inputs(w, h, n, seed=1000 * n + 10 * s + int(tone))
    sources = {abi.VIEW_DEFAULT: color, abi.VIEW_BLEND: color, abi.VIEW_NORMALS: nrm, abi.VIEW_ALBEDO: albedo,
               abi.VIEW_WHITE_FURNACE_THRESHOLD: color, abi.VIEW_PIXEL_CONVERGENCE_HEATMAP: counts,
               abi.VIEW_PIXEL_CONVERGED_MAP: counts}
    for view in abi.VIEWS:
        st = _settings(view, n, s, tone)
        src2 = second if view == abi.VIEW_BLEND else None
        got = mpt.display_host(st, sources[view], src2).astype(np.int64)
        lo, hi = reference_bounds(st, sources[view], src2)
        assert got.shape == (h, w, 4)
        assert (hi - lo <= 1).all(), f"view {view}: bounds wider than one code"
        share = float((lo != hi).mean())
        print(f"view {view} {w}x{h} s={s} tone={tone} n={n}: {100 * share:.3f} % of channels with two codes")
        if w * h > 1:
            assert share <= 0.01, f"view {view}: {100 * share:.2f} % of channels ambiguous"
        bad = (got < lo) | (got > hi)
        assert not bad.any(), f"view {view}: {int(bad.sum())} channels outside [low, high], first {np.argwhere(bad)[0]}"


# ------------------------------------------------------------------------------------------
# hand-derived cases
# ------------------------------------------------------------------------------------------
def _one(view, px, second=None, **kw):
    st = mpt.display_settings(view=view)
    for k, v in kw.items():
        setattr(st, k, v)
    counts = view in COUNT_VIEWS
    src = np.array(px, np.int32).reshape(1, 1) if counts else np.array(px, f32).reshape(1, 1, 3)
    sec = None if second is None else np.array(second, f32).reshape(1, 1, 3)
    return mpt.display_host(st, src, sec)[0, 0].tolist()


def test_exact_cases_default_and_white_furnace():
    assert _one(abi.VIEW_DEFAULT, [0, 0, 0]) == [0, 0, 0, 255]                      # 1 - exp(0) = 0
    assert _one(abi.VIEW_DEFAULT, [1e30, 3e38, np.inf]) == [255, 255, 255, 255]     # clamp 1e35, exp -> 0, pow(1) = 1
    assert _one(abi.VIEW_DEFAULT, [np.nan, -5.0, -np.inf]) == [0, 0, 0, 255]        # fmax(NaN, 0) = 0, negatives clamp
    assert _one(abi.VIEW_DEFAULT, [0.5, 1.0, 2.0], do_tonemapping=0) == [127, 255, 255, 255]
    assert _one(abi.VIEW_DEFAULT, [1.0, 2.0, 8.0], do_tonemapping=0, sample_number=4) == [63, 127, 255, 255]
    assert _one(abi.VIEW_ALBEDO, [0.0, 0.5, 1.0]) == [0, 127, 255, 255]
    assert _one(abi.VIEW_ALBEDO, [np.nan, -1.0, 1e9]) == [0, 0, 255, 255]           # saturation, NaN -> 0
    assert _one(abi.VIEW_NORMALS, [-1.0, 0.0, 1.0], do_tonemapping=0) == [0, 127, 255, 255]
    wf = abi.VIEW_WHITE_FURNACE_THRESHOLD
    # no clamp: a negative mean tonemaps to pow(negative) = NaN -> 0; without tonemapping it saturates to 0
    assert _one(wf, [-1.0, -1.0, -1.0]) == [0, 0, 0, 255]
    assert _one(wf, [-1.0, 0.25, 0.5], do_tonemapping=0) == [0, 63, 127, 255]
    assert _one(wf, [0.5, 0.52, 0.5], do_tonemapping=0) == [255, 0, 0, 255]         # above 0.51: red
    assert _one(wf, [0.5, 0.5, 0.5], do_tonemapping=0) == [127, 127, 127, 255]      # inside the band
    assert _one(wf, [0.5, 0.4, 0.5], do_tonemapping=0) == [127, 102, 127, 255]      # low threshold off by default
    assert _one(wf, [0.5, 0.4, 0.5], do_tonemapping=0, use_low_threshold=1) == [0, 255, 0, 255]
    assert _one(wf, [0.6, 0.4, 0.5], do_tonemapping=0, use_low_threshold=1) == [255, 0, 0, 255]   # high wins
    assert _one(wf, [0.6, 0.4, 0.5], do_tonemapping=0, use_high_threshold=0) == [153, 102, 127, 255]
    # the red of the tonemapped view: pow(1 - exp(-1.8), 1 / 2.2) = 0.92125 -> 234
    assert _one(wf, [2.0, 0.0, 0.0]) == [234, 0, 0, 255]


def test_exact_cases_heat_map_and_converged_map():
    hm = abi.VIEW_PIXEL_CONVERGENCE_HEATMAP
    kw = dict(min_val=2, max_val=10)
    assert _one(hm, 2, **kw) == [0, 0, 255, 255]        # min: the first stop
    assert _one(hm, 10, **kw) == [255, 0, 0, 255]       # max: the last stop
    assert _one(hm, 6, **kw) == [0, 255, 0, 255]        # the midpoint of three stops: the middle one
    assert _one(hm, 4, **kw) == [0, 127, 127, 255]      # half way between blue and green
    assert _one(hm, -1, **kw) == [255, 0, 0, 255]       # not converged: max
    assert _one(hm, 1, **kw) == [0, 0, 255, 255] and _one(hm, 50, **kw) == [255, 0, 0, 255]   # clamped
    assert _one(hm, 3, min_val=5, max_val=5) == [255, 0, 0, 255]                                # min == max: last stop
    assert _one(hm, 3, min_val=5, max_val=5, nb_stops=2) == [0, 255, 0, 255]
    cm = abi.VIEW_PIXEL_CONVERGED_MAP
    assert _one(cm, 3, threshold_val=4) == [255, 255, 255, 255]
    assert _one(cm, 4, threshold_val=4) == [0, 0, 0, 0]          # == threshold: not converged, alpha 0 too
    assert _one(cm, -1, threshold_val=4) == [0, 0, 0, 0]


def test_blend_at_factors_0_and_1_equals_the_default_views():
    rng = np.random.default_rng(5)
    a, b = (rng.random((9, 13, 3)) * 6).astype(f32), (rng.random((9, 13, 3)) * 4).astype(f32)
    for tone in (0, 1):
        st = mpt.display_settings(view=abi.VIEW_BLEND)
        st.sample_number, st.sample_number_2, st.do_tonemapping = 3, 2, tone
        d = mpt.display_settings(view=abi.VIEW_DEFAULT)
        d.do_tonemapping = tone
        for factor, src, n in ((0.0, a, 3), (1.0, b, 2)):
            st.blend_factor = factor
            d.sample_number = n
            assert np.array_equal(mpt.display_host(st, a, b), mpt.display_host(d, src))


def test_low_resolution_scaling_reads_the_top_left_block():
    rng = np.random.default_rng(6)
    a = rng.random((7, 10, 3)).astype(f32)
    st = mpt.display_settings(view=abi.VIEW_ALBEDO)
    full = mpt.display_host(st, a)
    st.resolution_scaling = 3
    assert np.array_equal(mpt.display_host(st, a), _upscale(full, 3))


def test_settings_default_and_size():
    assert mpt.abi_sizes()["DisplaySettings"] == C.sizeof(abi.DisplaySettings) == abi.ABI_SIZES["DisplaySettings"]
    assert bytes(mpt.display_settings()) == bytes(abi.DisplaySettings.default())
    st = mpt.display_settings()
    assert (st.do_tonemapping, st.use_low_threshold, st.use_high_threshold, st.nb_stops) == (1, 0, 1, 3)
    assert (st.gamma, st.exposure) == (float(f32(2.2)), float(f32(1.8)))
    assert [(c.r, c.g, c.b) for c in st.color_stops[:3]] == [(0, 0, 1), (0, 1, 0), (1, 0, 0)]


def test_host_errors():
    a = np.zeros((2, 2, 3), f32)
    st = mpt.display_settings()
    for bad in (3, 5, 9, -1):
        st.view = bad
        with pytest.raises(mpt.MptError, match="bad view"):
            mpt.display_host(st, a)
    st = mpt.display_settings(view=abi.VIEW_PIXEL_CONVERGENCE_HEATMAP)
    for n in (0, 17):
        st.nb_stops = n
        with pytest.raises(mpt.MptError, match="nb_stops"):
            mpt.display_host(st, np.zeros((2, 2), np.int32))
    with pytest.raises(mpt.MptError, match="second buffer"):
        mpt.display_host(mpt.display_settings(view=abi.VIEW_BLEND), a)
    st = mpt.display_settings()
    st.resolution_scaling = 0
    with pytest.raises(mpt.MptError, match="resolution_scaling"):
        mpt.display_host(st, a)
    assert mpt.lib().mpt_display(None, None, None, 0, None, 0) == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(mpt.MptError, match="cannot open"):
        mpt.write_png("/nonexistent-directory/x.png", np.zeros((1, 1, 4), np.uint8))


# (adaptive, min_samples, sample_number, low-resolution scaling, displayed low) -> (n, s, min, max = threshold)
UNIFORMS = [
    ((False, 96, 0, 2, False), (1, 1, 1.0, 1.0)),
    ((False, 96, 5, 2, False), (5, 1, 1.0, 5.0)),
    ((True, 96, 5, 2, False), (5, 1, 96.0, 96.0)),
    ((True, 4, 9, 3, True), (9, 3, 4.0, 9.0)),
    ((True, 4, 0, 4, True), (1, 4, 4.0, 4.0)),
    ((False, 4, 1, 4, True), (1, 4, 1.0, 1.0)),
]


@pytest.mark.parametrize("given,want", UNIFORMS)
def test_display_uniforms_table(given, want):
    adaptive, min_samples, n, scaling, low = given
    rs = abi.RenderSettings.default()
    rs.enable_adaptive_sampling, rs.adaptive_sampling_min_samples = adaptive, min_samples
    rs.sample_number, rs.render_low_resolution_scaling = n, scaling
    for view in abi.VIEWS:
        st = mpt.display_settings(rs, view, low)
        assert (st.view, st.sample_number, st.resolution_scaling, st.min_val, st.max_val, st.threshold_val) == \
            (view, want[0], want[1], want[2], want[3], want[3])
        assert (st.gamma, st.nb_stops, st.sample_number_2) == (float(f32(2.2)), 3, 1)    # the rest stays


# ------------------------------------------------------------------------------------------
# PNG writer
# ------------------------------------------------------------------------------------------
def _parse_png(data):
    """An independent reader: chunk CRCs, IHDR, the stored-block zlib stream through zlib."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, interlace) == (8, 6, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 4)


@pytest.mark.parametrize("w,h", [(1, 1), (47, 33), (1, 300), (200, 120)])
@pytest.mark.parametrize("flip", [False, True])
def test_write_png_round_trip(tmp_path, w, h, flip):
    """200 x 120: 96 120 bytes of scanlines, more than one stored block."""
    img = np.random.default_rng(w * h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    path = tmp_path / "out.png"
    mpt.write_png(path, img, flip_y=flip)
    data = path.read_bytes()
    want = img[::-1] if flip else img
    assert np.array_equal(image.decode_png(data), want)          # the library's own decoder
    assert np.array_equal(image.read_image(data, 4), want)       # ... through the texture loader's entry
    assert np.array_equal(_parse_png(data), want)


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
W, H = 47, 33


def make_frames(sd, n=4, w=W, h=H, low=(), s=2, band=(1, 0, 1)):
    """n frames of one accumulation, adaptive sampling with min_samples 1 and threshold 0.9 (as
    tests/test_low_res.py: converged counts exist after a few samples); `low`: at low resolution."""
    cam = scene.make_camera(sd.camera_info, w, h)
    out = []
    for k, seed in scene.cpu_seed_schedule(n):
        st = scene.parity_settings(3)
        st.denoiser_AOV_accumulation_counter = k
        st.do_update_status_buffers = k == n - 1
        st.wants_render_low_resolution = k in low
        st.render_low_resolution_scaling = s
        st.enable_adaptive_sampling = True
        st.adaptive_sampling_min_samples = 1
        st.adaptive_sampling_noise_threshold = 0.9
        out.append(scene.make_frame(cam, w, h, settings=st, sample_number=k, random_seed=seed, band=band))
    return out


def _renderer(sd, luts):
    r = mpt.GPURenderer(0)
    r.set_scene(sd)
    r.set_luts(luts)
    return r


def _host_view(r, view, st, second=None):
    """display_host of the context's own buffers."""
    if view in COUNT_VIEWS:
        return mpt.display_host(st, r.aux_buffer(abi.AUX_CONVERGED_SAMPLE_COUNT))
    kind = {abi.VIEW_NORMALS: abi.FB_NORMALS, abi.VIEW_ALBEDO: abi.FB_ALBEDO}.get(view, abi.FB_COLOR)
    return mpt.display_host(st, r.framebuffer(kind), second)


@pytest.fixture(scope="module")
def rendered(cornell, luts):
    """Cornell, 47x33, 4 adaptive samples, rendered once for the read-only tests."""
    r = _renderer(cornell, luts)
    r.render_samples(make_frames(cornell))
    r.synchronize_kernel()
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("view", abi.VIEWS)
def test_gpu_display_equals_host_path(rendered, view):
    import torch
    r = rendered
    st = r.display_settings(view)
    assert st.sample_number == 4 and (st.min_val, st.max_val) == (1.0, 4.0)
    st.sample_number_2 = 4
    st.blend_factor = 0.3
    albedo = r.framebuffer(abi.FB_ALBEDO) if view == abi.VIEW_BLEND else None
    want = _host_view(r, view, st, albedo)
    got = r.display(settings=st, second=albedo)
    assert got.shape == (H, W, 4)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    if view in COUNT_VIEWS:
        cnt = r.aux_buffer(abi.AUX_CONVERGED_SAMPLE_COUNT)
        assert (cnt >= 0).any() and (cnt == -1).any()      # converged and unconverged pixels both shown
    # device destination, and the second buffer as a device pointer
    dst = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    sec = torch.from_numpy(albedo).cuda() if albedo is not None else None
    r.display_to_device(dst.data_ptr(), settings=st, second_dev_ptr=sec.data_ptr() if sec is not None else None)
    r.synchronize_kernel()
    assert np.array_equal(dst.cpu().numpy().reshape(H, W, 4), want)
    if sec is not None:
        assert np.array_equal(r.display(settings=st, second=sec.data_ptr()), want)
    if view == abi.VIEW_DEFAULT:
        assert np.array_equal(r.display(), want)           # the defaults: this view, derived settings
        assert want[..., :3].max() > 100 and (want[..., 3] == 255).all()


@pytest.mark.gpu
def test_gpu_display_errors(rendered, cornell, luts):
    r = rendered
    st = r.display_settings(abi.VIEW_BLEND)
    with pytest.raises(mpt.MptError, match="second buffer"):
        r.display(settings=st)
    st = r.display_settings()
    st.view = 5
    with pytest.raises(mpt.MptError, match="bad view"):
        r.display(settings=st)
    st = r.display_settings(abi.VIEW_PIXEL_CONVERGENCE_HEATMAP)
    st.nb_stops = 17
    with pytest.raises(mpt.MptError, match="nb_stops"):
        r.display(settings=st)
    q = _renderer(cornell, luts)
    out = np.zeros((H, W, 4), np.uint8)
    st = mpt.display_settings()
    assert mpt.lib().mpt_display(q.h, C.byref(st), None, 0, out.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
    assert b"no frame rendered" in mpt.lib().mpt_last_error()
    # a frame without the adaptive-sampling buffers: no heat map, no converged map
    f = make_frames(cornell, n=1)[0]
    f.render_settings.enable_adaptive_sampling = False
    q.render(f)
    assert q.display().shape == (H, W, 4)
    for view in COUNT_VIEWS:
        with pytest.raises(mpt.MptError, match="adaptive"):
            q.display(view)
    q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 3])
def test_gpu_display_low_resolution_upscale(cornell, luts, s):
    r = _renderer(cornell, luts)
    r.render_samples(make_frames(cornell, n=4, low=(2, 3), s=s))
    for view in (abi.VIEW_DEFAULT, abi.VIEW_PIXEL_CONVERGENCE_HEATMAP, abi.VIEW_NORMALS):
        st = r.display_settings(view, low_resolution=True)
        assert st.resolution_scaling == s
        got = r.display(view, low_resolution=True)
        want = _host_view(r, view, st)
        assert np.array_equal(got, want), f"view {view}: {(got != want).sum()} bytes differ"
        full = _host_view(r, view, r.display_settings(view))
        assert np.array_equal(got, _upscale(full, s))       # the top-left block, scaled up
    r.close()


@pytest.mark.gpu
def test_gpu_display_partition_rows(rendered, cornell, luts):
    whole = {v: rendered.display(v) for v in (abi.VIEW_DEFAULT, abi.VIEW_PIXEL_CONVERGED_MAP)}
    for k in range(2):
        r = _renderer(cornell, luts)
        r.render_samples(make_frames(cornell, band=(8, k, 2)))
        ys = partition.rows_of(H, 8, k, 2)
        for v, img in whole.items():
            got = r.display(v)
            assert got.shape == (len(ys), W, 4)
            assert np.array_equal(got, img[ys]), f"band {k} view {v}"
        st = r.display_settings()
        st.resolution_scaling = 2
        with pytest.raises(mpt.MptError) as e:
            r.display(settings=st)
        assert e.value.code == abi.ERR_UNSUPPORTED
        r.close()


@pytest.mark.gpu
def test_gpu_display_is_ordered_after_the_frames_and_leaves_the_sums(cornell, luts, oracle_lib):
    import torch
    frs = make_frames(cornell, n=6)
    r = _renderer(cornell, luts)
    dst = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_samples(frs[:4])
    r.display_to_device(dst.data_ptr())                      # straight after the frames: no synchronise
    r.synchronize_kernel()
    early = dst.cpu().numpy().reshape(H, W, 4)
    before = r.framebuffer(abi.FB_COLOR)
    assert np.array_equal(early, r.display())
    for v in abi.VIEWS:
        r.display(v, second=before if v == abi.VIEW_BLEND else None)
    assert np.array_equal(r.framebuffer(abi.FB_COLOR), before)
    r.render_samples(frs[4:])
    r.synchronize_kernel()
    got = r.framebuffer(abi.FB_COLOR)
    cnt = r.aux_buffer(abi.AUX_CONVERGED_SAMPLE_COUNT)
    r.close()
    o = oracle_lib.Oracle(cornell, luts)
    ref = o.render(frs)
    conv = o.last_aux.get("converged_sample_count")
    o.close()
    assert np.array_equal(got, ref), f"{(got != ref).sum()} values differ from the oracle after displaying"
    if conv is not None:
        assert np.array_equal(cnt, conv)


@pytest.mark.gpu
def test_gpu_display_row_tails(cornell, luts):
    """Widths that are no multiple of the 4 pixels a lane handles (and one that is), two rows."""
    r = _renderer(cornell, luts)
    for w in (1, 3, 5, 64):
        r.render_samples(make_frames(cornell, n=2, w=w, h=2))
        for view in (abi.VIEW_DEFAULT, abi.VIEW_ALBEDO, abi.VIEW_PIXEL_CONVERGENCE_HEATMAP):
            st = r.display_settings(view)
            got = r.display(view)
            want = _host_view(r, view, st)
            assert got.shape == (2, w, 4)
            assert np.array_equal(got, want), f"width {w} view {view}"
    r.close()
