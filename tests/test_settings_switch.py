"""Settings switches in a used context: adaptive sampling, its minimum and the stop-noise
threshold changed between frames without a reset (what the reference's UI does), rendered
sample by sample and through mpt_render_frames.

The host scheduler carries state from frame to frame and from call to call: its bound on
pixel_sample_count, the adaptive buffers, the speculative batch's flags and the choice of which
frames share a wavefront.  A sequence is a list of segments (n_frames, mode, overrides), mode in
plain | stop | adaptive | both; only frame 0 is a reset frame.

CPU: the oracle's state at every switch is the mix the sequence needs (converged and sampling
pixels side by side), and a pixel that the stop-noise frames marked converged is frozen by the
adaptive frames that follow (AdaptiveSampling.h:45-48, CameraRays.h:107-121).
GPU: every schedule of the same frame list -- per frame, batched, batched with the library's
own cap, split over three calls -- equals the oracle's sequential render bit for bit."""
import functools

import numpy as np
import pytest

from mpt import abi
from test_restir import _renderer, frames, render_partitioned_local

W, H, N = 32, 24, 12
STOP_THRESHOLD, ADAPTIVE_THRESHOLD = 0.5, 0.9


def _min(m):
    return {"adaptive_sampling_min_samples": m}


SEQUENCES = {
    "stop3_then_adaptive_min6": [(3, "stop", {}), (9, "adaptive", _min(6))],
    "min2_then_min10": [(6, "adaptive", _min(2)), (6, "adaptive", _min(10))],
    "min8_then_min2": [(5, "adaptive", _min(8)), (7, "adaptive", _min(2))],
    "adaptive_stop_adaptive": [(5, "adaptive", _min(2)), (3, "stop", {}), (4, "adaptive", _min(9))],
    "plain_then_adaptive": [(4, "plain", {}), (8, "adaptive", _min(3))],
    "adaptive_plain_adaptive": [(5, "adaptive", _min(2)), (3, "plain", {}), (4, "adaptive", _min(8))],
    "both_then_adaptive": [(5, "both", _min(2)), (7, "adaptive", _min(9))],
}
STRATEGIES = {
    "restir_di": (abi.LSS_RESTIR_DI, dict(bounces=1, reuse_radius=5)),
    "mis": (abi.LSS_MIS_LIGHT_BSDF, dict(bounces=3)),
}
# The oracle's state at each switch, measured once on the CPU (768 pixels): the number of pixels
# with a converged count, then the range of pixel_sample_count.
AT_SWITCH = {
    "stop3_then_adaptive_min6": {"restir_di": [(35, 3, 3)], "mis": [(6, 3, 3)]},
    "min2_then_min10": {"restir_di": [(699, 3, 6)], "mis": [(716, 3, 6)]},
    "min8_then_min2": {"restir_di": [(0, 5, 5)], "mis": [(0, 5, 5)]},
    "adaptive_stop_adaptive": {"restir_di": [(666, 3, 5), (62, 6, 8)], "mis": [(691, 3, 5), (57, 6, 8)]},
    "plain_then_adaptive": {"restir_di": [(0, 0, 0)], "mis": [(0, 0, 0)]},
    "adaptive_plain_adaptive": {"restir_di": [(666, 3, 5), (666, 3, 5)], "mis": [(691, 3, 5), (691, 3, 5)]},
    "both_then_adaptive": {"restir_di": [(666, 3, 5)], "mis": [(691, 3, 5)]},
}
CASES = [(s, t) for s in SEQUENCES for t in STRATEGIES]
CASE_IDS = [f"{s}-{t}" for s, t in CASES]


def apply_segments(frs, segments):
    """Sets each frame's adaptive-sampling fields from its segment."""
    assert sum(n for n, _, _ in segments) == len(frs)
    k = 0
    for n, mode, overrides in segments:
        for f in frs[k:k + n]:
            rs = f.render_settings
            rs.enable_adaptive_sampling = mode in ("adaptive", "both")
            rs.adaptive_sampling_noise_threshold = ADAPTIVE_THRESHOLD
            rs.enable_pixel_stop_noise_threshold = mode in ("stop", "both")
            rs.stop_pixel_noise_threshold = STOP_THRESHOLD if mode in ("stop", "both") else 0.0
            for name, v in overrides.items():
                assert hasattr(rs, name), name
                setattr(rs, name, v)
            rs.do_update_status_buffers = True
        k += n
    return frs


def switches(segments):
    """Frame indices at which the settings change."""
    out, k = [], 0
    for n, _, _ in segments[:-1]:
        k += n
        out.append(k)
    return out


def sequence_frames(sd, seq, strat, w=W, h=H, band=(1, 0, 1)):
    lss, kw = STRATEGIES[strat]
    frs = apply_segments(frames(sd, lss, N, w=w, h=h, band=band, **kw), SEQUENCES[seq])
    assert [k for k, f in enumerate(frs) if f.render_settings.need_to_reset or f.render_settings.sample_number == 0] == [0]
    return frs


def _oracle_render(sd, luts, frs):
    from oracle import oracle as orc
    o = orc.Oracle(sd, luts)
    c, ca, cn = o.render(frs, aov=True)
    aux = o.last_aux
    o.close()
    out = {"color": c, "albedo": ca, "normals": cn, "sample_count": aux["sample_count"],
           "converged_sample_count": aux["converged_sample_count"], "squared_luminance": aux["squared_luminance"],
           "status": {"one_ray_active": aux["one_ray_active"], "pixel_converged_count": aux["pixel_converged_count"]}}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


_scene_of = {}


@functools.lru_cache(maxsize=None)
def _reference_cached(key, seq, strat, upto, w, h):
    sd, luts = _scene_of[key]
    return _oracle_render(sd, luts, sequence_frames(sd, seq, strat, w=w, h=h)[:upto])


def reference(sd, luts, seq, strat, upto=N, w=W, h=H):
    """The oracle's sequential render of the sequence's first `upto` frames in a fresh renderer:
    computed once per module run, shared read-only by the tests."""
    _scene_of[id(sd)] = (sd, luts)
    return _reference_cached(id(sd), seq, strat, upto, w, h)


# ---- CPU: the oracle's state at the switches ----

@pytest.mark.parametrize("seq,strat", CASES, ids=CASE_IDS)
def test_oracle_switch_preconditions(cornell, luts, oracle_lib, seq, strat):
    """A schedule test on a sequence whose switch happens with nothing converged proves nothing:
    at every switch the oracle holds at least 3 pixels with a converged count and at least 3
    without -- except min8_then_min2 (none converged, every count 5: the bound alone moves) and
    plain_then_adaptive (no adaptive buffers yet: every count 0) -- and exactly the recorded mix."""
    sws = switches(SEQUENCES[seq])
    assert len(sws) == len(AT_SWITCH[seq][strat])
    for k, want in zip(sws, AT_SWITCH[seq][strat]):
        ref = reference(cornell, luts, seq, strat, upto=k)
        conv, cnt = ref["converged_sample_count"], ref["sample_count"]
        got = (int((conv >= 0).sum()), int(cnt.min()), int(cnt.max()))
        print(f"{seq} {strat} switch at frame {k}: converged {got[0]} of {conv.size}, sample_count {got[1]}..{got[2]}")
        assert np.isfinite(ref["color"]).all()
        if seq == "min8_then_min2":
            assert got[0] == 0 and (cnt == 5).all()
        elif seq == "plain_then_adaptive":
            assert got[0] == 0 and (cnt == 0).all()
        else:
            assert got[0] >= 3 and conv.size - got[0] >= 3, got
        assert got == want, (got, want)
    full = reference(cornell, luts, seq, strat)
    assert np.isfinite(full["color"]).all() and full["color"].mean() > 0


@pytest.mark.parametrize("strat", list(STRATEGIES))
def test_oracle_stop_then_adaptive_freezes_converged(cornell, luts, oracle_lib, strat):
    """stop3_then_adaptive_min6: a pixel the three stop-noise frames left with a converged count is
    refused by every adaptive frame after them (the count is sticky, AdaptiveSampling.h:45-48),
    although its 3 samples are below the adaptive minimum of 6: it keeps sample_count 3 and its
    converged count, and its sum is the 3-frame sum rescaled by (k + 1) / k for k = 3..11
    (CameraRays.h:118), i.e. times 12 / 3 up to the rounding of those 9 fp32 steps.  The tolerance
    is 4x the largest relative deviation of that fp32 chain from the same chain in float64,
    measured 1.92e-07 (ReSTIR DI, 35 pixels) and 1.28e-07 (MIS, 6 pixels), so 7.7e-07 / 5.1e-07.
    The converged count
    is the pixel's sample count *before* its third sample, 2: the stop-noise branch stores
    pixel_sample_count (AdaptiveSampling.h:81-97) ahead of the increment (CameraRays.h:124), and
    the third frame is the first with sample_number > 1.  The pixels not converged at the switch
    keep sampling: their sums leave the frozen value."""
    seq = "stop3_then_adaptive_min6"
    at = reference(cornell, luts, seq, strat, upto=3)
    end = reference(cornell, luts, seq, strat)
    done = at["converged_sample_count"] >= 0
    assert done.sum() >= 3 and (~done).sum() >= 3
    assert (at["converged_sample_count"][done] == 2).all() and (at["sample_count"] == 3).all()
    assert (end["sample_count"][done] == 3).all()
    assert np.array_equal(end["converged_sample_count"][done], at["converged_sample_count"][done])
    s3 = at["color"][done]
    c32, c64 = s3.astype(np.float32), s3.astype(np.float64)
    for k in range(3, N):
        c32 = c32 / np.float32(k) * np.float32(k + 1)
        c64 = c64 / float(k) * float(k + 1)
    nz = c64 != 0.0
    dev = float(np.max(np.abs(c32.astype(np.float64)[nz] - c64[nz]) / np.abs(c64[nz])))
    tol = 4.0 * dev
    print(f"{strat}: {int(done.sum())} frozen pixels, fp32 rescale chain deviates {dev:.3e} from float64, tolerance {tol:.3e}")
    assert 0.0 < dev < 9 * 2 * 2.0 ** -24   # (at most half an ulp per fp32 operation, 18 of them)
    want = s3.astype(np.float64) * (N / 3.0)
    got = end["color"][done].astype(np.float64)
    assert nz.any() and np.array_equal(got[~nz], want[~nz])
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    assert rel.max() <= tol, (rel.max(), tol)
    # the others kept sampling: counted past the switch, and away from the frozen value -- where
    # the value can move at all: a pixel whose samples are all the same (a camera ray that sees
    # the light or leaves the scene; its variance rounds to a NaN confidence interval, so it
    # counts as unconverged) sums to the frozen value whether it samples or not, so the values are
    # compared at the pixels whose first three samples already vary
    live = ~done
    sampled = end["sample_count"][live] > 3
    assert sampled.all(), f"{int((~sampled).sum())} unconverged pixels stopped sampling at the switch"
    frozen = at["color"][live].astype(np.float64) * (N / 3.0)
    moved = np.abs(end["color"][live].astype(np.float64) - frozen).max(-1) > tol * np.abs(frozen).max(-1)
    lum = at["color"][live].astype(np.float64) @ np.array([0.3086, 0.6094, 0.0820])   # Color.h:85
    sq = at["squared_luminance"][live].astype(np.float64)
    varies = sq - lum * lum / 3.0 > 1e-4 * sq
    print(f"{strat}: {int(live.sum())} pixels sampling at the switch, {int(varies.sum())} with varying samples")
    assert varies.sum() >= live.sum() // 4
    assert moved[varies].all(), f"{int((~moved[varies]).sum())} unconverged pixels kept their frozen value"


# ---- GPU: every schedule equals the oracle ----

SCHEDULES = {
    # name: (calls as frame counts, or None for one mpt_render_frame per frame; max_batch; timed)
    "A": (None, 0, True),
    "B": ([12], 4, True),
    "C": ([12], 12, True),
    "D": ([2, 5, 5], 4, True),
    # per frame without the stage timing: one-sample frames of the plain path tracer replay a
    # captured graph, which the timing's events rule out
    "A_untimed": (None, 0, False),
}


def _run_schedule(r, frs, name):
    calls, max_batch, timed = SCHEDULES[name]
    if timed:
        r.enable_stats(timing=True)
    r.clear_status_buffers()
    if calls is None:
        for f in frs:
            r.render(f)
    else:
        assert sum(calls) == len(frs)
        k = 0
        for n in calls:
            r.render_samples(frs[k:k + n], max_batch=max_batch)
            k += n
    r.synchronize_kernel()
    got = {"color": r.framebuffer(abi.FB_COLOR), "albedo": r.framebuffer(abi.FB_ALBEDO),
           "normals": r.framebuffer(abi.FB_NORMALS), "sample_count": r.aux_buffer(abi.AUX_SAMPLE_COUNT),
           "converged_sample_count": r.aux_buffer(abi.AUX_CONVERGED_SAMPLE_COUNT),
           "squared_luminance": r.aux_buffer(abi.AUX_SQUARED_LUMINANCE), "status": r.get_status_buffer_values()}
    launches = r.stats().shade_launches if timed else None
    return got, launches


def _differences(got, ref, schedule):
    out = []
    for name, want in ref.items():
        g = got[name]
        if isinstance(want, np.ndarray):
            if g.shape != want.shape:
                out.append(f"schedule {schedule}: {name} has shape {g.shape}, not {want.shape}")
            elif not np.array_equal(g, want):
                # (bit patterns: a NaN differs from a number, and equals the same NaN)
                out.append(f"schedule {schedule}: {name} differs in {int((g != want).sum())} of {want.size} values")
        elif g != want:
            out.append(f"schedule {schedule}: {name} is {g}, the oracle's {want}")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seq,strat", CASES, ids=CASE_IDS)
def test_gpu_settings_switch_schedules_bit_exact(cornell, luts, seq, strat):
    """The sequence in a fresh context under each schedule -- A one mpt_render_frame per frame, B
    one mpt_render_frames call with max_batch 4, C with max_batch 12 (ReSTIR DI capped by the
    library), D three calls of 2, 5 and 5 frames with max_batch 4 (the host's bound on the sample
    counts survives the calls, a call boundary falls inside a segment) -- leaves the sums, AOVs,
    sample counts, converged counts, squared luminance and status values of the oracle's
    sequential render; and B did batch (fewer shading launches than A for the plain path tracer,
    no more under ReSTIR DI, whose adaptive frames run one by one once a pixel may have
    converged)."""
    ref = reference(cornell, luts, seq, strat)
    frs = sequence_frames(cornell, seq, strat)
    bad, launches = [], {}
    for name in SCHEDULES:
        r = _renderer(cornell, luts)
        got, launches[name] = _run_schedule(r, frs, name)
        r.close()
        bad += _differences(got, ref, name)
    assert not bad, f"{seq} {strat}: " + "; ".join(bad)
    assert launches["A"] > 0
    if strat == "mis":
        assert launches["B"] < launches["A"], launches
    else:
        assert launches["B"] <= launches["A"], launches


@pytest.mark.gpu
@pytest.mark.parametrize("seq", ["stop3_then_adaptive_min6", "min2_then_min10"])
def test_gpu_settings_switch_partitioned_bit_exact(cornell, luts, seq):
    """ReSTIR DI across a row partition (24x64 in 3 bands; the halo carries the neighbours'
    converged counts), batched and per frame: the assembled sums equal the whole-frame oracle."""
    w, h, nb = 24, 64, 3
    ref = reference(cornell, luts, seq, "restir_di", w=w, h=h)
    at = reference(cornell, luts, seq, "restir_di", upto=switches(SEQUENCES[seq])[0], w=w, h=h)
    n_conv = int((at["converged_sample_count"] >= 0).sum())
    assert 3 <= n_conv <= w * h - 3, n_conv   # the switch happens with converged and sampling pixels
    bad = []
    for name, batch in (("batched", 8), ("per_frame", None)):
        got = render_partitioned_local(cornell, luts, lambda band: sequence_frames(cornell, seq, "restir_di", w=w, h=h, band=band),
                                       w, h, nb, batch=batch)
        bad += _differences({"color": got}, {"color": ref["color"]}, name)
    assert not bad, f"{seq}: " + "; ".join(bad)
