"""mpt_set_temporal / mpt_temporal_accumulate / mpt_denoise_temporal on the GPU (csrc/temporal.hip:
k_primary_rays, the raw closest-hit traversal, k_temporal).

Everything is bit-identical to the host path (mpt.temporal_host, tests/test_temporal_host.py): the
visibility plane equals trace_closest on primary_rays_host's rays; motion, both history planes and
the output equal temporal_host on the downloaded visibility, get_vertices() before and after the
update and the downloaded framebuffers, over three consecutive calls per kind of motion.

With set_temporal never called nothing changes: the render after set_objects + update_transforms of
test_xform's "cornell_motion" case (40x24, 3 samples, MIS) still has the bytes it had on the parent
commit.  Golden values (first 32 hex digits of the SHA-256 of the colour, albedo and normals planes),
taken from the CPU oracle's render of the moved scene.  No GPU run of the parent commit produced
them: the oracle is independent of the code under test, and the parent commit's own suite pins its
GPU render of this very sequence to the oracle bit for bit
(tests/test_xform.py::test_render_after_update_transforms there):
    colour  2f7f172ee0dc35959a619947f0cc8498
    albedo  ed7cb23ae135a6669b3fc5ac9af59eaa
    normals b729e711d6c772997a3e7a456eb860c6
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import mpt
from mpt import abi, scene

from test_anim_host import tube
from test_gpu_parity import gpu_render
from test_refit import fresh
from test_skin import cornell_pose, cornell_skin
from test_temporal_host import same
from test_xform import case as xform_case, cornell_objects, rigid, rot_y

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = (abi.TEMPORAL_OUTPUT, abi.TEMPORAL_MOTION, abi.TEMPORAL_VISIBILITY, abi.TEMPORAL_HISTORY_A, abi.TEMPORAL_HISTORY_B)
SPP = 2


def cam_of(sd, w, h, offset=(0.0, 0.0, 0.0)):
    if sd.camera_info is None:            # (a file without a camera: make_camera's default one)
        return scene.make_camera(None, w, h)
    ci = dict(sd.camera_info)
    ci["position"] = np.asarray(ci["position"], np.float64) + np.asarray(offset, np.float64)
    return scene.make_camera(ci, w, h)


def frames_for(cam, w, h, n=SPP, band=(1, 0, 1)):
    opt = abi.KernelOptions.default()
    opt.direct_light_sampling = abi.LSS_MIS_LIGHT_BSDF
    return [scene.make_frame(cam, w, h, options=opt, settings=scene.parity_settings(3), sample_number=s, random_seed=seed, band=band)
            for s, seed in scene.cpu_seed_schedule(n)]


def all_planes(r):
    return {k: r.temporal_planes(k) for k in KINDS}


def check_call(r, sd, cam, prev_cam, prev_pos, hist, what, settings=None):
    """One r.temporal() after a render, against temporal_host; returns the new history."""
    w, h = r.frame.res_x, r.frame.res_y
    s = settings if settings is not None else r.temporal_settings()
    assert s.sample_number == SPP
    out = r.temporal(s, cam)
    got = all_planes(r)
    assert same(out, got[abi.TEMPORAL_OUTPUT]), what
    prim, t, u, v = r.trace_closest(mpt.primary_rays_host(cam, w, h))
    vis = np.stack([t, u, v, prim.view(f32)], -1).reshape(h, w, 4)
    assert same(got[abi.TEMPORAL_VISIBILITY], vis), f"{what}: visibility"
    pos = r.get_vertices()[0]
    fb = [r.framebuffer(k) for k in (abi.FB_COLOR, abi.FB_ALBEDO, abi.FB_NORMALS)]
    idx = np.asarray(sd.triangle_indices, np.int32)
    want = mpt.temporal_host(s, cam, prev_cam, vis, idx, pos, pos if prev_pos is None else prev_pos, *fb, hist)
    for name, k, x in (("output", abi.TEMPORAL_OUTPUT, want[0]), ("motion", abi.TEMPORAL_MOTION, want[1]),
                       ("history A", abi.TEMPORAL_HISTORY_A, want[2]), ("history B", abi.TEMPORAL_HISTORY_B, want[3])):
        bad = got[k].view(np.uint32) != np.ascontiguousarray(x).view(np.uint32)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[:3].tolist()}"
    return (want[2], want[3])


# ------------------------------------------------------------------------------------
# Three consecutive calls per kind of motion
# ------------------------------------------------------------------------------------
def mover(kind, luts, w, h):
    """(renderer, scene, [step_0, step_1, step_2]): step_k() moves the scene (or nothing) and returns
    the camera of call k."""
    if kind == "animation":
        _, sd = tube()
    else:
        sd = scene.load_scene("cornell_pbr")
    r = fresh(sd, luts)
    v0 = np.asarray(sd.vertices, f32).reshape(-1, 3)
    cam = cam_of(sd, w, h)
    still = lambda: cam                                                         # noqa: E731
    if kind == "camera":
        steps = [still, lambda: cam_of(sd, w, h, (0.07, 0.02, -0.1)), lambda: cam_of(sd, w, h, (0.16, 0.05, -0.25))]
    elif kind in ("vertices", "two updates"):
        sphere = (np.asarray(sd.vertex_object) == 1)[:, None]

        def to(k):
            def go():
                if kind == "two updates":                                       # a pose that no call sees comes first
                    r.update_vertices(np.where(sphere, v0 + f32([0.5, 0.3, 0]), v0).astype(f32))
                r.update_vertices(np.where(sphere, v0 + f32([0.06 * k, 0.02 * k, 0]), v0).astype(f32))
                return cam
            return go
        steps = [still, to(1), to(2)]
    elif kind == "transforms":
        ids, light, box = cornell_objects()
        c = v0[box].astype(np.float64).mean(0)
        r.set_objects(ids)

        def to(k):
            def go():
                r.update_transforms(np.stack([rigid(np.eye(3), 0, [0.05 * k, 0, 0]), rigid(rot_y(12.0 * k), c, [0.03 * k, 0.02 * k, 0])]))
                return cam
            return go
        steps = [still, to(1), to(2)]
    elif kind == "skin":
        J, Wt, _, _ = cornell_skin()
        r.set_skin(J, Wt, num_joints=4)

        def to(k):
            def go():
                r.update_skin(cornell_pose(k))
                return cam
            return go
        steps = [still, to(1), to(2)]
    else:
        assert kind == "animation"
        r.set_skin(sd.skin.joints, sd.skin.weights, num_joints=sd.skin.num_joints)
        r.set_morph(sd.morph)
        r.set_animation(sd, 0)

        def to(t):
            def go():
                r.update_animation(t)
                return cam
            return go
        steps = [to(0.3), to(0.5), to(0.8)]
    return r, sd, steps


CASES = [(k, 33, 17) for k in ("camera", "vertices", "transforms", "skin", "animation", "two updates")] + \
        [("vertices", 64, 48), ("camera", 64, 48), ("vertices", 1, 1), ("camera", 1, 1)]


@pytest.mark.parametrize("kind,w,h", CASES, ids=[f"{k}-{w}x{h}" for k, w, h in CASES])
def test_three_calls_equal_the_host_path(luts, kind, w, h):
    r, sd, steps = mover(kind, luts, w, h)
    try:
        r.set_temporal(True)
        hist, prev_cam = None, None
        for k, step in enumerate(steps):
            before = r.get_vertices()[0]
            cam = step()
            after = r.get_vertices()[0]
            if kind not in ("camera",) and (k > 0 or kind == "animation"):
                assert not np.array_equal(before, after), "the step moves the geometry"
            gpu_render(r, frames_for(cam, w, h))
            hist = check_call(r, sd, cam, cam if prev_cam is None else prev_cam, before, hist, f"{kind} {w}x{h} call {k}")
            prev_cam = cam
            lens = hist[1][..., 3]
            assert lens.max() == k + 1 or (w, h) == (1, 1), f"call {k}: lengths up to {lens.max()}"
    finally:
        r.close()


# ------------------------------------------------------------------------------------
# The denoised route, rebuilds, drops, stream ordering, refusals
# ------------------------------------------------------------------------------------
W, H = 33, 17


@pytest.fixture()
def moving(luts):
    """Cornell, 33x17, temporal on, one call made: (renderer, scene, camera, history)."""
    sd = scene.load_scene("cornell_pbr")
    r = fresh(sd, luts)
    r.set_temporal(True)
    cam = cam_of(sd, W, H)
    gpu_render(r, frames_for(cam, W, H))
    hist = check_call(r, sd, cam, cam, None, None, "first call")
    yield r, sd, cam, hist
    r.close()


def nudge(r, sd, k=1):
    v0 = np.asarray(sd.vertices, f32).reshape(-1, 3)
    sphere = (np.asarray(sd.vertex_object) == 1)[:, None]
    r.update_vertices(np.where(sphere, v0 + f32([0.05 * k, 0, 0.02 * k]), v0).astype(f32))


def test_denoise_temporal_is_the_filter_over_the_accumulated_plane(moving):
    import torch
    r, sd, cam, hist = moving
    before = r.get_vertices()[0]
    nudge(r, sd)
    fb = gpu_render(r, frames_for(cam, W, H))
    d = r.denoise_settings()
    got = r.denoise_temporal(camera=cam, denoise_settings=d)
    acc = r.temporal_planes(abi.TEMPORAL_OUTPUT)
    vis = r.temporal_planes(abi.TEMPORAL_VISIBILITY)
    want_acc = mpt.temporal_host(r.temporal_settings(), cam, cam, vis, np.asarray(sd.triangle_indices, np.int32), r.get_vertices()[0],
                                 before, *fb, hist)[0]
    assert same(acc, want_acc) and not same(acc, fb[0])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (acc, fb[1], fb[2])]
    dst = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.denoise_device(d, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), W, H, dst.data_ptr())
    r.synchronize_kernel()
    want = dst.cpu().numpy().reshape(H, W, 3)
    assert same(got, want) and same(want, mpt.denoise_host(d, acc, fb[1], fb[2]))
    ptr, n = r.denoised()
    assert n == SPP
    st = r.display_settings(abi.VIEW_BLEND)
    st.sample_number_2, st.blend_factor = n, 1.0
    assert np.array_equal(r.display_denoised(1.0), r.display(settings=st, second=want))
    # the two sample counts must agree
    d.sample_number = SPP + 1
    with pytest.raises(mpt.MptError, match="sample_number"):
        r.denoise_temporal(camera=cam, denoise_settings=d)


@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC, abi.BUILD_SAH], ids=["lbvh", "ploc", "sah"])
def test_history_survives_a_rebuild(moving, mode):
    r, sd, cam, hist = moving
    before = r.get_vertices()[0]
    nudge(r, sd)
    r.rebuild_bvh(mode=mode)
    gpu_render(r, frames_for(cam, W, H))
    hist = check_call(r, sd, cam, cam, before, hist, f"after a rebuild, mode {mode}")
    assert hist[1][..., 3].max() == 2 and np.median(hist[1][..., 3]) == 2


def test_set_scene_and_resize_drop_the_history(moving):
    r, sd, cam, hist = moving
    nudge(r, sd)
    r.set_scene(sd)                                                              # (the nudge goes with the old scene)
    gpu_render(r, frames_for(cam, W, H))
    hist = check_call(r, sd, cam, cam, None, None, "after set_scene")
    assert (hist[1][..., 3] == 1).all()
    hist = check_call(r, sd, cam, cam, None, hist, "a second call")
    assert (hist[1][..., 3] == 2).any()
    nudge(r, sd)
    r.resize(W, H)                                                               # drops the previous pose as well
    gpu_render(r, frames_for(cam, W, H))
    hist = check_call(r, sd, cam, cam, None, None, "after resize")
    assert (hist[1][..., 3] == 1).all()
    r.temporal_reset()
    assert (check_call(r, sd, cam, cam, None, None, "after reset")[1][..., 3] == 1).all()
    # another frame size: new planes, no history
    cam2 = cam_of(sd, 20, 12)
    gpu_render(r, frames_for(cam2, 20, 12))
    assert (check_call(r, sd, cam2, cam2, None, None, "another size")[1][..., 3] == 1).all()


def test_planes_of_another_frame_size_are_not_handed_out(moving):
    """A call at 33x17, then a frame at 20x12: the planes still have 33x17 elements, the wrapper's
    destination 20x12 -- the download is refused instead of overrunning it; a call at the new size
    starts over, and its planes come out at that size."""
    r, sd, cam, hist = moving
    L = mpt.lib()
    w2, h2 = 20, 12
    cam2 = cam_of(sd, w2, h2)
    gpu_render(r, frames_for(cam2, w2, h2))
    small = np.full(w2 * h2 * 4, 7.0, f32)
    for k in KINDS:
        assert L.mpt_get_temporal(r.h, k, small.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
    assert (small == 7.0).all()
    with pytest.raises(mpt.MptError, match="another frame size"):
        r.temporal_planes(abi.TEMPORAL_MOTION)
    first = check_call(r, sd, cam2, cam2, None, None, "the first call at 20x12")
    assert first[0].shape == (h2, w2, 4) and (first[1][..., 3] == 1).all()
    assert r.temporal_planes(abi.TEMPORAL_OUTPUT).shape == (h2, w2, 3)
    # and back: the 33x17 planes went with the call at 20x12
    gpu_render(r, frames_for(cam, W, H))
    with pytest.raises(mpt.MptError, match="another frame size"):
        r.temporal_planes(abi.TEMPORAL_MOTION)
    assert (check_call(r, sd, cam, cam, None, None, "back at 33x17")[1][..., 3] == 1).all()


def test_device_destination_and_stream_order(moving):
    import torch
    r, sd, cam, hist = moving
    before = r.get_vertices()[0]
    nudge(r, sd)
    dst = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    mot = torch.zeros(H * W * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for f in frames_for(cam, W, H):
        r.render(f)
    r.temporal_to_device(dst.data_ptr(), camera=cam)                             # straight after the frames: no synchronise
    r.temporal_planes_to_device(abi.TEMPORAL_MOTION, mot.data_ptr())
    r.synchronize_kernel()
    fb = [r.framebuffer(k) for k in (abi.FB_COLOR, abi.FB_ALBEDO, abi.FB_NORMALS)]
    vis = r.temporal_planes(abi.TEMPORAL_VISIBILITY)
    want = mpt.temporal_host(r.temporal_settings(), cam, cam, vis, np.asarray(sd.triangle_indices, np.int32), r.get_vertices()[0],
                             before, *fb, hist)
    assert same(dst.cpu().numpy().reshape(H, W, 3), want[0]) and same(mot.cpu().numpy().reshape(H, W, 4), want[1])
    assert (want[3][..., 3] == 2).any()


def test_refusals_change_nothing(moving, luts):
    r, sd, cam, hist = moving
    L = mpt.lib()
    snap = all_planes(r)

    def unchanged(what):
        now = all_planes(r)
        assert all(same(now[k], snap[k]) for k in KINDS), what

    for bad in (dict(sample_number=0), dict(max_history=0), dict(max_history=2000), dict(alpha=0.0), dict(alpha=float("nan")),
                dict(depth_tolerance=float("inf")), dict(normal_threshold=2.0)):
        s = r.temporal_settings()
        for k, v in bad.items():
            setattr(s, k, v)
        with pytest.raises(mpt.MptError) as e:
            r.temporal(s, cam)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT and list(bad)[0] in str(e.value)
        with pytest.raises(mpt.MptError):
            r.denoise_temporal(s, cam)
        unchanged(f"bad settings {bad}")
    s = r.temporal_settings()
    assert L.mpt_temporal_accumulate(r.h, None, C.byref(cam), None, 0) == abi.ERR_INVALID_ARGUMENT
    assert L.mpt_temporal_accumulate(r.h, C.byref(s), None, None, 0) == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(mpt.MptError):
        r.temporal_planes(17)
    unchanged("NULL arguments")
    # the refusals left the history alone: the next call continues it
    gpu_render(r, frames_for(cam, W, H))
    assert (check_call(r, sd, cam, cam, None, hist, "after the refusals")[1][..., 3] == 2).any()
    # a row partition: refused, and while the last frame is not of the planes' size they are not
    # handed out (the destination is sized from the frame); back at the size they are unchanged and
    # the history goes on
    snap = all_planes(r)
    gpu_render(r, frames_for(cam, W, H, band=(8, 0, 2)))
    with pytest.raises(mpt.MptError) as e:
        r.temporal(camera=cam)
    assert e.value.code == abi.ERR_UNSUPPORTED
    with pytest.raises(mpt.MptError):
        r.denoise_temporal(camera=cam)
    guard = np.full(W * H * 4 + 64, 7.0, f32)                                   # (room for the whole frame's plane)
    for k in KINDS:
        assert L.mpt_get_temporal(r.h, k, guard.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
        assert b"another frame size or partition" in L.mpt_last_error()
    assert (guard == 7.0).all(), "a refused download wrote to its destination"
    with pytest.raises(mpt.MptError, match="another frame size"):
        r.temporal_planes(abi.TEMPORAL_OUTPUT)
    gpu_render(r, frames_for(cam, W, H))
    unchanged("the row partition's refusal")
    assert check_call(r, sd, cam, cam, None, (snap[abi.TEMPORAL_HISTORY_A], snap[abi.TEMPORAL_HISTORY_B]),
                      "after the partition")[1][..., 3].max() == 3
    # off, and nothing rendered
    b = fresh(sd, luts)
    try:
        out = np.zeros((H, W, 3), f32)
        assert L.mpt_temporal_accumulate(b.h, C.byref(s), C.byref(cam), out.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
        assert b"mpt_set_temporal is off" in L.mpt_last_error()
        assert L.mpt_temporal_reset(b.h) == abi.ERR_INVALID_ARGUMENT
        assert L.mpt_get_temporal(b.h, abi.TEMPORAL_OUTPUT, out.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
        b.set_temporal(True)
        assert L.mpt_temporal_accumulate(b.h, C.byref(s), C.byref(cam), out.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
        assert b"no frame rendered" in L.mpt_last_error()
        assert L.mpt_get_temporal(b.h, abi.TEMPORAL_OUTPUT, out.ctypes.data, 0) == abi.ERR_INVALID_ARGUMENT
        assert not out.any()
        gpu_render(b, frames_for(cam, W, H))
        b.temporal(camera=cam)
        b.set_temporal(False)                                                    # frees the planes
        with pytest.raises(mpt.MptError, match="off"):
            b.temporal(camera=cam)
        with pytest.raises(mpt.MptError, match="off"):
            b.temporal_planes(abi.TEMPORAL_OUTPUT)
        b.set_temporal(True)                                                     # and on again it starts over
        assert (check_call(b, sd, cam, cam, None, None, "on again")[1][..., 3] == 1).all()
    finally:
        b.close()


def test_without_set_temporal_the_bytes_are_the_parents(luts):
    sd0, ids, M, sd, nv, nn = xform_case("cornell_motion")
    from test_gpu_parity import frames
    frs = frames(sd, 40, 24, 3, lss=abi.LSS_MIS_LIGHT_BSDF)
    r = fresh(sd0, luts)
    try:
        r.set_objects(ids)
        r.update_transforms(M)
        out = gpu_render(r, frs)
    finally:
        r.close()
    got = [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32] for a in out]
    assert got == ["2f7f172ee0dc35959a619947f0cc8498", "ed7cb23ae135a6669b3fc5ac9af59eaa", "b729e711d6c772997a3e7a456eb860c6"]
