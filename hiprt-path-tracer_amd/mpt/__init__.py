"""mpt -- MI355X path tracer: Python binding of libmpt.so (include/mpt.h).

``GPURenderer`` mirrors the launch surface of the reference's
``GPURenderer`` (src/Renderer/GPURenderer.h:69-260): a scene is uploaded once, the
envmap / LUTs are set, and every ``render()`` call enqueues one sample per pixel on the
context's HIP stream (``GPURenderer::render``, GPURenderer.cpp:245-271), accumulating
into the 'pixels' sum buffer and the denoiser AOVs.

There is no CPU fallback: if libmpt.so is missing or no HIP device exists, the
constructor raises.  Build the library with ``python -m mpt._build`` or
``__graft_entry__.build()``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi
from . import scene
from ._build import LIB_PATH

__all__ = ["abi", "scene", "lib", "GPURenderer", "MptError", "build_envmap", "partition_rows", "display_settings",
           "display_host", "write_png", "denoise_host", "bvh_refit_host", "bvh_build_host", "transform_host", "skin_host",
           "SKIN_LDS_JOINTS", "morph_host", "MORPH_LDS_TARGETS", "animation_tables", "animation_host", "ANIM_LDS_NODES",
           "normal_groups", "normal_flips", "normals_host", "primary_rays_host", "temporal_host"]

SYMBOLS = [
    "mpt_last_error", "mpt_version", "mpt_abi_sizes", "mpt_create", "mpt_destroy", "mpt_upload_scene",
    "mpt_update_materials", "mpt_set_envmap", "mpt_build_alias_table", "mpt_set_luts", "mpt_resize",
    "mpt_render_frame", "mpt_render_frames", "mpt_synchronize", "mpt_query_done", "mpt_get_framebuffer", "mpt_partition_rows",
    "mpt_enable_stats", "mpt_get_stats", "mpt_trace_closest", "mpt_trace_any", "mpt_clear_status",
    "mpt_query_status", "mpt_get_aux_buffer", "mpt_build_envmap_cdf", "mpt_set_envmap_cdf", "mpt_set_halo_exchange",
    "mpt_set_halo_native", "mpt_halo_plan", "mpt_set_pipeline",
    "mpt_bake_lut", "mpt_png_unfilter", "mpt_device_info", "mpt_gather", "mpt_comm_unique_id", "mpt_comm_init",
    "mpt_comm_gather", "mpt_jpeg_decode", "mpt_hdr_decode",
    "mpt_display_settings_default", "mpt_display_uniforms", "mpt_display", "mpt_display_host", "mpt_write_png",
    "mpt_denoise_settings_default", "mpt_denoise", "mpt_denoised_buffer", "mpt_denoise_device", "mpt_denoise_host",
    "mpt_update_vertices", "mpt_get_bvh", "mpt_bvh_refit_host", "mpt_rebuild_bvh", "mpt_bvh_build_host",
    "mpt_rebuild_bvh_mode", "mpt_bvh_build_host_mode", "mpt_upload_scene_mode",
    "mpt_set_objects", "mpt_update_transforms", "mpt_update_vertices_device", "mpt_transform_host",
    "mpt_set_skin", "mpt_update_skin", "mpt_skin_host",
    "mpt_set_morph", "mpt_update_morph", "mpt_update_morph_skin", "mpt_morph_host",
    "mpt_set_animation", "mpt_update_animation", "mpt_animation_host",
    "mpt_set_normals", "mpt_normals_host", "mpt_get_vertices",
    "mpt_temporal_settings_default", "mpt_set_temporal", "mpt_temporal_accumulate", "mpt_temporal_reset", "mpt_get_temporal",
    "mpt_denoise_temporal", "mpt_primary_rays_host", "mpt_temporal_host",
]

SKIN_LDS_JOINTS = abi.SKIN_LDS_JOINTS
MORPH_LDS_TARGETS = abi.MORPH_LDS_TARGETS
ANIM_LDS_NODES = abi.ANIM_LDS_NODES


class MptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mpt error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Loads the in-tree libmpt.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MPT_LIB_PATH", str(LIB_PATH))   # development variants
    if not os.path.exists(path):
        raise ImportError(f"libmpt.so not found at {path}; run __graft_entry__.build() (no CPU fallback)")
    # One HIP runtime per process.  The torch wheel ships its own libamdhip64 (same SONAME,
    # libamdhip64.so.7) next to libc10_hip; loading libmpt first would map /opt/rocm's copy
    # and torch's would then find no device.  Loading torch first makes libmpt bind to the
    # runtime torch already mapped, so libmpt buffers, torch tensors and RCCL share one
    # runtime (measured: same bit-exact results and the same C3 throughput on either).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.mpt_last_error.restype = C.c_char_p
    L.mpt_abi_sizes.argtypes = [vp, C.c_int]
    L.mpt_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.mpt_destroy.argtypes = [vp]
    L.mpt_upload_scene.argtypes = [vp, C.POINTER(abi.Scene)]
    L.mpt_update_materials.argtypes = [vp, vp, i32]
    L.mpt_set_envmap.argtypes = [vp, vp, i32, i32, vp, vp, f32]
    L.mpt_build_alias_table.argtypes = [vp, i32, i32, vp, vp, vp]
    L.mpt_set_luts.argtypes = [vp, C.POINTER(abi.Luts)]
    L.mpt_resize.argtypes = [vp, i32, i32]
    L.mpt_render_frame.argtypes = [vp, C.POINTER(abi.Frame)]
    L.mpt_render_frames.argtypes = [vp, C.POINTER(abi.Frame), i32, i32]
    L.mpt_synchronize.argtypes = [vp]
    L.mpt_query_done.argtypes = [vp, C.POINTER(C.c_int)]
    L.mpt_get_framebuffer.argtypes = [vp, C.c_int, vp, C.c_int]
    L.mpt_partition_rows.argtypes = [i32, i32, i32, i32]
    L.mpt_enable_stats.argtypes = [vp, C.c_int, C.c_int]
    L.mpt_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.mpt_trace_closest.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, C.c_int]
    L.mpt_trace_any.argtypes = [vp, vp, vp, i32, vp, C.c_int]
    L.mpt_png_unfilter.argtypes = [vp, C.c_int64, vp, i32, i32, i32]
    L.mpt_device_info.argtypes = [C.c_int, vp, i32, vp, i32, vp]
    L.mpt_build_envmap_cdf.argtypes = [vp, i32, i32, vp, vp]
    L.mpt_set_envmap_cdf.argtypes = [vp, vp, f32]
    L.mpt_clear_status.argtypes = [vp]
    L.mpt_query_status.argtypes = [vp, C.POINTER(abi.Status)]
    L.mpt_get_aux_buffer.argtypes = [vp, C.c_int, vp, C.c_int]
    L.mpt_set_halo_exchange.argtypes = [vp, abi.HaloExchangeFn, vp]
    L.mpt_set_halo_native.argtypes = [vp, C.c_int32]
    L.mpt_set_pipeline.argtypes = [vp, C.c_int32]
    L.mpt_halo_plan.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(abi.HaloOp), i32]
    L.mpt_bake_lut.argtypes = [vp, C.c_int, i32, i32, i32, i32, vp, C.c_int]
    L.mpt_gather.argtypes = [C.POINTER(vp), i32, i32, C.c_int, vp, C.c_int]
    L.mpt_comm_unique_id.argtypes = [vp, i32]
    L.mpt_comm_init.argtypes = [vp, i32, i32, vp]
    L.mpt_comm_gather.argtypes = [vp, i32, C.c_int, vp, C.c_int]
    L.mpt_jpeg_decode.argtypes = [vp, C.c_int64, i32, vp, C.c_int64, vp, vp, vp]
    L.mpt_hdr_decode.argtypes = [vp, C.c_int64, i32, vp, C.c_int64, vp, vp]
    L.mpt_display_settings_default.argtypes = [C.POINTER(abi.DisplaySettings)]
    L.mpt_display_uniforms.argtypes = [C.POINTER(abi.RenderSettings), i32, i32, C.POINTER(abi.DisplaySettings)]
    L.mpt_display.argtypes = [vp, C.POINTER(abi.DisplaySettings), vp, C.c_int, vp, C.c_int]
    L.mpt_display_host.argtypes = [C.POINTER(abi.DisplaySettings), vp, vp, i32, i32, vp]
    L.mpt_write_png.argtypes = [C.c_char_p, vp, i32, i32, i32]
    L.mpt_denoise_settings_default.argtypes = [C.POINTER(abi.DenoiseSettings)]
    L.mpt_denoise.argtypes = [vp, C.POINTER(abi.DenoiseSettings), vp, C.c_int]
    L.mpt_denoised_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    L.mpt_denoise_device.argtypes = [vp, C.POINTER(abi.DenoiseSettings), vp, vp, vp, i32, i32, vp]
    L.mpt_denoise_host.argtypes = [C.POINTER(abi.DenoiseSettings), vp, vp, vp, i32, i32, vp]
    L.mpt_update_vertices.argtypes = [vp, vp, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_get_bvh.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, vp]
    L.mpt_bvh_refit_host.argtypes = [vp, vp, i32, vp, i32, vp, C.c_int64, vp, C.c_int64, vp]
    L.mpt_rebuild_bvh.argtypes = [vp, C.POINTER(abi.RebuildInfo)]
    L.mpt_bvh_build_host.argtypes = [vp, i32, vp, i32, vp, i32, vp, C.c_int64, vp, C.c_int64, vp]
    L.mpt_rebuild_bvh_mode.argtypes = [vp, i32, C.POINTER(abi.RebuildInfo)]
    L.mpt_bvh_build_host_mode.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp, C.c_int64, vp, C.c_int64, vp]
    L.mpt_upload_scene_mode.argtypes = [vp, C.POINTER(abi.Scene), i32, C.POINTER(abi.RebuildInfo)]
    L.mpt_set_objects.argtypes = [vp, vp, i32, i32]
    L.mpt_update_transforms.argtypes = [vp, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_update_vertices_device.argtypes = [vp, vp, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_transform_host.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp]
    L.mpt_set_skin.argtypes = [vp, vp, vp, i32, i32]
    L.mpt_update_skin.argtypes = [vp, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_skin_host.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, vp]
    L.mpt_set_morph.argtypes = [vp, i32, vp, vp, vp, vp, i32]
    L.mpt_update_morph.argtypes = [vp, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_update_morph_skin.argtypes = [vp, vp, i32, vp, i32, C.POINTER(abi.RefitInfo)]
    L.mpt_morph_host.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.mpt_set_animation.argtypes = [vp, C.POINTER(abi.Animation)]
    L.mpt_update_animation.argtypes = [vp, C.c_float, C.POINTER(abi.RefitInfo)]
    L.mpt_animation_host.argtypes = [C.POINTER(abi.Animation), C.c_float, vp, vp]
    L.mpt_set_normals.argtypes = [vp, vp, vp, i32, i32]
    L.mpt_normals_host.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, vp]
    L.mpt_get_vertices.argtypes = [vp, vp, vp, i32]
    L.mpt_temporal_settings_default.argtypes = [C.POINTER(abi.TemporalSettings)]
    L.mpt_set_temporal.argtypes = [vp, C.c_int]
    L.mpt_temporal_accumulate.argtypes = [vp, C.POINTER(abi.TemporalSettings), C.POINTER(abi.Camera), vp, C.c_int]
    L.mpt_temporal_reset.argtypes = [vp]
    L.mpt_get_temporal.argtypes = [vp, C.c_int, vp, C.c_int]
    L.mpt_denoise_temporal.argtypes = [vp, C.POINTER(abi.TemporalSettings), C.POINTER(abi.Camera), C.POINTER(abi.DenoiseSettings),
                                       vp, C.c_int]
    L.mpt_primary_rays_host.argtypes = [C.POINTER(abi.Camera), i32, i32, vp]
    L.mpt_temporal_host.argtypes = [C.POINTER(abi.TemporalHostArgs)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MptError(rc, lib().mpt_last_error().decode(errors="replace"))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def abi_sizes():
    out = np.zeros(8, np.int32)
    _check(lib().mpt_abi_sizes(_p(out), 8))
    sizes = dict(zip(["Material", "RenderSettings", "WorldSettings", "Camera", "Frame", "Scene", "Stats",
                      "DisplaySettings"], out.tolist()))
    if sizes["DisplaySettings"] != C.sizeof(abi.DisplaySettings):
        raise MptError(abi.ERR_INVALID_ARGUMENT, f"MptDisplaySettings is {sizes['DisplaySettings']} bytes in libmpt.so, "
                       f"{C.sizeof(abi.DisplaySettings)} in mpt.abi")
    return sizes


def device_info(device=0):
    """(name, gfx arch, compute units) of a HIP device (mpt_device_info)."""
    name, arch, cus = C.create_string_buffer(256), C.create_string_buffer(64), C.c_int32()
    _check(lib().mpt_device_info(device, name, 256, arch, 64, C.byref(cus)))
    return name.value.decode(errors="replace"), arch.value.decode(errors="replace"), int(cus.value)


def build_id():
    """First 16 hex digits of the SHA-256 of the loaded libmpt.so (identifies the build a line ran)."""
    import hashlib
    return hashlib.sha256(open(lib()._name, "rb").read()).hexdigest()[:16]


def partition_rows(res_y, band_height, band_index, band_count):
    return lib().mpt_partition_rows(res_y, band_height, band_index, band_count)


def halo_plan(res_y, band_height, band_count, band_index, halo_rows, n_buffers=1):
    """mpt_halo_plan: the library's halo-exchange operations for one band, in issue order, as
    (peer, 'send' | 'recv', buffer, row_lo, row_hi) tuples (host only, no device needed)."""
    args = (res_y, band_height, band_count, band_index, halo_rows, n_buffers)
    n = lib().mpt_halo_plan(*args, None, 0)
    _check(min(n, 0))
    ops = (abi.HaloOp * max(n, 1))()
    m = lib().mpt_halo_plan(*args, ops, n)
    _check(min(m, 0))
    return [(o.peer, "recv" if o.recv else "send", o.buffer, o.row_lo, o.row_hi) for o in ops[:m]]


GATHER_AUX = 16   # mpt.h MPT_GATHER_AUX: gather kind of an MPT_AUX_* buffer


def _gather_out(f, kind):
    if kind >= GATHER_AUX:
        return np.zeros((f.res_y, f.res_x), np.float32 if kind == GATHER_AUX + abi.AUX_SQUARED_LUMINANCE else np.int32)
    return np.zeros((f.res_y, f.res_x, 3), np.float32)


def gather(renderers, root=0, kind=abi.FB_COLOR):
    """mpt_gather: the whole frame of buffer `kind` from the renderers that render the row
    partitions band_index = 0..n-1 of one frame (one process; peer copies between GPUs) ->
    host array [res_y, res_x(, 3)]."""
    f = renderers[root].frame
    out = _gather_out(f, kind)
    hs = (C.c_void_p * len(renderers))(*[r.h for r in renderers])
    _check(lib().mpt_gather(hs, len(renderers), root, kind, _p(out), 0))
    return out


def comm_unique_id() -> bytes:
    """mpt_comm_unique_id (rank 0; share the bytes with the other ranks out of band)."""
    buf = (C.c_uint8 * 128)()
    _check(lib().mpt_comm_unique_id(buf, 128))
    return bytes(buf)


def build_envmap(rgba):
    """float32 [H, W, 4] (already flipped as the reference's loader does) -> envmap dict
    with the alias table of Image32Bit::compute_alias_table (Image.cpp:579-659)."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    probas = np.zeros(h * w, np.float32)
    alias = np.full(h * w, -1, np.int32)
    s = np.zeros(1, np.float32)
    _check(lib().mpt_build_alias_table(_p(rgba), w, h, _p(probas), _p(alias), _p(s)))
    alias = np.where(alias < 0, np.arange(h * w, dtype=np.int32), alias).astype(np.int32)
    # ESS_BINARY_SEARCH: luminance CDF, Image32Bit::compute_cdf (Image.cpp:553-574)
    cdf = np.zeros(h * w, np.float32)
    cs = np.zeros(1, np.float32)
    _check(lib().mpt_build_envmap_cdf(_p(rgba), w, h, _p(cdf), _p(cs)))
    return {"rgba": rgba, "probas": probas, "alias": alias, "width": w, "height": h, "sum": float(s[0]),
            "cdf": cdf, "cdf_sum": float(cs[0])}


def display_settings(render_settings=None, view=abi.VIEW_DEFAULT, low_resolution=False, base=None):
    """abi.DisplaySettings for `view`: mpt_display_settings_default (or a copy of `base`), then,
    given the reference's render settings (sample_number = samples rendered so far), the per-view
    uniforms of mpt_display_uniforms."""
    s = abi.DisplaySettings()
    if base is not None:
        C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
    else:
        _check(lib().mpt_display_settings_default(C.byref(s)))
    s.view = view
    if render_settings is not None:
        _check(lib().mpt_display_uniforms(C.byref(render_settings), view, int(bool(low_resolution)), C.byref(s)))
    return s


def display_host(settings, src, src2=None):
    """mpt_display_host: the display view of host arrays, no GPU.  src: float32 [H, W, 3] (int32
    [H, W] for the heat map and the converged map), src2: the blend view's second buffer ->
    uint8 [H, W, 4]."""
    counts = settings.view in (abi.VIEW_PIXEL_CONVERGENCE_HEATMAP, abi.VIEW_PIXEL_CONVERGED_MAP)
    src = np.ascontiguousarray(src, np.int32 if counts else np.float32)
    if src.ndim != (2 if counts else 3) or (not counts and src.shape[2] != 3):
        raise ValueError(f"display_host: source of shape {src.shape}")
    h, w = src.shape[:2]
    if src2 is not None:
        src2 = np.ascontiguousarray(src2, np.float32)
        if src2.shape != (h, w, 3):
            raise ValueError(f"display_host: second buffer of shape {src2.shape}")
    out = np.zeros((h, w, 4), np.uint8)
    _check(lib().mpt_display_host(C.byref(settings), _p(src), _p(src2), w, h, _p(out)))
    return out


def write_png(path, rgba8, flip_y=False):
    """mpt_write_png: uint8 [H, W, 4] -> an 8-bit RGBA PNG (flip_y: last row first, as the
    reference's screenshots are written)."""
    img = np.ascontiguousarray(rgba8, np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"write_png: image of shape {img.shape}")
    _check(lib().mpt_write_png(os.fsencode(path), _p(img), img.shape[1], img.shape[0], int(bool(flip_y))))


def denoise_host(settings, color, albedo, normals):
    """mpt_denoise_host: the a-trous denoiser on host arrays, no GPU.  color (sums over
    settings.sample_number samples), albedo, normals: float32 [H, W, 3] -> float32 [H, W, 3], sums
    in the units of `color`."""
    color, albedo, normals = (np.ascontiguousarray(a, np.float32) for a in (color, albedo, normals))
    if color.ndim != 3 or color.shape[2] != 3 or albedo.shape != color.shape or normals.shape != color.shape:
        raise ValueError(f"denoise_host: planes of shapes {color.shape}, {albedo.shape}, {normals.shape}")
    out = np.zeros_like(color)
    _check(lib().mpt_denoise_host(C.byref(settings), _p(color), _p(albedo), _p(normals), color.shape[1], color.shape[0],
                                  _p(out)))
    return out


def primary_rays_host(camera, width, height):
    """mpt_primary_rays_host, no GPU: the centre rays of a width x height frame as
    GPURenderer.temporal traces them -> float32 [height * width, 8] in trace_closest's layout."""
    out = np.zeros((int(width) * int(height), 8), np.float32)
    _check(lib().mpt_primary_rays_host(C.byref(camera), int(width), int(height), _p(out)))
    return out


def temporal_host(settings, camera, prev_camera, visibility, indices, positions, prev_positions, color, albedo, normals,
                  history=None):
    """mpt_temporal_host, no GPU: one temporal accumulation on host arrays -- what GPURenderer.temporal
    computes.  visibility: float32 [H, W, 4] {t, u, v, prim bits} of the centre rays (the host has no
    traversal); indices int32 [T, 3]; positions, prev_positions float32 [V, 3]; color (sums over
    settings.sample_number samples), albedo, normals float32 [H, W, 3]; history: None or the
    (history_a, history_b) pair of the previous call.  Returns (output [H, W, 3], motion [H, W, 4],
    history_a [H, W, 4], history_b [H, W, 4])."""
    vis = np.ascontiguousarray(visibility, np.float32)
    if vis.ndim != 3 or vis.shape[2] != 4:
        raise ValueError(f"temporal_host: visibility of shape {vis.shape}")
    h, w = vis.shape[:2]
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    prev = np.ascontiguousarray(prev_positions, np.float32).reshape(-1, 3)
    if prev.shape != pos.shape:
        raise ValueError(f"temporal_host: {prev.shape[0]} previous positions for {pos.shape[0]}")
    color, albedo, normals = (np.ascontiguousarray(a, np.float32) for a in (color, albedo, normals))
    for a in (color, albedo, normals):
        if a.shape != (h, w, 3):
            raise ValueError(f"temporal_host: plane of shape {a.shape} for a {w} x {h} frame")
    ha = hb = None
    if history is not None:
        ha, hb = (np.ascontiguousarray(a, np.float32) for a in history)
        if ha.shape != (h, w, 4) or hb.shape != (h, w, 4):
            raise ValueError(f"temporal_host: history planes of shapes {ha.shape}, {hb.shape}")
    out, motion = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.float32)
    oa, ob = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    a = abi.TemporalHostArgs()
    a.settings, a.camera, a.prev_camera = settings, camera, prev_camera
    a.width, a.height, a.num_vertices, a.num_triangles = w, h, len(pos), len(idx)
    a.visibility, a.indices, a.positions, a.prev_positions = vis.ctypes.data, idx.ctypes.data, pos.ctypes.data, prev.ctypes.data
    a.color, a.albedo, a.normals = color.ctypes.data, albedo.ctypes.data, normals.ctypes.data
    a.history_in_a = None if ha is None else ha.ctypes.data
    a.history_in_b = None if hb is None else hb.ctypes.data
    a.history_out_a, a.history_out_b, a.output, a.motion = oa.ctypes.data, ob.ctypes.data, out.ctypes.data, motion.ctypes.data
    _check(lib().mpt_temporal_host(C.byref(a)))
    return out, motion, oa, ob


def _bvh_arrays(call):
    """The two-step download of a BVH8: counts first, then the arrays."""
    counts = np.zeros(3, np.int32)
    _check(call(None, 0, None, 0, _p(counts)))
    nodes = np.zeros(int(counts[0]), abi.NODE8_DTYPE)
    tris = np.zeros(int(counts[1]), abi.TRIREC_DTYPE)
    if counts[0] or counts[1]:
        # (an empty array still needs a non-NULL pointer)
        nb, tb = (a if a.size else np.zeros(1, a.dtype) for a in (nodes, tris))
        _check(call(_p(nb), nodes.nbytes, _p(tb), tris.nbytes, _p(counts)))
    return nodes, tris, int(counts[2])


def bvh_refit_host(build_vertices, indices, new_vertices=None):
    """mpt_bvh_refit_host, no GPU: the BVH8 built over build_vertices ([V, 3] float32) and indices
    ([T, 3] int32) as an upload builds it, refitted to new_vertices by the host loop (None: the
    builder's output).  Returns (nodes, tris, levels): structured arrays of abi.NODE8_DTYPE and
    abi.TRIREC_DTYPE, the bytes GPURenderer.get_bvh(0) returns after update_vertices (the records'
    flag lanes are 0 here)."""
    bv = np.ascontiguousarray(build_vertices, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    nv = None
    if new_vertices is not None:
        nv = np.ascontiguousarray(new_vertices, np.float32).reshape(-1, 3)
        if nv.shape != bv.shape:
            raise ValueError(f"bvh_refit_host: {nv.shape[0]} new vertices for {bv.shape[0]}")
    L = lib()
    return _bvh_arrays(lambda n, nc, t, tc, cnt: L.mpt_bvh_refit_host(_p(bv), _p(nv), bv.shape[0], _p(idx), idx.shape[0],
                                                                      n, nc, t, tc, cnt))


def bvh_build_host(vertices, indices, prims=None, mode=abi.BUILD_LBVH):
    """mpt_bvh_build_host_mode, no GPU: the BVH8 a rebuild makes (csrc/lbvh.h; mode abi.BUILD_PLOC:
    with the binary tree of csrc/ploc.h; mode abi.BUILD_SAH: with the binned-SAH tree of csrc/sah.h) over vertices ([V, 3] float32) and indices ([T, 3] int32),
    over all triangles or over the scene primitives listed in prims.  Returns (nodes, tris, levels)
    as bvh_refit_host does: the bytes GPURenderer.get_bvh returns after rebuild_bvh(mode=mode) (the
    records' flag lanes are 0 here)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    pr = None if prims is None else np.ascontiguousarray(prims, np.int32).reshape(-1)
    L = lib()
    return _bvh_arrays(lambda n, nc, t, tc, cnt: L.mpt_bvh_build_host_mode(_p(v), v.shape[0], _p(idx), idx.shape[0], _p(pr),
                                                                           0 if pr is None else pr.shape[0], int(mode),
                                                                           n, nc, t, tc, cnt))


def _matrices(matrices, who):
    """[K, 3, 4] or [K, 4, 4] (the bottom row dropped) -> contiguous float32 [K, 3, 4]."""
    m = np.asarray(matrices, np.float32)
    if m.ndim != 3 or m.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"{who}: matrices of shape {m.shape}, not [K, 3, 4] or [K, 4, 4]")
    return np.ascontiguousarray(m[:, :3, :])


def transform_host(rest_vertices, rest_normals, vertex_object, matrices):
    """mpt_transform_host, no GPU: the host loop of csrc/xform.h -- the positions ([V, 3] float32)
    and, when rest_normals is given, the vertex normals that GPURenderer.update_transforms(matrices)
    leaves on the device for this rest pose and object table (vertex_object: int32 [V], -1 for
    static vertices; matrices: [K, 3, 4] or [K, 4, 4]).  Returns (vertices, normals or None)."""
    v = np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 3)
    n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError(f"transform_host: {n.shape[0]} normals for {v.shape[0]} vertices")
    ids = np.ascontiguousarray(vertex_object, np.int32).reshape(-1)
    if len(ids) != len(v):
        raise ValueError(f"transform_host: {len(ids)} object ids for {len(v)} vertices")
    m = _matrices(matrices, "transform_host")
    ov = np.empty_like(v)
    on = None if n is None else np.empty_like(n)
    _check(lib().mpt_transform_host(_p(v), _p(n), _p(ids), len(v), _p(m), len(m), _p(ov), _p(on)))
    return ov, on


def _skin_table(joints, weights, who):
    """[V, 4] joint indices and weights -> contiguous int32 and float32 arrays."""
    j = np.ascontiguousarray(joints, np.int32)
    w = np.ascontiguousarray(weights, np.float32)
    if j.ndim != 2 or j.shape[1] != 4 or w.shape != j.shape:
        raise ValueError(f"{who}: joints of shape {j.shape} and weights of shape {w.shape}, not both [V, 4]")
    return j, w


def skin_host(rest_vertices, rest_normals, joints, weights, matrices):
    """mpt_skin_host, no GPU: the host loop of csrc/skin.h -- the positions ([V, 3] float32) and,
    when rest_normals is given, the vertex normals that GPURenderer.update_skin(matrices) leaves on
    the device for this rest pose and skin (joints: int32 [V, 4] into the palette, weights: float32
    [V, 4], all zero for a vertex that is not skinned; matrices: [J, 3, 4] or [J, 4, 4]).  Returns
    (vertices, normals or None)."""
    v = np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 3)
    n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError(f"skin_host: {n.shape[0]} normals for {v.shape[0]} vertices")
    j, w = _skin_table(joints, weights, "skin_host")
    if len(j) != len(v):
        raise ValueError(f"skin_host: {len(j)} rows of joints for {len(v)} vertices")
    m = _matrices(matrices, "skin_host")
    ov = np.empty_like(v)
    on = None if n is None else np.empty_like(n)
    _check(lib().mpt_skin_host(_p(v), _p(n), _p(j), _p(w), len(v), _p(m), len(m), _p(ov), _p(on)))
    return ov, on


def _morph_tables(morph, who):
    """A scene.MorphData, or a list with one (vertex ids, position deltas [n, 3], normal deltas
    [n, 3] or None) per target -> (T, offsets int32 [T + 1], ids int32 [N], position deltas float32
    [N, 3], normal deltas float32 [N, 3] or None: no target has any).  Each target's ids are sorted
    for the caller (a stable sort, the deltas follow); a vertex twice in one target raises
    ValueError here, before any library call."""
    if isinstance(morph, scene.MorphData):
        targets = [(morph.vertex_ids[a:b], morph.pos_deltas[a:b], None if morph.nrm_deltas is None else morph.nrm_deltas[a:b])
                   for a, b in zip(morph.target_offsets[:-1], morph.target_offsets[1:])]
    else:
        targets = list(morph)
    any_n = any(len(t) > 2 and t[2] is not None for t in targets)
    off, ids, dps, dns = [0], [], [], []
    for k, t in enumerate(targets):
        i = np.asarray(t[0], np.int64).reshape(-1)
        dp = np.asarray(t[1], np.float32).reshape(-1, 3)
        dn = None if len(t) < 3 or t[2] is None else np.asarray(t[2], np.float32).reshape(-1, 3)
        if len(dp) != len(i) or (dn is not None and len(dn) != len(i)):
            raise ValueError(f"{who}: target {k}: {len(i)} ids for {len(dp)} position deltas"
                             + ("" if dn is None else f" and {len(dn)} normal deltas"))
        if len(i) and (i.min() < -2**31 or i.max() >= 2**31):
            raise ValueError(f"{who}: target {k}: a vertex id outside int32")
        o = np.argsort(i, kind="stable")
        i = i[o]
        if np.any(i[1:] == i[:-1]):
            raise ValueError(f"{who}: target {k}: a vertex appears more than once")
        ids.append(i.astype(np.int32))
        dps.append(dp[o])
        if any_n:
            dns.append(np.zeros_like(dp) if dn is None else dn[o])
        off.append(off[-1] + len(i))
    cat = lambda parts, shape, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(shape, dt), dt)
    return (len(targets), np.asarray(off, np.int32), cat(ids, (0,), np.int32), cat(dps, (0, 3), np.float32),
            cat(dns, (0, 3), np.float32) if any_n else None)


def _morph_weights(weights, who):
    w = np.ascontiguousarray(weights, np.float32)
    if w.ndim != 1:
        raise ValueError(f"{who}: weights of shape {w.shape}, not [T]")
    return w


def morph_host(rest_vertices, rest_normals, morph, weights):
    """mpt_morph_host, no GPU: the host loop of csrc/morph.h -- the positions ([V, 3] float32) and,
    when rest_normals is given, the vertex normals that GPURenderer.update_morph(weights) leaves on
    the device for this rest pose and morph (a scene.MorphData or a list of (ids, position deltas,
    normal deltas or None) per target, as set_morph takes; weights: float32 [T]) when no skin is
    posed.  Returns (vertices, normals or None)."""
    v = np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 3)
    n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError(f"morph_host: {n.shape[0]} normals for {v.shape[0]} vertices")
    T, off, ids, dp, dn = _morph_tables(morph, "morph_host")
    w = _morph_weights(weights, "morph_host")
    if len(w) != T:
        raise ValueError(f"morph_host: {len(w)} weights for {T} targets")
    ov = np.empty_like(v)
    on = None if n is None else np.empty_like(n)
    _check(lib().mpt_morph_host(_p(v), _p(n), len(v), T, _p(off), _p(ids), _p(dp), _p(dn), _p(w), _p(ov), _p(on)))
    return ov, on


def _scene_arrays(sd_or_arrays, who):
    """A scene.SceneData, or (vertices, normals, indices[, has_normals]) -> contiguous float32 [V, 3]
    positions and normals, int32 [3T] indices and uint8 [V] normal flags (None: every vertex has one)."""
    if isinstance(sd_or_arrays, scene.SceneData):
        sd = sd_or_arrays
        parts = (sd.vertices, sd.normals, sd.triangle_indices, sd.has_normals)
    else:
        parts = tuple(sd_or_arrays)
        if len(parts) not in (3, 4):
            raise ValueError(f"{who}: a SceneData or (vertices, normals, indices[, has_normals]), not {len(parts)} arrays")
        parts = parts + (None,) * (4 - len(parts))
    v = np.ascontiguousarray(parts[0], np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(parts[1], np.float32).reshape(-1, 3)
    if n.shape != v.shape:
        raise ValueError(f"{who}: {n.shape[0]} normals for {v.shape[0]} vertices")
    idx = np.ascontiguousarray(parts[2], np.int32).reshape(-1)
    if len(idx) % 3:
        raise ValueError(f"{who}: {len(idx)} indices are no whole number of triangles")
    hn = None if parts[3] is None else np.ascontiguousarray(parts[3], np.uint8).reshape(-1)
    if hn is not None and len(hn) != len(v):
        raise ValueError(f"{who}: {len(hn)} normal flags for {len(v)} vertices")
    return v, n, idx, hn


def normal_groups(vertices, normals=None, only=None, weld=True):
    """The smoothing groups for GPURenderer.set_normals / mpt.normals_host, numpy only: returns
    (vertex_group int32 [V], num_groups).  vertices may be a scene.SceneData (its normals are then
    used).  weld=True: vertices whose position AND normal are bitwise equal share a group, which
    smooths across the splits that glTF needs at UV seams and keeps authored hard edges (their
    normals differ).  weld=False: every vertex is its own group.  only: a mask [V]; the vertices
    outside it get -1 and are never touched.  Groups are numbered in the order of their first
    vertex."""
    if isinstance(vertices, scene.SceneData):
        vertices, normals = vertices.vertices, vertices.normals
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    V = len(v)
    mask = np.ones(V, bool) if only is None else np.asarray(only, bool).reshape(-1)
    if len(mask) != V:
        raise ValueError(f"normal_groups: a mask of {len(mask)} for {V} vertices")
    sel = np.nonzero(mask)[0]
    group = np.full(V, -1, np.int32)
    if weld:
        if normals is None:
            raise ValueError("normal_groups: weld=True needs the normals")
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError(f"normal_groups: {n.shape[0]} normals for {V} vertices")
        keys = np.concatenate([v[sel], n[sel]], axis=1).view(np.uint32).reshape(len(sel), 6)
        _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        order = np.argsort(first, kind="stable")          # number the groups by their first vertex
        rank = np.empty(len(first), np.int64)
        rank[order] = np.arange(len(first))
        group[sel] = rank[inv].astype(np.int32)
        return group, int(len(first))
    group[sel] = np.arange(len(sel), dtype=np.int32)
    return group, int(len(sel))


def normals_host(vertices, indices, vertex_group, normals, flips=None, num_groups=None, has_normals=None):
    """mpt_normals_host, no GPU: the host loop of csrc/normals.h -- the vertex normals ([V, 3]
    float32, a new array) that an update leaves on the device after GPURenderer.set_normals(
    vertex_group, flips), for these positions, indices (int32 [3T]) and the normals the update itself
    produced (kept by the vertices of group -1, by vertices whose has_normals byte is 0 and wherever
    a group's sum has no positive finite length)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.array(normals, np.float32, order="C").reshape(-1, 3)
    if n.shape != v.shape:
        raise ValueError(f"normals_host: {n.shape[0]} normals for {v.shape[0]} vertices")
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
    if len(idx) % 3:
        raise ValueError(f"normals_host: {len(idx)} indices are no whole number of triangles")
    g, f, G = _normal_table(vertex_group, flips, num_groups, "normals_host")
    if len(g) != len(v):
        raise ValueError(f"normals_host: {len(g)} group ids for {len(v)} vertices")
    hn = None if has_normals is None else np.ascontiguousarray(has_normals, np.uint8).reshape(-1)
    if hn is not None and len(hn) != len(v):
        raise ValueError(f"normals_host: {len(hn)} normal flags for {len(v)} vertices")
    _check(lib().mpt_normals_host(_p(v), len(v), _p(idx), len(idx) // 3, _p(g), _p(f), G, _p(hn), _p(n)))
    return n


def _normal_table(vertex_group, flips, num_groups, who):
    g = np.ascontiguousarray(vertex_group, np.int32).reshape(-1)
    G = (int(g.max()) + 1 if len(g) else 0) if num_groups is None else int(num_groups)
    f = None if flips is None else np.ascontiguousarray(flips, np.uint8).reshape(-1)
    if f is not None and len(f) != G:
        raise ValueError(f"{who}: {len(f)} flip bytes for {G} groups")
    return g, f, G


def normal_flips(sd_or_arrays, vertex_group, num_groups):
    """The flip bytes (uint8 [num_groups]) for GPURenderer.set_normals: normals_host runs on the
    given pose -- a scene.SceneData or (vertices, normals, indices[, has_normals]) -- without flips,
    and every group whose result has a negative dot product with the authored normal of the group's
    first vertex gets its byte set.  For meshes whose winding was mirrored when the loader flattened
    a node with a negative determinant."""
    v, n, idx, hn = _scene_arrays(sd_or_arrays, "normal_flips")
    g, _, G = _normal_table(vertex_group, None, num_groups, "normal_flips")
    r = normals_host(v, idx, g, n, None, G, hn)
    flips = np.zeros(G, np.uint8)
    ids = np.nonzero(g >= 0)[0]
    _, first = np.unique(g[ids], return_index=True)
    fv = ids[first]                                        # the first vertex of every group that has one
    dot = np.einsum("ij,ij->i", r[fv].astype(np.float64), n[fv].astype(np.float64))
    flips[g[fv]] = dot < 0
    return flips


_ANIM_INTERP = {"STEP": abi.ANIM_STEP, "LINEAR": abi.ANIM_LINEAR, "CUBICSPLINE": abi.ANIM_CUBICSPLINE}
_ANIM_PATH = {"translation": abi.ANIM_PATH_TRANSLATION, "rotation": abi.ANIM_PATH_ROTATION, "scale": abi.ANIM_PATH_SCALE,
              "weights": abi.ANIM_PATH_WEIGHTS}
_ANIM_FIELDS = [("node_parents", np.int32), ("node_trs", np.float32), ("node_is_trs", np.uint8), ("node_locals", np.float64),
                ("joint_nodes", np.int32), ("joint_bind", np.float64), ("base_weights", np.float32),
                ("sampler_key_offsets", np.int32), ("key_times", np.float32), ("sampler_value_offsets", np.int32),
                ("values", np.float32), ("sampler_interp", np.int32), ("channel_sampler", np.int32), ("channel_node", np.int32),
                ("channel_path", np.int32), ("channel_first_target", np.int32), ("channel_num_targets", np.int32)]


def animation_tables(sd, clip=0):
    """The tables of MptAnimation for clip `clip` of a loaded glTF file (sd.animations, sd.nodes,
    sd.skin, sd.morph), as a dict of numpy arrays named like the struct's fields: what
    GPURenderer.set_animation and animation_host take, and what a caller may build by hand.
    node_locals and joint_bind are [.., 3, 4] float64.  A weights channel's node is mapped to its
    stretch of the target list through sd.morph.target_node, and the base weights are
    sd.morph.default_weights.  Channels that nothing can drive -- weights of a node without targets
    in sd.morph -- are left out."""
    if not 0 <= clip < len(sd.animations):
        raise ValueError(f"animation_tables: clip {clip} of {len(sd.animations)}")
    ad, nt = sd.animations[clip], sd.nodes
    t = {"node_parents": nt.parents, "node_trs": nt.trs, "node_is_trs": nt.is_trs, "node_locals": nt.locals[:, :3, :]}
    if sd.skin is not None:
        t["joint_nodes"], t["joint_bind"] = sd.skin.joint_nodes, sd.skin.bind[:, :3, :]
    if sd.morph is not None:
        t["base_weights"] = sd.morph.default_weights
    koff, voff = [0], [0]
    for sm in ad.samplers:
        koff.append(koff[-1] + len(sm.times))
        voff.append(voff[-1] + sm.values.size)
    t["sampler_key_offsets"], t["sampler_value_offsets"] = koff, voff
    t["key_times"] = np.concatenate([sm.times for sm in ad.samplers]) if ad.samplers else []
    t["values"] = np.concatenate([sm.values.reshape(-1) for sm in ad.samplers]) if ad.samplers else []
    t["sampler_interp"] = [_ANIM_INTERP[sm.interpolation] for sm in ad.samplers]
    cs, cn, cp, c0, ck = [], [], [], [], []
    for ch in ad.channels:
        first, count = 0, 0
        if ch.path == "weights":
            own = np.nonzero(sd.morph.target_node == ch.node)[0] if sd.morph is not None else []
            if len(own) == 0:
                continue
            first, count = int(own[0]), len(own)
        cs.append(ch.sampler); cn.append(ch.node); cp.append(_ANIM_PATH[ch.path]); c0.append(first); ck.append(count)
    t["channel_sampler"], t["channel_node"], t["channel_path"] = cs, cn, cp
    t["channel_first_target"], t["channel_num_targets"] = c0, ck
    return {k: np.ascontiguousarray(t.get(k, []), dt) for k, dt in _ANIM_FIELDS}


def _animation_struct(tables, clip, who):
    """(abi.Animation, the arrays it points to) from a SceneData or a dict as animation_tables gives."""
    if isinstance(tables, scene.SceneData):
        tables = animation_tables(tables, clip)
    a = {k: np.ascontiguousarray(tables.get(k, []), dt) for k, dt in _ANIM_FIELDS}
    N, J, T = len(a["node_parents"]), len(a["joint_nodes"]), len(a["base_weights"])
    S, Cn = len(a["sampler_interp"]), len(a["channel_sampler"])
    for k, n in (("node_trs", 10 * N), ("node_is_trs", N), ("node_locals", 12 * N), ("joint_bind", 12 * J),
                 ("sampler_key_offsets", S + 1 if S else 0), ("sampler_value_offsets", S + 1 if S else 0),
                 ("channel_node", Cn), ("channel_path", Cn), ("channel_first_target", Cn), ("channel_num_targets", Cn)):
        if a[k].size != n:
            raise ValueError(f"{who}: {k} has {a[k].size} entries, not {n}")
    if S and (a["key_times"].size != a["sampler_key_offsets"][-1] or a["values"].size != a["sampler_value_offsets"][-1]):
        raise ValueError(f"{who}: key_times / values do not have their offsets' last entry")
    st = abi.Animation()
    st.num_nodes, st.num_joints, st.num_targets, st.num_samplers, st.num_channels = N, J, T, S, Cn
    for k, _ in _ANIM_FIELDS:
        setattr(st, k, a[k].ctypes.data if a[k].size else None)
    return st, a


def animation_host(tables, t, clip=0):
    """mpt_animation_host, no GPU: the host loop of csrc/anim.h -- what GPURenderer.update_animation(t)
    evaluates for these tables (a SceneData with its clip number, or a dict as animation_tables
    gives).  Returns (weights float32 [T] or None without targets, matrices float32 [J, 3, 4] or None
    without joints): the arguments of update_morph_skin."""
    st, keep = _animation_struct(tables, clip, "animation_host")
    w = np.empty(st.num_targets, np.float32) if st.num_targets else None
    m = np.empty((st.num_joints, 3, 4), np.float32) if st.num_joints else None
    _check(lib().mpt_animation_host(C.byref(st), float(t), _p(m), _p(w)))
    return w, m


def _on_device(a):
    """A torch tensor in GPU memory (anything else, a CPU tensor included, is a host array)."""
    return bool(getattr(a, "is_cuda", False))


class GPURenderer:
    """One renderer context on one GPU (GPURenderer.h:69)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = lib()
        h = C.c_void_p()
        _check(L.mpt_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        self.frame = None
        self._n_mats = 0
        self._n_verts = 0

    # --- scene / resources -----------------------------------------------------
    def set_scene(self, sd: "scene.SceneData", build=None, info=False):
        """GPURenderer::set_scene (GPURenderer.cpp:1052-1130).  build=None: mpt_upload_scene, both
        BVHs by the host builder.  build=abi.BUILD_LBVH / BUILD_PLOC / BUILD_SAH:
        mpt_upload_scene_mode, both BVHs built on the GPU in that mode (the way to change topology
        at interactive rates); info=True then returns the abi.RebuildInfo, else None."""
        if build is not None and (isinstance(build, bool) or not isinstance(build, (int, np.integer))):
            # (an integer that is no mode, such as 2, is the library's to refuse: MPT_ERR_INVALID_ARGUMENT)
            raise TypeError(f"set_scene: build must be None or an abi.BUILD_* mode, not {build!r}")
        s = sd.to_abi()
        ri = None
        if build is None:
            _check(lib().mpt_upload_scene(self.h, C.byref(s)))
        else:
            ri = abi.RebuildInfo() if info else None
            _check(lib().mpt_upload_scene_mode(self.h, C.byref(s), int(build), C.byref(ri) if info else None))
        self._n_mats = len(sd.materials)
        self._n_verts = len(np.asarray(sd.vertices).reshape(-1, 3))
        return ri

    def update_materials(self, materials):
        arr = (abi.Material * len(materials))(*materials)
        _check(lib().mpt_update_materials(self.h, C.cast(arr, C.c_void_p), len(materials)))

    def update_vertices(self, vertices, normals=None, info=False):
        """mpt_update_vertices: new positions ([V, 3] float32, the scene's vertex count) and
        optionally new vertex normals for the uploaded scene; both BVHs are refitted on the GPU.
        The next frame must carry need_to_reset (sample_number 0).  info=True returns the
        abi.RefitInfo (a download of the node boxes), else None.
        Torch tensors on the context's device (positions, or positions and normals) go through
        mpt_update_vertices_device: no copy to the host and back.  A mix of host and device arrays
        raises TypeError."""
        if _on_device(vertices) or _on_device(normals):
            return self._update_vertices_device(vertices, normals, info)
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        n = None
        if normals is not None:
            n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if n.shape != v.shape:
                raise ValueError(f"update_vertices: {n.shape[0]} normals for {v.shape[0]} vertices")
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_vertices(self.h, _p(v), _p(n), v.shape[0], C.byref(ri) if info else None))
        return ri

    def _update_vertices_device(self, vertices, normals, info):
        import torch
        if not _on_device(vertices) or (normals is not None and not _on_device(normals)):
            raise TypeError("update_vertices: positions and normals must both be host arrays or both device tensors")
        ts = []
        for t in (vertices, normals):
            if t is None:
                ts.append(None)
                continue
            if t.device.index != self.device:
                raise ValueError(f"update_vertices: tensor on {t.device}, the context is on device {self.device}")
            ts.append(t.to(torch.float32).contiguous().reshape(-1, 3))
        v, n = ts
        if n is not None and n.shape != v.shape:
            raise ValueError(f"update_vertices: {n.shape[0]} normals for {v.shape[0]} vertices")
        # the library reads on its own stream: what torch has enqueued for the tensors must be done
        torch.cuda.current_stream(v.device).synchronize()
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_vertices_device(self.h, C.c_void_p(v.data_ptr()), C.c_void_p(n.data_ptr()) if n is not None else None,
                                                v.shape[0], C.byref(ri) if info else None))
        return ri

    def set_objects(self, vertex_object, num_objects=None):
        """mpt_set_objects: vertex_object is int32 [V], the object of every vertex of the scene in
        [-1, num_objects) (-1: static; num_objects=None: the largest id + 1).  Captures the rest
        pose -- the positions and normals on the device now -- which every update_transforms
        moves.  vertex_object=None removes the objects."""
        if vertex_object is None:
            _check(lib().mpt_set_objects(self.h, None, 0, 0))
            return
        ids = np.ascontiguousarray(vertex_object, np.int32).reshape(-1)
        k = int(ids.max()) + 1 if num_objects is None else int(num_objects)
        _check(lib().mpt_set_objects(self.h, _p(ids), len(ids), k))

    def update_transforms(self, matrices, info=False):
        """mpt_update_transforms: one matrix per object ([K, 3, 4], or [K, 4, 4] whose bottom row is
        dropped) applied to the rest pose on the GPU, then the refit of both BVHs: 48 bytes per
        object cross the bus, no vertex array.  The next frame must carry need_to_reset.
        info=True returns the abi.RefitInfo, else None."""
        m = _matrices(matrices, "update_transforms")
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_transforms(self.h, _p(m), len(m), C.byref(ri) if info else None))
        return ri

    def set_skin(self, joints, weights=None, num_joints=None):
        """mpt_set_skin: joints is int32 [V, 4], per vertex of the scene four indices into a palette
        of num_joints joints (None: the largest index + 1), weights float32 [V, 4] (all zero: the
        vertex is not skinned).  Captures the rest pose -- the positions and normals on the device
        now -- which every update_skin poses.  A skin and the objects of set_objects exclude each
        other: setting one drops the other.  joints=None removes the skin."""
        if joints is None:
            _check(lib().mpt_set_skin(self.h, None, None, 0, 0))
            return
        j, w = _skin_table(joints, weights, "set_skin")
        k = int(j.max()) + 1 if num_joints is None else int(num_joints)
        _check(lib().mpt_set_skin(self.h, _p(j), _p(w), len(j), k))

    def update_skin(self, matrices, info=False):
        """mpt_update_skin: one matrix per joint ([J, 3, 4], or [J, 4, 4] whose bottom row is
        dropped), relative to the pose at set_skin, blended per vertex and applied to the rest pose
        on the GPU, then the refit of both BVHs: 64 bytes per joint cross the bus, no vertex array.
        The next frame must carry need_to_reset.  info=True returns the abi.RefitInfo, else None."""
        m = _matrices(matrices, "update_skin")
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_skin(self.h, _p(m), len(m), C.byref(ri) if info else None))
        return ri

    def set_morph(self, morph):
        """mpt_set_morph: morph is a scene.MorphData (SceneData.morph) or a list with one (vertex
        ids, position deltas [n, 3], normal deltas [n, 3] or None) per target; each target's ids are
        sorted here and a vertex twice in one target raises ValueError.  Pose = skin(morph(rest
        pose)): a morph composes with the skin of set_skin -- they share the rest pose, captured by
        whichever is set first -- and excludes the objects of set_objects.  The weights start at
        zero.  morph=None removes the morph."""
        if morph is None:
            _check(lib().mpt_set_morph(self.h, 0, None, None, None, None, 0))
            return
        T, off, ids, dp, dn = _morph_tables(morph, "set_morph")
        # (the tables do not say how many vertices the scene has: set_scene's count)
        _check(lib().mpt_set_morph(self.h, T, _p(off), _p(ids), _p(dp), _p(dn), self._n_verts))

    def set_normals(self, vertex_group, flips=None, num_groups=None):
        """mpt_set_normals: from now on every geometry update (update_vertices, update_transforms,
        update_skin, update_morph, update_morph_skin, update_animation) ends with the smooth normals
        of the grouped vertices recomputed from the new positions on the GPU -- area-weighted sums
        of the face vectors per group, csrc/normals.h.  vertex_group is int32 [V] in [-1,
        num_groups) (mpt.normal_groups makes it; -1: never touched; num_groups=None: the largest id
        + 1), flips uint8 [num_groups] or None (mpt.normal_flips).  The call changes no normal
        itself.  Normals given to update_vertices are overwritten for the grouped vertices.
        Independent of objects, skin, morph and animation; set_scene drops it.
        vertex_group=None removes it."""
        if vertex_group is None:
            _check(lib().mpt_set_normals(self.h, None, None, 0, 0))
            return
        g, f, G = _normal_table(vertex_group, flips, num_groups, "set_normals")
        _check(lib().mpt_set_normals(self.h, _p(g), _p(f), len(g), G))

    def get_vertices(self):
        """mpt_get_vertices: (positions, normals), float32 [V, 3] each -- what the last update left
        on the device, downloaded with the streams drained."""
        v = np.empty((self._n_verts, 3), np.float32)
        n = np.empty((self._n_verts, 3), np.float32)
        _check(lib().mpt_get_vertices(self.h, _p(v), _p(n), self._n_verts))
        return v, n

    def update_morph(self, weights, info=False):
        """mpt_update_morph: one weight per target ([T] float32) applied to the rest pose on the
        GPU, followed in the same kernel by the skin's last pose when update_skin has set one, then
        the refit of both BVHs: 4 bytes per target cross the bus, no vertex array.  The next frame
        must carry need_to_reset.  info=True returns the abi.RefitInfo, else None."""
        w = _morph_weights(weights, "update_morph")
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_morph(self.h, _p(w), len(w), C.byref(ri) if info else None))
        return ri

    def update_morph_skin(self, weights, matrices, info=False):
        """mpt_update_morph_skin: update_morph(weights) and update_skin(matrices) as one call: one
        kernel, one refit."""
        w = _morph_weights(weights, "update_morph_skin")
        m = _matrices(matrices, "update_morph_skin")
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_morph_skin(self.h, _p(w), len(w), _p(m), len(m), C.byref(ri) if info else None))
        return ri

    def set_animation(self, tables, clip=0):
        """mpt_set_animation: tables is a SceneData loaded from a glTF file (its clip number `clip`)
        or a dict as mpt.animation_tables gives.  The skin and / or the morph that the clip drives
        must be set, with as many joints and targets; setting either anew, set_objects and set_scene
        drop the animation.  tables=None removes it."""
        if tables is None:
            _check(lib().mpt_set_animation(self.h, None))
            return
        st, keep = _animation_struct(tables, clip, "set_animation")
        _check(lib().mpt_set_animation(self.h, C.byref(st)))

    def update_animation(self, t, info=False):
        """mpt_update_animation: the clip sampled at t seconds, the hierarchy composed and the joint
        palette and morph weights written on the GPU, then the fused morph and skin kernel and the
        refit of both BVHs: one float crosses the bus.  The same bytes as
        update_morph_skin(*mpt.animation_host(tables, t)).  The next frame must carry
        need_to_reset.  info=True returns the abi.RefitInfo, else None."""
        ri = abi.RefitInfo() if info else None
        _check(lib().mpt_update_animation(self.h, float(t), C.byref(ri) if info else None))
        return ri

    def rebuild_bvh(self, info=False, mode=abi.BUILD_LBVH):
        """mpt_rebuild_bvh_mode: both BVHs rebuilt on the GPU from the positions on the device, as
        an LBVH (abi.BUILD_LBVH), by PLOC (abi.BUILD_PLOC: a better tree, a slower build) or top down
        with binned SAH (abi.BUILD_SAH: the host builder's tree quality, the slowest of the three).
        No frame reset is needed.  info=True returns the abi.RebuildInfo, else None."""
        ri = abi.RebuildInfo() if info else None
        _check(lib().mpt_rebuild_bvh_mode(self.h, int(mode), C.byref(ri) if info else None))
        return ri

    def get_bvh(self, which=0):
        """mpt_get_bvh: (nodes, tris, levels) of the scene BVH (0) or the light-hit BVH (1) as the
        kernels read them, structured arrays of abi.NODE8_DTYPE / abi.TRIREC_DTYPE."""
        L = lib()
        return _bvh_arrays(lambda n, nc, t, tc, cnt: L.mpt_get_bvh(self.h, which, n, nc, t, tc, cnt))

    def set_envmap(self, env):
        """GPURenderer::set_envmap (GPURenderer.cpp:1136-1174); env from build_envmap() or None."""
        if env is None:
            _check(lib().mpt_set_envmap(self.h, None, 0, 0, None, None, 0.0))
            return
        self._env = env
        _check(lib().mpt_set_envmap(self.h, _p(env["rgba"]), env["width"], env["height"], _p(env["probas"]),
                                    _p(env["alias"]), env["sum"]))
        if env.get("cdf") is not None:
            _check(lib().mpt_set_envmap_cdf(self.h, _p(env["cdf"]), env["cdf_sum"]))

    def set_luts(self, luts=None):
        luts = luts if luts is not None else scene.load_luts()
        L = scene.luts_to_abi(luts)
        _check(lib().mpt_set_luts(self.h, C.byref(L)))

    def resize(self, w, h):
        _check(lib().mpt_resize(self.h, w, h))

    def set_halo_exchange(self, exchange):
        """ReSTIR DI across a row partition (mpt.h MptHaloExchange): exchange(x) is called
        with an abi.HaloExchange at every exchange point of mpt_render_frame and fills the
        halo rows (mpt.partition.TorchHaloExchange / LocalHaloGroup).  None removes it."""
        if exchange is None:
            self._halo_cb = None
            _check(lib().mpt_set_halo_exchange(self.h, abi.HaloExchangeFn(), None))
            return

        def _cb(_user, xp):
            try:
                exchange(xp.contents)
                return 0
            except BaseException as e:   # reported by render(); never unwinds through C
                self._halo_error = e
                return 1

        self._halo_error = None
        self._halo_cb = abi.HaloExchangeFn(_cb)   # kept alive with the renderer
        _check(lib().mpt_set_halo_exchange(self.h, self._halo_cb, None))

    def set_halo_native(self, mode: int):
        """mpt_set_halo_native: 1 the library's RCCL halo exchange (after comm_init), 2 the one-GPU
        rehearsal (timing only), 0 off."""
        self._halo_cb = None
        _check(lib().mpt_set_halo_native(self.h, int(mode)))

    def set_pipeline(self, mode: int):
        """mpt_set_pipeline: 1 the bounce pipeline of single-stream wavefronts, 0 in line."""
        _check(lib().mpt_set_pipeline(self.h, int(mode)))

    # --- frames --------------------------------------------------------------------
    def render(self, frame: "abi.Frame"):
        """Enqueues one sample per pixel (asynchronous)."""
        rc = lib().mpt_render_frame(self.h, C.byref(frame))
        err = getattr(self, "_halo_error", None)
        if err is not None:
            self._halo_error = None
            raise MptError(rc or -1, f"halo exchange failed: {err!r}") from err
        _check(rc)
        self.frame = frame

    def render_samples(self, frames, max_batch: int = 0):
        """GPURenderer::render with samples_per_frame = len(frames): enqueues every frame's
        sample; runs of batchable frames (mpt.h mpt_render_frames) are traced as one
        wavefront of up to max_batch samples per pixel (0: the library maximum)."""
        if not frames:
            return
        arr = (abi.Frame * len(frames))(*frames)
        rc = lib().mpt_render_frames(self.h, arr, len(frames), int(max_batch))
        err = getattr(self, "_halo_error", None)
        if err is not None:
            self._halo_error = None
            raise MptError(rc or -1, f"halo exchange failed: {err!r}") from err
        _check(rc)
        self.frame = frames[-1]

    def synchronize_kernel(self):
        _check(lib().mpt_synchronize(self.h))

    def frame_render_done(self) -> bool:
        d = C.c_int()
        _check(lib().mpt_query_done(self.h, C.byref(d)))
        return bool(d.value)

    def rows(self):
        f = self.frame
        return partition_rows(f.res_y, f.band_height, f.band_index, f.band_count)

    def framebuffer(self, kind=abi.FB_COLOR):
        """Copies the partition's rows (band-major, increasing y) -> float32 [rows, W, 3]."""
        f = self.frame
        out = np.zeros((self.rows(), f.res_x, 3), np.float32)
        _check(lib().mpt_get_framebuffer(self.h, kind, _p(out), 0))
        return out

    def framebuffer_to_device(self, kind, dev_ptr: int):
        _check(lib().mpt_get_framebuffer(self.h, kind, C.c_void_p(dev_ptr), 1))

    # --- display views / screenshots (DisplayViewSystem, Screenshoter) ---------------------
    def display_settings(self, view=abi.VIEW_DEFAULT, low_resolution=False, base=None):
        """The view's settings from the last frame's render settings, as
        update_display_program_uniforms derives them after that frame: the reference's
        sample_number counts the samples rendered, i.e. the last MptFrame's sample_number + 1."""
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "display: no frame rendered")
        rs = abi.RenderSettings.from_buffer_copy(self.frame.render_settings)
        rs.sample_number += 1
        return display_settings(rs, view, low_resolution, base)

    def _display(self, view, settings, second, second_is_device, low_resolution, dst, dst_is_device):
        s = settings if settings is not None else self.display_settings(view, low_resolution)
        _check(lib().mpt_display(self.h, C.byref(s), second, int(second_is_device), dst, int(dst_is_device)))

    def display(self, view=abi.VIEW_DEFAULT, settings=None, second=None, low_resolution=False):
        """mpt_display to the host: the partition's rows as uint8 [rows, W, 4] (RGBA).  settings:
        an abi.DisplaySettings (its own view counts), else derived from the last frame
        (display_settings).  second (VIEW_BLEND): float32 [rows, W, 3] host array, or a device
        pointer (int) to such a buffer."""
        out = np.zeros((self.rows(), self.frame.res_x, 4), np.uint8)
        if isinstance(second, (int, np.integer)):
            sec, dev = C.c_void_p(int(second)), True
        else:
            second = None if second is None else np.ascontiguousarray(second, np.float32)
            if second is not None and second.size != 3 * out.shape[0] * out.shape[1]:
                raise ValueError(f"display: second buffer of shape {second.shape}")
            sec, dev = _p(second), False
        self._display(view, settings, sec, dev, low_resolution, _p(out), False)
        return out

    def display_to_device(self, dev_ptr: int, view=abi.VIEW_DEFAULT, settings=None, second_dev_ptr: int | None = None,
                          low_resolution=False):
        """mpt_display into device memory (rows * W * 4 bytes at dev_ptr): enqueued on the
        context's stream after the frames rendered so far, no host synchronisation."""
        sec = C.c_void_p(int(second_dev_ptr)) if second_dev_ptr else None
        self._display(view, settings, sec, True, low_resolution, C.c_void_p(int(dev_ptr)), True)

    # --- denoiser (RenderWindow::denoise; an a-trous filter in OIDN's place) ----------------
    def denoise_settings(self, base=None):
        """abi.DenoiseSettings (the defaults, or a copy of `base`) with sample_number = the samples
        rendered so far, i.e. the last MptFrame's sample_number + 1, as display_settings() counts."""
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "denoise: no frame rendered")
        s = abi.DenoiseSettings.default()
        if base is not None:
            C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
        s.sample_number = self.frame.render_settings.sample_number + 1
        return s

    def denoise(self, settings=None):
        """mpt_denoise to the host: the denoised sums, float32 [rows, W, 3]; the result also stays
        on the device (denoised()).  settings=None: denoise_settings()."""
        s = settings if settings is not None else self.denoise_settings()
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "denoise: no frame rendered")
        out = np.zeros((self.rows(), self.frame.res_x, 3), np.float32)
        _check(lib().mpt_denoise(self.h, C.byref(s), _p(out), 0))
        return out

    def denoise_to_device(self, dev_ptr: int | None = None, settings=None):
        """mpt_denoise on the context's stream, no host synchronisation; dev_ptr (rows * W float3
        of device memory) also receives the kept result, None keeps it only."""
        s = settings if settings is not None else self.denoise_settings()
        _check(lib().mpt_denoise(self.h, C.byref(s), C.c_void_p(int(dev_ptr)) if dev_ptr else None, 1))

    def denoised(self):
        """mpt_denoised_buffer: (device pointer of the kept result, the sample_number it was made at)."""
        p, n = C.c_void_p(), C.c_int32()
        _check(lib().mpt_denoised_buffer(self.h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def denoise_device(self, settings, color_ptr: int, albedo_ptr: int, normals_ptr: int, w: int, h: int, dst_ptr: int):
        """mpt_denoise_device: caller-owned device planes of w x h float3 (e.g. gathered from a row
        partition), on the context's stream; asynchronous."""
        _check(lib().mpt_denoise_device(self.h, C.byref(settings), C.c_void_p(int(color_ptr)), C.c_void_p(int(albedo_ptr)),
                                        C.c_void_p(int(normals_ptr)), w, h, C.c_void_p(int(dst_ptr))))

    def display_denoised(self, blend=1.0, settings=None):
        """The BLEND view of the sums and the kept denoised result (blend 0: the sums, 1: the
        denoised image) -> uint8 [rows, W, 4].  settings: an abi.DisplaySettings to start from."""
        ptr, n = self.denoised()
        s = self.display_settings(abi.VIEW_BLEND, base=settings)
        s.sample_number_2 = n
        s.blend_factor = blend
        return self.display(settings=s, second=ptr)

    # --- temporal accumulation (mpt_set_temporal, csrc/temporal.hip) ------------------------
    def set_temporal(self, on=True):
        """mpt_set_temporal: on, every geometry update first keeps the pose before it (the pose at
        the last temporal call) on the device, so that temporal() can follow each pixel's surface
        point back through skin, morph, animation, transforms and new vertices.  Off frees the
        previous pose and the history."""
        _check(lib().mpt_set_temporal(self.h, int(bool(on))))

    def temporal_settings(self, base=None):
        """abi.TemporalSettings (the defaults, or a copy of `base`) with sample_number = the samples
        rendered so far, as denoise_settings() counts."""
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "temporal: no frame rendered")
        s = abi.TemporalSettings.default()
        if base is not None:
            C.memmove(C.byref(s), C.byref(base), C.sizeof(s))
        s.sample_number = self.frame.render_settings.sample_number + 1
        return s

    def _temporal_args(self, settings, camera):
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "temporal: no frame rendered")
        s = settings if settings is not None else self.temporal_settings()
        cam = camera if camera is not None else self.frame.current_camera
        return s, cam

    def temporal(self, settings=None, camera=None):
        """mpt_temporal_accumulate to the host: the colour sums just rendered blended into the
        reprojected history -> float32 [rows, W, 3], sums in the units of the framebuffer.
        settings=None: temporal_settings(); camera=None: the last frame's current_camera.  The
        previous camera is the one of the previous call."""
        s, cam = self._temporal_args(settings, camera)
        out = np.zeros((self.rows(), self.frame.res_x, 3), np.float32)
        _check(lib().mpt_temporal_accumulate(self.h, C.byref(s), C.byref(cam), _p(out), 0))
        return out

    def temporal_to_device(self, dev_ptr: int | None = None, settings=None, camera=None):
        """mpt_temporal_accumulate on the context's stream, no host synchronisation; dev_ptr (rows *
        W float3 of device memory) also receives the result, None keeps it in the context only."""
        s, cam = self._temporal_args(settings, camera)
        _check(lib().mpt_temporal_accumulate(self.h, C.byref(s), C.byref(cam), C.c_void_p(int(dev_ptr)) if dev_ptr else None, 1))

    def temporal_reset(self):
        """mpt_temporal_reset: the next temporal() starts without history."""
        _check(lib().mpt_temporal_reset(self.h))

    def temporal_planes(self, kind):
        """mpt_get_temporal: a plane of the last temporal() -> float32 [rows, W, 3]
        (abi.TEMPORAL_OUTPUT) or [rows, W, 4] (TEMPORAL_MOTION, _VISIBILITY, _HISTORY_A, _HISTORY_B;
        the primitive ids are int32 bits in lane 3)."""
        if self.frame is None:
            raise MptError(abi.ERR_INVALID_ARGUMENT, "temporal: no frame rendered")
        out = np.zeros((self.rows(), self.frame.res_x, 3 if kind == abi.TEMPORAL_OUTPUT else 4), np.float32)
        _check(lib().mpt_get_temporal(self.h, int(kind), _p(out), 0))
        return out

    def temporal_planes_to_device(self, kind, dev_ptr: int):
        _check(lib().mpt_get_temporal(self.h, int(kind), C.c_void_p(int(dev_ptr)), 1))

    def denoise_temporal(self, settings=None, camera=None, denoise_settings=None, dev_ptr: int | None = None, to_host=True):
        """mpt_denoise_temporal: temporal(), then the a-trous filter over the accumulated plane into
        the kept denoise buffer (denoised(), display_denoised()).  to_host: returns float32 [rows, W,
        3]; else asynchronous, the result also copied to dev_ptr when given."""
        s, cam = self._temporal_args(settings, camera)
        d = denoise_settings if denoise_settings is not None else self.denoise_settings()
        if to_host:
            out = np.zeros((self.rows(), self.frame.res_x, 3), np.float32)
            _check(lib().mpt_denoise_temporal(self.h, C.byref(s), C.byref(cam), C.byref(d), _p(out), 0))
            return out
        _check(lib().mpt_denoise_temporal(self.h, C.byref(s), C.byref(cam), C.byref(d),
                                          C.c_void_p(int(dev_ptr)) if dev_ptr else None, 1))
        return None

    # --- one process per GPU (RCCL, mpt_comm_*) ----------------------------------------
    def comm_init(self, nranks: int, rank: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().mpt_comm_init(self.h, nranks, rank, buf))
        self.comm_rank = rank

    def comm_gather(self, root=0, kind=abi.FB_COLOR):
        """mpt_comm_gather (collective): the whole frame on the root (host array), None elsewhere."""
        out = _gather_out(self.frame, kind)
        _check(lib().mpt_comm_gather(self.h, root, kind, _p(out), 0))
        return out if self.comm_rank == root else None

    # --- status buffers / adaptive sampling (GPURenderer.cpp:269-283) ---------------
    def clear_status_buffers(self):
        """internal_update_clear_device_status_buffers: once per displayed frame."""
        _check(lib().mpt_clear_status(self.h))

    def get_status_buffer_values(self) -> dict:
        """copy_status_buffers + get_status_buffer_values (StatusBuffersValues)."""
        st = abi.Status()
        _check(lib().mpt_query_status(self.h, C.byref(st)))
        return {"one_ray_active": bool(st.one_ray_active), "pixel_converged_count": int(st.pixel_converged_count)}

    def aux_buffer(self, kind):
        """MPT_AUX_* buffer of the partition -> [rows, W] (int32, or float32 for squared luminance)."""
        f = self.frame
        if kind in (abi.AUX_RESTIR_OUTPUT, abi.AUX_RESTIR_OTHER, abi.AUX_RESTIR_INITIAL):
            # frame-sized reservoirs -> [H, W, 12] float32 (M and triangle as int bits in 0 / 3)
            out = np.zeros((f.res_y, f.res_x, 12), np.float32)
        else:
            out = np.zeros((self.rows(), f.res_x), np.float32 if kind == abi.AUX_SQUARED_LUMINANCE else np.int32)
        _check(lib().mpt_get_aux_buffer(self.h, kind, _p(out), 0))
        return out

    # --- stats / queries -------------------------------------------------------
    def enable_stats(self, timing=True, instrumented=False):
        _check(lib().mpt_enable_stats(self.h, int(timing), int(instrumented)))

    def stats(self) -> "abi.Stats":
        s = abi.Stats()
        _check(lib().mpt_get_stats(self.h, C.byref(s)))
        return s

    def trace_closest(self, rays, last_hit=None):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        prim = np.empty(n, np.int32)
        t, u, v = (np.empty(n, np.float32) for _ in range(3))
        lh = None if last_hit is None else np.ascontiguousarray(last_hit, np.int32)
        _check(lib().mpt_trace_closest(self.h, _p(rays), _p(lh), n, _p(prim), _p(t), _p(u), _p(v), 0))
        return prim, t, u, v

    def trace_any(self, rays, last_hit=None):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        occ = np.empty(n, np.uint8)
        lh = None if last_hit is None else np.ascontiguousarray(last_hit, np.int32)
        _check(lib().mpt_trace_any(self.h, _p(rays), _p(lh), n, _p(occ), 0))
        return occ.astype(bool)

    # --- LUT baker (GPUBaker, Renderer/Baker/GPUBaker.cpp:35-97) -------------------------
    def bake_lut(self, kind, width, height, depth=1, samples=65536):
        """abi.BAKE_* table -> float32 [depth, height, width], rows as the reference's baker
        writes them (the renderer's LUTs are each slice flipped: out[:, ::-1])."""
        out = np.zeros((depth, height, width), np.float32)
        _check(lib().mpt_bake_lut(self.h, kind, width, height, depth, samples, _p(out), 0))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().mpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
