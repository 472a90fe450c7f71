// display.hip -- the display step: the context's sums (or counts) as 8-bit RGBA, what the
// reference's display shaders do once per displayed frame (DisplayViewSystem::display) and
// Screenshoter::write_to_png does for a screenshot.  k_display<VIEW> reads the partition's buffers
// in place -- AoS float3 per pixel slot, or the int32 count plane -- and writes RGBA8 words; the
// pixel functions are display.h's, which mpt_display_host (below) runs on host arrays.
//
// Memory-bound: 12 B read and 4 B written per pixel.  256-thread blocks; a lane handles 4
// consecutive pixels of a compact row: at resolution_scaling 1 three 16-B loads (48 contiguous
// bytes) and one 16-B store of four RGBA8 words; rows whose pixels are not 16-B aligned (a width
// that is no multiple of 4), the row tail, and resolution_scaling > 1 (a gather of (x / s, y / s))
// go pixel by pixel.  No LDS.
#include <hip/hip_runtime.h>

#include <cstring>

#include "display.h"
#include "mpt_internal.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mptdisp;

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// 12 consecutive floats (4 float3 texels): three 16-B loads where the address allows
__device__ __forceinline__ void load12(const float* __restrict__ p, float* v) {
    if (aligned16(p)) {
        const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1], c = ((const float4*)p)[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
        for (int k = 0; k < 12; k++) v[k] = p[k];
    }
}

template <int VIEW>
__global__ __launch_bounds__(256) void k_display(const MptDisplaySettings S, const float* __restrict__ src,
                                                  const float* __restrict__ src2, const int32_t* __restrict__ cnt, int W,
                                                  int rows, int quads, uint32_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * quads) return;
    const int row = (int)(i / quads), x0 = (int)(i % quads) * 4;
    const int n = W - x0 < 4 ? W - x0 : 4;
    const int s = S.resolution_scaling;
    const int64_t p0 = (int64_t)row * W + x0;   // first of the lane's pixels, < rows * W
    constexpr bool COUNTS = VIEW == MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP || VIEW == MPT_VIEW_PIXEL_CONVERGED_MAP;
    constexpr bool SECOND = VIEW == MPT_VIEW_BLEND;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    if (s == 1 && n == 4) {
        if constexpr (COUNTS) {
            int32_t c[4];
            if (aligned16(cnt + p0)) {
                const int4 v = *(const int4*)(cnt + p0);
                c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            } else {
                for (int k = 0; k < 4; k++) c[k] = cnt[p0 + k];
            }
            for (int k = 0; k < 4; k++) out[k] = pixel_count<VIEW>(S, c[k]);
        } else {
            float a[12], b[12];
            load12(src + 3 * p0, a);
            if constexpr (SECOND) load12(src2 + 3 * p0, b);
            for (int k = 0; k < 4; k++) out[k] = pixel_rgb<VIEW>(S, a + 3 * k, SECOND ? b + 3 * k : a + 3 * k);
        }
    } else {
        // source texel (x / s, y / s): row / s <= row and x / s <= x, so the slot is inside the partition
        for (int k = 0; k < n; k++) {
            const int64_t sp = (int64_t)(row / s) * W + (x0 + k) / s;
            if constexpr (COUNTS) {
                out[k] = pixel_count<VIEW>(S, cnt[sp]);
            } else {
                const float a[3] = {src[3 * sp], src[3 * sp + 1], src[3 * sp + 2]};
                float b[3] = {0.0f, 0.0f, 0.0f};
                if constexpr (SECOND) { b[0] = src2[3 * sp]; b[1] = src2[3 * sp + 1]; b[2] = src2[3 * sp + 2]; }
                out[k] = pixel_rgb<VIEW>(S, a, b);
            }
        }
    }
    if (n == 4 && aligned16(dst + p0)) {
        *(uint4*)(dst + p0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (int k = 0; k < n; k++) dst[p0 + k] = out[k];
    }
}

template <int VIEW>
void host_view(const MptDisplaySettings& S, const void* src, const float* src2, int W, int H, uint8_t* dst) {
    const int s = S.resolution_scaling;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t sp = (size_t)(y / s) * W + x / s;
            uint32_t px;
            if constexpr (VIEW == MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP || VIEW == MPT_VIEW_PIXEL_CONVERGED_MAP)
                px = pixel_count<VIEW>(S, ((const int32_t*)src)[sp]);
            else
                px = pixel_rgb<VIEW>(S, (const float*)src + 3 * sp, VIEW == MPT_VIEW_BLEND ? src2 + 3 * sp : nullptr);
            std::memcpy(dst + 4 * ((size_t)y * W + x), &px, 4);
        }
}

}  // namespace

#define MPT_DISPLAY_VIEWS(X)                                                                                       \
    X(MPT_VIEW_DEFAULT) X(MPT_VIEW_BLEND) X(MPT_VIEW_NORMALS) X(MPT_VIEW_ALBEDO) X(MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP) \
    X(MPT_VIEW_PIXEL_CONVERGED_MAP) X(MPT_VIEW_WHITE_FURNACE_THRESHOLD)

// rows x W pixels of the partition (compact rows); src / src2: 3 floats per slot, cnt: one int32
hipError_t launch_display(const MptDisplaySettings& S, const float* src, const float* src2, const int32_t* cnt, int W,
                          int rows, uint32_t* dst, hipStream_t st) {
    if (W <= 0 || rows <= 0) return hipSuccess;
    const int quads = (W + 3) / 4;
    const int64_t lanes = (int64_t)rows * quads;
    const dim3 g((unsigned)((lanes + 255) / 256)), b(256);
    switch (S.view) {
#define X(V) case V: hipLaunchKernelGGL(k_display<V>, g, b, 0, st, S, src, src2, cnt, W, rows, quads, dst); break;
        MPT_DISPLAY_VIEWS(X)
#undef X
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mpt

extern "C" {

int mpt_display_settings_default(MptDisplaySettings* out) {
    if (!out) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    MptDisplaySettings s{};
    s.view = MPT_VIEW_DEFAULT;
    s.sample_number = 1;
    s.sample_number_2 = 1;
    s.resolution_scaling = 1;
    s.do_tonemapping = 1;        // DisplaySettings.h
    s.gamma = 2.2f;
    s.exposure = 1.8f;
    s.blend_factor = 1.0f;       // denoiser_blend
    s.use_low_threshold = 0;
    s.use_high_threshold = 1;
    s.min_val = s.max_val = s.threshold_val = 1.0f;
    s.nb_stops = 3;              // DisplayViewSystem.cpp:294
    s.color_stops[0] = MptColor{0.0f, 0.0f, 1.0f};
    s.color_stops[1] = MptColor{0.0f, 1.0f, 0.0f};
    s.color_stops[2] = MptColor{1.0f, 0.0f, 0.0f};
    *out = s;
    return MPT_OK;
}

int mpt_display_uniforms(const MptRenderSettings* rs, int32_t view, int32_t low_resolution_displayed, MptDisplaySettings* io) {
    if (!rs || !io) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!mptdisp::view_is_valid(view)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "display: bad view");
    // DisplayViewSystem.cpp:203-209
    const int sample_number = rs->sample_number > 1 ? rs->sample_number : 1;
    io->view = view;
    io->sample_number = sample_number;
    io->resolution_scaling = low_resolution_displayed ? rs->render_low_resolution_scaling : 1;
    // :300-301, :316-319
    const float min_val = rs->enable_adaptive_sampling ? (float)rs->adaptive_sampling_min_samples : 1.0f;
    const float max_val = (float)sample_number > min_val ? (float)sample_number : min_val;
    io->min_val = min_val;
    io->max_val = max_val;
    io->threshold_val = max_val;
    return MPT_OK;
}

int mpt_display_host(const MptDisplaySettings* settings, const void* src, const float* src2, int32_t width, int32_t height,
                     uint8_t* dst) {
    if (!settings || !src || !dst) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width < 0 || height < 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "display: bad size");
    if (const char* e = mptdisp::display_settings_error(*settings)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, e);
    if (settings->view == MPT_VIEW_BLEND && !src2)
        return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "display: the blend view needs a second buffer");
    switch (settings->view) {
#define X(V) case V: mpt::host_view<V>(*settings, src, src2, width, height, dst); break;
        MPT_DISPLAY_VIEWS(X)
#undef X
    }
    return MPT_OK;
}

}  // extern "C"
