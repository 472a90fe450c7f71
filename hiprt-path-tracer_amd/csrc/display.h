// display.h -- the pixel functions of the display views, shared verbatim by the display kernel
// (display.hip, k_display) and the host path (mpt_display_host), the way tmath.h is shared by
// the kernels and the oracle: one fixed sequence of fp32 operations per view, compiled with
// -ffp-contract=off on both sides, so that the GPU and the CPU produce the same bytes.
//
// Each function restates one display shader of the reference (src/Shaders/*.frag, run as compute
// by Screenshoter::write_to_png with COMPUTE_SCREENSHOTER defined) in the order written:
//   MPT_VIEW_DEFAULT                    default_display.frag:40-54
//   MPT_VIEW_BLEND                      blend_2_display.frag:51-73
//   MPT_VIEW_NORMALS                    normal_display.frag:39-53
//   MPT_VIEW_ALBEDO                     albedo_display.frag:30
//   MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP  heatmap_int.frag:43-94
//   MPT_VIEW_PIXEL_CONVERGED_MAP        boolmap_int.frag:35-54
//   MPT_VIEW_WHITE_FURNACE_THRESHOLD    white_furnace_threshold.frag:57-75
// The source textures are RGB32F (texelFetch returns alpha 1) or R32I (the count converted to
// float).  exp / pow are tmath.h's.
#ifndef MPT_DISPLAY_H
#define MPT_DISPLAY_H

#include <math.h>
#include <stdint.h>

#include "mpt.h"
#include "tmath.h"

#if defined(__HIPCC__)
#define DISP_FN __host__ __device__ static inline
#else
#define DISP_FN static inline
#endif

namespace mptdisp {

// uvec4(v * 255): truncation toward zero of the fp32 product.  GLSL leaves the conversion of
// negative, too large and NaN values undefined; here they saturate to [0, 255] and NaN is 0
// (DESIGN.md §2).
DISP_FN uint32_t to_byte(float v) {
    const float p = v * 255.0f;
    if (!(p > 0.0f)) return 0u;   // negative, -0 and NaN
    if (p >= 255.0f) return 255u;
    return (uint32_t)(int32_t)p;
}
// one RGBA8 pixel as a little-endian word: bytes r, g, b, a in memory order
DISP_FN uint32_t pack(float r, float g, float b, float a) {
    return to_byte(r) | (to_byte(g) << 8) | (to_byte(b) << 16) | (to_byte(a) << 24);
}
// pow(1 - exp(-c * exposure), 1 / gamma)
DISP_FN float tonemap(float c, const MptDisplaySettings& s) {
    const float tone_mapped = 1.0f - tmath::expf_(-c * s.exposure);
    return tmath::powf_(tone_mapped, 1.0f / s.gamma);
}

DISP_FN bool view_reads_counts(int view) {
    return view == MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP || view == MPT_VIEW_PIXEL_CONVERGED_MAP;
}
DISP_FN bool view_is_valid(int view) {
    return view == MPT_VIEW_DEFAULT || view == MPT_VIEW_BLEND || view == MPT_VIEW_NORMALS || view == MPT_VIEW_ALBEDO ||
           view == MPT_VIEW_WHITE_FURNACE_THRESHOLD || view_reads_counts(view);
}

// The views of a float3 texel c (BLEND: and the second buffer's texel c2, else unused).
template <int VIEW>
DISP_FN uint32_t pixel_rgb(const MptDisplaySettings& s, const float* c, const float* c2) {
    float r = c[0], g = c[1], b = c[2];
    if (VIEW == MPT_VIEW_ALBEDO) return pack(r, g, b, 1.0f);
    if (VIEW == MPT_VIEW_NORMALS) {
        r = (r + 1.0f) * 0.5f; g = (g + 1.0f) * 0.5f; b = (b + 1.0f) * 0.5f;
    } else if (VIEW == MPT_VIEW_BLEND) {
        const float n1 = (float)(s.sample_number > 1 ? s.sample_number : 1);
        const float n2 = (float)(s.sample_number_2 > 1 ? s.sample_number_2 : 1);
        float r2 = c2[0] / n2, g2 = c2[1] / n2, b2 = c2[2] / n2;
        r = r / n1; g = g / n1; b = b / n1;
        if (s.do_tonemapping == 1) {
            r = tonemap(r, s); g = tonemap(g, s); b = tonemap(b, s);
            r2 = tonemap(r2, s); g2 = tonemap(g2, s); b2 = tonemap(b2, s);
        }
        const float f = s.blend_factor, f1 = 1.0f - s.blend_factor;
        return pack(r * f1 + r2 * f, g * f1 + g2 * f, b * f1 + b2 * f, 1.0f * f1 + 1.0f * f);
    } else {
        const float n = (float)s.sample_number;
        r = r / n; g = g / n; b = b / n;
        if (VIEW == MPT_VIEW_DEFAULT) {
            // clamp(c, 0, 1e35); a NaN becomes 0
            r = fminf(fmaxf(r, 0.0f), 1.0e35f); g = fminf(fmaxf(g, 0.0f), 1.0e35f); b = fminf(fmaxf(b, 0.0f), 1.0e35f);
        } else {   // MPT_VIEW_WHITE_FURNACE_THRESHOLD: no clamp
            if ((r > 0.51f || g > 0.51f || b > 0.51f) && s.use_high_threshold) { r = 1.0f; g = 0.0f; b = 0.0f; }
            else if ((r < 0.49f || g < 0.49f || b < 0.49f) && s.use_low_threshold) { r = 0.0f; g = 1.0f; b = 0.0f; }
        }
    }
    if (s.do_tonemapping == 1) { r = tonemap(r, s); g = tonemap(g, s); b = tonemap(b, s); }
    return pack(r, g, b, 1.0f);
}

// The views of pixel_converged_sample_count (-1: not converged).  nb_stops in [1, 16] and
// min_val <= max_val are the caller's to check (display_settings_error); the stop indices are
// clamped all the same, so that no settings read outside color_stops.
template <int VIEW>
DISP_FN uint32_t pixel_count(const MptDisplaySettings& s, int32_t count) {
    float scalar = (float)count;
    if (VIEW == MPT_VIEW_PIXEL_CONVERGED_MAP) {
        // vec4(1) where converged, else vec4(0): alpha 0 too
        return (scalar < s.threshold_val && scalar != -1.0f) ? 0xffffffffu : 0u;
    }
    const int last = s.nb_stops - 1;
    if (s.min_val == s.max_val) {
        const MptColor e = s.color_stops[last];
        return to_byte(e.r) | (to_byte(e.g) << 8) | (to_byte(e.b) << 16) | (255u << 24);
    }
    if (scalar == -1.0f) scalar = s.max_val;
    scalar = fminf(fmaxf(scalar, s.min_val), s.max_val);
    const float normalized = (scalar - s.min_val) / (s.max_val - s.min_val);
    const float stop = normalized * (float)last;
    int low_stop = (int)floorf(stop), high_stop = (int)ceilf(stop);
    const float fraction_of_high_stop = stop - (float)low_stop;
    low_stop = low_stop < 0 ? 0 : (low_stop > last ? last : low_stop);
    high_stop = high_stop < 0 ? 0 : (high_stop > last ? last : high_stop);
    const MptColor lo = s.color_stops[low_stop], hi = s.color_stops[high_stop];
    const float f = fraction_of_high_stop, f1 = 1.0f - fraction_of_high_stop;   // mix(a, b, f) = a (1 - f) + b f
    return pack(lo.r * f1 + hi.r * f, lo.g * f1 + hi.g * f, lo.b * f1 + hi.b * f, 1.0f);
}

// What is wrong with the settings (NULL: nothing) -- the checks mpt_display and mpt_display_host share.
static inline const char* display_settings_error(const MptDisplaySettings& s) {
    if (!view_is_valid(s.view)) return "display: bad view";
    if (s.resolution_scaling < 1) return "display: resolution_scaling < 1";
    if (s.view == MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP) {
        if (s.nb_stops < 1 || s.nb_stops > MPT_DISPLAY_MAX_STOPS) return "display: nb_stops outside 1..16";
        if (!(s.min_val <= s.max_val) || !(s.max_val - s.min_val < INFINITY))
            return "display: heat map needs finite min_val <= max_val";
    }
    return nullptr;
}

}  // namespace mptdisp

#undef DISP_FN
#endif
