// temporal.h -- the pixel arithmetic of the temporal accumulation, shared verbatim by the kernels
// (temporal.hip: k_primary_rays, k_temporal) and the host path (mpt_primary_rays_host,
// mpt_temporal_host), the way denoise.h and display.h are shared: one fixed sequence of fp32
// operations per pixel, compiled with -ffp-contract=off on both sides, so that the GPU and the CPU
// produce the same bits.  No fast-math intrinsics.
//
// The history of a pixel is reprojected with exact motion vectors: the closest hit of the pixel's
// centre ray gives a primitive and barycentrics, the same combination of that triangle's vertices
// in the previous pose gives the point the surface came from, and the previous camera's
// view_projection gives where that point was seen (DESIGN.md §2 has the definition; mpt.h
// MptTemporalSettings the settings).  The blend runs on the denoiser's demodulated mean
// (denoise.h prepare / demodulator / output), so the accumulated plane is in the units of the
// input sums and goes straight into the a-trous filter.
//
//   ray        through the pixel centre with k_camera's operations (mpt_kernels.hip), no jitter
//   points     w = 1 - u - v, P = ((w A) + (u B)) + (v C) over the current positions, Q the same
//              over the previous ones; A, B, C the triangle's first, second, third vertex (u
//              weighs the second, v the third, as the traversal reports them); a miss: Q =
//              o_prev + d, both depths -1
//   reproject  restir_reproject's operations with the previous view_projection, the clip-space w
//              explicit: w <= 0 has no history (motion -1, -1)
//   taps       the 2 x 2 pixels around (fx, fy), bilinear weights, tested against the history
//   blend      a = max(alpha, 1 / (len + 1)); e + a (e_cur - e), a = 1: e_cur itself
#ifndef MPT_TEMPORAL_H
#define MPT_TEMPORAL_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "denoise.h"
#include "mpt.h"

#if defined(__HIPCC__)
#define TMP_FN __host__ __device__ static inline
#else
#define TMP_FN static inline
#endif

namespace mpttemp {

struct V3 {
    float x, y, z;
};

// One pixel of the two history planes: {e.r, e.g, e.b, depth} and {n.x, n.y, n.z, length}.
struct HistPx {
    float a[4], b[4];
};

// The constants of one call.
struct Consts {
    MptTemporalSettings S;
    MptCamera cur, prev;
    int32_t W, H;
    int32_t has_history;
};

TMP_FN V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
TMP_FN V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
TMP_FN V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
TMP_FN V3 scale(float k, V3 a) { return mk(k * a.x, k * a.y, k * a.z); }
TMP_FN float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TMP_FN float length3(V3 a) { return sqrtf(dot3(a, a)); }
TMP_FN bool near_zero(float x) { return x < 1.0e-10f && x > -1.0e-10f; }
TMP_FN float int_bits(int32_t i) { float f; memcpy(&f, &i, 4); return f; }
TMP_FN int32_t float_bits(float f) { int32_t i; memcpy(&i, &f, 4); return i; }

// dev_math.h mat_x_point with the clip-space w handed out as well
TMP_FN V3 mat_point(const float m[4][4], V3 p, float* w_out) {
    const float xt = m[0][0] * p.x + m[0][1] * p.y + m[0][2] * p.z + m[0][3];
    const float yt = m[1][0] * p.x + m[1][1] * p.y + m[1][2] * p.z + m[1][3];
    const float zt = m[2][0] * p.x + m[2][1] * p.y + m[2][2] * p.z + m[2][3];
    const float wt = m[3][0] * p.x + m[3][1] * p.y + m[3][2] * p.z + m[3][3];
    float iw = 1.0f;
    if (!near_zero(wt)) iw = 1.0f / wt;
    *w_out = wt;
    return mk(xt * iw, yt * iw, zt * iw);
}

TMP_FN V3 camera_origin(const MptCamera& cam) {
    float w;
    return mat_point(cam.inverse_view.m, mk(0.0f, 0.0f, 0.0f), &w);
}

// The ray through the centre of pixel (x, y): k_camera without jitter and low resolution.
TMP_FN void primary_ray(const MptCamera& cam, int x, int y, int W, int H, V3* o, V3* d) {
    const float xd = (float)x + 0.5f, yd = (float)y + 0.5f;
    const float xn = xd / (float)W * 2.0f - 1.0f;
    const float yn = yd / (float)H * 2.0f - 1.0f;
    float w;
    *o = camera_origin(cam);
    const V3 pvs = mat_point(cam.inverse_projection.m, mk(xn, yn, -1.0f), &w);
    const V3 pws = mat_point(cam.inverse_view.m, pvs, &w);
    const V3 t = sub(pws, *o);
    const float l = sqrtf(dot3(t, t));
    *d = mk(t.x / l, t.y / l, t.z / l);
}

// restir_reproject's operations; false: the point is not in front of the previous camera.
TMP_FN bool reproject(const MptCamera& prev, V3 q, int W, int H, float* fx, float* fy) {
    float w;
    const V3 ss = mat_point(prev.view_projection.m, q, &w);
    if (!(w > 0.0f)) return false;
    float sx = ss.x, sy = ss.y;
    sx = sx + 1.0f; sy = sy + 1.0f;
    sx = sx * 0.5f; sy = sy * 0.5f;
    float x = sx * (float)W, y = sy * (float)H;
    x = x - 0.5f; y = y - 0.5f;
    *fx = x; *fy = y;
    return true;
}

TMP_FN V3 load3(const float* p, int32_t i) { return mk(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }
TMP_FN V3 bary(float w, float u, float v, V3 A, V3 B, V3 C) { return add(add(scale(w, A), scale(u, B)), scale(v, C)); }

// The denoiser's view of the settings: what prepare, demodulator and output read.
TMP_FN MptDenoiseSettings denoise_view(const MptTemporalSettings& s) {
    MptDenoiseSettings d{};
    d.sample_number = s.sample_number;
    d.use_albedo = s.use_albedo;
    return d;
}

// One pixel.  hit: the closest hit of the pixel's ray {t, u, v, prim bits} (prim < 0: a miss);
// idx / pos / prev_pos: the scene's indices and the two poses; color / albedo / normal: this
// pixel's three floats of each plane; fetch(x, y): the previous call's history at a position
// inside the image (never called without history).  Writes the pixel's two history elements, its
// float3 output and its motion element.
template <typename Fetch>
TMP_FN void pixel(const Consts& K, int x, int y, const float* hit, const int32_t* idx, const float* pos, const float* prev_pos,
                  const float* color, const float* albedo, const float* normal, const Fetch& fetch, float* out_a, float* out_b,
                  float* out_rgb, float* out_motion) {
    const MptDenoiseSettings D = denoise_view(K.S);
    const mptden::Px p = mptden::prepare(D, color, albedo, normal);
    V3 o, d;
    primary_ray(K.cur, x, y, K.W, K.H, &o, &d);
    const V3 o_prev = camera_origin(K.prev);
    const int32_t prim = float_bits(hit[3]);
    const bool is_hit = prim >= 0;
    V3 Q;
    float depth_cur = -1.0f, depth_exp = -1.0f;
    if (is_hit) {
        const int32_t i0 = idx[3 * (size_t)prim], i1 = idx[3 * (size_t)prim + 1], i2 = idx[3 * (size_t)prim + 2];
        const float u = hit[1], v = hit[2];
        const float w = 1.0f - u - v;
        const V3 P = bary(w, u, v, load3(pos, i0), load3(pos, i1), load3(pos, i2));
        Q = bary(w, u, v, load3(prev_pos, i0), load3(prev_pos, i1), load3(prev_pos, i2));
        depth_cur = length3(sub(P, o));
        depth_exp = length3(sub(Q, o_prev));
    } else {
        Q = add(o_prev, d);
    }
    float fx = -1.0f, fy = -1.0f;
    bool have = reproject(K.prev, Q, K.W, K.H, &fx, &fy);
    if (!have) { fx = -1.0f; fy = -1.0f; }
    out_motion[0] = fx; out_motion[1] = fy; out_motion[2] = depth_exp; out_motion[3] = hit[3];

    float e_h[3] = {0.0f, 0.0f, 0.0f}, len_h = 0.0f;
    // (every tap of a position outside (-1, W) x (-1, H) lies outside the image; a NaN too)
    have = have && K.has_history && fx > -1.0f && fx < (float)K.W && fy > -1.0f && fy < (float)K.H;
    if (have) {
        const float flx = floorf(fx), fly = floorf(fy);
        const int x0 = (int)flx, y0 = (int)fly;
        const float tx = fx - flx, ty = fy - fly;
        const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
        float num[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
        bool any = false;
        for (int j = 0; j < 2; j++) {
            const int qy = y0 + j;
            if (qy < 0 || qy >= K.H) continue;
            for (int i = 0; i < 2; i++) {
                const int qx = x0 + i;
                if (qx < 0 || qx >= K.W) continue;
                const HistPx q = fetch(qx, qy);
                const float len_q = q.b[3], depth_q = q.a[3];
                if (!(len_q >= 1.0f)) continue;
                if (is_hit) {
                    if (!(depth_q >= 0.0f)) continue;
                    if (!(fabsf(depth_q - depth_exp) <= K.S.depth_tolerance * depth_exp)) continue;
                    const float c = p.n[0] * q.b[0] + p.n[1] * q.b[1] + p.n[2] * q.b[2];
                    if (!(c >= K.S.normal_threshold)) continue;
                } else {
                    if (!(depth_q < 0.0f)) continue;
                }
                const float wq = wx[i] * wy[j];
                for (int k = 0; k < 3; k++) num[k] = num[k] + wq * q.a[k];
                wsum = wsum + wq;
                len_h = any ? fminf(len_h, len_q) : len_q;
                any = true;
            }
        }
        have = any && wsum > 0.0f;
        if (have)
            for (int k = 0; k < 3; k++) e_h[k] = num[k] / wsum;
    }
    float e_new[3], len_new = 1.0f;
    if (have) {
        const float a = fmaxf(K.S.alpha, 1.0f / (len_h + 1.0f));
        for (int k = 0; k < 3; k++) e_new[k] = a < 1.0f ? e_h[k] + a * (p.e[k] - e_h[k]) : p.e[k];
        len_new = fminf(len_h + 1.0f, (float)K.S.max_history);
    } else {
        for (int k = 0; k < 3; k++) e_new[k] = p.e[k];
    }
    for (int k = 0; k < 3; k++) {
        out_a[k] = e_new[k];
        out_b[k] = p.n[k];
        out_rgb[k] = mptden::output(D, e_new[k], p.a[k]);
    }
    out_a[3] = depth_cur;
    out_b[3] = len_new;
}

// What is wrong with the settings (NULL: nothing) -- the checks every entry point shares.
static inline const char* temporal_settings_error(const MptTemporalSettings& s) {
    if (s.sample_number < 1) return "temporal: sample_number < 1";
    if (s.max_history < 1 || s.max_history > MPT_TEMPORAL_MAX_HISTORY) return "temporal: max_history outside 1..1024";
    if (!(s.alpha > 0.0f) || !(s.alpha <= 1.0f)) return "temporal: alpha outside (0, 1]";
    if (!(s.depth_tolerance > 0.0f) || !(s.depth_tolerance < INFINITY)) return "temporal: depth_tolerance must be finite and positive";
    if (!(s.normal_threshold >= -1.0f) || !(s.normal_threshold <= 1.0f)) return "temporal: normal_threshold outside -1..1";
    return nullptr;
}

}  // namespace mpttemp

#undef TMP_FN
#endif
