// denoise.h -- the pixel arithmetic of the denoiser, shared verbatim by the kernels
// (denoise.hip: k_denoise_prepare, k_atrous_gather, k_atrous_tiled) and the host path
// (mpt_denoise_host), the way display.h is shared: one fixed sequence of fp32 operations per
// pixel, compiled with -ffp-contract=off on both sides, so that the GPU and the CPU produce the
// same bits.
//
// The filter is an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
// albedo-demodulated radiance, guided by the albedo AOV, the normals AOV and the colour itself
// (DESIGN.md §2 has the definition; mpt.h MptDenoiseSettings the settings).  It stands where the
// reference calls OIDN (RenderWindow::denoise, OpenImageDenoiser.cpp) and claims no parity with it.
//
//   prepare     m = clamp(color / n, 0, 1e35) (NaN -> 0), albedo / normal components that are not
//               finite -> 0, d = use_albedo ? max(albedo, 0.01) : 1, e = m / d
//   iteration i step 1 << i, 5 x 5 taps of the B3 kernel {1/16, 1/4, 3/8, 1/4, 1/16}^2, dy outer and
//               dx inner, taps outside the image skipped; weight() below per tap
//   output      e * d * n: in the units of the input sums
#ifndef MPT_DENOISE_H
#define MPT_DENOISE_H

#include <math.h>
#include <stdint.h>

#include "mpt.h"
#include "tmath.h"

#if defined(__HIPCC__)
#define DEN_FN __host__ __device__ static inline
#else
#define DEN_FN static inline
#endif

namespace mptden {

// One pixel of the working planes: demodulated colour, sanitised albedo, sanitised normal.
struct Px {
    float e[3], a[3], n[3];
};

// The constants of iteration i, computed once on the host for both paths.
struct IterConsts {
    float inv_c, inv_a;
};
static inline IterConsts iteration_consts(const MptDenoiseSettings& s, int i) {
    const float sc = s.sigma_color * ldexpf(1.0f, -i);
    IterConsts k;
    k.inv_c = 1.0f / (sc * sc);
    k.inv_a = 1.0f / (s.sigma_albedo * s.sigma_albedo);
    return k;
}

DEN_FN float finite_or_zero(float v) { return fabsf(v) <= 3.4028234663852886e38f ? v : 0.0f; }   // NaN, +-inf -> 0
DEN_FN float demodulator(const MptDenoiseSettings& s, float albedo) { return s.use_albedo ? fmaxf(albedo, 0.01f) : 1.0f; }

DEN_FN Px prepare(const MptDenoiseSettings& s, const float* color, const float* albedo, const float* normal) {
    Px p;
    const float n = (float)s.sample_number;
    for (int k = 0; k < 3; k++) {
        float m = color[k] / n;
        m = fminf(fmaxf(m, 0.0f), 1.0e35f);   // a NaN becomes 0, as in the default view
        p.a[k] = finite_or_zero(albedo[k]);
        p.n[k] = finite_or_zero(normal[k]);
        p.e[k] = m / demodulator(s, p.a[k]);
    }
    return p;
}

DEN_FN float output(const MptDenoiseSettings& s, float e, float albedo) {
    return e * demodulator(s, albedo) * (float)s.sample_number;
}

// The weight of a tap q != p with kernel weight h; false: the tap is skipped.
DEN_FN bool weight(const MptDenoiseSettings& s, const IterConsts& c, float h, const Px& p, const Px& q, float* w_out) {
    const float dr = p.e[0] - q.e[0], dg = p.e[1] - q.e[1], db = p.e[2] - q.e[2];
    const float dc = dr * dr + dg * dg + db * db;
    const float mm = ((p.e[0] + p.e[1] + p.e[2]) + (q.e[0] + q.e[1] + q.e[2])) / 6.0f;
    float xx = dc / (mm * mm + 1.0e-4f) * c.inv_c;
    if (s.use_albedo) {
        const float ar = p.a[0] - q.a[0], ag = p.a[1] - q.a[1], ab = p.a[2] - q.a[2];
        xx = xx + (ar * ar + ag * ag + ab * ab) * c.inv_a;
    }
    if (!(xx <= 80.0f)) return false;   // also inf and NaN
    float w = h * tmath::expf_(-xx);
    if (s.use_normals) {
        float t = p.n[0] * q.n[0] + p.n[1] * q.n[1] + p.n[2] * q.n[2];
        if (!(t > 0.0f)) return false;
        t = fminf(t, 1.0f);
        for (int k = 0; k < s.normal_power_log2; k++) t = t * t;
        w = w * t;
    }
    *w_out = w;
    return true;
}

// The new colour of the pixel at (cx, cy) of an X x Y grid whose taps are `step` apart;
// fetch(x, y) returns the pixel at a position inside the grid.  The image with step 1 << i, and a
// sub-lattice of it with step 1 (the tiled kernel), visit the same pixels in the same order.
template <typename Fetch>
DEN_FN void filter_pixel(const MptDenoiseSettings& s, const IterConsts& c, int cx, int cy, int step, int X, int Y,
                         const Fetch& fetch, float* out) {
    const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const Px p = fetch(cx, cy);
    float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = cy + dy * step;
        if (qy < 0 || qy >= Y) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = cx + dx * step;
            if (qx < 0 || qx >= X) continue;
            const float h = K[dy + 2] * K[dx + 2];
            float w = h;
            if (dx == 0 && dy == 0) {
                for (int k = 0; k < 3; k++) num[k] = num[k] + w * p.e[k];
            } else {
                const Px q = fetch(qx, qy);
                if (!weight(s, c, h, p, q, &w)) continue;
                for (int k = 0; k < 3; k++) num[k] = num[k] + w * q.e[k];
            }
            den = den + w;
        }
    }
    for (int k = 0; k < 3; k++) out[k] = num[k] / den;   // den >= 9/64: the centre tap
}

// What is wrong with the settings (NULL: nothing) -- the checks every entry point shares.
static inline const char* denoise_settings_error(const MptDenoiseSettings& s) {
    if (s.sample_number < 1) return "denoise: sample_number < 1";
    if (s.iterations < 1 || s.iterations > MPT_DENOISE_MAX_ITERATIONS) return "denoise: iterations outside 1..8";
    if (s.normal_power_log2 < 0 || s.normal_power_log2 > 10) return "denoise: normal_power_log2 outside 0..10";
    if (!(s.sigma_color > 0.0f) || !(s.sigma_color < INFINITY)) return "denoise: sigma_color must be finite and positive";
    if (!(s.sigma_albedo > 0.0f) || !(s.sigma_albedo < INFINITY)) return "denoise: sigma_albedo must be finite and positive";
    return nullptr;
}

}  // namespace mptden

#undef DEN_FN
#endif
