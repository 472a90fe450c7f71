// denoise.hip -- the denoiser's kernels and its host path; the pixel arithmetic is denoise.h's.
//
// Working planes (context-owned, W * H elements each, 40 B per pixel):
//   E0, E1  float4  the demodulated colour {e.r, e.g, e.b, unused}; the iterations ping-pong
//   G0      float4  {albedo.r, albedo.g, albedo.b, normal.x}   } the guides, unmodified fp32
//   G1      float2  {normal.y, normal.z}                       } (non-finite components are 0)
//
// k_denoise_prepare   one lane per pixel: 36 B read (three float3 planes), 40 B written.
// k_atrous_gather     one lane per pixel, the 25 taps read from global memory (L2): consecutive
//                     lanes read consecutive elements at every tap, whatever the step.
// k_atrous_tiled      for step s the image is s * s independent sub-lattices (x % s, y % s).  A
//                     256-thread block takes a 32 x 8 tile of one sub-lattice and stages the tile
//                     and its 2-pixel halo (36 x 12 elements of E, G0 and G1, 17,280 B) in LDS,
//                     where the 5 x 5 stencil is dense.  LDS reads are one ds_read_b128 per plane
//                     element with consecutive lanes on consecutive elements: every 16-lane group
//                     covers 256 contiguous bytes, all 64 banks once (G1: ds_read_b64, 32 lanes on
//                     256 contiguous bytes).  The global reads of a sub-lattice row are 16-B
//                     elements 16 * s bytes apart.
// Both filter kernels visit the taps in the definition's order, so they give the same bits; which
// one runs at a step is a table (TILED_STEPS) set from measurements.  The last
// iteration writes the remodulated float3 result instead of E.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "denoise.h"
#include "mpt_internal.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mptden;

constexpr int TILE_W = 32, TILE_H = 8, HALO = 2;
constexpr int LDS_W = TILE_W + 2 * HALO, LDS_H = TILE_H + 2 * HALO, LDS_N = LDS_W * LDS_H;
// bit i: the tiled kernel at step 1 << i.  Measured at 1920x1080: faster than the
// gather at steps 1..32, slower at 64 and 128, where a sub-lattice row is spread over many lines
constexpr uint32_t TILED_STEPS = 0x3fu;

__host__ __device__ inline Px unpack(const float4 e, const float4 g0, const float2 g1) {
    Px p;
    p.e[0] = e.x; p.e[1] = e.y; p.e[2] = e.z;
    p.a[0] = g0.x; p.a[1] = g0.y; p.a[2] = g0.z;
    p.n[0] = g0.w; p.n[1] = g1.x; p.n[2] = g1.y;
    return p;
}

__global__ __launch_bounds__(256) void k_denoise_prepare(const MptDenoiseSettings S, const float* __restrict__ color,
                                                          const float* __restrict__ albedo, const float* __restrict__ normals,
                                                          int64_t n, float4* __restrict__ E, float4* __restrict__ G0,
                                                          float2* __restrict__ G1) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float c[3] = {color[3 * i], color[3 * i + 1], color[3 * i + 2]};
    const float a[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
    const float m[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    const Px p = prepare(S, c, a, m);
    E[i] = make_float4(p.e[0], p.e[1], p.e[2], 0.0f);
    G0[i] = make_float4(p.a[0], p.a[1], p.a[2], p.n[0]);
    G1[i] = make_float2(p.n[1], p.n[2]);
}

// the filtered pixel goes to the other E plane, or (the last iteration) remodulated to dst
template <bool LAST>
__device__ __forceinline__ void store_pixel(const MptDenoiseSettings& S, const float* v, const float4 g0, int64_t px,
                                            float4* __restrict__ Eout, float* __restrict__ dst) {
    if constexpr (LAST) {
        dst[3 * px] = output(S, v[0], g0.x);
        dst[3 * px + 1] = output(S, v[1], g0.y);
        dst[3 * px + 2] = output(S, v[2], g0.z);
    } else {
        Eout[px] = make_float4(v[0], v[1], v[2], 0.0f);
    }
}

struct GlobalFetch {
    const float4* __restrict__ E;
    const float4* __restrict__ G0;
    const float2* __restrict__ G1;
    int W;
    __device__ Px operator()(int x, int y) const {
        const int64_t q = (int64_t)y * W + x;
        return unpack(E[q], G0[q], G1[q]);
    }
};

template <bool LAST>
__global__ __launch_bounds__(256) void k_atrous_gather(const MptDenoiseSettings S, const IterConsts C, int step, int W, int H,
                                                        const float4* __restrict__ Ein, const float4* __restrict__ G0,
                                                        const float2* __restrict__ G1, float4* __restrict__ Eout,
                                                        float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const int y = (int)(i / W), x = (int)(i % W);
    float v[3];
    filter_pixel(S, C, x, y, step, W, H, GlobalFetch{Ein, G0, G1, W}, v);
    store_pixel<LAST>(S, v, G0[i], i, Eout, dst);
}

struct LdsFetch {
    const float4* e;
    const float4* g0;
    const float2* g1;
    int i0, j0;   // lattice position of LDS element (0, 0)
    __device__ Px operator()(int i, int j) const {
        const int k = (j - j0) * LDS_W + (i - i0);
        return unpack(e[k], g0[k], g1[k]);
    }
};

// grid: x = sub-lattice column ox (outer) x tile column, y = sub-lattice row oy (outer) x tile row
template <bool LAST>
__global__ __launch_bounds__(256) void k_atrous_tiled(const MptDenoiseSettings S, const IterConsts C, int step, int W, int H,
                                                       int tiles_x, int tiles_y, const float4* __restrict__ Ein,
                                                       const float4* __restrict__ G0, const float2* __restrict__ G1,
                                                       float4* __restrict__ Eout, float* __restrict__ dst) {
    __shared__ float4 s_e[LDS_N];
    __shared__ float4 s_g0[LDS_N];
    __shared__ float2 s_g1[LDS_N];
    const int ox = blockIdx.x / tiles_x, oy = blockIdx.y / tiles_y;
    if (ox >= W || oy >= H) return;   // a step larger than the image: this sub-lattice is empty (whole block)
    const int LW = (W - ox + step - 1) / step, LH = (H - oy + step - 1) / step;   // the sub-lattice's size
    const int ti = (blockIdx.x % tiles_x) * TILE_W, tj = (blockIdx.y % tiles_y) * TILE_H;
    if (ti >= LW || tj >= LH) return;   // whole block
    const int i0 = ti - HALO, j0 = tj - HALO;
    for (int k = threadIdx.x; k < LDS_N; k += 256) {
        const int i = i0 + k % LDS_W, j = j0 + k / LDS_W;
        if (i >= 0 && i < LW && j >= 0 && j < LH) {   // elements outside stay unwritten: filter_pixel skips those taps
            const int64_t q = (int64_t)(oy + j * step) * W + (ox + i * step);   // x < W and y < H by LW, LH
            s_e[k] = Ein[q];
            s_g0[k] = G0[q];
            s_g1[k] = G1[q];
        }
    }
    __syncthreads();
    const int i = ti + (int)threadIdx.x % TILE_W, j = tj + (int)threadIdx.x / TILE_W;
    if (i >= LW || j >= LH) return;
    float v[3];
    filter_pixel(S, C, i, j, 1, LW, LH, LdsFetch{s_e, s_g0, s_g1, i0, j0}, v);
    const int64_t px = (int64_t)(oy + j * step) * W + (ox + i * step);
    store_pixel<LAST>(S, v, s_g0[(j - j0) * LDS_W + (i - i0)], px, Eout, dst);
}

// Steps (log2) at which the tiled kernel runs; the gather runs at the others.  MPT_DENOISE_TILED
// (a bit mask over log2 step, read at every call) overrides the table for A/B measurements
// (tools/denoise_time.py).
uint32_t tiled_steps() {
    const char* e = std::getenv("MPT_DENOISE_TILED");
    return e ? (uint32_t)std::strtoul(e, nullptr, 0) : TILED_STEPS;
}

struct HostFetch {
    const Px* p;
    int W;
    Px operator()(int x, int y) const { return p[(size_t)y * W + x]; }
};

}  // namespace

size_t denoise_scratch_floats(int64_t pixels) { return (size_t)pixels * 14; }   // E0, E1, G0: 4 each, G1: 2

// color / albedo / normals: W * H float3 on the device; scratch: denoise_scratch_floats(W * H)
// floats, 16-byte aligned; dst: W * H float3.  Enqueues 1 + iterations kernels on st.
hipError_t launch_denoise(const MptDenoiseSettings& S, const float* color, const float* albedo, const float* normals,
                          int W, int H, float* scratch, float* dst, hipStream_t st) {
    if (W <= 0 || H <= 0) return hipSuccess;
    const int64_t n = (int64_t)W * H;
    float4* E[2] = {(float4*)scratch, (float4*)scratch + n};
    float4* G0 = (float4*)scratch + 2 * n;
    float2* G1 = (float2*)((float4*)scratch + 3 * n);
    const dim3 b(256), g((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_denoise_prepare, g, b, 0, st, S, color, albedo, normals, n, E[0], G0, G1);
    const uint32_t tiled = tiled_steps();
    for (int i = 0; i < S.iterations; i++) {
        const IterConsts C = iteration_consts(S, i);
        const int step = 1 << i;
        const bool last = i == S.iterations - 1;
        const float4* in = E[i & 1];
        float4* out = E[(i & 1) ^ 1];
        if ((tiled >> i) & 1u) {
            const int lw = (W + step - 1) / step, lh = (H + step - 1) / step;   // the largest sub-lattice
            const int tx = (lw + TILE_W - 1) / TILE_W, ty = (lh + TILE_H - 1) / TILE_H;
            const dim3 gt((unsigned)(tx * step), (unsigned)(ty * step));
            if (last) hipLaunchKernelGGL(k_atrous_tiled<true>, gt, b, 0, st, S, C, step, W, H, tx, ty, in, G0, G1, out, dst);
            else hipLaunchKernelGGL(k_atrous_tiled<false>, gt, b, 0, st, S, C, step, W, H, tx, ty, in, G0, G1, out, dst);
        } else {
            if (last) hipLaunchKernelGGL(k_atrous_gather<true>, g, b, 0, st, S, C, step, W, H, in, G0, G1, out, dst);
            else hipLaunchKernelGGL(k_atrous_gather<false>, g, b, 0, st, S, C, step, W, H, in, G0, G1, out, dst);
        }
    }
    return hipGetLastError();
}

}  // namespace mpt

extern "C" {

int mpt_denoise_settings_default(MptDenoiseSettings* out) {
    if (!out) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    MptDenoiseSettings s{};
    s.sample_number = 1;
    s.iterations = 5;
    s.use_albedo = 1;
    s.use_normals = 1;
    s.sigma_color = 4.0f;
    s.sigma_albedo = 0.1f;
    s.normal_power_log2 = 6;
    *out = s;
    return MPT_OK;
}

int mpt_denoise_host(const MptDenoiseSettings* settings, const float* color, const float* albedo, const float* normals,
                     int32_t width, int32_t height, float* dst) {
    using namespace mptden;
    if (!settings || !color || !albedo || !normals || !dst) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width < 0 || height < 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "denoise: bad size");
    if (const char* e = denoise_settings_error(*settings)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, e);
    const MptDenoiseSettings& S = *settings;
    const size_t n = (size_t)width * height;
    std::vector<Px> cur(n), next(n);
    for (size_t i = 0; i < n; i++) cur[i] = prepare(S, color + 3 * i, albedo + 3 * i, normals + 3 * i);
    next = cur;   // the guides travel with the colour
    for (int it = 0; it < S.iterations; it++) {
        const IterConsts C = iteration_consts(S, it);
        const mpt::HostFetch fetch{cur.data(), width};
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) filter_pixel(S, C, x, y, 1 << it, width, height, fetch, next[(size_t)y * width + x].e);
        cur.swap(next);
    }
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) dst[3 * i + k] = output(S, cur[i].e[k], cur[i].a[k]);
    return MPT_OK;
}

}  // extern "C"
