// temporal.hip -- the temporal accumulation's kernels and its host path; the pixel arithmetic is
// temporal.h's.
//
// Planes (context-owned, W * H elements each):
//   HA0, HA1  float4  {e.r, e.g, e.b, depth}   } the history, ping-pong: a call reads the planes
//   HB0, HB1  float4  {n.x, n.y, n.z, length}  } the previous call wrote and writes the others
//   VIS       float4  {t, u, v, prim bits}: the raw closest-hit launch's output
//   MOTION    float4  {fx, fy, expected depth, prim bits}
//   OUT       float3  the accumulated colour, remodulated: the a-trous filter's input
//
// k_primary_rays  one lane per pixel: two 16-B stores (the raw layout of launch_trace_raw).
// k_temporal      one lane per pixel, 256-lane blocks, no LDS: a 2 x 2 footprint shares too little
//                 to stage.  Per lane: 16 B of VIS, 36 B of the three float3 planes, on a hit 12 B
//                 of indices and 72 B of vertices (two poses; neighbouring pixels mostly share the
//                 triangle), up to four taps of 32 B from the history (16 B per plane and lane;
//                 under small motion consecutive lanes read consecutive elements), 60 B written.
#include <hip/hip_runtime.h>

#include <vector>

#include "mpt_internal.h"
#include "temporal.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mpttemp;

__global__ __launch_bounds__(256) void k_primary_rays(const MptCamera cam, int W, int H, float4* __restrict__ ro,
                                                       float4* __restrict__ rd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const int y = (int)(i / W), x = (int)(i % W);
    V3 o, d;
    primary_ray(cam, x, y, W, H, &o, &d);
    ro[i] = make_float4(o.x, o.y, o.z, int_bits(-1));
    rd[i] = make_float4(d.x, d.y, d.z, INFINITY);
}

struct GlobalFetch {
    const float4* __restrict__ a;
    const float4* __restrict__ b;
    int W;
    __device__ HistPx operator()(int x, int y) const {
        const int64_t q = (int64_t)y * W + x;
        const float4 va = a[q], vb = b[q];
        HistPx h;
        h.a[0] = va.x; h.a[1] = va.y; h.a[2] = va.z; h.a[3] = va.w;
        h.b[0] = vb.x; h.b[1] = vb.y; h.b[2] = vb.z; h.b[3] = vb.w;
        return h;
    }
};

__global__ __launch_bounds__(256) void k_temporal(const TemporalLaunch A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)A.W * A.H) return;
    const int y = (int)(i / A.W), x = (int)(i % A.W);
    Consts K;
    K.S = A.S; K.cur = A.cur; K.prev = A.prev; K.W = A.W; K.H = A.H; K.has_history = A.has_history;
    const float4 h4 = A.hit[i];
    const float hit[4] = {h4.x, h4.y, h4.z, h4.w};
    const float c[3] = {A.color[3 * i], A.color[3 * i + 1], A.color[3 * i + 2]};
    const float al[3] = {A.albedo[3 * i], A.albedo[3 * i + 1], A.albedo[3 * i + 2]};
    const float nr[3] = {A.normals[3 * i], A.normals[3 * i + 1], A.normals[3 * i + 2]};
    float oa[4], ob[4], rgb[3], mo[4];
    pixel(K, x, y, hit, A.idx, A.pos, A.prev_pos, c, al, nr, GlobalFetch{A.hist_in_a, A.hist_in_b, A.W}, oa, ob, rgb, mo);
    A.hist_out_a[i] = make_float4(oa[0], oa[1], oa[2], oa[3]);
    A.hist_out_b[i] = make_float4(ob[0], ob[1], ob[2], ob[3]);
    A.motion[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
    A.out[3 * i] = rgb[0];
    A.out[3 * i + 1] = rgb[1];
    A.out[3 * i + 2] = rgb[2];
}

struct HostFetch {
    const float* a;
    const float* b;
    int W;
    HistPx operator()(int x, int y) const {
        const size_t q = (size_t)y * W + x;
        HistPx h;
        for (int k = 0; k < 4; k++) { h.a[k] = a[4 * q + k]; h.b[k] = b[4 * q + k]; }
        return h;
    }
};

}  // namespace

hipError_t launch_primary_rays(const MptCamera& cam, int W, int H, float4* o, float4* d, hipStream_t st) {
    if (W <= 0 || H <= 0) return hipSuccess;
    const int64_t n = (int64_t)W * H;
    hipLaunchKernelGGL(k_primary_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cam, W, H, o, d);
    return hipGetLastError();
}

hipError_t launch_temporal(const TemporalLaunch& a, hipStream_t st) {
    if (a.W <= 0 || a.H <= 0) return hipSuccess;
    const int64_t n = (int64_t)a.W * a.H;
    hipLaunchKernelGGL(k_temporal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mpt

extern "C" {

int mpt_temporal_settings_default(MptTemporalSettings* out) {
    if (!out) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    MptTemporalSettings s{};
    s.sample_number = 1;
    s.max_history = 32;
    s.alpha = 0.1f;
    s.depth_tolerance = 0.02f;
    s.normal_threshold = 0.9f;
    s.use_albedo = 1;
    *out = s;
    return MPT_OK;
}

int mpt_primary_rays_host(const MptCamera* camera, int32_t width, int32_t height, float* out_rays) {
    using namespace mpttemp;
    if (!camera || !out_rays) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width <= 0 || height <= 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: bad size");
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            V3 o, d;
            primary_ray(*camera, x, y, width, height, &o, &d);
            float* r = out_rays + 8 * ((size_t)y * width + x);
            r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = 0.0f;
            r[4] = d.x; r[5] = d.y; r[6] = d.z; r[7] = INFINITY;
        }
    return MPT_OK;
}

int mpt_temporal_host(const MptTemporalHostArgs* a) {
    using namespace mpttemp;
    if (!a || !a->visibility || !a->indices || !a->positions || !a->prev_positions || !a->color || !a->albedo || !a->normals ||
        !a->history_out_a || !a->history_out_b || !a->output || !a->motion)
        return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((a->history_in_a == nullptr) != (a->history_in_b == nullptr))
        return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: one history plane without the other");
    if (a->width <= 0 || a->height <= 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: bad size");
    if (a->num_vertices <= 0 || a->num_triangles <= 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: bad scene size");
    if (const char* e = temporal_settings_error(a->settings)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, e);
    if (a->history_in_a && (a->history_in_a == a->history_out_a || a->history_in_b == a->history_out_b))
        return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: the history is read and written in different planes");
    const size_t n = (size_t)a->width * a->height;
    // the kernel trusts the traversal; the host checks what it is handed
    for (size_t i = 0; i < n; i++) {
        const int32_t prim = float_bits(a->visibility[4 * i + 3]);
        if (prim >= a->num_triangles) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: primitive id out of range");
    }
    for (size_t k = 0; k < 3 * (size_t)a->num_triangles; k++)
        if (a->indices[k] < 0 || a->indices[k] >= a->num_vertices)
            return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "temporal: vertex index out of range");
    Consts K;
    K.S = a->settings; K.cur = a->camera; K.prev = a->prev_camera; K.W = a->width; K.H = a->height;
    K.has_history = a->history_in_a ? 1 : 0;
    const mpt::HostFetch fetch{a->history_in_a, a->history_in_b, a->width};
    for (int y = 0; y < a->height; y++)
        for (int x = 0; x < a->width; x++) {
            const size_t i = (size_t)y * a->width + x;
            pixel(K, x, y, a->visibility + 4 * i, a->indices, a->positions, a->prev_positions, a->color + 3 * i, a->albedo + 3 * i,
                  a->normals + 3 * i, fetch, a->history_out_a + 4 * i, a->history_out_b + 4 * i, a->output + 3 * i, a->motion + 4 * i);
        }
    return MPT_OK;
}

}  // extern "C"
