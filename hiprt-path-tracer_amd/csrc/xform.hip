// xform.hip -- per-object motion for gfx950 (mpt_update_transforms, mpt_update_vertices_device) and
// the host loop of the same arithmetic (xform.h; DESIGN.md §2 "Geometry updates", Transforms).
//
//   k_xform<G>   G vertices per lane.  The rest pose (positions, normals: 12 B each per vertex), the
//                object ids and the used-vertex mask are read, the object's 21-float record is
//                fetched through the cache whenever the id changes along the lane's vertices (ids
//                run in long uniform stretches), and the moved positions and normals are written to
//                staging arrays.  G = 4: a lane's 4 vertices are 48 B, three 16-byte loads and
//                stores per array, the ids one 16-byte load, the mask one dword.  G = 1: dword
//                accesses (the last, partial group of G = 4 takes the same per-vertex path).
//   k_check<G>   the same reduction over an array that is already there (no transform).
//   reduction    per lane fmaxf of |coordinate| over the used vertices and a non-finite flag over
//                all of them; fmaxf across the wave by shuffles, across the block's 4 waves through
//                LDS, then one atomicMax on the float's bits (non-negative floats order as their
//                bits) and, when set, one atomicOr per block.  A NaN never wins an fmaxf, so it
//                cannot hide in the maximum: the flag carries it.  Exact and order-free -- no
//                floating-point sum crosses lanes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "vert_io.h"
#include "xform.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mptxform;

using namespace vertio;

template <int G>
__device__ inline void load_ids(const int32_t* __restrict__ obj, size_t v0, int cnt, int32_t* id) {
    if constexpr (G == 4) {
        if (cnt == 4) {
            const int4 w = *(const int4*)(obj + v0);
            id[0] = w.x; id[1] = w.y; id[2] = w.z; id[3] = w.w;
            return;
        }
    }
    for (int k = 0; k < G; k++) id[k] = k < cnt ? obj[v0 + k] : -1;
}

template <int G>
__global__ void __launch_bounds__(256) k_xform(const float* __restrict__ rest_pos, const float* __restrict__ rest_nrm,
                                               const int32_t* __restrict__ obj, const uint8_t* __restrict__ used,
                                               const float* __restrict__ recs, int n, float* __restrict__ out_pos,
                                               float* __restrict__ out_nrm, uint32_t* __restrict__ red) {
    const size_t v0 = (size_t)G * (size_t)(blockIdx.x * blockDim.x + threadIdx.x);
    float m = 0.0f;
    bool bad = false;
    if (v0 < (size_t)n) {
        const int cnt = (size_t)n - v0 < (size_t)G ? (int)((size_t)n - v0) : G;
        float p[3 * G], q[3 * G], po[3 * G], qo[3 * G];
        int32_t id[G];
        bool u[G];
        load_group<G>(rest_pos, v0, cnt, p);
        load_group<G>(rest_nrm, v0, cnt, q);
        load_ids<G>(obj, v0, cnt, id);
        load_mask<G>(used, v0, cnt, u);
        float rec[REC];
        int32_t cur = -1;
        bool ident = true;
#pragma unroll
        for (int k = 0; k < G; k++) {
            if (id[k] != cur) {
                cur = id[k];
                if (cur >= 0) {
                    const float* r = recs + (size_t)REC * (size_t)cur;
                    for (int j = 0; j < REC; j++) rec[j] = r[j];
                    ident = is_identity(rec);
                }
            }
            xform_vertex(rec, cur < 0 || ident, p + 3 * k, q + 3 * k, po + 3 * k, qo + 3 * k);
            if (k < cnt) {
                bad |= !finite3(po + 3 * k);
                if (u[k]) m = fmaxf(m, abs_max3(po + 3 * k));
            }
        }
        store_group<G>(out_pos, v0, cnt, po);
        store_group<G>(out_nrm, v0, cnt, qo);
    }
    reduce_block(m, bad, red);
}

template <int G>
__global__ void __launch_bounds__(256) k_check(const float* __restrict__ pos, const uint8_t* __restrict__ used, int n,
                                               uint32_t* __restrict__ red) {
    const size_t v0 = (size_t)G * (size_t)(blockIdx.x * blockDim.x + threadIdx.x);
    float m = 0.0f;
    bool bad = false;
    if (v0 < (size_t)n) {
        const int cnt = (size_t)n - v0 < (size_t)G ? (int)((size_t)n - v0) : G;
        float p[3 * G];
        bool u[G];
        load_group<G>(pos, v0, cnt, p);
        load_mask<G>(used, v0, cnt, u);
#pragma unroll
        for (int k = 0; k < G; k++)
            if (k < cnt) {
                bad |= !finite3(p + 3 * k);
                if (u[k]) m = fmaxf(m, abs_max3(p + 3 * k));
            }
    }
    reduce_block(m, bad, red);
}

}  // namespace

// n vertices of the rest pose moved by their objects' records into out_pos / out_nrm; red (2 words)
// is zeroed on the stream first and then holds the reduction.  group: vertices per lane, 4 or 1.
hipError_t launch_xform(const float* rest_pos, const float* rest_nrm, const int32_t* obj, const uint8_t* used, const float* recs,
                        int n, float* out_pos, float* out_nrm, uint32_t* red, int group, hipStream_t st) {
    hipError_t e = hipMemsetAsync(red, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess || n <= 0) return e;
    const bool wide = group == 4 && aligned16(rest_pos) && aligned16(rest_nrm) && aligned16(obj) && aligned16(out_pos) &&
                      aligned16(out_nrm) && aligned16(used);
    if (wide)
        hipLaunchKernelGGL(k_xform<4>, dim3(blocks_for(n, 4)), dim3(256), 0, st, rest_pos, rest_nrm, obj, used, recs, n, out_pos,
                           out_nrm, red);
    else
        hipLaunchKernelGGL(k_xform<1>, dim3(blocks_for(n, 1)), dim3(256), 0, st, rest_pos, rest_nrm, obj, used, recs, n, out_pos,
                           out_nrm, red);
    return hipGetLastError();
}

// The reduction alone over n vertices at pos (a caller's array: any alignment).
hipError_t launch_xform_check(const float* pos, const uint8_t* used, int n, uint32_t* red, int group, hipStream_t st) {
    hipError_t e = hipMemsetAsync(red, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess || n <= 0) return e;
    if (group == 4 && aligned16(pos) && aligned16(used))
        hipLaunchKernelGGL(k_check<4>, dim3(blocks_for(n, 4)), dim3(256), 0, st, pos, used, n, red);
    else
        hipLaunchKernelGGL(k_check<1>, dim3(blocks_for(n, 1)), dim3(256), 0, st, pos, used, n, red);
    return hipGetLastError();
}

// The host loop: false when an output coordinate is not finite (the outputs are then unspecified).
bool transform_host(const float* rest_pos, const float* rest_nrm, const int32_t* obj, size_t n, const float* recs, float* out_pos,
                    float* out_nrm) {
    using namespace mptxform;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    bool ok = true;
    int32_t cur = -1;
    bool ident = true;
    for (size_t i = 0; i < n; i++) {
        if (obj[i] != cur) {
            cur = obj[i];
            if (cur >= 0) ident = is_identity(recs + (size_t)REC * (size_t)cur);
        }
        float no[3];
        xform_vertex(cur >= 0 ? recs + (size_t)REC * (size_t)cur : nullptr, cur < 0 || ident, rest_pos + 3 * i,
                     rest_nrm ? rest_nrm + 3 * i : zero, out_pos + 3 * i, out_nrm ? out_nrm + 3 * i : no);
        ok &= finite3(out_pos + 3 * i);
    }
    return ok;
}

// Every entry of num_objects x 12 floats finite.
bool matrices_finite(const float* matrices, int32_t num_objects) {
    for (size_t k = 0; k < 12 * (size_t)num_objects; k++)
        if (!(std::fabs(matrices[k]) <= mptxform::F_MAX)) return false;
    return true;
}

void make_xform_records(const float* matrices, int32_t num_objects, std::vector<float>& recs) {
    recs.resize((size_t)mptxform::REC * (size_t)num_objects);
    mptxform::make_records(matrices, num_objects, recs.data());
}

}  // namespace mpt

extern "C" {

int mpt_transform_host(const float* rest_vertices, const float* rest_normals, const int32_t* vertex_object, int32_t num_vertices,
                       const float* matrices, int32_t num_objects, float* out_vertices, float* out_normals) {
    using namespace mpt;
    if (!rest_vertices || !vertex_object || !out_vertices || (num_objects > 0 && !matrices))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_vertices <= 0 || num_objects < 0) return api_fail(MPT_ERR_INVALID_ARGUMENT, "transform: bad size");
    if (out_normals && !rest_normals) return api_fail(MPT_ERR_INVALID_ARGUMENT, "transform: normals out without normals in");
    for (int32_t i = 0; i < num_vertices; i++)
        if (vertex_object[i] < -1 || vertex_object[i] >= num_objects)
            return api_fail(MPT_ERR_INVALID_ARGUMENT, "object id out of range");
    if (!matrices_finite(matrices, num_objects)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite matrix entry");
    std::vector<float> recs;
    make_xform_records(matrices, num_objects, recs);
    if (!transform_host(rest_vertices, rest_normals, vertex_object, (size_t)num_vertices, recs.data(), out_vertices, out_normals))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    return MPT_OK;
}

}  // extern "C"
