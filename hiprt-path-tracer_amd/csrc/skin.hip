// skin.hip -- linear-blend skinning for gfx950 (mpt_update_skin) and the host loop of the same
// arithmetic (skin.h; DESIGN.md §2 "Geometry updates", Skinning).
//
//   k_skin<G, LDS>  G vertices per lane, as k_xform<G> (xform.hip): the rest pose (positions,
//                normals: 12 B each per vertex) and the used-vertex mask are read the same way, the
//                four joint indices and the four weights of a vertex are one 16-byte load each
//                (G = 4) and the skinned positions and normals are written to staging arrays.
//                G = 4 needs every array 16-byte aligned; the last, partial group takes the
//                per-vertex path.
//   palette      up to four 64-byte records per vertex, gathered by index.  LDS = false: through
//                the cache.  LDS = true: the block first copies the whole palette into LDS with
//                coalesced 16-byte loads and gathers from there with 16-byte LDS reads; at most
//                MPT_SKIN_LDS_JOINTS records, 16 KiB, so that even eight blocks of 256 threads,
//                the most a CU holds, use 128 of its 160 KiB (k_skin<4> runs four per CU, by its
//                registers).  Both read the same bytes, so the output is the same.  Measured
//                (DESIGN.md §4): the kernel is a tenth faster with the palette in LDS.
//   reduction    vert_io.h's reduce_block, as k_xform: exact and order-free.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "skin.h"
#include "vert_io.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

static_assert(MPT_SKIN_LDS_JOINTS * mptskin::REC * sizeof(float) == 16384, "the LDS palette's budget is 16 KiB");

namespace {

using mptskin::REC;
using mptskin::skin_vertex;
using mptxform::abs_max3;
using mptxform::finite3;
using namespace vertio;

template <int G, bool LDS>
__global__ void __launch_bounds__(256) k_skin(const float* __restrict__ rest_pos, const float* __restrict__ rest_nrm,
                                              const int32_t* __restrict__ joints, const float* __restrict__ weights,
                                              const uint8_t* __restrict__ used, const float* __restrict__ recs, int num_joints,
                                              int n, float* __restrict__ out_pos, float* __restrict__ out_nrm,
                                              uint32_t* __restrict__ red) {
    extern __shared__ float4 s_pal[];   // LDS: num_joints records
    if constexpr (LDS) {
        const float4* src = (const float4*)recs;
        for (int i = (int)threadIdx.x; i < (REC / 4) * num_joints; i += 256) s_pal[i] = src[i];
        __syncthreads();
    }
    const size_t v0 = (size_t)G * (size_t)(blockIdx.x * blockDim.x + threadIdx.x);
    float m = 0.0f;
    bool bad = false;
    if (v0 < (size_t)n) {
        const int cnt = (size_t)n - v0 < (size_t)G ? (int)((size_t)n - v0) : G;
        float p[3 * G], q[3 * G], po[3 * G], qo[3 * G];
        bool u[G];
        load_group<G>(rest_pos, v0, cnt, p);
        load_group<G>(rest_nrm, v0, cnt, q);
        load_mask<G>(used, v0, cnt, u);
#pragma unroll
        for (int k = 0; k < G; k++) {
            if (k < cnt) {
                int32_t j[4];
                float w[4];
                load_influences<G>(joints, weights, v0 + k, j, w);
                if constexpr (LDS)
                    skin_vertex((const float*)s_pal, j, w, p + 3 * k, q + 3 * k, po + 3 * k, qo + 3 * k);
                else
                    skin_vertex(recs, j, w, p + 3 * k, q + 3 * k, po + 3 * k, qo + 3 * k);
                bad |= !finite3(po + 3 * k);
                if (u[k]) m = fmaxf(m, abs_max3(po + 3 * k));
            }
        }
        store_group<G>(out_pos, v0, cnt, po);
        store_group<G>(out_nrm, v0, cnt, qo);
    }
    reduce_block(m, bad, red);
}

}  // namespace

// n vertices of the rest pose skinned by the num_joints records at recs into out_pos / out_nrm; red
// (2 words) is zeroed on the stream first and then holds the reduction.  group: vertices per lane,
// 4 or 1; lds: stage the palette in LDS when it fits.
hipError_t launch_skin(const float* rest_pos, const float* rest_nrm, const int32_t* joints, const float* weights,
                       const uint8_t* used, const float* recs, int num_joints, int n, float* out_pos, float* out_nrm,
                       uint32_t* red, int group, bool lds, hipStream_t st) {
    hipError_t e = hipMemsetAsync(red, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess || n <= 0) return e;
    const bool wide = group == 4 && aligned16(rest_pos) && aligned16(rest_nrm) && aligned16(joints) && aligned16(weights) &&
                      aligned16(out_pos) && aligned16(out_nrm) && aligned16(used);
    const bool stage = lds && num_joints <= MPT_SKIN_LDS_JOINTS && aligned16(recs);
    const size_t shm = stage ? (size_t)num_joints * REC * sizeof(float) : 0;
    const dim3 grid(blocks_for(n, wide ? 4 : 1)), block(256);
#define SKIN_LAUNCH(G, L)                                                                                                    \
    hipLaunchKernelGGL((k_skin<G, L>), grid, block, shm, st, rest_pos, rest_nrm, joints, weights, used, recs, num_joints, n, \
                       out_pos, out_nrm, red)
    if (wide && stage) SKIN_LAUNCH(4, true);
    else if (wide) SKIN_LAUNCH(4, false);
    else if (stage) SKIN_LAUNCH(1, true);
    else SKIN_LAUNCH(1, false);
#undef SKIN_LAUNCH
    return hipGetLastError();
}

// The host loop: false when an output coordinate is not finite (the outputs are then unspecified).
bool skin_host(const float* rest_pos, const float* rest_nrm, const int32_t* joints, const float* weights, size_t n,
               const float* recs, float* out_pos, float* out_nrm) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    bool ok = true;
    for (size_t i = 0; i < n; i++) {
        float no[3];
        mptskin::skin_vertex(recs, joints + 4 * i, weights + 4 * i, rest_pos + 3 * i, rest_nrm ? rest_nrm + 3 * i : zero,
                             out_pos + 3 * i, out_nrm ? out_nrm + 3 * i : no);
        ok &= mptxform::finite3(out_pos + 3 * i);
    }
    return ok;
}

// Every index in [0, num_joints) and every weight finite: NULL, or what is wrong.
const char* check_skin_table(const int32_t* joints, const float* weights, size_t num_vertices, int32_t num_joints) {
    for (size_t k = 0; k < 4 * num_vertices; k++) {
        if (joints[k] < 0 || joints[k] >= num_joints) return "joint index out of range";
        if (!(std::fabs(weights[k]) <= mptxform::F_MAX)) return "non-finite weight";
    }
    return nullptr;
}

// 16-byte aligned, as skin.h's loads of a record assume
void make_skin_records(const float* matrices, int32_t num_joints, std::vector<float4>& recs) {
    recs.resize((size_t)(mptskin::REC / 4) * (size_t)num_joints);
    mptskin::make_records(matrices, num_joints, (float*)recs.data());
}

}  // namespace mpt

extern "C" {

int mpt_skin_host(const float* rest_vertices, const float* rest_normals, const int32_t* joints, const float* weights,
                  int32_t num_vertices, const float* joint_matrices, int32_t num_joints, float* out_vertices, float* out_normals) {
    using namespace mpt;
    if (!rest_vertices || !joints || !weights || !joint_matrices || !out_vertices)
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_vertices <= 0 || num_joints < 1) return api_fail(MPT_ERR_INVALID_ARGUMENT, "skin: bad size");
    if (out_normals && !rest_normals) return api_fail(MPT_ERR_INVALID_ARGUMENT, "skin: normals out without normals in");
    if (const char* bad = check_skin_table(joints, weights, (size_t)num_vertices, num_joints))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, bad);
    if (!matrices_finite(joint_matrices, num_joints)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite matrix entry");
    std::vector<float4> recs;
    make_skin_records(joint_matrices, num_joints, recs);
    if (!skin_host(rest_vertices, rest_normals, joints, weights, (size_t)num_vertices, (const float*)recs.data(), out_vertices,
                   out_normals))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    return MPT_OK;
}

}  // extern "C"
