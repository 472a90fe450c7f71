// morph.hip -- morph targets for gfx950 (mpt_update_morph, mpt_update_morph_skin) and the host loop
// of the same arithmetic (morph.h; DESIGN.md §2 "Geometry updates", Morph targets).
//
//   k_morph<G, SKIN, LDS>  G vertices per lane, as k_skin<G> (skin.hip); G = 1 is the default, by
//                the measurement of DESIGN.md §4 (mpt_geometry.cpp: morph_group).  The rest pose and the
//                used-vertex mask are read through vert_io.h, the G + 1 row offsets of the lane's
//                group are one 16-byte load plus a dword (G = 4), and the lane walks the entries
//                of each of its vertices in turn: target index (4 B), position delta (12 B) and,
//                when the morph has them, normal delta (12 B).  The loop is divergent by entry
//                count; counts are uniform inside a mesh.
//   weights      gathered by the entry's target index.  LDS = false: through the cache.
//                LDS = true: the block first copies all T weights (padded to a multiple of four)
//                into LDS with coalesced 16-byte loads; at most MPT_MORPH_LDS_TARGETS, 16 KiB.
//   SKIN         the lane then calls mptskin::skin_vertex on the morphed position and normal in
//                registers and writes only the skinned pose: the morphed pose never goes to
//                memory.  The palette follows the weights in LDS (16-byte aligned: the weights
//                take a whole number of float4) under skin.hip's rule (<= MPT_SKIN_LDS_JOINTS);
//                the fused kernel stages only when both fit, 32 KiB per block.
//   reduction    vert_io.h's reduce_block: exact and order-free.  Its two static arrays take 32
//                bytes, so the dynamic region stays 16-byte aligned.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "morph.h"
#include "mpt.h"
#include "mpt_internal.h"
#include "skin.h"
#include "vert_io.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

static_assert(MPT_MORPH_LDS_TARGETS * sizeof(float) == 16384, "the LDS weights' budget is 16 KiB");

namespace {

using mptmorph::morph_vertex;
using mptskin::skin_vertex;
using mptxform::abs_max3;
using mptxform::finite3;
using namespace vertio;

template <int G, bool SKIN, bool LDS>
__global__ void __launch_bounds__(256) k_morph(const MorphLaunch a) {
    extern __shared__ float4 s_mem[];   // LDS: wq float4 of weights, then (SKIN) num_joints records
    const int wq = (a.num_targets + 3) / 4;
    if constexpr (LDS) {
        const float4* src = (const float4*)a.mweights;
        for (int i = (int)threadIdx.x; i < wq; i += 256) s_mem[i] = src[i];
        if constexpr (SKIN) {
            const float4* pal = (const float4*)a.recs;
            for (int i = (int)threadIdx.x; i < (mptskin::REC / 4) * a.num_joints; i += 256) s_mem[wq + i] = pal[i];
        }
        __syncthreads();
    }
    const float* w = LDS ? (const float*)s_mem : a.mweights;
    const float* pal = LDS ? (const float*)(s_mem + wq) : a.recs;
    const int n = a.n;
    const size_t v0 = (size_t)G * (size_t)(blockIdx.x * blockDim.x + threadIdx.x);
    float m = 0.0f;
    bool bad = false;
    if (v0 < (size_t)n) {
        const int cnt = (size_t)n - v0 < (size_t)G ? (int)((size_t)n - v0) : G;
        float p[3 * G], q[3 * G], po[3 * G], qo[3 * G];
        bool u[G];
        int32_t r[G + 1];
        load_group<G>(a.rest_pos, v0, cnt, p);
        load_group<G>(a.rest_nrm, v0, cnt, q);
        load_mask<G>(a.used, v0, cnt, u);
        load_rows<G>(a.row, v0, cnt, r);
#pragma unroll
        for (int k = 0; k < G; k++) {
            if (k < cnt) {
                if constexpr (SKIN) {
                    float pm[3], qm[3], sw[4];
                    int32_t j[4];
                    morph_vertex(a.tgt, a.dpos, a.dnrm, r[k], r[k + 1], w, p + 3 * k, q + 3 * k, pm, qm);
                    load_influences<G>(a.joints, a.sweights, v0 + k, j, sw);
                    skin_vertex(pal, j, sw, pm, qm, po + 3 * k, qo + 3 * k);
                } else {
                    morph_vertex(a.tgt, a.dpos, a.dnrm, r[k], r[k + 1], w, p + 3 * k, q + 3 * k, po + 3 * k, qo + 3 * k);
                }
                bad |= !finite3(po + 3 * k);
                if (u[k]) m = fmaxf(m, abs_max3(po + 3 * k));
            }
        }
        store_group<G>(a.out_pos, v0, cnt, po);
        store_group<G>(a.out_nrm, v0, cnt, qo);
    }
    reduce_block(m, bad, a.red);
}

template <int G, bool SKIN>
void launch_one(const MorphLaunch& a, bool stage, size_t shm, hipStream_t st) {
    const dim3 grid(blocks_for(a.n, G)), block(256);
    if (stage) hipLaunchKernelGGL((k_morph<G, SKIN, true>), grid, block, shm, st, a);
    else hipLaunchKernelGGL((k_morph<G, SKIN, false>), grid, block, 0, st, a);
}

}  // namespace

// The rest pose morphed (and, with a.recs, skinned) into a.out_pos / a.out_nrm; a.red (2 words) is
// zeroed on the stream first and then holds the reduction.  a.mweights holds the weights padded to
// a multiple of four floats.  group: vertices per lane, 4 or 1; lds: stage in LDS when it fits.
hipError_t launch_morph(const MorphLaunch& a, int group, bool lds, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.red, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess || a.n <= 0) return e;
    const bool skin = a.recs != nullptr;
    const bool wide = group == 4 && aligned16(a.rest_pos) && aligned16(a.rest_nrm) && aligned16(a.row) && aligned16(a.out_pos) &&
                      aligned16(a.out_nrm) && aligned16(a.used) && (!skin || (aligned16(a.joints) && aligned16(a.sweights)));
    const bool stage = lds && a.num_targets <= MPT_MORPH_LDS_TARGETS && aligned16(a.mweights) &&
                       (!skin || (a.num_joints <= MPT_SKIN_LDS_JOINTS && aligned16(a.recs)));
    const size_t shm = !stage ? 0 : (size_t)((a.num_targets + 3) / 4) * sizeof(float4) +
                                        (skin ? (size_t)a.num_joints * mptskin::REC * sizeof(float) : 0);
    if (wide && skin) launch_one<4, true>(a, stage, shm, st);
    else if (wide) launch_one<4, false>(a, stage, shm, st);
    else if (skin) launch_one<1, true>(a, stage, shm, st);
    else launch_one<1, false>(a, stage, shm, st);
    return hipGetLastError();
}

// The host loop: false when an output coordinate is not finite (the outputs are then unspecified).
bool morph_host(const float* rest_pos, const float* rest_nrm, size_t n, const mptmorph::Csr& m, const float* weights, float* out_pos,
                float* out_nrm) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    bool ok = true;
    for (size_t i = 0; i < n; i++) {
        float no[3];
        mptmorph::morph_vertex(m.tgt.data(), m.dpos.data(), m.dnrm.empty() ? nullptr : m.dnrm.data(), m.row[i], m.row[i + 1], weights,
                               rest_pos + 3 * i, rest_nrm ? rest_nrm + 3 * i : zero, out_pos + 3 * i, out_nrm ? out_nrm + 3 * i : no);
        ok &= mptxform::finite3(out_pos + 3 * i);
    }
    return ok;
}

bool weights_finite(const float* w, int32_t n) {
    for (int32_t k = 0; k < n; k++)
        if (!(std::fabs(w[k]) <= mptxform::F_MAX)) return false;
    return true;
}

}  // namespace mpt

extern "C" {

int mpt_morph_host(const float* rest_vertices, const float* rest_normals, int32_t num_vertices, int32_t num_targets,
                   const int32_t* target_offsets, const int32_t* vertex_ids, const float* pos_deltas, const float* nrm_deltas,
                   const float* weights, float* out_vertices, float* out_normals) {
    using namespace mpt;
    if (!rest_vertices || !target_offsets || !weights || !out_vertices) return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_vertices <= 0) return api_fail(MPT_ERR_INVALID_ARGUMENT, "morph: bad size");
    if (out_normals && !rest_normals) return api_fail(MPT_ERR_INVALID_ARGUMENT, "morph: normals out without normals in");
    mptmorph::Csr csr;
    if (const char* bad = mptmorph::to_csr(num_targets, target_offsets, vertex_ids, pos_deltas, nrm_deltas, num_vertices, csr))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, bad);
    if (!weights_finite(weights, num_targets)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite morph weight");
    if (!morph_host(rest_vertices, rest_normals, (size_t)num_vertices, csr, weights, out_vertices, out_normals))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    return MPT_OK;
}

}  // extern "C"
