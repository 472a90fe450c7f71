// anim.hip -- glTF animation clips for gfx950 (mpt_update_animation) and the host loop of the same
// arithmetic (anim.h; DESIGN.md §2 "Geometry updates", Animation).
//
//   k_anim<LDS>  ONE workgroup of 256 lanes: the phases depend on each other and the counts are
//                small.  The lanes stride over the work of a phase, a barrier between phases:
//                  0  base TRS and base weights copied into the sampled TRS / weights (scratch)
//                  1  one lane per channel samples into them (no two channels write one component)
//                  2  one lane per node makes its local matrix, stored in the node's world slot
//                  3  level by level from the roots, one lane per node of the level:
//                     world = world[parent] * world (its own slot still holds the local); a barrier
//                     per level
//                  4  one lane per joint writes its 16-word record with four 16-byte stores
//                  5  one lane per four targets writes the zero-padded weights
//                Every lane carries a non-finite bit; the block ORs them and one lane stores the
//                word.
//   world        12 doubles per node.  LDS = true: in LDS, up to MPT_ANIM_LDS_NODES nodes (48 KiB).
//                LDS = false: in the tables' scratch array in memory.  The sampled TRS and weights
//                are scratch in memory either way, so every barrier is preceded by a workgroup
//                fence: one workgroup runs on one CU and shares its vector cache, and the fence
//                orders each wave's stores before the barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "anim.h"
#include "mpt.h"
#include "mpt_internal.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

static_assert(MPT_ANIM_LDS_NODES * 12 * sizeof(double) == 49152, "the LDS world matrices' budget is 48 KiB");

namespace {

using mptanim::Tables;

__device__ inline void phase_end() {
    __threadfence_block();
    __syncthreads();
}

template <bool LDS>
__global__ void __launch_bounds__(256) k_anim(const Tables a, const float t, float4* recs, float4* wout, uint32_t* flag) {
    __shared__ double s_world[LDS ? 12 * MPT_ANIM_LDS_NODES : 12];
    double* world = LDS ? s_world : a.world_g;
    const int tid = (int)threadIdx.x;
    bool bad = false;
    for (int i = tid; i < mptanim::TRS * a.N; i += 256) a.trs_s[i] = a.trs[i];
    for (int i = tid; i < a.T; i += 256) a.w_s[i] = a.basew[i];
    phase_end();
    for (int c = tid; c < a.C; c += 256) bad |= !mptanim::sample_channel(a, c, t);
    phase_end();
    for (int n = tid; n < a.N; n += 256) mptanim::make_local(a, n, world + 12 * (size_t)n);
    phase_end();
    for (int l = 1; l < a.levels; l++) {
        const int e = a.level_begin[l + 1];
        for (int i = a.level_begin[l] + tid; i < e; i += 256) {
            const int n = a.order[i];
            double* w = world + 12 * (size_t)n;
            mptanim::mul34(world + 12 * (size_t)a.parent[n], w, w);
        }
        phase_end();
    }
    for (int j = tid; j < a.J; j += 256) {
        float rec[mptskin::REC];
        bad |= !mptanim::joint_record(world + 12 * (size_t)a.jnode[j], a.bind + 12 * (size_t)j, rec);
        for (int q = 0; q < mptskin::REC / 4; q++)
            recs[(mptskin::REC / 4) * (size_t)j + q] = make_float4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
    }
    for (int q = tid; q < (a.T + 3) / 4; q += 256) {
        float w[4];
        for (int e = 0; e < 4; e++) {
            w[e] = 4 * q + e < a.T ? a.w_s[4 * q + e] : 0.0f;
            bad |= !mptanim::finite_f(w[e]);
        }
        wout[q] = make_float4(w[0], w[1], w[2], w[3]);
    }
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) *flag = any ? 1u : 0u;
}

// The sections of the packed tables, each 16-byte aligned.
enum { SEC_PARENT, SEC_TRS, SEC_IS_TRS, SEC_LOCAL, SEC_JNODE, SEC_BIND, SEC_BASEW, SEC_KOFF, SEC_TIMES, SEC_VOFF, SEC_VALUES,
       SEC_INTERP, SEC_CSAMP, SEC_CNODE, SEC_CPATH, SEC_CTGT0, SEC_CTGTN, SEC_ORDER, SEC_LEVELS, SEC_TRS_S, SEC_W_S, SEC_WORLD, SEC_COUNT };
static_assert(SEC_COUNT == AnimPacked::SECTIONS, "AnimPacked::off");

size_t add_section(std::vector<unsigned char>& blob, const void* src, size_t bytes) {
    const size_t o = (blob.size() + 15) & ~(size_t)15;
    blob.resize(o + std::max(bytes, (size_t)16), 0);   // (no section is empty: no pointer past the end)
    if (src && bytes) std::memcpy(&blob[o], src, bytes);
    return o;
}

}  // namespace

// check_animation, then the tables and their scratch packed into one array of 16-byte aligned
// sections (one upload, one buffer to swap).  Returns NULL, or what is wrong with the tables.
const char* pack_animation(const MptAnimation& a, AnimPacked& out) {
    std::vector<int32_t> order, level_begin;
    if (const char* bad = mptanim::check_animation(a, order, level_begin)) return bad;
    const size_t N = (size_t)a.num_nodes, J = (size_t)a.num_joints, T = (size_t)a.num_targets, S = (size_t)a.num_samplers,
                 C = (size_t)a.num_channels;
    const size_t K = S ? (size_t)a.sampler_key_offsets[S] : 0, V = S ? (size_t)a.sampler_value_offsets[S] : 0;
    out.N = a.num_nodes; out.J = a.num_joints; out.T = a.num_targets; out.S = a.num_samplers; out.C = a.num_channels;
    out.levels = (int32_t)level_begin.size() - 1;
    std::vector<unsigned char>& b = out.blob;
    b.clear();
    size_t* o = out.off;
    o[SEC_PARENT] = add_section(b, a.node_parents, N * sizeof(int32_t));
    o[SEC_TRS] = add_section(b, a.node_trs, mptanim::TRS * N * sizeof(float));
    o[SEC_IS_TRS] = add_section(b, a.node_is_trs, N);
    o[SEC_LOCAL] = add_section(b, a.node_locals, 12 * N * sizeof(double));
    o[SEC_JNODE] = add_section(b, a.joint_nodes, J * sizeof(int32_t));
    o[SEC_BIND] = add_section(b, a.joint_bind, 12 * J * sizeof(double));
    o[SEC_BASEW] = add_section(b, a.base_weights, T * sizeof(float));
    o[SEC_KOFF] = add_section(b, a.sampler_key_offsets, S ? (S + 1) * sizeof(int32_t) : 0);
    o[SEC_TIMES] = add_section(b, a.key_times, K * sizeof(float));
    o[SEC_VOFF] = add_section(b, a.sampler_value_offsets, S ? (S + 1) * sizeof(int32_t) : 0);
    o[SEC_VALUES] = add_section(b, a.values, V * sizeof(float));
    o[SEC_INTERP] = add_section(b, a.sampler_interp, S * sizeof(int32_t));
    o[SEC_CSAMP] = add_section(b, a.channel_sampler, C * sizeof(int32_t));
    o[SEC_CNODE] = add_section(b, a.channel_node, C * sizeof(int32_t));
    o[SEC_CPATH] = add_section(b, a.channel_path, C * sizeof(int32_t));
    o[SEC_CTGT0] = add_section(b, a.channel_first_target, C * sizeof(int32_t));
    o[SEC_CTGTN] = add_section(b, a.channel_num_targets, C * sizeof(int32_t));
    o[SEC_ORDER] = add_section(b, order.data(), N * sizeof(int32_t));
    o[SEC_LEVELS] = add_section(b, level_begin.data(), level_begin.size() * sizeof(int32_t));
    o[SEC_TRS_S] = add_section(b, nullptr, mptanim::TRS * N * sizeof(float));
    o[SEC_W_S] = add_section(b, nullptr, T * sizeof(float));
    o[SEC_WORLD] = add_section(b, nullptr, 12 * N * sizeof(double));
    b.resize((b.size() + 15) & ~(size_t)15, 0);
    return nullptr;
}

// The tables of p as they lie at base (the host's blob, or its copy on the device).
Tables anim_tables(const AnimPacked& p, unsigned char* base) {
    Tables t{};
    t.N = p.N; t.J = p.J; t.T = p.T; t.S = p.S; t.C = p.C; t.levels = p.levels;
    const size_t* o = p.off;
    t.parent = (const int32_t*)(base + o[SEC_PARENT]);
    t.trs = (const float*)(base + o[SEC_TRS]);
    t.is_trs = (const uint8_t*)(base + o[SEC_IS_TRS]);
    t.local = (const double*)(base + o[SEC_LOCAL]);
    t.jnode = (const int32_t*)(base + o[SEC_JNODE]);
    t.bind = (const double*)(base + o[SEC_BIND]);
    t.basew = (const float*)(base + o[SEC_BASEW]);
    t.koff = (const int32_t*)(base + o[SEC_KOFF]);
    t.times = (const float*)(base + o[SEC_TIMES]);
    t.voff = (const int32_t*)(base + o[SEC_VOFF]);
    t.values = (const float*)(base + o[SEC_VALUES]);
    t.interp = (const int32_t*)(base + o[SEC_INTERP]);
    t.csamp = (const int32_t*)(base + o[SEC_CSAMP]);
    t.cnode = (const int32_t*)(base + o[SEC_CNODE]);
    t.cpath = (const int32_t*)(base + o[SEC_CPATH]);
    t.ctgt0 = (const int32_t*)(base + o[SEC_CTGT0]);
    t.ctgtn = (const int32_t*)(base + o[SEC_CTGTN]);
    t.order = (const int32_t*)(base + o[SEC_ORDER]);
    t.level_begin = (const int32_t*)(base + o[SEC_LEVELS]);
    t.trs_s = (float*)(base + o[SEC_TRS_S]);
    t.w_s = (float*)(base + o[SEC_W_S]);
    t.world_g = (double*)(base + o[SEC_WORLD]);
    return t;
}

// The clip at time t into recs (a.J 16-word records) and wout ((a.T + 3) / 4 float4 of padded
// weights), both 16-byte aligned; flag: one word, 1 when a value, weight or matrix entry is not
// finite.  lds: keep the world matrices in LDS when a.N <= MPT_ANIM_LDS_NODES.
hipError_t launch_anim(const Tables& a, float t, float4* recs, float4* wout, uint32_t* flag, bool lds, hipStream_t st) {
    if (lds && a.N <= MPT_ANIM_LDS_NODES) hipLaunchKernelGGL((k_anim<true>), dim3(1), dim3(256), 0, st, a, t, recs, wout, flag);
    else hipLaunchKernelGGL((k_anim<false>), dim3(1), dim3(256), 0, st, a, t, recs, wout, flag);
    return hipGetLastError();
}

// The host loop: the phases of k_anim in order.  false: a value, weight or matrix entry is not
// finite (the outputs are then unspecified).  a's scratch is written.
bool animation_host(const Tables& a, float t, float* out_matrices, float* out_weights) {
    bool ok = true;
    for (size_t i = 0; i < (size_t)mptanim::TRS * (size_t)a.N; i++) a.trs_s[i] = a.trs[i];
    for (int32_t i = 0; i < a.T; i++) a.w_s[i] = a.basew[i];
    for (int32_t c = 0; c < a.C; c++) ok &= mptanim::sample_channel(a, c, t);
    for (int32_t n = 0; n < a.N; n++) mptanim::make_local(a, n, a.world_g + 12 * (size_t)n);
    for (int32_t i = a.level_begin[1]; i < a.N; i++) {
        const int32_t n = a.order[i];
        double* w = a.world_g + 12 * (size_t)n;
        mptanim::mul34(a.world_g + 12 * (size_t)a.parent[n], w, w);
    }
    for (int32_t j = 0; j < a.J; j++) {
        float rec[mptskin::REC];
        ok &= mptanim::joint_record(a.world_g + 12 * (size_t)a.jnode[j], a.bind + 12 * (size_t)j, rec);
        if (out_matrices) std::memcpy(out_matrices + 12 * (size_t)j, rec, 12 * sizeof(float));
    }
    for (int32_t k = 0; k < a.T; k++) {
        ok &= mptanim::finite_f(a.w_s[k]);
        if (out_weights) out_weights[k] = a.w_s[k];
    }
    return ok;
}

}  // namespace mpt

extern "C" {

int mpt_animation_host(const MptAnimation* anim, float time, float* out_matrices, float* out_weights) {
    using namespace mpt;
    if (!anim) return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(std::fabs(time) <= mptxform::F_MAX)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "animation: time not finite");
    AnimPacked p;
    if (const char* bad = pack_animation(*anim, p)) return api_fail(MPT_ERR_INVALID_ARGUMENT, bad);
    if (!animation_host(anim_tables(p, p.blob.data()), time, out_matrices, out_weights))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "animation: non-finite value");
    return MPT_OK;
}

}  // extern "C"
