// anim.h -- the arithmetic of glTF animation clips (mpt_update_animation), shared verbatim by the
// kernel (anim.hip: k_anim) and the host loop (animation_host, behind mpt_animation_host), the way
// skin.h and morph.h are: compiled with -ffp-contract=off on both sides, so that the GPU and the
// CPU produce the same bytes.  The transcendentals are tmath.h's; libm is never used.
//
// Tables (struct Tables; check_animation below refuses what does not fit them):
//   nodes      parent (-1: a root), base TRS as 10 floats (translation 3, rotation x y z w, scale
//              3), a byte that is 1 when the node was given as TRS, and the row-major 3x4 float64
//              local matrix, which is what a node given as a `matrix` uses
//   joints     node and row-major 3x4 float64 bind matrix (SkinData.bind)
//   targets    T base weights
//   samplers   K key times (float32, strictly ascending), the values, and the interpolation:
//              STEP 0, LINEAR 1, CUBICSPLINE 2.  A value has W components: 3 (translation, scale),
//              4 (rotation) or the channel's target count (weights).  STEP / LINEAR store K values;
//              CUBICSPLINE stores per key the in-tangent a, the value v and the out-tangent b, three
//              blocks of W
//   channels   sampler, node, path (translation 0, rotation 1, scale 2, weights 3) and, for
//              weights, the stretch [first target, first target + count) of the weight vector
//
// Key search, time t (float32, finite):
//   t is clamped to [times[0], times[K-1]].  K == 1, or t equal to the last key: that key's value
//   (v for CUBICSPLINE), no arithmetic.  Otherwise k with times[k] <= t < times[k+1] by binary
//   search, dt = times[k+1] - times[k], u = (t - times[k]) / dt in fp32.  u == 0 (t on a key):
//   key k's value, no arithmetic (a + 0*(b - a) would turn a -0 into +0), for every interpolation.
// Interpolation, all fp32, no fma, per component unless said otherwise:
//   STEP         the value at k
//   LINEAR       a + u*(b - a)                                  translation, scale, weights
//   LINEAR rot.  d = ((x0*x1 + y0*y1) + z0*z1) + w0*w1; d < 0: q1 and d negated;
//                d > SLERP_LERP (0.9995): q = q0 + u*(q1 - q0);
//                else th = acosf_(d), s = sinf_(th), c0 = sinf_((1 - u)*th)/s, c1 = sinf_(u*th)/s,
//                q = c0*q0 + c1*q1;  then normalised (below)
//   CUBICSPLINE  u2 = u*u, u3 = u2*u,
//                h00 = (2*u3 - 3*u2) + 1, h10 = (u3 - 2*u2) + u, h01 = 3*u2 - 2*u3, h11 = u3 - u2,
//                p = ((h00*v_k + (dt*h10)*b_k) + h01*v_k1) + (dt*h11)*a_k1;  rotations normalised
//   normalised   l2 = ((x*x + y*y) + z*z) + w*w, q / sqrtf(l2): a zero quaternion becomes NaN and
//                raises the flag
//   A sampled component that is not finite raises the flag.
// Local matrices and the hierarchy, float64, no fma:
//   a TRS node: the fp32 components widened (exact); R from the quaternion as scene._quat_to_mat
//   does (1 - 2*(y*y + z*z), 2*(x*y - z*w), ...), L[r][c] = R[r][c]*s[c], L[r][3] = t[r];
//   a matrix node: its stored local.
//   world = world[parent] * local as 3x4 affine products:
//     P[r][c] = (A[r][0]*B[0][c] + A[r][1]*B[1][c]) + A[r][2]*B[2][c]   (+ A[r][3] for c == 3, last)
//   level by level from the roots (order / level_begin, made by check_animation: the numbering of
//   the nodes does not matter).  M_j = world[joint node] * bind[j], each entry rounded to float.
// Joint record: skin.h's 16 words -- the 12 floats, the identity word from mptxform::is_identity on
// the rounded floats, 3 words of padding.  A non-finite entry raises the flag.
// Weights: the base weights with the sampled stretches over them; a non-finite weight raises the flag.
#ifndef MPT_ANIM_H
#define MPT_ANIM_H

#include <vector>

#include "mpt.h"
#include "skin.h"
#include "tmath.h"
#include "xform.h"

#if defined(__HIPCC__)
#define ANIM_FN __host__ __device__ static inline
#else
#define ANIM_FN static inline
#endif

namespace mptanim {

enum { STEP = 0, LINEAR = 1, CUBIC = 2 };
enum { P_TRANSLATION = 0, P_ROTATION = 1, P_SCALE = 2, P_WEIGHTS = 3 };
constexpr float SLERP_LERP = 0.9995f;
constexpr int TRS = 10;   // floats per node: translation, rotation, scale

// The tables as both sides read them (device pointers in the kernel, host pointers in the host
// loop), with the scratch the evaluation writes: the sampled TRS (10 floats per node), the sampled
// weights (T floats) and, for the path that keeps them in memory, the world matrices (12 doubles
// per node).
struct Tables {
    int32_t N, J, T, S, C, levels;
    const int32_t* parent;
    const float* trs;
    const uint8_t* is_trs;
    const double* local;
    const int32_t* jnode;
    const double* bind;
    const float* basew;
    const int32_t* koff;
    const float* times;
    const int32_t* voff;
    const float* values;
    const int32_t* interp;
    const int32_t* csamp;
    const int32_t* cnode;
    const int32_t* cpath;
    const int32_t* ctgt0;
    const int32_t* ctgtn;
    const int32_t* order;         // the nodes by depth
    const int32_t* level_begin;   // levels + 1 entries into order
    float* trs_s;
    float* w_s;
    double* world_g;
};

ANIM_FN bool finite_f(float f) { return fabsf(f) <= mptxform::F_MAX; }

// false: key k's value as it is stored; true: interpolate between k and k + 1 with u and dt.
ANIM_FN bool find_key(const float* times, int32_t K, float t, int32_t& k, float& u, float& dt) {
    if (t < times[0]) t = times[0];
    if (t > times[K - 1]) t = times[K - 1];
    u = 0.0f;
    dt = 0.0f;
    if (K == 1 || t == times[K - 1]) {
        k = K - 1;
        return false;
    }
    int32_t lo = 0, hi = K - 1;   // times[lo] <= t < times[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (times[mid] <= t) lo = mid;
        else hi = mid;
    }
    k = lo;
    dt = times[k + 1] - times[k];
    u = (t - times[k]) / dt;
    return u != 0.0f;
}

ANIM_FN float lerp1(float a, float b, float u) { return a + u * (b - a); }

ANIM_FN float cubic1(float vk, float bk, float vk1, float ak1, float u, float dt) {
    const float u2 = u * u, u3 = u2 * u;
    const float h00 = (2.0f * u3 - 3.0f * u2) + 1.0f, h10 = (u3 - 2.0f * u2) + u, h01 = 3.0f * u2 - 2.0f * u3, h11 = u3 - u2;
    return ((h00 * vk + (dt * h10) * bk) + h01 * vk1) + (dt * h11) * ak1;
}

ANIM_FN void normalise4(float* q) {
    const float l = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int e = 0; e < 4; e++) q[e] = q[e] / l;
}

ANIM_FN void slerp(const float* q0, const float* q1in, float u, float* q) {
    float q1[4] = {q1in[0], q1in[1], q1in[2], q1in[3]};
    float d = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3];
    if (d < 0.0f) {
        for (int e = 0; e < 4; e++) q1[e] = -q1[e];
        d = -d;
    }
    if (d > SLERP_LERP) {
        for (int e = 0; e < 4; e++) q[e] = lerp1(q0[e], q1[e], u);
    } else {
        const float th = tmath::acosf_(d), s = tmath::sinf_(th);
        const float c0 = tmath::sinf_((1.0f - u) * th) / s, c1 = tmath::sinf_(u * th) / s;
        for (int e = 0; e < 4; e++) q[e] = c0 * q0[e] + c1 * q1[e];
    }
    normalise4(q);
}

// One channel at time t into the sampled TRS of its node or its stretch of the sampled weights.
// false: a sampled component is not finite.
ANIM_FN bool sample_channel(const Tables& a, int32_t c, float t) {
    const int32_t s = a.csamp[c], path = a.cpath[c];
    const int32_t K = a.koff[s + 1] - a.koff[s];
    const float* times = a.times + a.koff[s];
    const float* vals = a.values + a.voff[s];
    const int32_t interp = a.interp[s];
    const int32_t W = path == P_WEIGHTS ? a.ctgtn[c] : path == P_ROTATION ? 4 : 3;
    float* out = path == P_WEIGHTS ? a.w_s + a.ctgt0[c]
                                   : a.trs_s + (size_t)TRS * (size_t)a.cnode[c] + (path == P_TRANSLATION ? 0 : path == P_ROTATION ? 3 : 7);
    int32_t k;
    float u, dt;
    const bool ip = find_key(times, K, t, k, u, dt);
    const size_t stride = interp == CUBIC ? 3 * (size_t)W : (size_t)W;   // floats per key
    const float* vk = vals + stride * (size_t)k + (interp == CUBIC ? W : 0);
    bool ok = true;
    if (!ip || interp == STEP) {
        for (int32_t e = 0; e < W; e++) { out[e] = vk[e]; ok = ok && finite_f(vk[e]); }
        return ok;
    }
    const float* vk1 = vk + stride;
    if (interp == LINEAR && path == P_ROTATION) {
        float q[4];
        slerp(vk, vk1, u, q);
        for (int e = 0; e < 4; e++) { out[e] = q[e]; ok = ok && finite_f(q[e]); }
        return ok;
    }
    if (interp == LINEAR) {
        for (int32_t e = 0; e < W; e++) { out[e] = lerp1(vk[e], vk1[e], u); ok = ok && finite_f(out[e]); }
        return ok;
    }
    const float* bk = vk + W;        // key k's out-tangent
    const float* ak1 = vk1 - W;      // key k + 1's in-tangent
    if (path == P_ROTATION) {
        float q[4];
        for (int e = 0; e < 4; e++) q[e] = cubic1(vk[e], bk[e], vk1[e], ak1[e], u, dt);
        normalise4(q);
        for (int e = 0; e < 4; e++) { out[e] = q[e]; ok = ok && finite_f(q[e]); }
        return ok;
    }
    for (int32_t e = 0; e < W; e++) { out[e] = cubic1(vk[e], bk[e], vk1[e], ak1[e], u, dt); ok = ok && finite_f(out[e]); }
    return ok;
}

// A node's local matrix (12 doubles) from its sampled TRS, or its stored local.
ANIM_FN void make_local(const Tables& a, int32_t n, double* L) {
    if (!a.is_trs[n]) {
        for (int e = 0; e < 12; e++) L[e] = a.local[12 * (size_t)n + e];
        return;
    }
    const float* f = a.trs_s + (size_t)TRS * (size_t)n;
    const double x = (double)f[3], y = (double)f[4], z = (double)f[5], w = (double)f[6];
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                         2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                         2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) L[4 * r + c] = R[3 * r + c] * (double)f[7 + c];
        L[4 * r + 3] = (double)f[r];
    }
}

// P = A * B, 3x4 affine (P may be A or B).
ANIM_FN void mul34(const double* A, const double* B, double* P) {
    double o[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++) o[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        o[4 * r + 3] = o[4 * r + 3] + A[4 * r + 3];
    }
    for (int e = 0; e < 12; e++) P[e] = o[e];
}

// Joint j's 16-word record from its node's world matrix.  false: an entry is not finite.
ANIM_FN bool joint_record(const double* world, const double* bind, float* rec) {
    double M[12];
    mul34(world, bind, M);
    bool ok = true;
    for (int e = 0; e < 12; e++) {
        rec[e] = (float)M[e];
        ok = ok && finite_f(rec[e]);
    }
    const uint32_t tail[4] = {mptxform::is_identity(rec) ? 1u : 0u, 0u, 0u, 0u};
    memcpy(rec + mptskin::FLAG, tail, sizeof(tail));
    return ok;
}

// The host check of the tables: NULL, or what is wrong with them (order and level_begin are then
// unspecified).  It also orders the nodes by depth: order[level_begin[l] .. level_begin[l + 1]) are
// the nodes of depth l, the roots first.
static inline const char* check_animation(const MptAnimation& a, std::vector<int32_t>& order, std::vector<int32_t>& level_begin) {
    const int32_t N = a.num_nodes, J = a.num_joints, T = a.num_targets, S = a.num_samplers, C = a.num_channels;
    if (N < 1 || J < 0 || T < 0 || S < 0 || C < 0) return "animation: bad count";
    if (J == 0 && T == 0) return "animation: neither joints nor targets";
    if (!a.node_parents || !a.node_trs || !a.node_is_trs || !a.node_locals) return "NULL argument";
    if (J > 0 && (!a.joint_nodes || !a.joint_bind)) return "NULL argument";
    if (T > 0 && !a.base_weights) return "NULL argument";
    if (S > 0 && (!a.sampler_key_offsets || !a.key_times || !a.sampler_value_offsets || !a.values || !a.sampler_interp)) return "NULL argument";
    if (C > 0 && (S < 1 || !a.channel_sampler || !a.channel_node || !a.channel_path || !a.channel_first_target || !a.channel_num_targets))
        return "NULL argument";
    for (int32_t n = 0; n < N; n++)
        if (a.node_parents[n] < -1 || a.node_parents[n] >= N) return "animation: parent index out of range";
    // depths, walking up from every node to one whose depth is known (more than N steps: a cycle)
    std::vector<int32_t> depth((size_t)N, -1), path;
    int32_t levels = 0;
    for (int32_t n = 0; n < N; n++) {
        path.clear();
        int32_t m = n;
        while (m >= 0 && depth[m] < 0) {
            if ((int32_t)path.size() > N) return "animation: cycle in the node parents";
            path.push_back(m);
            m = a.node_parents[m];
        }
        int32_t d = m < 0 ? 0 : depth[m] + 1;
        // (a cycle never reaches a known depth or a root: the walk above has stopped it)
        for (size_t k = path.size(); k-- > 0;) depth[path[k]] = d++;
        if (d > levels) levels = d;
    }
    level_begin.assign((size_t)levels + 1, 0);
    for (int32_t n = 0; n < N; n++) level_begin[(size_t)depth[n] + 1]++;
    for (int32_t l = 0; l < levels; l++) level_begin[(size_t)l + 1] += level_begin[l];
    order.resize((size_t)N);
    {
        std::vector<int32_t> at(level_begin.begin(), level_begin.end() - 1);
        for (int32_t n = 0; n < N; n++) order[(size_t)at[depth[n]]++] = n;
    }
    for (size_t k = 0; k < (size_t)TRS * (size_t)N; k++)
        if (!finite_f(a.node_trs[k])) return "animation: non-finite value";
    for (size_t k = 0; k < 12 * (size_t)N; k++)
        if (!(fabs(a.node_locals[k]) <= 1.7976931348623157e308)) return "animation: non-finite value";
    for (int32_t n = 0; n < N; n++) {
        const float* q = a.node_trs + (size_t)TRS * (size_t)n + 3;
        if (a.node_is_trs[n] && q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f) return "animation: rotation of zero length";
    }
    for (int32_t j = 0; j < J; j++)
        if (a.joint_nodes[j] < 0 || a.joint_nodes[j] >= N) return "animation: joint node out of range";
    for (size_t k = 0; k < 12 * (size_t)J; k++)
        if (!(fabs(a.joint_bind[k]) <= 1.7976931348623157e308)) return "animation: non-finite value";
    for (int32_t k = 0; k < T; k++)
        if (!finite_f(a.base_weights[k])) return "animation: non-finite value";
    if (S > 0 && (a.sampler_key_offsets[0] != 0 || a.sampler_value_offsets[0] != 0)) return "animation: offsets do not start at 0";
    for (int32_t s = 0; s < S; s++) {
        if (a.sampler_key_offsets[s + 1] < a.sampler_key_offsets[s] || a.sampler_value_offsets[s + 1] < a.sampler_value_offsets[s])
            return "animation: offsets decrease";
        if (a.sampler_key_offsets[s + 1] == a.sampler_key_offsets[s]) return "animation: sampler without keys";
        if (a.sampler_interp[s] < STEP || a.sampler_interp[s] > CUBIC) return "animation: bad interpolation";
        for (int32_t k = a.sampler_key_offsets[s]; k < a.sampler_key_offsets[s + 1]; k++) {
            if (!finite_f(a.key_times[k])) return "animation: key time not finite";
            if (k > a.sampler_key_offsets[s] && !(a.key_times[k] > a.key_times[k - 1])) return "animation: key times not strictly ascending";
        }
    }
    if (S > 0)
        for (int32_t k = 0; k < a.sampler_value_offsets[S]; k++)
            if (!finite_f(a.values[k])) return "animation: non-finite value";
    // what every channel writes: a node's translation / rotation / scale, or targets
    std::vector<uint8_t> wrote_trs(3 * (size_t)N, 0), wrote_w((size_t)T, 0);
    for (int32_t c = 0; c < C; c++) {
        const int32_t s = a.channel_sampler[c], n = a.channel_node[c], path = a.channel_path[c];
        if (s < 0 || s >= S) return "animation: channel sampler out of range";
        if (n < 0 || n >= N) return "animation: channel node out of range";
        if (path < P_TRANSLATION || path > P_WEIGHTS) return "animation: bad channel path";
        const int32_t K = a.sampler_key_offsets[s + 1] - a.sampler_key_offsets[s];
        const int32_t cubic = a.sampler_interp[s] == CUBIC ? 3 : 1;
        int32_t W = path == P_ROTATION ? 4 : 3;
        if (path == P_WEIGHTS) {
            const int32_t t0 = a.channel_first_target[c];
            W = a.channel_num_targets[c];
            if (t0 < 0 || W < 1 || t0 > T || W > T - t0) return "animation: weights channel outside the targets";
            for (int32_t k = t0; k < t0 + W; k++) {
                if (wrote_w[k]) return "animation: two channels write the same component";
                wrote_w[k] = 1;
            }
        } else {
            if (!a.node_is_trs[n]) return "animation: channel on a node given as a matrix";
            if (wrote_trs[3 * (size_t)n + path]) return "animation: two channels write the same component";
            wrote_trs[3 * (size_t)n + path] = 1;
        }
        if ((int64_t)(a.sampler_value_offsets[s + 1] - a.sampler_value_offsets[s]) != (int64_t)K * W * cubic)
            return "animation: value count does not match the key count";
        if (path == P_ROTATION) {
            const float* v = a.values + a.sampler_value_offsets[s];
            for (int32_t k = 0; k < K; k++) {
                const float* q = v + (size_t)4 * cubic * k + (cubic == 3 ? 4 : 0);
                if (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f) return "animation: rotation of zero length";
            }
        }
    }
    return nullptr;
}

}  // namespace mptanim

#undef ANIM_FN
#endif
