// lbvh.h -- the definition of the BVH8 rebuild (mpt_rebuild_bvh, mpt_bvh_build_host), shared
// verbatim by the kernels (lbvh.hip) and the host loop (build_lbvh_host), the way refit.h,
// display.h and denoise.h are shared: compiled with -ffp-contract=off on both sides, so that the
// GPU and the CPU produce the same topology and record order (DESIGN.md §2 "Rebuilds").
//
// The build runs over a primitive list (position -> scene primitive) and produces a topology and
// a record order only: imask, meta, child_base, tri_base and the records' w lanes.  Every byte
// that follows from a coordinate is then written by the refit (refit.h) run on that topology.
//   key       10 bits per axis from the centre of the triangle's padded box relative to the bounds
//             of all centres of the list (all in double: no overflow, no out-of-range conversion),
//             interleaved x, y, z from the top; the low 32 bits hold the list position
//   order     ascending by key (keys are unique)
//   tree      Karras' radix tree over the sorted keys; a node's box is the union of its range
//             (MPT_BUILD_PLOC: the tree of ploc.h instead, over the same keys, with its own leaf order;
//             MPT_BUILD_SAH: the tree of sah.h, likewise)
//   collapse  breadth first: a subtree of at most LEAF_MAX triangles is a leaf slot; a node opens
//             its non-leaf-slot child of the largest fp32 box area until it has 8 children
//   slots     the octant heuristic of bvh8.cpp, with centres and costs in double
#ifndef MPT_LBVH_H
#define MPT_LBVH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bvh8.h"
#include "refit.h"

#if defined(__HIPCC__)
#define LBVH_FN __host__ __device__ static inline
#else
#define LBVH_FN static inline
#endif

namespace mptlbvh {

using mptrefit::Box;

constexpr int LEAF_MAX = 3;                   // triangles per leaf slot (the host builder's max_leaf)
constexpr int32_t NO_REF = INT32_MIN;         // an empty slot
constexpr int SORT_TILE = 2048;               // keys per workgroup of a radix-sort pass

// A reference to a node of the binary tree: k >= 0 the internal node k, ~k < 0 the leaf (sorted
// position) k.
struct Tree {
    const int32_t* left;      // per internal node
    const int32_t* right;
    const int32_t* first;     // the range of sorted positions [first, last]
    const int32_t* last;
    const float* nbox;        // 6 floats per internal node (lo, hi)
    const float* pbox;        // 6 floats per list position
    const uint32_t* order;    // sorted position -> list position
};

// The centre of [lo, hi] on one axis: exact halves, one rounding, never inf.
LBVH_FN double centre(float lo, float hi) { return 0.5 * (double)lo + 0.5 * (double)hi; }

// 10 bits of c in [cmin, cmax]; a zero extent gives 0.
LBVH_FN uint32_t quant10(double c, double cmin, double cmax) {
    const double ext = cmax - cmin;
    if (!(ext > 0.0)) return 0u;
    const double t = (c - cmin) / ext;        // in [0, 1]: cmin <= c <= cmax, the division is monotone
    const double q = fmin(fmax(floor(t * 1024.0), 0.0), 1023.0);
    return (uint32_t)(int)q;
}

LBVH_FN uint32_t spread10(uint32_t v) {       // bit k of v to bit 3 k
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The 30-bit code of a padded box; bounds: min of the centres (3 doubles), then max.
LBVH_FN uint32_t morton_code(const float* box, const double* bounds) {
    uint32_t q[3];
    for (int a = 0; a < 3; a++) q[a] = quant10(centre(box[a], box[3 + a]), bounds[a], bounds[3 + a]);
    return (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
}

LBVH_FN int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// Length of the common key prefix of sorted positions i and j; -1 outside [0, n).
LBVH_FN int key_delta(const uint32_t* code, const uint32_t* order, int n, int i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t a = ((uint64_t)code[i] << 32) | order[i], b = ((uint64_t)code[j] << 32) | order[j];
    return clz64(a ^ b);                      // keys are unique: a != b
}

// Internal node i of Karras' radix tree over n > 1 sorted keys: its range and its two children.
LBVH_FN void radix_node(const uint32_t* code, const uint32_t* order, int n, int i, int32_t* left, int32_t* right,
                        int32_t* first, int32_t* last) {
    const int d = key_delta(code, order, n, i, (int64_t)i + 1) - key_delta(code, order, n, i, (int64_t)i - 1) >= 0 ? 1 : -1;
    const int dmin = key_delta(code, order, n, i, (int64_t)i - d);
    int64_t lmax = 2;
    while (key_delta(code, order, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (key_delta(code, order, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = key_delta(code, order, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (key_delta(code, order, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    *left = lo == g ? ~(int32_t)g : (int32_t)g;
    *right = hi == g + 1 ? ~(int32_t)(g + 1) : (int32_t)(g + 1);
    *first = (int32_t)lo;
    *last = (int32_t)hi;
}

LBVH_FN int ref_count(const Tree& T, int32_t r) { return r < 0 ? 1 : T.last[r] - T.first[r] + 1; }
LBVH_FN int ref_first(const Tree& T, int32_t r) { return r < 0 ? ~r : T.first[r]; }
LBVH_FN Box ref_box(const Tree& T, int32_t r) {
    const float* p = r < 0 ? T.pbox + 6 * (size_t)T.order[~r] : T.nbox + 6 * (size_t)r;
    Box b;
    for (int a = 0; a < 3; a++) { b.lo[a] = p[a]; b.hi[a] = p[3 + a]; }
    return b;
}

// AABB::area() of bvh8.cpp, fp32.
LBVH_FN float box_area(const Box& b) {
    const float d0 = fmaxf(0.0f, b.hi[0] - b.lo[0]), d1 = fmaxf(0.0f, b.hi[1] - b.lo[1]), d2 = fmaxf(0.0f, b.hi[2] - b.lo[2]);
    return 2.0f * (d0 * d1 + d1 * d2 + d2 * d0);
}

// The BVH8 node that stands for `ref`: its children chosen greedily and placed into slots.
// slot[s]: the child in slot s or NO_REF; n_int: children that become nodes; n_rec: records.
LBVH_FN void collapse_node(const Tree& T, int32_t ref, int32_t slot[8], int* n_int, int* n_rec) {
    int32_t ch[8];
    int nch = 0;
    if (ref_count(T, ref) <= LEAF_MAX) {
        ch[nch++] = ref;                      // (only a root: the whole list is one leaf slot)
    } else {
        ch[nch++] = T.left[ref];
        ch[nch++] = T.right[ref];
        while (nch < 8) {
            int best = -1;
            float ba = 0.0f;
            for (int i = 0; i < nch; i++) {
                if (ref_count(T, ch[i]) <= LEAF_MAX) continue;
                const float a = box_area(ref_box(T, ch[i]));
                if (best < 0 || a > ba) { ba = a; best = i; }   // strictly greater wins; the first candidate always stands
            }
            if (best < 0) break;
            const int32_t o = ch[best];
            ch[best] = T.left[o];
            ch[nch++] = T.right[o];
        }
    }
    Box cb[8], nb = mptrefit::box_empty();
    for (int i = 0; i < nch; i++) { cb[i] = ref_box(T, ch[i]); mptrefit::box_grow(nb, cb[i]); }
    double v[8][3];
    for (int i = 0; i < nch; i++)
        for (int a = 0; a < 3; a++) v[i][a] = centre(cb[i].lo[a], cb[i].hi[a]) - centre(nb.lo[a], nb.hi[a]);
    int in_slot[8];
    bool used[8];
    for (int s = 0; s < 8; s++) { in_slot[s] = -1; used[s] = false; }
    for (int round = 0; round < nch; round++) {
        double best = 0.0;
        int bi = -1, bs = -1;
        for (int i = 0; i < nch; i++) {
            if (used[i]) continue;
            for (int s = 0; s < 8; s++) {
                if (in_slot[s] >= 0) continue;
                const double cost = -(((s & 1) ? v[i][0] : -v[i][0]) + ((s & 2) ? v[i][1] : -v[i][1]) + ((s & 4) ? v[i][2] : -v[i][2]));
                if (bi < 0 || cost < best) { best = cost; bi = i; bs = s; }
            }
        }
        used[bi] = true;
        in_slot[bs] = bi;
    }
    *n_int = 0;
    *n_rec = 0;
    for (int s = 0; s < 8; s++) {
        slot[s] = in_slot[s] < 0 ? NO_REF : ch[in_slot[s]];
        if (in_slot[s] < 0) continue;
        const int c = ref_count(T, slot[s]);
        if (c > LEAF_MAX) (*n_int)++;
        else *n_rec += c;
    }
}

// The node's topology bytes (everything else zero), its internal children's references into
// next[0 .. n_int) in slot order, and its records' w lanes at recs[tri_base ..): prims maps a list
// position to the scene primitive (NULL: the identity), flags holds two words per scene primitive
// (NULL: zeros).
LBVH_FN void emit_node(const Tree& T, const int32_t slot[8], uint32_t child_base, uint32_t tri_base, const int32_t* prims,
                       const uint32_t* flags, mpt::Node8* node, int32_t* next, mpt::TriRec* recs) {
    mpt::Node8 nd;
    memset(&nd, 0, sizeof(nd));
    nd.child_base = child_base;
    nd.tri_base = tri_base;
    int rank = 0, off = 0;
    for (int s = 0; s < 8; s++) {
        const int32_t r = slot[s];
        if (r == NO_REF) continue;
        const int cnt = ref_count(T, r);
        if (cnt > LEAF_MAX) {
            nd.imask |= (uint8_t)(1u << s);
            nd.meta[s] = (uint8_t)rank;
            next[rank++] = r;
            continue;
        }
        nd.meta[s] = (uint8_t)((cnt << 5) | off);
        const int f = ref_first(T, r);
        for (int k = 0; k < cnt; k++) {
            const uint32_t li = T.order[f + k];
            const int32_t prim = prims ? prims[li] : (int32_t)li;
            const uint32_t f0 = flags ? flags[2 * (size_t)prim] : 0u, f1 = flags ? flags[2 * (size_t)prim + 1] : 0u;
            mpt::TriRec& tr = recs[(size_t)tri_base + off + k];
            memcpy(&tr.prim_bits, &prim, 4);
            memcpy(&tr.pad0, &f0, 4);
            memcpy(&tr.pad1, &f1, 4);
        }
        off += cnt;
    }
    *node = nd;
}

}  // namespace mptlbvh

namespace mpt {
// The host loop: the BVH8 over the list prims (NULL: the identity) of n_list primitives, with the
// refit's bytes (refit_host) for pos and pad; the records' flag lanes are 0.
// mode: MPT_BUILD_LBVH the radix tree above, MPT_BUILD_PLOC the binary tree of ploc.h (iterations:
// optional, how many it took), MPT_BUILD_SAH the binary tree of sah.h (iterations: its levels).
void build_lbvh_host(const float* pos, const int32_t* idx, const int32_t* prims, int n_list, float pad, BVH8& out, int mode = 0,
                     int* iterations = nullptr);
}  // namespace mpt

#undef LBVH_FN
#endif
