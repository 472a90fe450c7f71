// sah.h -- the binary tree of the rebuild's binned-SAH mode (MPT_BUILD_SAH): a top-down build with
// SAH_BINS bins per axis, the algorithm of the host builder (bvh8.cpp, Builder::build2) made level
// synchronous, shared verbatim by the kernels (sah.hip) and the host loop (sah_tree_host) and
// compiled with -ffp-contract=off on both sides (DESIGN.md §2 "Rebuilds").  Boxes, centres, keys
// and the initial order are lbvh.h's; what comes out is what mptlbvh::Tree holds, so that
// collapse_node and emit_node run on it unmodified, started at the root this build reports.
//
//   node       a range [first, last] of sorted positions at binary depth d (the level of the build);
//              B: the min / max union of its members' pbox; CB: the min / max of its members'
//              centres (lbvh.h centre(), double).  At most LEAF_MAX positions: not split.
//   bins       (d < sah_depth) per axis with CB.hi - CB.lo > 0: bin = floor((c - CB.lo) / ext *
//              SAH_BINS) clamped to [0, SAH_BINS - 1], in double (quant10's shape); per bin the
//              count and the union of the members' pbox
//   split      s from SAH_BINS - 1 down to 1: left = bins [0, s), right = bins [s, SAH_BINS); s is
//              skipped when either side is empty; cost = (double)area(L) * nL + (double)area(R) * nR
//              with lbvh.h's fp32 box_area; not-a-number counts as +inf; the best starts at +inf and
//              a candidate wins only when strictly lower; axes ascend (ties: the earlier axis, the
//              larger s)
//   partition  members with bin < s go left, the others right, stable on both sides; without a
//              split (no extent, every cost +inf, d >= sah_depth) the first count / 2 positions of
//              the current order go left.  Both children are non-empty.
//   ids        a node that splits between positions m - 1 and m is node m - 1; an unsplit node of 2
//              or 3 positions is node `first`; a single position is the leaf ~first.  Both children's
//              ids lie in their own ranges, on either side of m - 1: ids are unique and below n - 1.
//   depth      every level halves a range at worst after sah_depth levels: at most sah_depth +
//              ceil(log2 n) + 1 levels; the loops stop with an error at SAH_MAX_LEVELS.
//
// Every reduction is a min, a max or an integer count: exact in any order, so the kernels' atomics
// and the host's loops agree bit for bit.  -0 against +0, the one case where min / max depend on
// the order, does not occur (a padded box side is x -+ pad with pad > 0, a centre is a sum of halves
// of opposite sign or of one sign: neither rounds to -0) and would be harmless: extents, bins, areas
// and comparisons do not see the sign of a zero, and no coordinate of this tree reaches the output
// (the refit writes those from the triangles).
#ifndef MPT_SAH_H
#define MPT_SAH_H

#include "lbvh.h"

#if defined(__HIPCC__)
#define SAH_FN __host__ __device__ static inline
#else
#define SAH_FN static inline
#endif

namespace mptsah {

using mptrefit::Box;

constexpr int SAH_BINS = 32;
constexpr int SAH_DEPTH = 40;                 // build2's sah_depth: below it only count splits
constexpr int SAH_TAIL = 1024;                // a node of at most this many positions: one wave, its bins in LDS
constexpr int SAH_MAX_LEVELS = SAH_DEPTH + 34;
constexpr int BIN_WORDS = 3 * 7 * SAH_BINS;   // per node: [axis][count, lo x y z, hi x y z][bin]
constexpr int32_t BY_COUNT = -1;              // a decision: no split found

// A member's bin on an axis of extent > 0.
SAH_FN int bin_of(double c, double lo, double hi) {
    const double t = (c - lo) / (hi - lo);    // in [0, 1]
    const double q = fmin(fmax(floor(t * (double)SAH_BINS), 0.0), (double)(SAH_BINS - 1));
    return (int)q;
}

// The best split of one axis: cnt(b) and box(b) of bin b (box_empty() where cnt is 0).  Returns the
// cost (+inf: none) and sets *split.
template <class CntAt, class BoxAt>
SAH_FN double sweep_axis(const CntAt& cnt, const BoxAt& box, int* split) {
    float la[SAH_BINS];
    int lc[SAH_BINS];
    Box acc = mptrefit::box_empty();
    int ac = 0;
    for (int b = 0; b < SAH_BINS; b++) {
        const int c = cnt(b);
        if (c > 0) mptrefit::box_grow(acc, box(b));
        ac += c;
        la[b] = ac > 0 ? mptlbvh::box_area(acc) : 0.0f;
        lc[b] = ac;
    }
    double best = INFINITY;
    *split = 0;
    acc = mptrefit::box_empty();
    ac = 0;
    for (int s = SAH_BINS - 1; s > 0; s--) {
        const int c = cnt(s);
        if (c > 0) mptrefit::box_grow(acc, box(s));
        ac += c;
        if (lc[s - 1] == 0 || ac == 0) continue;
        double cost = (double)la[s - 1] * (double)lc[s - 1] + (double)mptlbvh::box_area(acc) * (double)ac;
        if (!(cost == cost)) cost = INFINITY;
        if (cost < best) { best = cost; *split = s; }
    }
    return best;
}

// The decision of a node from its three axes' sweeps (cost[a] = +inf: no split on a): axis << 8 | s,
// or BY_COUNT.
SAH_FN int32_t decide(const double cost[3], const int split[3]) {
    double best = INFINITY;
    int32_t d = BY_COUNT;
    for (int a = 0; a < 3; a++)
        if (cost[a] < best) { best = cost[a]; d = (int32_t)((a << 8) | split[a]); }
    return d;
}

// Whether the member at offset k of a node of `count` positions goes left; box: its pbox (6 floats),
// cb: the node's centre bounds (lo 3, hi 3).
SAH_FN bool goes_left(int32_t decision, const float* box, const double* cb, int k, int count) {
    if (decision == BY_COUNT) return k < count / 2;
    const int a = decision >> 8, s = decision & 0xff;
    return bin_of(mptlbvh::centre(box[a], box[3 + a]), cb[a], cb[3 + a]) < s;
}

}  // namespace mptsah

namespace mpt {
// The host loop: the SAH tree over n >= 2 sorted positions (pbox per list position, order: sorted
// position -> list position) into left / right / first / last / nbox (n - 1 nodes) and order_out;
// returns the root's reference and sets *levels (optional) to the number of levels it took.
int32_t sah_tree_host(int n, const float* pbox, const uint32_t* order, int sah_depth, int32_t* left, int32_t* right,
                      int32_t* first, int32_t* last, float* nbox, uint32_t* order_out, int* levels);
// MPT_SAH_DEPTH (a test hook, read at the call): a lower SAH_DEPTH.
int sah_depth_from_env();
}  // namespace mpt

#undef SAH_FN
#endif
