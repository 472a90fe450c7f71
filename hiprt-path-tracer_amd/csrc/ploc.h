// ploc.h -- the binary tree of the rebuild's quality mode (MPT_BUILD_PLOC): parallel locally-ordered
// clustering (Meister & Bittner 2018) over the Morton order of lbvh.h, shared verbatim by the
// kernels (ploc.hip) and the host loop (ploc_tree_host) and compiled with -ffp-contract=off on both
// sides (DESIGN.md §2 "Rebuilds").  Boxes, bounds, keys and order are lbvh.h's; what comes out is
// what mptlbvh::Tree holds, so that collapse_node and emit_node run on it unmodified, started at
// the root n - 2 instead of 0.
//
//   clusters   an ordered list of m entries (reference, box, triangle count); at first m = n and
//              entry p is the leaf ~p with the box pbox[order[p]] and count 1
//   iteration  (while m > 1) position i looks at the candidates j != i within PLOC_RADIUS positions;
//              d(i, j) is lbvh.h's fp32 box_area of the union, a value that is not a number counts
//              as +inf (and -0 as +0); key(i, j) = bits(d) << 32 | (i ^ j); nn(i) is the candidate
//              of least key.  The key is symmetric in (i, j), and unique over j for a fixed i
//              because i ^ j is.  A pair i < j merges iff nn(i) = j and nn(j) = i.
//   progress   Take a pair (i, j) whose key is the least over all pairs within the radius.  Every
//              candidate j' of i has key(i, j') >= key(i, j), and j' != j makes it differ, so
//              nn(i) = j; by symmetry nn(j) = i.  Every iteration therefore merges at least one
//              pair, and there are at most n - 1 iterations.  Equal boxes give equal d, the key
//              falls to i ^ j, and the pairs are (2 k, 2 k + 1): they halve per iteration.
//   merge      the merging pairs of an iteration are numbered in position order by a scan; pair k
//              becomes the internal node next_id + k with left = entry i's reference, right = entry
//              j's, box = the union, count = the sum.  The node takes position i, position j
//              disappears, survivors keep their order; then next_id += merges.  Children have
//              smaller ids than their parent; for n >= 2 the root is node n - 2.
//   leaf order a subtree does not cover a contiguous sorted range, and the collapse needs one:
//              first(root) = 0, first(left) = first(node), first(right) = first(node) + count(left),
//              last = first + count - 1, assigned parents before children.  The leaf that sat at
//              sorted position p moves to first(leaf): order'[first] = order[p], and the reference
//              ~p in left / right becomes ~first.
#ifndef MPT_PLOC_H
#define MPT_PLOC_H

#include "lbvh.h"

#if defined(__HIPCC__)
#define PLOC_FN __host__ __device__ static inline
#else
#define PLOC_FN static inline
#endif

namespace mptploc {

using mptrefit::Box;

constexpr int PLOC_RADIUS = 8;
constexpr int PLOC_TAIL = 1024;               // at most this many clusters: one workgroup finishes the build
constexpr int32_t PLAIN = -1;                 // mate(): the position survives unmerged
constexpr int32_t ABSORBED = -2;              // mate(): the position is the second of a merging pair

PLOC_FN Box box_union(const Box& a, const Box& b) {
    Box u = a;
    mptrefit::box_grow(u, b);
    return u;
}

// bits(d): the fp32 area of the union as an unsigned word.  d is never negative, so the words order
// as the values do; not-a-number (inf * 0) counts as +inf, and -0 becomes +0.
PLOC_FN uint32_t dist_bits(const Box& a, const Box& b) {
    float d = mptlbvh::box_area(box_union(a, b));
    if (!(d == d)) d = INFINITY;
    d = d + 0.0f;
    uint32_t u;
    memcpy(&u, &d, 4);
    return u;
}

PLOC_FN uint64_t pair_key(const Box& a, const Box& b, int i, int j) {
    return ((uint64_t)dist_bits(a, b) << 32) | (uint32_t)(i ^ j);
}

// nn(i) among m > 1 positions; at(j): the box of position j.
template <class BoxAt>
PLOC_FN int nearest(const BoxAt& at, int i, int m) {
    const int j0 = i - PLOC_RADIUS < 0 ? 0 : i - PLOC_RADIUS, j1 = i + PLOC_RADIUS > m - 1 ? m - 1 : i + PLOC_RADIUS;
    const Box bi = at(i);
    int best = -1;
    uint64_t bk = 0;
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        const uint64_t k = pair_key(bi, at(j), i, j);
        if (best < 0 || k < bk) { bk = k; best = j; }
    }
    return best;
}

// What becomes of position i: the partner j > i when i heads a merging pair, ABSORBED when i is
// the second of one, PLAIN otherwise.  nn(k): nearest() of position k.
template <class NnAt>
PLOC_FN int32_t mate(const NnAt& nn, int i) {
    const int j = nn(i);
    if (j < 0 || nn(j) != i) return PLAIN;
    return i < j ? (int32_t)j : ABSORBED;
}

// The word whose exclusive scan numbers the merges (high half) and the survivors (low half).
PLOC_FN uint64_t scan_word(int32_t mt) { return mt == ABSORBED ? 0ull : mt == PLAIN ? 1ull : ((1ull << 32) | 1ull); }

// The leaf-order step of internal node `id` whose first is set: its children's firsts, its last,
// its leaf children moved to their new sorted positions.  count: per internal node.
PLOC_FN void place_children(int32_t id, int32_t* left, int32_t* right, int32_t* first, int32_t* last, const int32_t* count,
                            const uint32_t* order, uint32_t* order_out) {
    const int32_t f = first[id];
    int32_t c[2] = {left[id], right[id]};
    int32_t at = f;
    for (int k = 0; k < 2; k++) {
        if (c[k] < 0) {
            order_out[at] = order[~c[k]];
            c[k] = ~at;
            at += 1;
        } else {
            first[c[k]] = at;
            at += count[c[k]];
        }
    }
    left[id] = c[0];
    right[id] = c[1];
    last[id] = at - 1;
}

}  // namespace mptploc

namespace mpt {
// The host loop: the PLOC tree over n >= 2 sorted positions (pbox per list position, order: sorted
// position -> list position) into left / right / first / last / nbox (n - 1 nodes) and order_out;
// returns the number of iterations.
int ploc_tree_host(int n, const float* pbox, const uint32_t* order, int32_t* left, int32_t* right, int32_t* first,
                   int32_t* last, float* nbox, uint32_t* order_out);
}  // namespace mpt

#undef PLOC_FN
#endif
