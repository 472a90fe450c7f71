// sah.hip -- the binary tree of the rebuild's binned-SAH mode (mpt_rebuild_bvh_mode, MPT_BUILD_SAH)
// for gfx950, and the host loop of the same definition (sah.h; DESIGN.md §2 "Rebuilds").
//
// The build is level synchronous: level d holds the nodes of binary depth d with more than LEAF_MAX
// positions as a list in position order (first, last, the parent's slot), and every sorted
// position knows its node's index in that list (-1: its node is finished).  Per level:
//   nodes of more than `tail` positions (the grid path)
//     k_sah_bounds_big  one thread per position: B and CB of its node.  A workgroup that lies inside
//                       one node reduces in LDS first; the result is combined with atomic max on an
//                       order-preserving integer encoding (mins are stored complemented), into the
//                       slot first / tail -- two such nodes never share one
//     k_sah_bins_big    one thread per position: its three bins; counts by atomic add, bin boxes by
//                       the same atomic max; a workgroup inside one node privatises the bins in LDS
//                       (planes of SAH_BINS words: a wave's lanes spread over the banks by bin)
//   all nodes
//     k_sah_node        one wave per node.  At most `tail` positions: B and CB by wave reduction, the
//                       bins by atomics in LDS.  More: the wave fetches what the grid path left.
//                       Then lanes 0 to 2 sweep one axis each (sah.h) and lane 0 decides
//     k_sah_flags       one thread per position: whether it goes left (scan_u64 of lbvh.hip then
//                       numbers the left-goers in position order)
//     k_sah_plan        one thread per node: where it splits, hence its id; its range and box; its
//                       reference into its parent; how many children go on (scanned in node order)
//     k_sah_scatter     one thread per position: the stable partition, the new node index
//     k_sah_children    the next level's list; a child of 2 or 3 positions is finished: its box
//   and one readback: the number of nodes of the next level, and how many of them take the grid path.
// MPT_SAH_TAIL=0 (read at the call) sends every node down the grid path: the same bytes.
// No kernel waits on, or depends on seeing, what another workgroup writes in the same launch;
// positions and node order come from scans; atomics combine by max or integer add only; there is
// no floating-point sum across lanes.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "sah.h"

namespace mpt {

namespace {

using namespace mptsah;
using mptlbvh::centre;
using mptlbvh::LEAF_MAX;

constexpr int BLK = 256;
constexpr int WAVE = 64;

// floats and doubles as unsigned words that order as the values do
__host__ __device__ inline uint32_t enc32(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__host__ __device__ inline float dec32(uint32_t e) {
    const uint32_t u = e ^ ((e >> 31) ? 0x80000000u : 0xffffffffu);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__host__ __device__ inline uint64_t enc64(double f) {
    uint64_t u;
    memcpy(&u, &f, 8);
    return u ^ ((u >> 63) ? ~0ull : (1ull << 63));
}
__host__ __device__ inline double dec64(uint64_t e) {
    const uint64_t u = e ^ ((e >> 63) ? (1ull << 63) : ~0ull);
    double f;
    memcpy(&f, &u, 8);
    return f;
}

struct NodeList {
    int32_t* first;
    int32_t* last;
    int32_t* pslot;          // 2 * parent id + side, -1: the root
};

// bins of one node as written by the atomics: counts, complemented encoded mins, encoded maxes
struct BinCnt {
    const uint32_t* w;       // the axis' 7 planes
    __host__ __device__ int operator()(int b) const { return (int)w[b]; }
};
struct BinBox {
    const uint32_t* w;
    __host__ __device__ Box operator()(int b) const {
        Box x;
        for (int k = 0; k < 3; k++) { x.lo[k] = dec32(~w[(1 + k) * SAH_BINS + b]); x.hi[k] = dec32(w[(4 + k) * SAH_BINS + b]); }
        return x;
    }
};

__device__ inline void bin_add(uint32_t* bins, int axis, int b, const float* box) {
    uint32_t* w = bins + axis * 7 * SAH_BINS + b;
    atomicAdd(w, 1u);
    for (int k = 0; k < 3; k++) {
        atomicMax(w + (1 + k) * SAH_BINS, ~enc32(box[k]));
        atomicMax(w + (4 + k) * SAH_BINS, enc32(box[3 + k]));
    }
}

__device__ inline void load_box(const float* __restrict__ pbox, const uint32_t* __restrict__ ord, int n, int p, float box[6]) {
    const uint32_t li = ord[p] < (uint32_t)n ? ord[p] : 0u;
    for (int k = 0; k < 6; k++) box[k] = pbox[6 * (size_t)li + k];
}

__device__ inline int big_slot(int first, int tail) { return tail > 0 ? first / tail : first; }

// Whether the whole workgroup lies in one grid-path node (mine: this thread's node index or -1).
__device__ inline bool block_uniform(int mine) {
    __shared__ int s_idx, s_uni;
    if (threadIdx.x == 0) { s_idx = mine >= 0 ? mine : -2; s_uni = 1; }
    __syncthreads();
    if (mine != s_idx) s_uni = 0;
    __syncthreads();
    return s_uni != 0;
}

__global__ void __launch_bounds__(BLK) k_sah_bounds_big(int n, int tail, const int32_t* __restrict__ nid, NodeList L,
                                                        const uint32_t* __restrict__ ord, const float* __restrict__ pbox,
                                                        uint32_t* __restrict__ gB, unsigned long long* __restrict__ gCB) {
    __shared__ float sf[6][BLK];
    __shared__ double sd[6][BLK];
    const int t = (int)threadIdx.x;
    const int p = (int)(blockIdx.x * BLK) + t;
    int idx = p < n ? nid[p] : -1, slot = 0;
    if (idx >= 0) {
        const int f = L.first[idx], cnt = L.last[idx] - f + 1;
        if (cnt > tail) slot = big_slot(f, tail);
        else idx = -1;
    }
    float box[6] = {0, 0, 0, 0, 0, 0};
    double c[3] = {0, 0, 0};
    if (idx >= 0) {
        load_box(pbox, ord, n, p, box);
        for (int a = 0; a < 3; a++) c[a] = centre(box[a], box[3 + a]);
    }
    if (block_uniform(idx)) {
        for (int k = 0; k < 6; k++) { sf[k][t] = box[k]; sd[k][t] = c[k % 3]; }
        __syncthreads();
        for (int o = BLK / 2; o > 0; o >>= 1) {
            if (t < o)
                for (int k = 0; k < 3; k++) {
                    sf[k][t] = fminf(sf[k][t], sf[k][t + o]);
                    sf[3 + k][t] = fmaxf(sf[3 + k][t], sf[3 + k][t + o]);
                    sd[k][t] = fmin(sd[k][t], sd[k][t + o]);
                    sd[3 + k][t] = fmax(sd[3 + k][t], sd[3 + k][t + o]);
                }
            __syncthreads();
        }
        if (t < 6) atomicMax(&gB[6 * (size_t)slot + t], t < 3 ? ~enc32(sf[t][0]) : enc32(sf[t][0]));
        else if (t < 12) atomicMax(&gCB[6 * (size_t)slot + t - 6], (unsigned long long)(t < 9 ? ~enc64(sd[t - 6][0]) : enc64(sd[t - 6][0])));
        return;
    }
    if (idx < 0) return;
    for (int k = 0; k < 3; k++) {
        atomicMax(&gB[6 * (size_t)slot + k], ~enc32(box[k]));
        atomicMax(&gB[6 * (size_t)slot + 3 + k], enc32(box[3 + k]));
        atomicMax(&gCB[6 * (size_t)slot + k], (unsigned long long)~enc64(c[k]));
        atomicMax(&gCB[6 * (size_t)slot + 3 + k], (unsigned long long)enc64(c[k]));
    }
}

__global__ void __launch_bounds__(BLK) k_sah_bins_big(int n, int tail, const int32_t* __restrict__ nid, NodeList L,
                                                      const uint32_t* __restrict__ ord, const float* __restrict__ pbox,
                                                      const unsigned long long* __restrict__ gCB, uint32_t* __restrict__ gbins) {
    __shared__ uint32_t sbins[BIN_WORDS];
    const int t = (int)threadIdx.x;
    const int p = (int)(blockIdx.x * BLK) + t;
    int idx = p < n ? nid[p] : -1, slot = 0;
    if (idx >= 0) {
        const int f = L.first[idx], cnt = L.last[idx] - f + 1;
        if (cnt > tail && cnt > LEAF_MAX) slot = big_slot(f, tail);
        else idx = -1;
    }
    const bool uni = block_uniform(idx);
    if (uni) {
        for (int w = t; w < BIN_WORDS; w += BLK) sbins[w] = 0u;
        __syncthreads();
    }
    if (idx >= 0) {
        float box[6];
        load_box(pbox, ord, n, p, box);
        uint32_t* bins = uni ? sbins : gbins + (size_t)slot * BIN_WORDS;
        for (int a = 0; a < 3; a++) {
            const double lo = dec64(~gCB[6 * (size_t)slot + a]), hi = dec64(gCB[6 * (size_t)slot + 3 + a]);
            if (!(hi - lo > 0.0)) continue;
            bin_add(bins, a, bin_of(centre(box[a], box[3 + a]), lo, hi), box);
        }
    }
    if (!uni) return;
    __syncthreads();
    uint32_t* g = gbins + (size_t)slot * BIN_WORDS;      // (uniform: every thread has the slot)
    for (int w = t; w < BIN_WORDS; w += BLK) {
        const uint32_t v = sbins[w];
        if (v == 0u) continue;
        if ((w / SAH_BINS) % 7 == 0) atomicAdd(&g[w], v);
        else atomicMax(&g[w], v);
    }
}

// One wave per node of the level.  At most `tail` positions: B, CB and the bins are the wave's own
// work.  More: the grid path left them in global memory, and the wave fetches them.  Then the sweep.
__global__ void __launch_bounds__(WAVE) k_sah_node(int n, int tail, int binning, NodeList L, const uint32_t* __restrict__ ord,
                                                   const float* __restrict__ pbox, const uint32_t* __restrict__ gB,
                                                   const unsigned long long* __restrict__ gCB, const uint32_t* __restrict__ gbins,
                                                   int32_t* __restrict__ dec, float* __restrict__ nB, double* __restrict__ nCB) {
    __shared__ uint32_t sbins[BIN_WORDS];
    __shared__ double scost[3];
    __shared__ int ssplit[3];
    const int idx = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int f = L.first[idx], cnt = L.last[idx] - f + 1;
    if (cnt < 1 || f < 0 || f > n - cnt) return;                      // (uniform in the wave; never by sah.h)
    const bool big = cnt > tail;
    const size_t slot = (size_t)big_slot(f, tail);
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    double cb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (big) {
        for (int k = 0; k < 3; k++) {
            b[k] = dec32(~gB[6 * slot + k]);
            b[3 + k] = dec32(gB[6 * slot + 3 + k]);
            cb[k] = dec64(~gCB[6 * slot + k]);
            cb[3 + k] = dec64(gCB[6 * slot + 3 + k]);
        }
    } else {
        for (int k = lane; k < cnt; k += WAVE) {
            float box[6];
            load_box(pbox, ord, n, f + k, box);
            for (int a = 0; a < 3; a++) {
                const double c = centre(box[a], box[3 + a]);
                b[a] = fminf(b[a], box[a]);
                b[3 + a] = fmaxf(b[3 + a], box[3 + a]);
                cb[a] = fmin(cb[a], c);
                cb[3 + a] = fmax(cb[3 + a], c);
            }
        }
        for (int o = WAVE / 2; o > 0; o >>= 1)
            for (int a = 0; a < 3; a++) {
                b[a] = fminf(b[a], __shfl_xor(b[a], o, WAVE));
                b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], o, WAVE));
                cb[a] = fmin(cb[a], __shfl_xor(cb[a], o, WAVE));
                cb[3 + a] = fmax(cb[3 + a], __shfl_xor(cb[3 + a], o, WAVE));
            }
    }
    if (lane < 6) { nB[6 * (size_t)idx + lane] = b[lane]; nCB[6 * (size_t)idx + lane] = cb[lane]; }
    if (!binning || cnt <= LEAF_MAX) {
        if (lane == 0) dec[idx] = BY_COUNT;
        return;
    }
    if (big) {
        for (int w = lane; w < BIN_WORDS; w += WAVE) sbins[w] = gbins[slot * BIN_WORDS + w];
    } else {
        for (int w = lane; w < BIN_WORDS; w += WAVE) sbins[w] = 0u;
        __syncthreads();
        for (int k = lane; k < cnt; k += WAVE) {
            float box[6];
            load_box(pbox, ord, n, f + k, box);
            for (int a = 0; a < 3; a++) {
                if (!(cb[3 + a] - cb[a] > 0.0)) continue;
                bin_add(sbins, a, bin_of(centre(box[a], box[3 + a]), cb[a], cb[3 + a]), box);
            }
        }
    }
    __syncthreads();
    if (lane < 3) {
        double cost = INFINITY;
        int split = 0;
        if (cb[3 + lane] - cb[lane] > 0.0) {
            const uint32_t* w = sbins + lane * 7 * SAH_BINS;
            cost = sweep_axis(BinCnt{w}, BinBox{w}, &split);
        }
        scost[lane] = cost;
        ssplit[lane] = split;
    }
    __syncthreads();
    if (lane == 0) {
        const double cost[3] = {scost[0], scost[1], scost[2]};
        const int split[3] = {ssplit[0], ssplit[1], ssplit[2]};
        dec[idx] = decide(cost, split);
    }
}

// words[0 .. n]: 1 where the position goes left; words[n] = 0 so that the scan holds the total.
__global__ void __launch_bounds__(BLK) k_sah_flags(int n, const int32_t* __restrict__ nid, NodeList L, const int32_t* __restrict__ dec,
                                                   const double* __restrict__ nCB, const uint32_t* __restrict__ ord,
                                                   const float* __restrict__ pbox, uint64_t* __restrict__ words) {
    const int p = (int)(blockIdx.x * BLK + threadIdx.x);
    if (p > n) return;
    uint64_t w = 0;
    const int idx = p < n ? nid[p] : -1;
    if (idx >= 0) {
        const int f = L.first[idx], cnt = L.last[idx] - f + 1;
        if (cnt > LEAF_MAX) {
            float box[6];
            load_box(pbox, ord, n, p, box);
            double cb[6];
            for (int k = 0; k < 6; k++) cb[k] = nCB[6 * (size_t)idx + k];
            w = goes_left(dec[idx], box, cb, p - f, cnt) ? 1ull : 0ull;
        }
    }
    words[p] = w;
}

// E: the exclusive scan of k_sah_flags' words.  cw[idx]: (children that take the grid path) << 32 |
// (children of more than LEAF_MAX positions: the next level's list).  A child of 2 or 3 positions is
// finished here but for its box (k_sah_children, once the new order stands); one position is a leaf.  err: set when a count contradicts sah.h (never by it).
__global__ void __launch_bounds__(BLK) k_sah_plan(int m, int n, int tail, NodeList L, const uint64_t* __restrict__ E,
                                                  const float* __restrict__ nB, int32_t* __restrict__ left,
                                                  int32_t* __restrict__ right, int32_t* __restrict__ first,
                                                  int32_t* __restrict__ last, float* __restrict__ nbox, int32_t* __restrict__ rootref,
                                                  int32_t* __restrict__ nmid, uint64_t* __restrict__ cw, int32_t* __restrict__ err) {
    const int idx = (int)(blockIdx.x * BLK + threadIdx.x);
    if (idx >= m) return;
    cw[idx] = 0;
    nmid[idx] = 0;
    const int f = L.first[idx], l = L.last[idx], cnt = l - f + 1, ps = L.pslot[idx];
    if (f < 0 || l >= n || cnt <= LEAF_MAX || ps < -1 || (ps >> 1) >= n - 1) { *err = 1; return; }
    const int nl = (int)(E[l + 1] - E[f]);
    if (nl < 1 || nl > cnt - 1) { *err = 1; return; }
    const int mid = f + nl, nr = cnt - nl;
    const int32_t id = mid - 1;
    nmid[idx] = mid;
    if (nl <= LEAF_MAX) {
        left[id] = nl == 1 ? ~f : f;
        if (nl > 1) { first[f] = f; last[f] = mid - 1; }
    }
    if (nr <= LEAF_MAX) {
        right[id] = nr == 1 ? ~mid : mid;
        if (nr > 1) { first[mid] = mid; last[mid] = l; }
    }
    cw[idx] = ((uint64_t)((nl > tail && nl > LEAF_MAX) + (nr > tail && nr > LEAF_MAX)) << 32) |
              (uint64_t)((nl > LEAF_MAX) + (nr > LEAF_MAX));
    first[id] = f;
    last[id] = l;
    for (int k = 0; k < 6; k++) nbox[6 * (size_t)id + k] = nB[6 * (size_t)idx + k];
    if (ps < 0) *rootref = id;
    else (ps & 1 ? right : left)[ps >> 1] = id;
}

// cw: scanned; ord: the new order.  The next level's list, in position order, and the boxes of the
// children of 2 or 3 positions.
__global__ void __launch_bounds__(BLK) k_sah_children(int m, int n, int cap, NodeList L, const int32_t* __restrict__ nmid,
                                                      const uint64_t* __restrict__ cw, const uint32_t* __restrict__ ord,
                                                      const float* __restrict__ pbox, float* __restrict__ nbox, NodeList N) {
    const int idx = (int)(blockIdx.x * BLK + threadIdx.x);
    if (idx >= m) return;
    const int mid = nmid[idx];
    if (mid <= 0) return;
    const int l = L.last[idx];
    const int cf[2] = {L.first[idx], mid}, cl[2] = {mid - 1, l};
    uint32_t at = (uint32_t)cw[idx];
    for (int side = 0; side < 2; side++) {
        const int c = cl[side] - cf[side] + 1;
        if (c > LEAF_MAX) {
            if (at < (uint32_t)cap) { N.first[at] = cf[side]; N.last[at] = cl[side]; N.pslot[at] = 2 * (mid - 1) + side; }
            at++;
        } else if (c > 1 && cf[side] >= 0 && cl[side] < n) {          // node cf[side]: its id is its first position
            Box b = mptrefit::box_empty();
            for (int k = 0; k < c; k++) {
                float box[6];
                load_box(pbox, ord, n, cf[side] + k, box);
                for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], box[a]); b.hi[a] = fmaxf(b.hi[a], box[3 + a]); }
            }
            for (int a = 0; a < 3; a++) { nbox[6 * (size_t)cf[side] + a] = b.lo[a]; nbox[6 * (size_t)cf[side] + 3 + a] = b.hi[a]; }
        }
    }
}

__global__ void __launch_bounds__(BLK) k_sah_scatter(int n, const int32_t* __restrict__ nid, NodeList L,
                                                     const int32_t* __restrict__ nmid, const uint64_t* __restrict__ cw,
                                                     const uint64_t* __restrict__ E, const uint32_t* __restrict__ ord,
                                                     uint32_t* __restrict__ ord_out, int32_t* __restrict__ nid_out) {
    const int p = (int)(blockIdx.x * BLK + threadIdx.x);
    if (p >= n) return;
    const int idx = nid[p];
    const int mid = idx >= 0 ? nmid[idx] : 0;
    if (mid <= 0) {                                    // a finished node: the position stays
        ord_out[p] = ord[p];
        nid_out[p] = -1;
        return;
    }
    const int f = L.first[idx], l = L.last[idx];
    const bool goes = E[p + 1] != E[p];
    const int rank = (int)(E[p] - E[f]);               // left-goers of the node before p
    const uint32_t base = (uint32_t)cw[idx];
    int q, ccnt;
    uint32_t cidx;
    if (goes) { q = f + rank; ccnt = mid - f; cidx = base; }
    else { q = mid + (p - f - rank); ccnt = l - mid + 1; cidx = base + (mid - f > LEAF_MAX ? 1u : 0u); }
    if (q < f || q > l) return;                        // (never by sah.h)
    ord_out[q] = ord[p];
    nid_out[q] = ccnt > LEAF_MAX ? (int32_t)cidx : -1;
}

inline unsigned blocks(int n) { return (unsigned)((n + BLK - 1) / BLK); }

}  // namespace

int sah_depth_from_env() {
    int d = SAH_DEPTH;
    if (const char* e = std::getenv("MPT_SAH_DEPTH")) d = std::max(0, std::min(SAH_DEPTH, std::atoi(e)));
    return d;
}

int sah_tail_from_env() {
    if (const char* e = std::getenv("MPT_SAH_TAIL")) return std::atoi(e) == 0 ? 0 : SAH_TAIL;
    return SAH_TAIL;
}

#define SA(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t sah_tree_device(int n, const float* pbox, uint32_t* const ord[2], int cur, int32_t* left, int32_t* right, int32_t* first,
                           int32_t* last, float* nbox, const SahScratch& B, hipStream_t st, int32_t* root, int* order_at,
                           SahStats* stats) {
    if (n <= LEAF_MAX) return hipErrorInvalidValue;
    const int tail = B.tail, sah_depth = sah_depth_from_env();
    NodeList L[2] = {{B.lfirst[0], B.llast[0], B.lpslot[0]}, {B.lfirst[1], B.llast[1], B.lpslot[1]}};
    const int32_t root_node[3] = {0, n - 1, -1};
    SA(hipMemcpyAsync(L[0].first, &root_node[0], sizeof(int32_t), hipMemcpyHostToDevice, st));
    SA(hipMemcpyAsync(L[0].last, &root_node[1], sizeof(int32_t), hipMemcpyHostToDevice, st));
    SA(hipMemcpyAsync(L[0].pslot, &root_node[2], sizeof(int32_t), hipMemcpyHostToDevice, st));
    SA(hipMemsetAsync(B.nid[0], 0, (size_t)n * sizeof(int32_t), st));
    SA(hipMemsetAsync(B.report, 0, 2 * sizeof(int32_t), st));          // the root's reference, the error flag
    SA(hipMemsetAsync(left, 0, (size_t)(n - 1) * sizeof(int32_t), st));
    SA(hipMemsetAsync(right, 0, (size_t)(n - 1) * sizeof(int32_t), st));
    SA(hipMemsetAsync(first, 0, (size_t)(n - 1) * sizeof(int32_t), st));
    SA(hipMemsetAsync(last, 0, (size_t)(n - 1) * sizeof(int32_t), st));
    int m = 1, n_big = n > tail ? 1 : 0, level = 0, d = 0, grid_levels = 0;
    while (m > 0) {
        if (level >= SAH_MAX_LEVELS) return hipErrorUnknown;
        const int binning = level < sah_depth ? 1 : 0;
        if (n_big > 0) {
            SA(hipMemsetAsync(B.gB, 0, 6 * (size_t)B.big_slots * sizeof(uint32_t), st));
            SA(hipMemsetAsync(B.gCB, 0, 6 * (size_t)B.big_slots * sizeof(uint64_t), st));
            hipLaunchKernelGGL(k_sah_bounds_big, dim3(blocks(n)), dim3(BLK), 0, st, n, tail, B.nid[d], L[d], ord[cur], pbox, B.gB,
                               (unsigned long long*)B.gCB);
            if (binning) {
                SA(hipMemsetAsync(B.gbins, 0, (size_t)BIN_WORDS * B.big_slots * sizeof(uint32_t), st));
                hipLaunchKernelGGL(k_sah_bins_big, dim3(blocks(n)), dim3(BLK), 0, st, n, tail, B.nid[d], L[d], ord[cur], pbox,
                                   (const unsigned long long*)B.gCB, B.gbins);
            }
            grid_levels++;
        }
        hipLaunchKernelGGL(k_sah_node, dim3((unsigned)m), dim3(WAVE), 0, st, n, tail, binning, L[d], ord[cur], pbox, B.gB,
                           (const unsigned long long*)B.gCB, B.gbins, B.dec, B.nB, B.nCB);
        hipLaunchKernelGGL(k_sah_flags, dim3(blocks(n + 1)), dim3(BLK), 0, st, n, B.nid[d], L[d], B.dec, B.nCB, ord[cur], pbox, B.words);
        SA(scan_u64(B.words, n + 1, B.partial, st));
        hipLaunchKernelGGL(k_sah_plan, dim3(blocks(m)), dim3(BLK), 0, st, m, n, tail, L[d], B.words, B.nB, left, right, first, last,
                           nbox, B.report, B.nmid, B.cw, B.report + 1);
        SA(scan_u64(B.cw, m, B.partial, st));
        uint64_t total = 0;
        SA(hipMemcpyAsync(&total, B.partial + blocks(m), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SA(hipStreamSynchronize(st));
        const int next_m = (int)(uint32_t)total, next_big = (int)(total >> 32);
        // (checked before the next list is written)
        if (next_m < 0 || next_m > B.list_cap || next_m > 2 * m || next_big > next_m) return hipErrorUnknown;
        hipLaunchKernelGGL(k_sah_scatter, dim3(blocks(n)), dim3(BLK), 0, st, n, B.nid[d], L[d], B.nmid, B.cw, B.words, ord[cur],
                           ord[cur ^ 1], B.nid[d ^ 1]);
        hipLaunchKernelGGL(k_sah_children, dim3(blocks(m)), dim3(BLK), 0, st, m, n, B.list_cap, L[d], B.nmid, B.cw, ord[cur ^ 1], pbox,
                           nbox, L[d ^ 1]);
        SA(hipGetLastError());
        m = next_m;
        n_big = next_big;
        d ^= 1;
        cur ^= 1;
        level++;
    }
    int32_t report[2] = {0, 0};
    SA(hipMemcpyAsync(report, B.report, sizeof(report), hipMemcpyDeviceToHost, st));
    SA(hipStreamSynchronize(st));
    if (report[1] != 0 || report[0] < 0 || report[0] >= n - 1) return hipErrorUnknown;
    *root = report[0];
    *order_at = cur;
    if (stats) { stats->levels = level; stats->grid_levels = grid_levels; }
    return hipSuccess;
}
#undef SA

int32_t sah_tree_host(int n, const float* pbox, const uint32_t* order, int sah_depth, int32_t* left, int32_t* right, int32_t* first,
                      int32_t* last, float* nbox, uint32_t* order_out, int* levels) {
    struct Nd { int f, l, ps; };
    std::vector<uint32_t> ord(order, order + n), nxt(n);
    std::vector<Nd> cur{{0, n - 1, -1}}, next;
    std::vector<uint8_t> goes;
    int32_t root = mptlbvh::NO_REF;
    int level = 0;
    while (!cur.empty()) {
        if (level >= SAH_MAX_LEVELS) return mptlbvh::NO_REF;
        nxt = ord;                                     // finished nodes: the positions stay
        next.clear();
        for (const Nd& nd : cur) {
            const int f = nd.f, cnt = nd.l - nd.f + 1;
            Box b = mptrefit::box_empty();
            double cb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
            for (int k = 0; k < cnt; k++) {
                const float* box = pbox + 6 * (size_t)ord[f + k];
                for (int a = 0; a < 3; a++) {
                    const double c = centre(box[a], box[3 + a]);
                    b.lo[a] = fminf(b.lo[a], box[a]);
                    b.hi[a] = fmaxf(b.hi[a], box[3 + a]);
                    cb[a] = fmin(cb[a], c);
                    cb[3 + a] = fmax(cb[3 + a], c);
                }
            }
            int32_t id = f;
            if (cnt > LEAF_MAX) {
                int32_t dcs = BY_COUNT;
                if (level < sah_depth) {
                    double cost[3] = {INFINITY, INFINITY, INFINITY};
                    int split[3] = {0, 0, 0};
                    for (int a = 0; a < 3; a++) {
                        if (!(cb[3 + a] - cb[a] > 0.0)) continue;
                        int bc[SAH_BINS] = {0};
                        Box bb[SAH_BINS];
                        for (int k = 0; k < SAH_BINS; k++) bb[k] = mptrefit::box_empty();
                        for (int k = 0; k < cnt; k++) {
                            const float* box = pbox + 6 * (size_t)ord[f + k];
                            const int bi = bin_of(centre(box[a], box[3 + a]), cb[a], cb[3 + a]);
                            Box x;
                            for (int j = 0; j < 3; j++) { x.lo[j] = box[j]; x.hi[j] = box[3 + j]; }
                            mptrefit::box_grow(bb[bi], x);
                            bc[bi]++;
                        }
                        cost[a] = sweep_axis([&](int k) { return bc[k]; }, [&](int k) { return bb[k]; }, &split[a]);
                    }
                    dcs = decide(cost, split);
                }
                goes.assign(cnt, 0);
                int nl = 0;
                for (int k = 0; k < cnt; k++) {
                    goes[k] = goes_left(dcs, pbox + 6 * (size_t)ord[f + k], cb, k, cnt) ? 1 : 0;
                    nl += goes[k];
                }
                if (nl < 1 || nl > cnt - 1) return mptlbvh::NO_REF;            // (never by sah.h)
                const int mid = f + nl;
                int at[2] = {mid, f};                  // where the next right-goer / left-goer lands
                for (int k = 0; k < cnt; k++) nxt[at[goes[k]]++] = ord[f + k];
                id = mid - 1;
                if (nl == 1) left[id] = ~f;
                else next.push_back({f, mid - 1, 2 * id});
                if (cnt - nl == 1) right[id] = ~mid;
                else next.push_back({mid, nd.l, 2 * id + 1});
            }
            first[id] = nd.f;
            last[id] = nd.l;
            for (int a = 0; a < 3; a++) { nbox[6 * (size_t)id + a] = b.lo[a]; nbox[6 * (size_t)id + 3 + a] = b.hi[a]; }
            if (nd.ps < 0) root = id;
            else (nd.ps & 1 ? right : left)[nd.ps >> 1] = id;
        }
        ord.swap(nxt);
        cur.swap(next);
        level++;
    }
    for (int p = 0; p < n; p++) order_out[p] = ord[p];
    if (levels) *levels = level;
    return root;
}

}  // namespace mpt
