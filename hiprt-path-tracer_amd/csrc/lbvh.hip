// lbvh.hip -- the BVH8 rebuild of mpt_rebuild_bvh for gfx950, and the host loop of the same
// definition (lbvh.h; DESIGN.md §2 "Rebuilds").
//
//   k_prim_boxes      one thread per list position: the triangle's padded box (refit_tri), the
//                     workgroup's min / max of the box centres; k_bounds_final reduces those
//   k_codes           the 30-bit Morton code per list position, the payload = the position
//   k_sort_hist / k_sort_scatter   a stable LSD radix sort, 8 bits per pass, SORT_TILE keys per
//                     workgroup: digit counts per workgroup, their exclusive scan (digit major),
//                     then the scatter with ranks from wave ballots (stable within the tile)
//   k_scan_*          exclusive scan of 64-bit words: reduce per workgroup, scan of the partial
//                     sums by one workgroup, scan per workgroup -- three launches
//   k_radix_tree      one thread per internal node of Karras' radix tree (MPT_BUILD_PLOC: ploc.hip,
//                     MPT_BUILD_SAH: sah.hip builds the binary tree and its boxes instead; everything
//                     else is shared)
//   k_box_round       one launch per round: a node whose children were finished by an earlier
//                     launch (its stamp is set and smaller than this round's) takes their union
//   k_collapse_count / k_collapse_emit   per breadth-first level: one thread per node chooses its
//                     children and slots, the counts are scanned in node order, the emit writes the
//                     nodes' topology bytes, the next level's list and the records' w lanes
//   k_flag_scatter    the old records' flag lanes into a per-primitive scratch (gathered by the emit;
//                     not run when the caller brings the words: mpt_upload_scene_mode, upload.hip)
// No kernel waits on, or depends on seeing, what another workgroup writes in the same launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lbvh.h"
#include "ploc.h"
#include "sah.h"
#include "mpt.h"
#include "mpt_internal.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mptlbvh;
using mptrefit::Box;

constexpr int BLK = 256;
constexpr int SORT_ROUNDS = SORT_TILE / BLK;

__global__ void __launch_bounds__(BLK) k_prim_boxes(const int32_t* __restrict__ prims, int n, const int32_t* __restrict__ idx,
                                                    const float* __restrict__ pos, float pad, float* __restrict__ pbox,
                                                    double* __restrict__ partial) {
    __shared__ double sh[6][BLK];
    const int t = (int)threadIdx.x;
    const int i = (int)(blockIdx.x * BLK) + t;
    double c[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const int32_t prim = prims ? prims[i] : i;
        float v[3][3];
        for (int k = 0; k < 3; k++) {
            const size_t vi = (size_t)idx[3 * (size_t)prim + k];
            for (int a = 0; a < 3; a++) v[k][a] = pos[3 * vi + a];
        }
        TriRec tr;
        const Box b = mptrefit::refit_tri(v[0], v[1], v[2], pad, tr);
        for (int a = 0; a < 3; a++) {
            pbox[6 * (size_t)i + a] = b.lo[a];
            pbox[6 * (size_t)i + 3 + a] = b.hi[a];
            c[a] = c[3 + a] = centre(b.lo[a], b.hi[a]);
        }
    }
    for (int k = 0; k < 6; k++) sh[k][t] = c[k];
    __syncthreads();
    for (int o = BLK / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < 3; k++) {
                sh[k][t] = fmin(sh[k][t], sh[k][t + o]);
                sh[3 + k][t] = fmax(sh[3 + k][t], sh[3 + k][t + o]);
            }
        __syncthreads();
    }
    if (t < 6) partial[6 * (size_t)blockIdx.x + t] = sh[t][0];
}

__global__ void __launch_bounds__(BLK) k_bounds_final(const double* __restrict__ partial, int nb, double* __restrict__ bounds) {
    __shared__ double sh[6][BLK];
    const int t = (int)threadIdx.x;
    double c[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = t; b < nb; b += BLK)
        for (int k = 0; k < 3; k++) {
            c[k] = fmin(c[k], partial[6 * (size_t)b + k]);
            c[3 + k] = fmax(c[3 + k], partial[6 * (size_t)b + 3 + k]);
        }
    for (int k = 0; k < 6; k++) sh[k][t] = c[k];
    __syncthreads();
    for (int o = BLK / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < 3; k++) {
                sh[k][t] = fmin(sh[k][t], sh[k][t + o]);
                sh[3 + k][t] = fmax(sh[3 + k][t], sh[3 + k][t + o]);
            }
        __syncthreads();
    }
    if (t < 6) bounds[t] = sh[t][0];
}

__global__ void __launch_bounds__(BLK) k_codes(const float* __restrict__ pbox, int n, const double* __restrict__ bounds,
                                               uint32_t* __restrict__ code, uint32_t* __restrict__ pay) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n) return;
    double b[6];
    for (int k = 0; k < 6; k++) b[k] = bounds[k];
    float box[6];
    for (int k = 0; k < 6; k++) box[k] = pbox[6 * (size_t)i + k];
    code[i] = morton_code(box, b);
    pay[i] = (uint32_t)i;
}

// ---- exclusive scan of 64-bit words ---------------------------------------------------
__device__ inline uint64_t block_excl_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
    const int t = (int)threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < BLK; o <<= 1) {
        const uint64_t x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[BLK - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(BLK) k_scan_reduce(const uint64_t* __restrict__ a, int n, uint64_t* __restrict__ partial) {
    __shared__ uint64_t sh[BLK];
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    uint64_t total;
    (void)block_excl_scan(i < n ? a[i] : 0, sh, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: partial[0 .. nb) in place, the sum of all into partial[nb]
__global__ void __launch_bounds__(BLK) k_scan_partials(uint64_t* __restrict__ partial, int nb) {
    __shared__ uint64_t sh[BLK];
    uint64_t carry = 0;
    for (int base = 0; base < nb; base += BLK) {
        const int i = base + (int)threadIdx.x;
        uint64_t total;
        const uint64_t e = block_excl_scan(i < nb ? partial[i] : 0, sh, &total);
        if (i < nb) partial[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) partial[nb] = carry;
}

__global__ void __launch_bounds__(BLK) k_scan_down(uint64_t* __restrict__ a, int n, const uint64_t* __restrict__ partial) {
    __shared__ uint64_t sh[BLK];
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    uint64_t total;
    const uint64_t e = block_excl_scan(i < n ? a[i] : 0, sh, &total);
    if (i < n) a[i] = partial[blockIdx.x] + e;
}

// ---- radix sort -------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) k_sort_hist(const uint32_t* __restrict__ code, int n, int shift, uint64_t* __restrict__ table,
                                                   int nblocks) {
    __shared__ uint32_t hist[256];
    const int t = (int)threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; r++) {
        const int64_t i = base + r * BLK + t;
        if (i < n) atomicAdd(&hist[(code[i] >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    table[(size_t)t * nblocks + blockIdx.x] = hist[t];
}

__global__ void __launch_bounds__(BLK) k_sort_scatter(const uint32_t* __restrict__ code, const uint32_t* __restrict__ pay, int n,
                                                      int shift, const uint64_t* __restrict__ table, int nblocks,
                                                      uint32_t* __restrict__ code_out, uint32_t* __restrict__ pay_out) {
    __shared__ uint32_t run[256];
    __shared__ uint32_t whist[BLK / 64][256];
    const int t = (int)threadIdx.x, w = t >> 6, lane = t & 63;
    run[t] = (uint32_t)table[(size_t)t * nblocks + blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; r++) {
        for (int k = 0; k < BLK / 64; k++) whist[k][t] = 0;
        __syncthreads();
        const int64_t i = base + r * BLK + t;
        const bool valid = i < n;
        const uint32_t c = valid ? code[i] : 0u, p = valid ? pay[i] : 0u;
        const uint32_t digit = (c >> shift) & 0xffu;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot((digit >> b) & 1u);
            peers &= ((digit >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) whist[w][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t at = run[digit] + rank;
            for (int k = 0; k < w; k++) at += whist[k][digit];
            if (at < (uint32_t)n) { code_out[at] = c; pay_out[at] = p; }
        }
        __syncthreads();
        uint32_t add = 0;
        for (int k = 0; k < BLK / 64; k++) add += whist[k][t];
        run[t] += add;
        __syncthreads();
    }
}

// ---- the binary tree --------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) k_radix_tree(const uint32_t* __restrict__ code, const uint32_t* __restrict__ order, int n,
                                                    int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                    int32_t* __restrict__ first, int32_t* __restrict__ last,
                                                    int32_t* __restrict__ stamp) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n - 1) return;
    int32_t l, r, f, e;
    radix_node(code, order, n, i, &l, &r, &f, &e);
    left[i] = l; right[i] = r; first[i] = f; last[i] = e;
    stamp[i] = 0;
}

// round >= 1.  A child counts as finished when its stamp is set and below this round's: written by
// an earlier launch.  A stamp written in this launch reads as 0 or as `round`: unfinished either way.
__global__ void __launch_bounds__(BLK) k_box_round(Tree T, float* __restrict__ nbox, int32_t* __restrict__ stamp, int n_internal,
                                                   int round) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n_internal) return;
    if (stamp[i] != 0) return;
    const int32_t c[2] = {T.left[i], T.right[i]};
    for (int k = 0; k < 2; k++)
        if (c[k] >= 0) {
            const int32_t s = stamp[c[k]];
            if (s == 0 || s >= round) return;
        }
    Box b = ref_box(T, c[0]);
    mptrefit::box_grow(b, ref_box(T, c[1]));
    for (int a = 0; a < 3; a++) { nbox[6 * (size_t)i + a] = b.lo[a]; nbox[6 * (size_t)i + 3 + a] = b.hi[a]; }
    stamp[i] = round;
}

// ---- the collapse -------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) k_collapse_count(Tree T, const int32_t* __restrict__ defs, int n_level,
                                                        int32_t* __restrict__ slots, uint64_t* __restrict__ cnt) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n_level) return;
    int32_t slot[8];
    int n_int, n_rec;
    collapse_node(T, defs[i], slot, &n_int, &n_rec);
    for (int s = 0; s < 8; s++) slots[8 * (size_t)i + s] = slot[s];
    cnt[i] = ((uint64_t)n_int << 32) | (uint32_t)n_rec;
}

// cnt: the exclusive scan of k_collapse_count's words.  Node begin + i; its internal children
// become the nodes next_begin + (scanned n_int) ..., its records start at rec_begin + (scanned n_rec).
__global__ void __launch_bounds__(BLK) k_collapse_emit(Tree T, const int32_t* __restrict__ slots, const uint64_t* __restrict__ cnt,
                                                       int n_level, int begin, int next_begin, int rec_begin,
                                                       const int32_t* __restrict__ prims, const uint32_t* __restrict__ flags,
                                                       Node8* __restrict__ nodes, int32_t* __restrict__ next_defs,
                                                       TriRec* __restrict__ recs) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n_level) return;
    int32_t slot[8];
    for (int s = 0; s < 8; s++) slot[s] = slots[8 * (size_t)i + s];
    const uint32_t e_int = (uint32_t)(cnt[i] >> 32), e_rec = (uint32_t)cnt[i];
    emit_node(T, slot, (uint32_t)next_begin + e_int, (uint32_t)rec_begin + e_rec, prims, flags, nodes + begin + i,
              next_defs + e_int, recs);
}

__global__ void __launch_bounds__(BLK) k_flag_scatter(const TriRec* __restrict__ old, int n_old, int n_prims,
                                                      uint32_t* __restrict__ flags) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n_old) return;
    const float4* rec = (const float4*)(old + i);
    const int32_t prim = __float_as_int(rec[0].w);
    if (prim < 0 || prim >= n_prims) return;
    flags[2 * (size_t)prim] = __float_as_uint(rec[1].w);
    flags[2 * (size_t)prim + 1] = __float_as_uint(rec[2].w);
}

inline unsigned blocks(int n) { return (unsigned)((n + BLK - 1) / BLK); }

struct Scratch {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    template <class T>
    T* get(size_t count) {
        if (err != hipSuccess) return nullptr;
        void* p = nullptr;
        err = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (T*)p;
    }
    ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
};

}  // namespace

// a[0 .. n) -> its exclusive scan; the sum of all is left in partial[ceil(n / BLK)]
hipError_t scan_u64(uint64_t* a, int n, uint64_t* partial, hipStream_t st) {
    const int nb = (n + BLK - 1) / BLK;
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(BLK), 0, st, a, n, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(BLK), 0, st, partial, nb);
    hipLaunchKernelGGL(k_scan_down, dim3((unsigned)nb), dim3(BLK), 0, st, a, n, partial);
    return hipGetLastError();
}

void free_lbvh(LbvhDevice& o) {
    if (o.nodes) (void)hipFree(o.nodes);
    if (o.tris) (void)hipFree(o.tris);
    if (o.nbox) (void)hipFree(o.nbox);
    o.nodes = nullptr; o.tris = nullptr; o.nbox = nullptr;
}

#define LB(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { free_lbvh(out); return e_; } } while (0)

hipError_t build_lbvh_device(const int32_t* d_prims, int n, int n_scene_prims, const int32_t* idx, const float* pos, float pad,
                             const TriRec* old_tris, int n_old, float* tbox, LbvhDevice& out, hipStream_t st, int mode,
                             PlocStats* stats, const uint32_t* ready_flags) {
    out = LbvhDevice{};
    if (n <= 0 || (mode != MPT_BUILD_LBVH && mode != MPT_BUILD_PLOC && mode != MPT_BUILD_SAH)) return hipErrorInvalidValue;
    const bool ploc = mode == MPT_BUILD_PLOC && n > 1;
    const bool sah = mode == MPT_BUILD_SAH && n > LEAF_MAX;   // (up to LEAF_MAX: one leaf slot whatever the tree, the radix tree's path)
    const int cap = n / 2 + 1;                         // nodes: a node without internal children holds >= 4 triangles,
                                                       // one with a single internal child 7 leaf slots (lbvh.h); the
                                                       // argument uses no property of the radix tree: any binary tree
    const int n_int = n - 1;
    const int sort_blocks = (n + SORT_TILE - 1) / SORT_TILE;
    const int table_n = 256 * sort_blocks;
    const int scan_max = std::max(table_n, sah ? n + 1 : ploc ? n : cap);
    Scratch S;
    float* pbox = S.get<float>(6 * (size_t)n);
    double* bpart = S.get<double>(6 * (size_t)blocks(n) + 6);
    uint32_t* code[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)};
    uint32_t* pay[2] = {S.get<uint32_t>(n), S.get<uint32_t>(n)};
    uint64_t* table = S.get<uint64_t>(scan_max);
    uint64_t* partial = S.get<uint64_t>((size_t)blocks(scan_max) + 1);
    int32_t* left = S.get<int32_t>(n_int);
    int32_t* right = S.get<int32_t>(n_int);
    int32_t* first = S.get<int32_t>(n_int);
    int32_t* last = S.get<int32_t>(n_int);
    int32_t* stamp = S.get<int32_t>(n_int);
    float* bbox = S.get<float>(6 * (size_t)n_int);
    int32_t* defs[2] = {S.get<int32_t>(cap), S.get<int32_t>(cap)};
    int32_t* slots = S.get<int32_t>(8 * (size_t)cap);
    uint32_t* scattered = ready_flags ? nullptr : S.get<uint32_t>(2 * (size_t)n_scene_prims);
    const uint32_t* flags = ready_flags ? ready_flags : scattered;
    Node8* nodes = S.get<Node8>(cap);
    PlocScratch PS{};
    if (ploc) {
        for (int k = 0; k < 2; k++) {
            PS.cref[k] = S.get<int32_t>(n);
            PS.ccnt[k] = S.get<int32_t>(n);
            PS.cbox[k] = S.get<float>(6 * (size_t)n);
        }
        PS.mate = S.get<int32_t>(n);
        PS.tail_info = S.get<int32_t>(mptploc::PLOC_TAIL + 2);
        PS.words = table;
        PS.partial = partial;
        PS.count = stamp;
    }
    SahScratch SS{};
    if (sah) {
        SS.tail = sah_tail_from_env();
        SS.big_slots = SS.tail > 0 ? n / SS.tail + 1 : n;
        SS.list_cap = n / 2 + 1;
        for (int k = 0; k < 2; k++) {
            SS.nid[k] = S.get<int32_t>(n);
            SS.lfirst[k] = S.get<int32_t>(SS.list_cap);
            SS.llast[k] = S.get<int32_t>(SS.list_cap);
            SS.lpslot[k] = S.get<int32_t>(SS.list_cap);
        }
        SS.dec = S.get<int32_t>(SS.list_cap);
        SS.nmid = S.get<int32_t>(SS.list_cap);
        SS.nB = S.get<float>(6 * (size_t)SS.list_cap);
        SS.nCB = S.get<double>(6 * (size_t)SS.list_cap);
        SS.cw = S.get<uint64_t>(SS.list_cap);
        SS.words = table;
        SS.partial = partial;
        SS.gB = S.get<uint32_t>(6 * (size_t)SS.big_slots);
        SS.gCB = S.get<uint64_t>(6 * (size_t)SS.big_slots);
        SS.gbins = S.get<uint32_t>((size_t)mptsah::BIN_WORDS * SS.big_slots);
        SS.report = S.get<int32_t>(2);
    }
    LB(S.err);
    LB(hipMalloc(&out.tris, (size_t)n * sizeof(TriRec)));

    // the flag lanes per scene primitive: the caller's words, or those of the old records
    if (scattered) {
        LB(hipMemsetAsync(scattered, 0, 2 * (size_t)n_scene_prims * sizeof(uint32_t), st));
        if (old_tris && n_old > 0)
            hipLaunchKernelGGL(k_flag_scatter, dim3(blocks(n_old)), dim3(BLK), 0, st, old_tris, n_old, n_scene_prims, scattered);
    }
    // keys
    hipLaunchKernelGGL(k_prim_boxes, dim3(blocks(n)), dim3(BLK), 0, st, d_prims, n, idx, pos, pad, pbox, bpart + 6);
    hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(BLK), 0, st, bpart + 6, (int)blocks(n), bpart);
    hipLaunchKernelGGL(k_codes, dim3(blocks(n)), dim3(BLK), 0, st, pbox, n, bpart, code[0], pay[0]);
    LB(hipGetLastError());
    // order (the second pair zeroed: every sorted position holds a valid list position whatever happens)
    LB(hipMemsetAsync(code[1], 0, (size_t)n * sizeof(uint32_t), st));
    LB(hipMemsetAsync(pay[1], 0, (size_t)n * sizeof(uint32_t), st));
    int cur = 0;
    for (int shift = 0; shift < 32; shift += 8) {
        hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)sort_blocks), dim3(BLK), 0, st, code[cur], n, shift, table, sort_blocks);
        LB(scan_u64(table, table_n, partial, st));
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)sort_blocks), dim3(BLK), 0, st, code[cur], pay[cur], n, shift, table,
                           sort_blocks, code[cur ^ 1], pay[cur ^ 1]);
        cur ^= 1;
    }
    LB(hipGetLastError());
    Tree T{left, right, first, last, bbox, pbox, ploc ? pay[cur ^ 1] : pay[cur]};
    // tree and boxes
    int32_t root = ~0;
    if (sah) {
        int at = cur;
        SahStats ss;
        LB(sah_tree_device(n, pbox, pay, cur, left, right, first, last, bbox, SS, st, &root, &at, &ss));
        T.order = pay[at];
        if (stats) { stats->iterations = ss.levels; stats->tail_iterations = ss.levels - ss.grid_levels; }
    } else if (ploc) {
        root = n - 2;
        LB(ploc_tree_device(n, pbox, pay[cur], left, right, first, last, bbox, pay[cur ^ 1], PS, st, stats));
    } else if (n_int > 0) {
        root = 0;
        hipLaunchKernelGGL(k_radix_tree, dim3(blocks(n_int)), dim3(BLK), 0, st, code[cur], pay[cur], n, left, right, first, last, stamp);
        int32_t root_stamp = 0;
        for (int round = 1; round <= 64 && root_stamp == 0; round++) {
            hipLaunchKernelGGL(k_box_round, dim3(blocks(n_int)), dim3(BLK), 0, st, T, bbox, stamp, n_int, round);
            if (round % 8 == 0 || round == 64) {     // the root is the last to finish
                LB(hipMemcpyAsync(&root_stamp, stamp, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                LB(hipStreamSynchronize(st));
            }
        }
        if (root_stamp == 0) { free_lbvh(out); return hipErrorUnknown; }   // (a 62-bit key: at most 63 rounds)
    }
    // collapse, level by level
    LB(hipMemcpyAsync(defs[0], &root, sizeof(int32_t), hipMemcpyHostToDevice, st));
    int begin = 0, n_level = 1, rec_begin = 0, d = 0;
    out.level_begin.clear();
    while (n_level > 0) {
        if (begin + n_level > cap) { free_lbvh(out); return hipErrorUnknown; }
        out.level_begin.push_back(begin);
        hipLaunchKernelGGL(k_collapse_count, dim3(blocks(n_level)), dim3(BLK), 0, st, T, defs[d], n_level, slots, table);
        LB(scan_u64(table, n_level, partial, st));
        uint64_t total = 0;
        LB(hipMemcpyAsync(&total, partial + blocks(n_level), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        LB(hipStreamSynchronize(st));
        const int next_n = (int)(total >> 32), n_rec = (int)(uint32_t)total;
        // (checked before the emit writes: the next level's list, the nodes, the records)
        if (next_n > cap || begin + n_level + next_n > cap || rec_begin + n_rec > n) { free_lbvh(out); return hipErrorUnknown; }
        hipLaunchKernelGGL(k_collapse_emit, dim3(blocks(n_level)), dim3(BLK), 0, st, T, slots, table, n_level, begin,
                           begin + n_level, rec_begin, d_prims, flags, nodes, defs[d ^ 1], out.tris);
        LB(hipGetLastError());
        begin += n_level;
        rec_begin += n_rec;
        n_level = next_n;
        d ^= 1;
    }
    if (rec_begin != n) { free_lbvh(out); return hipErrorUnknown; }
    out.level_begin.push_back(begin);
    out.depth = (int)out.level_begin.size() - 1;
    out.n_nodes = begin;
    out.n_tris = n;
    LB(hipMalloc(&out.nodes, (size_t)begin * sizeof(Node8)));
    LB(hipMalloc(&out.nbox, 6 * (size_t)begin * sizeof(float)));
    LB(hipMemcpyAsync(out.nodes, nodes, (size_t)begin * sizeof(Node8), hipMemcpyDeviceToDevice, st));
    // the bytes that follow from the positions: the refit, on the new topology
    LB(launch_refit_tris(out.tris, n, idx, pos, pad, tbox, st));
    LB(launch_refit_levels(out.nodes, out.nbox, tbox, out.level_begin.data(), out.depth, st));
    LB(hipStreamSynchronize(st));
    return hipSuccess;
}
#undef LB

void build_lbvh_host(const float* pos, const int32_t* idx, const int32_t* prims, int n, float pad, BVH8& out, int mode,
                     int* iterations) {
    out = BVH8{};
    if (n <= 0) return;
    std::vector<float> pbox(6 * (size_t)n);
    double bounds[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; i++) {
        const int32_t prim = prims ? prims[i] : i;
        const float* v[3];
        for (int k = 0; k < 3; k++) v[k] = pos + 3 * (size_t)idx[3 * (size_t)prim + k];
        TriRec tr;
        const Box b = mptrefit::refit_tri(v[0], v[1], v[2], pad, tr);
        for (int a = 0; a < 3; a++) {
            pbox[6 * (size_t)i + a] = b.lo[a];
            pbox[6 * (size_t)i + 3 + a] = b.hi[a];
            const double c = centre(b.lo[a], b.hi[a]);
            bounds[a] = std::fmin(bounds[a], c);
            bounds[3 + a] = std::fmax(bounds[3 + a], c);
        }
    }
    std::vector<uint64_t> keys(n);
    for (int i = 0; i < n; i++) keys[i] = ((uint64_t)morton_code(&pbox[6 * (size_t)i], bounds) << 32) | (uint32_t)i;
    std::sort(keys.begin(), keys.end());
    std::vector<uint32_t> code(n), order(n);
    for (int i = 0; i < n; i++) { code[i] = (uint32_t)(keys[i] >> 32); order[i] = (uint32_t)keys[i]; }
    const int n_int = n - 1;
    std::vector<int32_t> left(n_int), right(n_int), first(n_int), last(n_int);
    std::vector<float> bbox(6 * (size_t)n_int);
    const bool sah = mode == MPT_BUILD_SAH && n > 1;
    const bool ploc = (mode == MPT_BUILD_PLOC && n > 1) || sah;       // (below: a tree with its own order and root)
    std::vector<uint32_t> order2(ploc ? n : 0);
    Tree T{left.data(), right.data(), first.data(), last.data(), bbox.data(), pbox.data(), ploc ? order2.data() : order.data()};
    if (iterations) *iterations = 0;
    int32_t sah_root = NO_REF;
    if (sah) {
        int levels = 0;
        sah_root = sah_tree_host(n, pbox.data(), order.data(), sah_depth_from_env(), left.data(), right.data(), first.data(),
                                 last.data(), bbox.data(), order2.data(), &levels);
        if (iterations) *iterations = levels;
        if (sah_root == NO_REF) return;                // (never by sah.h: an empty tree is the report)
    } else
    if (ploc) {
        const int its = ploc_tree_host(n, pbox.data(), order.data(), left.data(), right.data(), first.data(), last.data(),
                                       bbox.data(), order2.data());
        if (iterations) *iterations = its;
    }
    for (int i = 0; i < n_int && !ploc; i++) radix_node(code.data(), order.data(), n, i, &left[i], &right[i], &first[i], &last[i]);
    if (n_int > 0 && !ploc) {   // boxes: children before parents, by an explicit stack (min / max: exact in any order)
        std::vector<int32_t> stk{0}, post;
        while (!stk.empty()) {
            const int32_t x = stk.back();
            stk.pop_back();
            post.push_back(x);
            if (left[x] >= 0) stk.push_back(left[x]);
            if (right[x] >= 0) stk.push_back(right[x]);
        }
        for (size_t k = post.size(); k-- > 0;) {
            const int32_t x = post[k];
            Box b = ref_box(T, left[x]);
            mptrefit::box_grow(b, ref_box(T, right[x]));
            for (int a = 0; a < 3; a++) { bbox[6 * (size_t)x + a] = b.lo[a]; bbox[6 * (size_t)x + 3 + a] = b.hi[a]; }
        }
    }
    std::vector<int32_t> defs{sah ? sah_root : ploc ? n - 2 : n_int > 0 ? 0 : ~0}, next;
    out.tris.resize(n);
    int begin = 0, rec_begin = 0;
    while (!defs.empty()) {
        out.level_begin.push_back(begin);
        const int n_level = (int)defs.size();
        std::vector<int32_t> slots(8 * (size_t)n_level);
        std::vector<int> ci(n_level), cr(n_level);
        int sum_i = 0, sum_r = 0;
        for (int i = 0; i < n_level; i++) collapse_node(T, defs[i], &slots[8 * (size_t)i], &ci[i], &cr[i]);
        for (int i = 0; i < n_level; i++) { sum_i += ci[i]; sum_r += cr[i]; }
        out.nodes.resize((size_t)begin + n_level);
        next.assign(sum_i, 0);
        int e_int = 0, e_rec = 0;
        for (int i = 0; i < n_level; i++) {
            emit_node(T, &slots[8 * (size_t)i], (uint32_t)(begin + n_level + e_int), (uint32_t)(rec_begin + e_rec), prims, nullptr,
                      &out.nodes[(size_t)begin + i], next.data() + e_int, out.tris.data());
            e_int += ci[i];
            e_rec += cr[i];
        }
        begin += n_level;
        rec_begin += sum_r;
        defs.swap(next);
    }
    out.level_begin.push_back(begin);
    out.depth = (int)out.level_begin.size() - 1;
    refit_host(out, idx, pos, pad, out.node_box);
}

}  // namespace mpt

extern "C" {

int mpt_bvh_build_host(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                       const int32_t* prims, int32_t num_prims, void* nodes, int64_t nodes_cap_bytes, void* tris,
                       int64_t tris_cap_bytes, int32_t* out_counts) {
    return mpt_bvh_build_host_mode(vertices, num_vertices, indices, num_triangles, prims, num_prims, MPT_BUILD_LBVH, nodes,
                                   nodes_cap_bytes, tris, tris_cap_bytes, out_counts);
}

int mpt_bvh_build_host_mode(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                            const int32_t* prims, int32_t num_prims, int32_t mode, void* nodes, int64_t nodes_cap_bytes,
                            void* tris, int64_t tris_cap_bytes, int32_t* out_counts) {
    using namespace mpt;
    if (mode != MPT_BUILD_LBVH && mode != MPT_BUILD_PLOC && mode != MPT_BUILD_SAH)
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "bvh: unknown build mode");
    if (!vertices || !indices) return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_vertices <= 0 || num_triangles <= 0 || nodes_cap_bytes < 0 || tris_cap_bytes < 0)
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "bvh: bad size");
    if (prims && num_prims <= 0) return api_fail(MPT_ERR_INVALID_ARGUMENT, "bvh: empty primitive list");
    for (int64_t i = 0; i < 3 * (int64_t)num_triangles; i++)
        if (indices[i] < 0 || indices[i] >= num_vertices) return api_fail(MPT_ERR_INVALID_ARGUMENT, "triangle index out of range");
    for (int64_t i = 0; prims && i < num_prims; i++)
        if (prims[i] < 0 || prims[i] >= num_triangles) return api_fail(MPT_ERR_INVALID_ARGUMENT, "primitive index out of range");
    for (int64_t i = 0; i < 3 * (int64_t)num_vertices; i++)
        if (!(std::fabs(vertices[i]) <= 3.4028234663852886e38f)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    BVH8 bvh;
    build_lbvh_host(vertices, indices, prims, prims ? num_prims : num_triangles, scene_box_pad(vertices, num_triangles, indices), bvh,
                    mode);
    return copy_bvh_out(bvh.nodes.data(), bvh.nodes.size(), bvh.tris.data(), bvh.tris.size(), bvh.depth, nodes, nodes_cap_bytes,
                        tris, tris_cap_bytes, out_counts);
}

}  // extern "C"
