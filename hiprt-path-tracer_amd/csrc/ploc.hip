// ploc.hip -- the binary tree of the rebuild's quality mode (mpt_rebuild_bvh_mode, MPT_BUILD_PLOC)
// for gfx950, and the host loop of the same definition (ploc.h; DESIGN.md §2 "Rebuilds").
//
//   k_ploc_init       one thread per sorted position: the leaf clusters (reference, count, box planes)
//   k_ploc_nn         one thread per position: the boxes of the workgroup's tile and a halo of
//                     2 PLOC_RADIUS positions on either side staged in LDS as six planes, nn() of
//                     the tile and PLOC_RADIUS positions on either side, a barrier, the mutual test;
//                     writes what becomes of the position and the word (merges << 32 | survivors)
//   (scan_u64 of lbvh.hip numbers the merges and the survivors in position order)
//   k_ploc_emit       survivors into the other cluster buffer; the heads of merging pairs also
//                     write their node's left / right / count / box
//   k_ploc_tail       once at most PLOC_TAIL clusters are left: one workgroup, the clusters in LDS,
//                     all remaining iterations in one launch; it records where each iteration's
//                     node ids begin
//   k_ploc_order      the leaf order, one launch per iteration from the last to the first: the
//                     nodes of an iteration are a contiguous id range and their parents belong to
//                     later iterations
// No kernel waits on, or depends on seeing, what another workgroup writes in the same launch; order
// comes from scans, never from atomics; every loop is bounded by the n - 1 iterations of ploc.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "ploc.h"

namespace mpt {

namespace {

using namespace mptploc;

constexpr int BLK = 256;
constexpr int HALO = 2 * PLOC_RADIUS;
constexpr int TILE = BLK + 2 * HALO;

// six planes of `stride` floats: lo x, y, z, hi x, y, z
struct PlaneBox {
    const float* p;
    int stride, origin;
    __host__ __device__ Box operator()(int j) const {
        Box b;
        for (int a = 0; a < 3; a++) { b.lo[a] = p[a * stride + (j - origin)]; b.hi[a] = p[(3 + a) * stride + (j - origin)]; }
        return b;
    }
};
struct NnAt {
    const int32_t* p;
    int origin;
    __host__ __device__ int operator()(int k) const { return p[k - origin]; }
};

__global__ void __launch_bounds__(BLK) k_ploc_init(int n, const float* __restrict__ pbox, const uint32_t* __restrict__ order,
                                                   int32_t* __restrict__ cref, int32_t* __restrict__ ccnt,
                                                   float* __restrict__ cbox) {
    const int p = (int)(blockIdx.x * BLK + threadIdx.x);
    if (p >= n) return;
    const uint32_t li = order[p] < (uint32_t)n ? order[p] : 0u;
    cref[p] = ~p;
    ccnt[p] = 1;
    for (int k = 0; k < 6; k++) cbox[(size_t)k * n + p] = pbox[6 * (size_t)li + k];
}

__global__ void __launch_bounds__(BLK) k_ploc_nn(const float* __restrict__ cbox, int stride, int m, int32_t* __restrict__ mate_out,
                                                 uint64_t* __restrict__ words) {
    __shared__ float sb[6 * TILE];
    __shared__ int32_t snn[TILE];
    const int t = (int)threadIdx.x;
    const int base = (int)(blockIdx.x * BLK), g0 = base - HALO;
    for (int l = t; l < TILE; l += BLK) {
        const int g = g0 + l;
        const bool in = g >= 0 && g < m;
        for (int k = 0; k < 6; k++) sb[k * TILE + l] = in ? cbox[(size_t)k * stride + g] : 0.0f;
    }
    __syncthreads();
    const PlaneBox at{sb, TILE, g0};
    for (int l = PLOC_RADIUS + t; l < TILE - PLOC_RADIUS; l += BLK) {
        const int g = g0 + l;
        snn[l] = g >= 0 && g < m ? nearest(at, g, m) : -1;
    }
    __syncthreads();
    const int i = base + t;
    if (i >= m) return;
    const int32_t mt = mate(NnAt{snn, g0}, i);
    mate_out[i] = mt;
    words[i] = scan_word(mt);
}

// words: the exclusive scan of k_ploc_nn's.  src / dst: the two cluster buffers (planes of `stride`).
__global__ void __launch_bounds__(BLK) k_ploc_emit(const int32_t* __restrict__ sref, const int32_t* __restrict__ scnt,
                                                   const float* __restrict__ sbox, int stride, int m,
                                                   const int32_t* __restrict__ mate_in, const uint64_t* __restrict__ words,
                                                   int next_id, int n_int, int32_t* __restrict__ dref, int32_t* __restrict__ dcnt,
                                                   float* __restrict__ dbox, int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                   int32_t* __restrict__ count, float* __restrict__ nbox) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= m) return;
    const int32_t mt = mate_in[i];
    if (mt == ABSORBED) return;
    const uint32_t p = (uint32_t)words[i], k = (uint32_t)(words[i] >> 32);
    if (p >= (uint32_t)m) return;
    const PlaneBox at{sbox, stride, 0};
    Box b = at(i);
    int32_t r = sref[i], c = scnt[i];
    if (mt >= 0 && mt < m) {
        const uint32_t id = (uint32_t)next_id + k;
        if (id >= (uint32_t)n_int) return;
        b = box_union(b, at(mt));
        left[id] = r;
        right[id] = sref[mt];
        c += scnt[mt];
        count[id] = c;
        for (int a = 0; a < 3; a++) { nbox[6 * (size_t)id + a] = b.lo[a]; nbox[6 * (size_t)id + 3 + a] = b.hi[a]; }
        r = (int32_t)id;
    }
    dref[p] = r;
    dcnt[p] = c;
    for (int a = 0; a < 3; a++) { dbox[(size_t)a * stride + p] = b.lo[a]; dbox[(size_t)(3 + a) * stride + p] = b.hi[a]; }
}

// One workgroup, m0 <= PLOC_TAIL clusters: every remaining iteration.  info[0]: the number of
// iterations run (-1: the build did not finish), info[1 + k]: next_id before iteration k, and
// after the last.
__global__ void __launch_bounds__(PLOC_TAIL) k_ploc_tail(const int32_t* __restrict__ cref, const int32_t* __restrict__ ccnt,
                                                         const float* __restrict__ cbox, int stride, int m0, int next_id0,
                                                         int n_int, int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                         int32_t* __restrict__ count, float* __restrict__ nbox,
                                                         int32_t* __restrict__ info) {
    __shared__ float sb[6 * PLOC_TAIL];
    __shared__ int32_t sref[PLOC_TAIL], scnt[PLOC_TAIL], snn[PLOC_TAIL];
    __shared__ uint32_t sscan[2][PLOC_TAIL];
    const int t = (int)threadIdx.x;
    if (t < m0) {
        sref[t] = cref[t];
        scnt[t] = ccnt[t];
        for (int k = 0; k < 6; k++) sb[k * PLOC_TAIL + t] = cbox[(size_t)k * stride + t];
    }
    if (t == 0) info[1] = next_id0;
    __syncthreads();
    const PlaneBox at{sb, PLOC_TAIL, 0};
    int m = m0, next_id = next_id0, it = 0;            // the same in every thread
    while (m > 1 && it < PLOC_TAIL) {
        if (t < m) snn[t] = nearest(at, t, m);
        __syncthreads();
        int32_t mt = ABSORBED;
        uint32_t w = 0;
        if (t < m) {
            mt = mate(NnAt{snn, 0}, t);
            const uint64_t word = scan_word(mt);
            w = ((uint32_t)(word >> 32) << 16) | (uint32_t)word;     // merges <= 512, survivors <= 1024
        }
        int src = 0;
        sscan[0][t] = w;
        __syncthreads();
        for (int o = 1; o < PLOC_TAIL; o <<= 1) {
            sscan[src ^ 1][t] = sscan[src][t] + (t >= o ? sscan[src][t - o] : 0u);
            __syncthreads();
            src ^= 1;
        }
        const uint32_t excl = sscan[src][t] - w, total = sscan[src][PLOC_TAIL - 1];
        const int merges = (int)(total >> 16), survivors = (int)(total & 0xffffu);
        if (merges < 1 || survivors != m - merges || next_id + merges > n_int) break;   // (uniform; never by ploc.h)
        const bool keep = t < m && mt != ABSORBED;
        Box b;
        int32_t r = 0, c = 0;
        if (keep) {
            b = at(t);
            r = sref[t];
            c = scnt[t];
            if (mt >= 0) {
                const int32_t id = next_id + (int32_t)(excl >> 16);
                b = box_union(b, at(mt));
                left[id] = r;
                right[id] = sref[mt];
                c += scnt[mt];
                count[id] = c;
                for (int a = 0; a < 3; a++) { nbox[6 * (size_t)id + a] = b.lo[a]; nbox[6 * (size_t)id + 3 + a] = b.hi[a]; }
                r = id;
            }
        }
        __syncthreads();                               // every read of the old list is done
        if (keep) {
            const uint32_t p = excl & 0xffffu;         // < survivors <= PLOC_TAIL
            sref[p] = r;
            scnt[p] = c;
            for (int a = 0; a < 3; a++) { sb[a * PLOC_TAIL + p] = b.lo[a]; sb[(3 + a) * PLOC_TAIL + p] = b.hi[a]; }
        }
        next_id += merges;
        m = survivors;
        it++;
        if (t == 0) info[1 + it] = next_id;
        __syncthreads();
    }
    if (t == 0) info[0] = m == 1 ? it : -1;
}

// The nodes begin .. begin + cnt - 1 of one iteration; their firsts were set by their parents.
__global__ void __launch_bounds__(BLK) k_ploc_order(int begin, int cnt, int n, int32_t* left, int32_t* right, int32_t* first,
                                                    int32_t* last, const int32_t* __restrict__ count,
                                                    const uint32_t* __restrict__ order, uint32_t* __restrict__ order_out) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= cnt) return;
    const int32_t id = begin + i;
    const int32_t f = first[id], c = count[id], l = left[id], r = right[id];
    // (never by ploc.h: nothing is written out of bounds whatever the arrays hold)
    if (f < 0 || c < 2 || f > n - c || l >= id || r >= id || l < -n || r < -n) return;
    if ((l < 0 ? 1 : count[l]) + (r < 0 ? 1 : count[r]) != c) return;
    place_children(id, left, right, first, last, count, order, order_out);
}

inline unsigned blocks(int n) { return (unsigned)((n + BLK - 1) / BLK); }

}  // namespace

#define PL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t ploc_tree_device(int n, const float* pbox, const uint32_t* order, int32_t* left, int32_t* right, int32_t* first,
                            int32_t* last, float* nbox, uint32_t* order_out, const PlocScratch& B, hipStream_t st,
                            PlocStats* stats) {
    if (n < 2) return hipErrorInvalidValue;
    const int n_int = n - 1;
    int tail = PLOC_TAIL;
    if (const char* e = std::getenv("MPT_PLOC_TAIL")) tail = std::atoi(e) == 0 ? 0 : PLOC_TAIL;
    hipLaunchKernelGGL(k_ploc_init, dim3(blocks(n)), dim3(BLK), 0, st, n, pbox, order, B.cref[0], B.ccnt[0], B.cbox[0]);
    PL(hipMemsetAsync(first, 0, (size_t)n_int * sizeof(int32_t), st));
    PL(hipMemsetAsync(last, 0, (size_t)n_int * sizeof(int32_t), st));
    PL(hipMemsetAsync(B.count, 0, (size_t)n_int * sizeof(int32_t), st));
    PL(hipMemsetAsync(order_out, 0, (size_t)n * sizeof(uint32_t), st));
    std::vector<int32_t> begins{0};                    // next_id before each iteration, and after the last
    int m = n, next_id = 0, cur = 0, tail_iterations = 0;
    while (m > 1) {
        if ((int)begins.size() > n_int) return hipErrorUnknown;          // at most n - 1 iterations
        if (m <= tail) {
            hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(PLOC_TAIL), 0, st, B.cref[cur], B.ccnt[cur], B.cbox[cur], n, m, next_id,
                               n_int, left, right, B.count, nbox, B.tail_info);
            PL(hipGetLastError());
            std::vector<int32_t> info(PLOC_TAIL + 2);
            PL(hipMemcpyAsync(info.data(), B.tail_info, info.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            PL(hipStreamSynchronize(st));
            const int its = info[0];
            if (its < 1 || its > PLOC_TAIL || info[1] != next_id) return hipErrorUnknown;
            for (int k = 1; k <= its; k++) {
                if (info[1 + k] <= info[k] || info[1 + k] > n_int) return hipErrorUnknown;
                begins.push_back(info[1 + k]);
            }
            next_id = begins.back();
            tail_iterations = its;
            m = 1;
            break;
        }
        hipLaunchKernelGGL(k_ploc_nn, dim3(blocks(m)), dim3(BLK), 0, st, B.cbox[cur], n, m, B.mate, B.words);
        PL(scan_u64(B.words, m, B.partial, st));
        uint64_t total = 0;
        PL(hipMemcpyAsync(&total, B.partial + blocks(m), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        PL(hipStreamSynchronize(st));
        const int merges = (int)(total >> 32), survivors = (int)(uint32_t)total;
        // (checked before the emit writes: the node ids, the next list)
        if (merges < 1 || survivors != m - merges || next_id + merges > n_int) return hipErrorUnknown;
        hipLaunchKernelGGL(k_ploc_emit, dim3(blocks(m)), dim3(BLK), 0, st, B.cref[cur], B.ccnt[cur], B.cbox[cur], n, m, B.mate,
                           B.words, next_id, n_int, B.cref[cur ^ 1], B.ccnt[cur ^ 1], B.cbox[cur ^ 1], left, right, B.count, nbox);
        PL(hipGetLastError());
        next_id += merges;
        begins.push_back(next_id);
        m = survivors;
        cur ^= 1;
    }
    if (next_id != n_int) return hipErrorUnknown;
    // the leaf order: first(root) = 0 (the memset), then the iterations from the last to the first
    for (size_t k = begins.size() - 1; k-- > 0;) {
        const int cnt = begins[k + 1] - begins[k];
        hipLaunchKernelGGL(k_ploc_order, dim3(blocks(cnt)), dim3(BLK), 0, st, begins[k], cnt, n, left, right, first, last, B.count,
                           order, order_out);
    }
    PL(hipGetLastError());
    if (stats) { stats->iterations = (int)begins.size() - 1; stats->tail_iterations = tail_iterations; }
    return hipSuccess;
}
#undef PL

int ploc_tree_host(int n, const float* pbox, const uint32_t* order, int32_t* left, int32_t* right, int32_t* first,
                   int32_t* last, float* nbox, uint32_t* order_out) {
    const int n_int = n - 1;
    // the cluster list as the kernels hold it: six planes
    std::vector<float> box[2] = {std::vector<float>(6 * (size_t)n), std::vector<float>(6 * (size_t)n)};
    std::vector<int32_t> ref[2] = {std::vector<int32_t>(n), std::vector<int32_t>(n)};
    std::vector<int32_t> cnt[2] = {std::vector<int32_t>(n), std::vector<int32_t>(n)};
    std::vector<int32_t> nn(n), mt(n), count(n_int);
    for (int p = 0; p < n; p++) {
        ref[0][p] = ~p;
        cnt[0][p] = 1;
        for (int k = 0; k < 6; k++) box[0][(size_t)k * n + p] = pbox[6 * (size_t)order[p] + k];
    }
    int m = n, next_id = 0, cur = 0, iterations = 0;
    while (m > 1) {
        const PlaneBox at{box[cur].data(), n, 0};
        for (int i = 0; i < m; i++) nn[i] = nearest(at, i, m);
        for (int i = 0; i < m; i++) mt[i] = mate(NnAt{nn.data(), 0}, i);
        uint64_t run = 0;
        for (int i = 0; i < m; i++) {
            const uint64_t e = run;
            run += scan_word(mt[i]);
            if (mt[i] == ABSORBED) continue;
            const uint32_t p = (uint32_t)e;
            Box b = at(i);
            int32_t r = ref[cur][i], c = cnt[cur][i];
            if (mt[i] >= 0) {
                const int32_t id = next_id + (int32_t)(e >> 32), j = mt[i];
                b = box_union(b, at(j));
                left[id] = r;
                right[id] = ref[cur][j];
                c += cnt[cur][j];
                count[id] = c;
                for (int a = 0; a < 3; a++) { nbox[6 * (size_t)id + a] = b.lo[a]; nbox[6 * (size_t)id + 3 + a] = b.hi[a]; }
                r = id;
            }
            ref[cur ^ 1][p] = r;
            cnt[cur ^ 1][p] = c;
            for (int a = 0; a < 3; a++) { box[cur ^ 1][(size_t)a * n + p] = b.lo[a]; box[cur ^ 1][(size_t)(3 + a) * n + p] = b.hi[a]; }
        }
        next_id += (int)(run >> 32);
        m = (int)(uint32_t)run;
        cur ^= 1;
        iterations++;
    }
    first[n_int - 1] = 0;                              // children have smaller ids: parents first by descending id
    for (int32_t id = n_int - 1; id >= 0; id--) place_children(id, left, right, first, last, count.data(), order, order_out);
    return iterations;
}

}  // namespace mpt
