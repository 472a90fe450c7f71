// upload.hip -- the per-primitive passes of mpt_upload_scene_mode for gfx950 (upload.h).
//
//   k_prim_flags     one thread per primitive: the two flag words the build's emit gathers
//   k_light_mark     one thread per primitive: 1 / 0 into the scan's words
//   k_light_scatter  one thread per primitive: a marked primitive writes its index at its scanned
//                    position
// One thread per primitive, grids bounded by n; every index read from memory is checked before it
// is used as one.  No kernel depends on what another workgroup writes in the same launch.
#include "upload.h"

namespace mpt {

namespace {

constexpr int BLK = 256;

inline unsigned blocks(int n) { return (unsigned)((n + BLK - 1) / BLK); }

__device__ inline uint32_t material_flags(const int32_t* __restrict__ mat_idx, int i, const uint32_t* __restrict__ mat_flags,
                                          int n_mats, int32_t* m_out) {
    const int32_t m = mat_idx[i];
    *m_out = m;
    return (m >= 0 && m < n_mats) ? mat_flags[m] : 0u;
}

__global__ void __launch_bounds__(BLK) k_prim_flags(const int32_t* __restrict__ mat_idx, int n, const uint32_t* __restrict__ mat_flags,
                                                    const int32_t* __restrict__ mat_tex, int n_mats, int32_t class_keep,
                                                    uint2* __restrict__ flags) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n) return;
    int32_t m;
    const uint32_t mf = material_flags(mat_idx, i, mat_flags, n_mats, &m);
    const uint32_t cls = (m >= 0 && m < n_mats) ? (uint32_t)(mat_tex[m] & class_keep) : 0u;
    flags[i] = make_uint2((mf & MF_ALPHA) ? 1u : 0u, cls);
}

__global__ void __launch_bounds__(BLK) k_light_mark(const int32_t* __restrict__ mat_idx, int n, const uint32_t* __restrict__ mat_flags,
                                                    int n_mats, uint64_t* __restrict__ words) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n) return;
    int32_t m;
    words[i] = (material_flags(mat_idx, i, mat_flags, n_mats, &m) & MF_LIT) ? 1u : 0u;
}

__global__ void __launch_bounds__(BLK) k_light_scatter(const int32_t* __restrict__ mat_idx, int n,
                                                       const uint32_t* __restrict__ mat_flags, int n_mats,
                                                       const uint64_t* __restrict__ scanned, int32_t* __restrict__ out, int cap) {
    const int i = (int)(blockIdx.x * BLK + threadIdx.x);
    if (i >= n) return;
    int32_t m;
    if (!(material_flags(mat_idx, i, mat_flags, n_mats, &m) & MF_LIT)) return;
    const uint64_t at = scanned[i];
    if (at < (uint64_t)cap) out[at] = i;
}

}  // namespace

hipError_t launch_prim_flags(const int32_t* mat_idx, int n, const uint32_t* mat_flags, const int32_t* mat_tex, int n_mats,
                             int32_t class_keep, uint32_t* flags, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_prim_flags, dim3(blocks(n)), dim3(BLK), 0, st, mat_idx, n, mat_flags, mat_tex, n_mats, class_keep,
                       (uint2*)flags);
    return hipGetLastError();
}

hipError_t launch_light_mark(const int32_t* mat_idx, int n, const uint32_t* mat_flags, int n_mats, uint64_t* words, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_light_mark, dim3(blocks(n)), dim3(BLK), 0, st, mat_idx, n, mat_flags, n_mats, words);
    return hipGetLastError();
}

hipError_t launch_light_scatter(const int32_t* mat_idx, int n, const uint32_t* mat_flags, int n_mats, const uint64_t* scanned,
                                int32_t* out, int cap, hipStream_t st) {
    if (n <= 0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_light_scatter, dim3(blocks(n)), dim3(BLK), 0, st, mat_idx, n, mat_flags, n_mats, scanned, out, cap);
    return hipGetLastError();
}

}  // namespace mpt
