// vert_io.h -- what the kernels over vertex arrays share (xform.hip, skin.hip, morph.hip): a lane's
// group of G vertices loaded and stored with 16-byte accesses, the used-vertex mask, a vertex's skin
// influences, a group's CSR row offsets, and the block reduction of the largest |coordinate| and
// the non-finite flag.  Device code: included by .hip files only.
#ifndef MPT_VERT_IO_H
#define MPT_VERT_IO_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpt {
namespace vertio {

// red[0]: bits of the maximum, red[1]: 1 when a coordinate is not finite.  Every thread of the
// block arrives here (no early return before it).
__device__ static inline void reduce_block(float m, bool bad, uint32_t* __restrict__ red) {
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const int wbad = __any(bad ? 1 : 0);
    __shared__ float sm[4];
    __shared__ int sb[4];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    if (lane == 0) { sm[w] = m; sb[w] = wbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float mm = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if (mm > 0.0f) atomicMax(red, __float_as_uint(mm));
        if (sb[0] | sb[1] | sb[2] | sb[3]) atomicOr(red + 1, 1u);
    }
}

// 3 * G floats of a lane's group: 16-byte accesses for a whole group of 4, dwords otherwise.
template <int G>
__device__ static inline void load_group(const float* __restrict__ src, size_t v0, int cnt, float* x) {
    if (G == 4 && cnt == 4) {
        const float4* s = (const float4*)(src + 3 * v0);
        const float4 a = s[0], b = s[1], c = s[2];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
    } else {
        for (int k = 0; k < G; k++)
            for (int a = 0; a < 3; a++) x[3 * k + a] = k < cnt ? src[3 * (v0 + k) + a] : 0.0f;
    }
}
template <int G>
__device__ static inline void store_group(float* __restrict__ dst, size_t v0, int cnt, const float* x) {
    if (G == 4 && cnt == 4) {
        float4* d = (float4*)(dst + 3 * v0);
        d[0] = make_float4(x[0], x[1], x[2], x[3]);
        d[1] = make_float4(x[4], x[5], x[6], x[7]);
        d[2] = make_float4(x[8], x[9], x[10], x[11]);
    } else {
        for (int k = 0; k < G; k++)
            if (k < cnt)
                for (int a = 0; a < 3; a++) dst[3 * (v0 + k) + a] = x[3 * k + a];
    }
}
template <int G>
__device__ static inline void load_mask(const uint8_t* __restrict__ used, size_t v0, int cnt, bool* u) {
    if (G == 4 && cnt == 4) {
        const uint32_t w = *(const uint32_t*)(used + v0);
        for (int k = 0; k < 4; k++) u[k] = ((w >> (8 * k)) & 0xffu) != 0;
    } else {
        for (int k = 0; k < G; k++) u[k] = k < cnt && used[v0 + k] != 0;
    }
}

// The 4 joint indices and 4 weights of vertex v (skin.hip, morph.hip): 16-byte loads when the
// arrays are aligned (G = 4).
template <int G>
__device__ static inline void load_influences(const int32_t* __restrict__ joints, const float* __restrict__ weights, size_t v, int32_t* j,
                                              float* w) {
    if constexpr (G == 4) {
        const int4 a = *(const int4*)(joints + 4 * v);
        const float4 b = *(const float4*)(weights + 4 * v);
        j[0] = a.x; j[1] = a.y; j[2] = a.z; j[3] = a.w;
        w[0] = b.x; w[1] = b.y; w[2] = b.z; w[3] = b.w;
    } else {
        for (int s = 0; s < 4; s++) { j[s] = joints[4 * v + s]; w[s] = weights[4 * v + s]; }
    }
}

// The G + 1 CSR row offsets row[v0 .. v0 + cnt] of a lane's group (morph.hip): one 16-byte load and
// a dword for a whole group of 4; the offsets past cnt repeat the last one (empty rows).
template <int G>
__device__ static inline void load_rows(const int32_t* __restrict__ row, size_t v0, int cnt, int32_t* r) {
    if (G == 4 && cnt == 4) {
        const int4 a = *(const int4*)(row + v0);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
        r[4] = row[v0 + 4];
    } else {
        for (int k = 0; k <= G; k++) r[k] = row[v0 + (size_t)(k < cnt ? k : cnt)];
    }
}

static inline unsigned blocks_for(int n, int G) { return (unsigned)((((size_t)n + G - 1) / G + 255) / 256); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }


}  // namespace vertio
}  // namespace mpt

#endif
