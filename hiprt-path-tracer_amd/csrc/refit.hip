// refit.hip -- the BVH8 refit of mpt_update_vertices for gfx950, and the host loop of the same
// arithmetic (refit.h; DESIGN.md §2 "Geometry updates").
//
//   k_refit_tris    one thread per triangle record: A / e1 / e2 from idx and pos (the w lanes
//                   kept), the record's padded box into a temporary plane (6 floats per record)
//   k_refit_level   one launch per breadth-first level, the deepest first: 8 lanes per node (a
//                   wave covers 8 nodes), each lane gathers one slot's exact box -- the union of
//                   a leaf slot's triangle boxes, or the exact box of the child node written by
//                   the previous launch; the node box is a min / max across the 8 lanes, each lane
//                   quantises its own slot, the bytes are collected across the lanes and four
//                   lanes store the node's four changed 16-byte quarters (child_base, tri_base and
//                   meta keep theirs), three more the exact box.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "refit.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using namespace mptrefit;

__global__ void __launch_bounds__(256) k_refit_tris(TriRec* __restrict__ tris, int n, const int32_t* __restrict__ idx,
                                                    const float* __restrict__ pos, float pad, float2* __restrict__ tbox) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float4* rec = (float4*)(tris + i);
    float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const int32_t prim = __float_as_int(r0.w);
    float v[3][3];
    for (int k = 0; k < 3; k++) {
        const size_t vi = (size_t)idx[3 * (size_t)prim + k];
        for (int a = 0; a < 3; a++) v[k][a] = pos[3 * vi + a];
    }
    TriRec tr;
    const Box b = refit_tri(v[0], v[1], v[2], pad, tr);
    rec[0] = make_float4(tr.ax, tr.ay, tr.az, r0.w);
    rec[1] = make_float4(tr.e1x, tr.e1y, tr.e1z, r1.w);
    rec[2] = make_float4(tr.e2x, tr.e2y, tr.e2z, r2.w);
    float2* o = tbox + 3 * (size_t)i;
    o[0] = make_float2(b.lo[0], b.lo[1]);
    o[1] = make_float2(b.lo[2], b.hi[0]);
    o[2] = make_float2(b.hi[1], b.hi[2]);
}

__device__ inline uint32_t or8(uint32_t v) {   // OR over the 8 lanes of a node
    v |= (uint32_t)__shfl_xor((int)v, 1);
    v |= (uint32_t)__shfl_xor((int)v, 2);
    v |= (uint32_t)__shfl_xor((int)v, 4);
    return v;
}

// nodes [begin, end): one level.  node_box: 6 floats per node; tbox: 6 floats per record.
__global__ void __launch_bounds__(256) k_refit_level(Node8* __restrict__ nodes, float* __restrict__ node_box,
                                                     const float* __restrict__ tbox, int begin, int end) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int s = t & 7;
    const int ni = begin + (t >> 3);
    const bool live = ni < end;          // lanes past the level gather nothing and store nothing
    Box b = box_empty();
    bool empty = true;
    if (live) {
        const uint4 h0 = ((const uint4*)(nodes + ni))[0];
        const uint4 h1 = ((const uint4*)(nodes + ni))[1];
        const uint32_t imask = h0.w >> 24;
        const uint32_t meta = ((s < 4 ? h1.z : h1.w) >> (8 * (s & 3))) & 0xffu;
        if ((imask >> s) & 1u) {
            const float* c = node_box + 6 * (size_t)(h1.x + meta);
            for (int a = 0; a < 3; a++) { b.lo[a] = c[a]; b.hi[a] = c[3 + a]; }
            empty = false;
        } else if (meta != 0) {
            const size_t first = (size_t)h1.y + (meta & 31u);
            const int cnt = (int)(meta >> 5);
            for (int k = 0; k < cnt; k++) {
                const float* c = tbox + 6 * (first + k);
                Box tb;
                for (int a = 0; a < 3; a++) { tb.lo[a] = c[a]; tb.hi[a] = c[3 + a]; }
                box_grow(b, tb);
            }
            empty = false;
        }
    }
    Box nb = b;                          // the node box: across the node's 8 lanes
    for (int m = 1; m < 8; m <<= 1)
        for (int a = 0; a < 3; a++) {
            nb.lo[a] = fminf(nb.lo[a], __shfl_xor(nb.lo[a], m));
            nb.hi[a] = fmaxf(nb.hi[a], __shfl_xor(nb.hi[a], m));
        }
    uint32_t ebyte[3], q[6] = {0, 0, 0, 0, 0, 0};
    for (int a = 0; a < 3; a++) {
        const int e = live ? quant_exp_exact(nb.hi[a], nb.lo[a]) : -126;
        ebyte[a] = (uint32_t)(e + 127);
        if (!empty) {
            q[a] = quant_lo(b.lo[a], nb.lo[a], e);
            q[3 + a] = quant_hi(b.hi[a], nb.lo[a], e);
        }
    }
    // every lane ends with the node's 48 bound bytes: plane k's low dword from slots 0-3, high from 4-7
    uint32_t w[12];
    const uint32_t sh = 8u * (uint32_t)(s & 3);
    for (int k = 0; k < 6; k++) {
        w[2 * k] = or8(s < 4 ? q[k] << sh : 0u);
        w[2 * k + 1] = or8(s >= 4 ? q[k] << sh : 0u);
    }
    if (!live) return;
    uint4* out = (uint4*)(nodes + ni);
    if (s == 0) {
        const uint4 h0 = out[0];
        const uint32_t imask = h0.w & 0xff000000u;
        out[0] = make_uint4(__float_as_uint(nb.lo[0]), __float_as_uint(nb.lo[1]), __float_as_uint(nb.lo[2]),
                            ebyte[0] | (ebyte[1] << 8) | (ebyte[2] << 16) | imask);
    } else if (s <= 3) {
        out[1 + s] = make_uint4(w[4 * (s - 1)], w[4 * (s - 1) + 1], w[4 * (s - 1) + 2], w[4 * (s - 1) + 3]);
    } else if (s <= 6) {
        float2* o = (float2*)(node_box + 6 * (size_t)ni) + (s - 4);
        *o = s == 4 ? make_float2(nb.lo[0], nb.lo[1]) : s == 5 ? make_float2(nb.lo[2], nb.hi[0]) : make_float2(nb.hi[1], nb.hi[2]);
    }
}

}  // namespace

// The records of a tree (n records) refitted to pos, their boxes into tbox (6 * n floats).
hipError_t launch_refit_tris(TriRec* tris, int n, const int32_t* idx, const float* pos, float pad, float* tbox, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_refit_tris, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tris, n, idx, pos, pad, (float2*)tbox);
    return hipGetLastError();
}

// The node levels from the deepest to the root; level_begin: levels + 1 entries (BVH8::level_begin).
hipError_t launch_refit_levels(Node8* nodes, float* node_box, const float* tbox, const int32_t* level_begin, int levels,
                               hipStream_t st) {
    for (int l = levels - 1; l >= 0; l--) {
        const int begin = level_begin[l], end = level_begin[l + 1];
        if (end <= begin) continue;
        const unsigned threads = 8u * (unsigned)(end - begin);
        hipLaunchKernelGGL(k_refit_level, dim3((threads + 255) / 256), dim3(256), 0, st, nodes, node_box, tbox, begin, end);
    }
    return hipGetLastError();
}

void refit_host(BVH8& bvh, const int32_t* idx, const float* pos, float pad, std::vector<float>& node_box) {
    using namespace mptrefit;
    const size_t nt = bvh.tris.size(), nn = bvh.nodes.size();
    std::vector<Box> tbox(nt);
    for (size_t i = 0; i < nt; i++) {
        int32_t prim;
        std::memcpy(&prim, &bvh.tris[i].prim_bits, 4);
        const float* v[3];
        for (int k = 0; k < 3; k++) v[k] = pos + 3 * (size_t)idx[3 * (size_t)prim + k];
        tbox[i] = refit_tri(v[0], v[1], v[2], pad, bvh.tris[i]);
    }
    node_box.resize(6 * nn);
    for (size_t ni = nn; ni-- > 0;) {   // children have larger indices than their parent
        Node8& n = bvh.nodes[ni];
        Box sb[8], nb = box_empty();
        for (int s = 0; s < 8; s++) {
            sb[s] = box_empty();
            if (slot_internal(n, s)) {
                const float* c = &node_box[6 * ((size_t)n.child_base + n.meta[s])];
                for (int a = 0; a < 3; a++) { sb[s].lo[a] = c[a]; sb[s].hi[a] = c[3 + a]; }
            } else if (!slot_empty(n, s)) {
                const size_t first = (size_t)n.tri_base + (n.meta[s] & 31u);
                for (int k = 0; k < (n.meta[s] >> 5); k++) box_grow(sb[s], tbox[first + k]);
            } else {
                continue;
            }
            box_grow(nb, sb[s]);
        }
        n.px = nb.lo[0]; n.py = nb.lo[1]; n.pz = nb.lo[2];
        int e[3];
        for (int a = 0; a < 3; a++) e[a] = quant_exp_exact(nb.hi[a], nb.lo[a]);
        n.ex = (uint8_t)(e[0] + 127); n.ey = (uint8_t)(e[1] + 127); n.ez = (uint8_t)(e[2] + 127);
        for (int s = 0; s < 8; s++) {
            if (slot_empty(n, s)) continue;
            n.qlox[s] = quant_lo(sb[s].lo[0], nb.lo[0], e[0]); n.qhix[s] = quant_hi(sb[s].hi[0], nb.lo[0], e[0]);
            n.qloy[s] = quant_lo(sb[s].lo[1], nb.lo[1], e[1]); n.qhiy[s] = quant_hi(sb[s].hi[1], nb.lo[1], e[1]);
            n.qloz[s] = quant_lo(sb[s].lo[2], nb.lo[2], e[2]); n.qhiz[s] = quant_hi(sb[s].hi[2], nb.lo[2], e[2]);
        }
        for (int a = 0; a < 3; a++) { node_box[6 * ni + a] = nb.lo[a]; node_box[6 * ni + 3 + a] = nb.hi[a]; }
    }
}

double node_box_area_sum(const float* node_box, size_t nodes) {
    double sum = 0.0;
    for (size_t i = 0; i < nodes; i++) {
        const float* b = node_box + 6 * i;
        const double d0 = (double)b[3] - (double)b[0], d1 = (double)b[4] - (double)b[1], d2 = (double)b[5] - (double)b[2];
        sum += 2.0 * (d0 * d1 + d1 * d2 + d2 * d0);
    }
    return sum;
}

int build_scene_bvh8(const float* vertices, const int32_t* indices, int32_t num_triangles, BVH8& out, int stack_limit) {
    // triangles per leaf child: 3 (MPT_BVH_LEAF, 1..4, development A/B)
    int max_leaf = 3;
    if (const char* e = std::getenv("MPT_BVH_LEAF")) max_leaf = std::max(1, std::min(4, std::atoi(e)));
    // per level: at most one node group and one postponed triangle group on the stack; a
    // tree too deep for the traversal stack is rebuilt with balanced splits from a smaller
    // depth on (test hook MPT_BVH_MAX_STACK: a lower limit)
    int stack_cap = stack_limit;
    if (const char* e = std::getenv("MPT_BVH_MAX_STACK")) stack_cap = std::max(4, std::min(stack_limit, std::atoi(e)));
    for (int sah_depth = 40;; sah_depth = sah_depth * 2 / 3) {
        build_bvh8(vertices, indices, num_triangles, out, max_leaf, -1.0f, sah_depth);
        if (2 * out.depth + 2 <= stack_cap || sah_depth == 0) break;
    }
    return stack_cap;
}

// nodes / tris of a tree into caller buffers (both caps 0: the counts only)
int copy_bvh_out(const Node8* nodes, size_t n_nodes, const TriRec* tris, size_t n_tris, int levels, void* out_nodes,
                 int64_t nodes_cap, void* out_tris, int64_t tris_cap, int32_t* out_counts) {
    if (out_counts) { out_counts[0] = (int32_t)n_nodes; out_counts[1] = (int32_t)n_tris; out_counts[2] = levels; }
    if (nodes_cap == 0 && tris_cap == 0) return MPT_OK;
    if (!out_nodes || !out_tris) return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (nodes_cap < (int64_t)(n_nodes * sizeof(Node8)) || tris_cap < (int64_t)(n_tris * sizeof(TriRec)))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "bvh: output buffer too small");
    if (nodes) std::memcpy(out_nodes, nodes, n_nodes * sizeof(Node8));
    if (tris) std::memcpy(out_tris, tris, n_tris * sizeof(TriRec));
    return MPT_OK;
}

}  // namespace mpt

extern "C" {

int mpt_bvh_refit_host(const float* build_vertices, const float* new_vertices, int32_t num_vertices, const int32_t* indices,
                       int32_t num_triangles, void* nodes, int64_t nodes_cap_bytes, void* tris, int64_t tris_cap_bytes,
                       int32_t* out_counts) {
    using namespace mpt;
    if (!build_vertices || !indices) return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_vertices <= 0 || num_triangles <= 0 || nodes_cap_bytes < 0 || tris_cap_bytes < 0)
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "bvh: bad size");
    for (int64_t i = 0; i < 3 * (int64_t)num_triangles; i++)
        if (indices[i] < 0 || indices[i] >= num_vertices) return api_fail(MPT_ERR_INVALID_ARGUMENT, "triangle index out of range");
    BVH8 bvh;
    build_scene_bvh8(build_vertices, indices, num_triangles, bvh, TRAV_LDS_STACK + TRAV_SPILL_DEPTH);
    if (new_vertices) {
        for (int64_t i = 0; i < 3 * (int64_t)num_vertices; i++)
            if (!(std::fabs(new_vertices[i]) <= 3.4028234663852886e38f)) return api_fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
        std::vector<float> node_box;
        refit_host(bvh, indices, new_vertices, scene_box_pad(new_vertices, num_triangles, indices), node_box);
    }
    return copy_bvh_out(bvh.nodes.data(), bvh.nodes.size(), bvh.tris.data(), bvh.tris.size(), bvh.depth, nodes, nodes_cap_bytes,
                        tris, tris_cap_bytes, out_counts);
}

}  // extern "C"
