// normals.hip -- recomputed vertex normals for gfx950 (mpt_set_normals; called by every geometry
// update before the per-triangle attribute records are made) and the host loop of the same
// arithmetic (normals.h; DESIGN.md §2 "Geometry updates", Normals).
//
// Two structures with the same bytes (mpt_geometry.cpp: normals_fused chooses):
//   k_face + k_gather   one lane per triangle writes the face vector as a float4 to a scratch
//                array: the indices are read coalesced, the positions gathered, as k_refit_tris
//                does.  Then one lane per vertex walks the row of its group, gathers the 16-byte
//                face vectors in table order, sums, normalises and stores its own normal.
//   k_fused      one lane per vertex gathers, per entry of its row, the triangle's three indices and
//                three positions and forms the face vector in registers: no scratch array, but
//                every face vector is formed once per corner in a group.
// One lane per VERTEX, not per group: the vertices of a welded group repeat the group's sum (the
// same additions in the same order: the same bytes), their group ids, normal flags and normals are
// read and written coalesced, and no second table from groups to vertices is needed.  The row loop
// is divergent by row length and sequential by definition: no reduction over lanes, which would
// change the order of the additions.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpt.h"
#include "mpt_internal.h"
#include "normals.h"

namespace mpt {

int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error

namespace {

using mptnormals::add_face;
using mptnormals::face_vector;
using mptnormals::finish_vertex;
using mptnormals::normal_vertex;

__global__ void __launch_bounds__(256) k_face(const NormalsLaunch a) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.num_tris) return;
    float f[3];
    face_vector(a.idx, a.pos, p, f);
    a.face[p] = make_float4(f[0], f[1], f[2], 0.0f);
}

template <bool FUSED>
__global__ void __launch_bounds__(256) k_vertex(const NormalsLaunch a) {
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= a.n) return;
    const int32_t g = a.group[v];
    if (g < 0 || !a.has_n[v]) return;
    float* n = a.nrm + 3 * (size_t)v;
    if constexpr (FUSED) {
        normal_vertex(a.row, a.tri, a.flip, a.idx, a.pos, g, n, n);
    } else {
        float s[3] = {0.0f, 0.0f, 0.0f};
        const int32_t e = a.row[g + 1];
        for (int32_t k = a.row[g]; k < e; k++) {
            const float4 q = a.face[a.tri[k]];
            const float f[3] = {q.x, q.y, q.z};
            add_face(s, f);
        }
        finish_vertex(s, a.flip[g] != 0, n, n);
    }
}

unsigned blocks(int n) { return (unsigned)(((size_t)n + 255) / 256); }

}  // namespace

hipError_t launch_normals(const NormalsLaunch& a, bool fused, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (fused) {
        hipLaunchKernelGGL((k_vertex<true>), dim3(blocks(a.n)), dim3(256), 0, st, a);
    } else {
        if (a.num_tris > 0) hipLaunchKernelGGL(k_face, dim3(blocks(a.num_tris)), dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_vertex<false>), dim3(blocks(a.n)), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

// The host loop over the same tables (has_n NULL: every vertex has a normal).
void normals_host(const float* pos, size_t n, const int32_t* idx, const int32_t* group, const uint8_t* flip, const uint8_t* has_n,
                  const mptnormals::Csr& t, float* nrm) {
    for (size_t v = 0; v < n; v++) {
        const int32_t g = group[v];
        if (g < 0 || (has_n && !has_n[v])) continue;
        mptnormals::normal_vertex(t.row.data(), t.tri.data(), flip, idx, pos, g, nrm + 3 * v, nrm + 3 * v);
    }
}

}  // namespace mpt

extern "C" {

int mpt_normals_host(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                     const int32_t* vertex_group, const uint8_t* group_flip, int32_t num_groups, const uint8_t* has_vertex_normals,
                     float* inout_normals) {
    using namespace mpt;
    if (!vertices || !vertex_group || !inout_normals || (!indices && num_triangles != 0))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    mptnormals::Csr csr;
    if (const char* bad = mptnormals::to_csr(vertex_group, num_vertices, num_groups, indices, num_triangles, csr))
        return api_fail(MPT_ERR_INVALID_ARGUMENT, bad);
    const std::vector<uint8_t> zeros(group_flip ? 0 : (size_t)num_groups, 0);
    normals_host(vertices, (size_t)num_vertices, indices, vertex_group, group_flip ? group_flip : zeros.data(), has_vertex_normals, csr,
                 inout_normals);
    return MPT_OK;
}

}  // extern "C"
