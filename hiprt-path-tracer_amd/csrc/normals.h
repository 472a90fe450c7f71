// normals.h -- the arithmetic of recomputed vertex normals (mpt_set_normals), shared verbatim by the
// kernels (normals.hip: k_face, k_gather, k_fused) and the host loop (normals_host, behind
// mpt_normals_host), the way morph.h, skin.h and xform.h are: compiled with -ffp-contract=off on
// both sides, so that the GPU and the CPU produce the same bytes.
//
// Every vertex has a group id in [-1, G).  The vertices of one group receive one common normal;
// -1: never touched.  Both sides read the groups as a CSR over the scene's index buffer (to_csr
// below): row[G + 1] offsets; per entry the id p of a triangle, one entry for every corner (p, k)
// whose vertex idx[3p + k] lies in the group, in ascending p, then k (a triangle with two corners
// in one group appears twice).  A gather: a scatter with atomics would have no fixed order of
// additions.
//
//   face vector   of triangle p with the positions a, b, c of its corners: e1 = b - a, e2 = c - a,
//                 f = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x); fp32, no fma,
//                 every product rounded before the difference.  Its length is twice the area.
//   group sum     s = +0, then s[r] = s[r] + f[r] over the group's entries in table order:
//                 sequential, fp32 (area weighting).  s = -s when the group's flip byte is set.
//   output        for every vertex v of the group with has_vertex_normals[v] != 0:
//                 mptxform::nrm_tail(s, n_v): s / sqrtf((s0*s0 + s1*s1) + s2*s2) when that squared
//                 length is positive and finite, else the normal n_v that the update left there.
//                 An empty group, a group of degenerate triangles and an overflowing cross product
//                 pass through.
//   untouched     vertices of group -1 and vertices without has_vertex_normals keep their bytes.
#ifndef MPT_NORMALS_H
#define MPT_NORMALS_H

#include <vector>

#include "xform.h"

#if defined(__HIPCC__)
#define NORMALS_FN __host__ __device__ static inline
#else
#define NORMALS_FN static inline
#endif

namespace mptnormals {

// The face vector of triangle p.
NORMALS_FN void face_vector(const int32_t* idx, const float* pos, int32_t p, float* f) {
    const float* a = pos + 3 * (size_t)idx[3 * (size_t)p];
    const float* b = pos + 3 * (size_t)idx[3 * (size_t)p + 1];
    const float* c = pos + 3 * (size_t)idx[3 * (size_t)p + 2];
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    f[0] = e1[1] * e2[2] - e1[2] * e2[1];
    f[1] = e1[2] * e2[0] - e1[0] * e2[2];
    f[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// One step of the group sum.
NORMALS_FN void add_face(float* s, const float* f) {
    for (int r = 0; r < 3; r++) s[r] = s[r] + f[r];
}

// The end of a group's sum for one of its vertices: the flip, then the tail over that vertex's own
// normal n into o (o may be n).
NORMALS_FN void finish_vertex(const float* s, bool flip, const float* n, float* o) {
    const float t[3] = {flip ? -s[0] : s[0], flip ? -s[1] : s[1], flip ? -s[2] : s[2]};
    const float keep[3] = {n[0], n[1], n[2]};
    mptxform::nrm_tail(t, keep, o);
}

// One vertex of group g (>= 0) from the face vectors formed on the spot.
NORMALS_FN void normal_vertex(const int32_t* row, const int32_t* tri, const uint8_t* flip, const int32_t* idx, const float* pos,
                              int32_t g, const float* n, float* o) {
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int32_t k = row[g]; k < row[g + 1]; k++) {
        float f[3];
        face_vector(idx, pos, tri[k], f);
        add_face(s, f);
    }
    finish_vertex(s, flip[g] != 0, n, o);
}

// The by-group CSR.
struct Csr {
    std::vector<int32_t> row, tri;
};

// The groups checked -- vertex_group[V] in [-1, G), the indices of the T triangles in [0, V) -- and
// the corners transposed by a stable counting sort in memory order, so that a group's entries come
// in ascending triangle, then corner.  Returns NULL, or what is wrong with the input (out is then
// unspecified).
static inline const char* to_csr(const int32_t* vertex_group, int32_t V, int32_t G, const int32_t* idx, int32_t T, Csr& out) {
    if (G < 1) return "normals: bad group count";
    if (V < 1 || T < 0 || (size_t)T > (size_t)0x7fffffff / 3) return "normals: bad size";
    for (int32_t v = 0; v < V; v++)
        if (vertex_group[v] < -1 || vertex_group[v] >= G) return "normals: group id out of range";
    const size_t C = 3 * (size_t)T;
    for (size_t k = 0; k < C; k++)
        if (idx[k] < 0 || idx[k] >= V) return "normals: vertex index out of range";
    out.row.assign((size_t)G + 1, 0);
    for (size_t k = 0; k < C; k++) {
        const int32_t g = vertex_group[idx[k]];
        if (g >= 0) out.row[(size_t)g + 1]++;
    }
    for (size_t g = 0; g < (size_t)G; g++) out.row[g + 1] += out.row[g];   // (at most 3T: no overflow)
    out.tri.resize((size_t)out.row[G]);
    std::vector<int32_t> at(out.row.begin(), out.row.end() - 1);
    for (size_t k = 0; k < C; k++) {
        const int32_t g = vertex_group[idx[k]];
        if (g >= 0) out.tri[(size_t)at[g]++] = (int32_t)(k / 3);
    }
    return nullptr;
}

}  // namespace mptnormals

#undef NORMALS_FN
#endif
