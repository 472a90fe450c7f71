// skin.h -- the arithmetic of linear-blend skinning (mpt_update_skin), shared verbatim by the kernel
// (skin.hip: k_skin) and the host loop (skin_host, behind mpt_skin_host), the way xform.h is:
// compiled with -ffp-contract=off on both sides, so that the GPU and the CPU produce the same bytes.
//
// A joint's record is 16 words (64 bytes, fetched with 16-byte loads): the row-major 3x4 matrix m
// (12 floats), one word that is 1 when those 12 floats are exactly the identity (xform.h's
// is_identity, made once per joint on the host by make_records) and 0 otherwise, and 3 words of
// padding.  No normal matrix is stored: it is derived per vertex from the blended matrix.
//
// A vertex has four joint indices j[0..3] and four weights w[0..3].
//   blend      B[e] = ((w0*M_j0[e] + w1*M_j1[e]) + w2*M_j2[e]) + w3*M_j3[e]   for the 12 entries e,
//              fp32, this order, no fma; all four terms always (the matrices are finite, so a zero
//              weight contributes a zero)
//   position   mptxform::xform_pos(B, p)
//   normal     a = B's linear part; the cofactors, each with two rounded products,
//                co[r][c] = a[r1][c1]*a[r2][c2] - a[r1][c2]*a[r2][c1]    r1 = (r+1)%3, r2 = (r+2)%3,
//                                                                        c1 = (c+1)%3, c2 = (c+2)%3
//                det      = (a[0][0]*co[0][0] + a[0][1]*co[0][1]) + a[0][2]*co[0][2]
//                N[r][c]  = det < 0 ? -co[r][c] : co[r][c]               all in fp32
//              then mptxform::xform_nrm(N, n): a zero or non-finite squared length passes the rest
//              normal through
//   pass       position and normal pass through byte for byte, and no matrix is read, when all four
//              weights are +0 or -0 (an unskinned vertex) or when every joint whose weight is not
//              zero carries the identity word.  So an all-identity pose changes no bit, whatever
//              the weights sum to.
#ifndef MPT_SKIN_H
#define MPT_SKIN_H

#include "xform.h"

#if defined(__HIPCC__)
#define SKIN_FN __host__ __device__ static inline
#else
#define SKIN_FN static inline
#endif

namespace mptskin {

constexpr int REC = 16;    // words per joint: m (12), the identity word, 3 of padding
constexpr int FLAG = 12;   // the identity word's place

// The joints of a vertex need not be read: every weight zero, or every weighted joint an identity.
// pal: the records, 16-byte aligned.
SKIN_FN bool passes(const float* pal, const int32_t* j, const float* w) {
    bool pass = true;
    for (int s = 0; s < 4; s++)
        if (w[s] != 0.0f) pass = pass && mptxform::fbits(pal[(size_t)REC * (size_t)j[s] + FLAG]) != 0u;
    return pass;
}

SKIN_FN void blend(const float* pal, const int32_t* j, const float* w, float* B) {
    const float* m0 = (const float*)__builtin_assume_aligned(pal + (size_t)REC * (size_t)j[0], 16);
    const float* m1 = (const float*)__builtin_assume_aligned(pal + (size_t)REC * (size_t)j[1], 16);
    const float* m2 = (const float*)__builtin_assume_aligned(pal + (size_t)REC * (size_t)j[2], 16);
    const float* m3 = (const float*)__builtin_assume_aligned(pal + (size_t)REC * (size_t)j[3], 16);
    for (int e = 0; e < 12; e++) B[e] = ((w[0] * m0[e] + w[1] * m1[e]) + w[2] * m2[e]) + w[3] * m3[e];
}

// The normal matrix of B's linear part: its cofactor matrix times the sign of its determinant.
SKIN_FN void normal_matrix(const float* B, float* N) {
    float co[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            co[3 * r + c] = B[4 * r1 + c1] * B[4 * r2 + c2] - B[4 * r1 + c2] * B[4 * r2 + c1];
        }
    const float det = (B[0] * co[0] + B[1] * co[1]) + B[2] * co[2];
    for (int k = 0; k < 9; k++) N[k] = det < 0.0f ? -co[k] : co[k];
}

// One vertex: rest position p and normal n into po / no.
SKIN_FN void skin_vertex(const float* pal, const int32_t* j, const float* w, const float* p, const float* n, float* po,
                         float* no) {
    if (passes(pal, j, w)) {
        for (int r = 0; r < 3; r++) { po[r] = p[r]; no[r] = n[r]; }
        return;
    }
    float B[12], N[9];
    blend(pal, j, w, B);
    mptxform::xform_pos(B, p, po);
    normal_matrix(B, N);
    mptxform::xform_nrm(N, n, no);
}

// The 16-word records of num_joints matrices (12 floats each).
static inline void make_records(const float* matrices, int32_t num_joints, float* rec) {
    for (int32_t k = 0; k < num_joints; k++) {
        float* r = rec + (size_t)REC * (size_t)k;
        memcpy(r, matrices + 12 * (size_t)k, 12 * sizeof(float));
        const uint32_t tail[4] = {mptxform::is_identity(r) ? 1u : 0u, 0u, 0u, 0u};
        memcpy(r + FLAG, tail, sizeof(tail));
    }
}

}  // namespace mptskin

#undef SKIN_FN
#endif
