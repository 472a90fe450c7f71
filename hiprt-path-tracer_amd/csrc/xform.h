// xform.h -- the arithmetic of per-object motion (mpt_update_transforms), shared verbatim by the
// kernel (xform.hip: k_xform) and the host loop (transform_host, behind mpt_transform_host), the
// way refit.h, display.h and denoise.h are shared: compiled with -ffp-contract=off on both sides,
// so that the GPU and the CPU produce the same bytes.
//
// An object's record is 21 floats: the row-major 3x4 matrix m, then the normal matrix N (3x3, row
// major) made once per object on the host by normal_matrix (below).
//   position   p'[r] = ((m[r][0]*x + m[r][1]*y) + m[r][2]*z) + m[r][3]   fp32, this order, no fma
//   normal     n'[r] = (N[r][0]*nx + N[r][1]*ny) + N[r][2]*nz
//              l2    = (n'x*n'x + n'y*n'y) + n'z*n'z
//              l2 > 0 and finite: n' / sqrtf(l2) (IEEE square root and division, as tmath.h relies
//              on); else the rest normal unchanged (the zero normals of vertices without one)
//   identity   an object whose 12 floats are exactly 1 and +0 passes positions and normals through
//              byte for byte (x + 0*y would turn a -0 into +0 and renormalise a non-unit normal)
//   static     vertices of object -1 pass through
#ifndef MPT_XFORM_H
#define MPT_XFORM_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define XFORM_FN __host__ __device__ static inline
#else
#define XFORM_FN static inline
#endif

namespace mptxform {

constexpr int REC = 21;   // floats per object: m (12), N (9)
constexpr float F_MAX = 3.4028234663852886e38f;

XFORM_FN uint32_t fbits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// The 12 floats are exactly the identity: 1 on the diagonal, +0 elsewhere.
XFORM_FN bool is_identity(const float* m) {
    uint32_t diff = 0;
    for (int k = 0; k < 12; k++) diff |= fbits(m[k]) ^ ((k == 0 || k == 5 || k == 10) ? 0x3f800000u : 0u);
    return diff == 0;
}

XFORM_FN void xform_pos(const float* m, const float* p, float* o) {
    for (int r = 0; r < 3; r++) o[r] = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
}

// The tail of every normal: t normalised when its squared length is positive and finite, else the
// rest normal n unchanged (morph.h shares it).
XFORM_FN void nrm_tail(const float* t, const float* n, float* o) {
    const float l2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    if (l2 > 0.0f && l2 <= F_MAX) {
        const float l = sqrtf(l2);
        for (int r = 0; r < 3; r++) o[r] = t[r] / l;
    } else {
        for (int r = 0; r < 3; r++) o[r] = n[r];
    }
}

XFORM_FN void xform_nrm(const float* N, const float* n, float* o) {
    float t[3];
    for (int r = 0; r < 3; r++) t[r] = (N[3 * r] * n[0] + N[3 * r + 1] * n[1]) + N[3 * r + 2] * n[2];
    nrm_tail(t, n, o);
}

// One vertex of an object (rec: its 21 floats).  pass: the vertex passes through -- object -1, or
// is_identity of the record -- and rec is not read.
XFORM_FN void xform_vertex(const float* rec, bool pass, const float* p, const float* n, float* po, float* no) {
    if (pass) {
        for (int r = 0; r < 3; r++) { po[r] = p[r]; no[r] = n[r]; }
        return;
    }
    xform_pos(rec, p, po);
    xform_nrm(rec + 12, n, no);
}

// What the reductions of an update see of one output vertex: the largest |coordinate| (a NaN never
// wins an fmaxf) and whether any coordinate is not finite (a NaN fails the comparison).
XFORM_FN float abs_max3(const float* p) { return fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2])); }
XFORM_FN bool finite3(const float* p) { return fabsf(p[0]) <= F_MAX && fabsf(p[1]) <= F_MAX && fabsf(p[2]) <= F_MAX; }

// The normal matrix of m's linear part A: its cofactor matrix (det(A) times the inverse transpose)
// in double, times the sign of det(A) so that a mirroring transform keeps normals on their side,
// rounded to float.  Host only: the device path and the host mirror both receive these 9 floats.
static inline void normal_matrix(const float* m, float* N) {
    double a[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r][c] = (double)m[4 * r + c];
    double co[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            co[r][c] = a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1];
        }
    const double det = a[0][0] * co[0][0] + a[0][1] * co[0][1] + a[0][2] * co[0][2];
    const double sg = det < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) N[3 * r + c] = (float)(sg * co[r][c]);
}

// The 21-float records of num_objects matrices (12 floats each).
static inline void make_records(const float* matrices, int32_t num_objects, float* rec) {
    for (int32_t k = 0; k < num_objects; k++) {
        memcpy(rec + (size_t)REC * k, matrices + 12 * (size_t)k, 12 * sizeof(float));
        normal_matrix(matrices + 12 * (size_t)k, rec + (size_t)REC * k + 12);
    }
}

}  // namespace mptxform

#undef XFORM_FN
#endif
