// refit.h -- the arithmetic of a BVH8 refit (mpt_update_vertices), shared verbatim by the
// kernels (refit.hip: k_refit_tris, k_refit_level) and the host loop (refit_host, behind
// mpt_bvh_refit_host), the way display.h and denoise.h are shared: compiled with
// -ffp-contract=off on both sides, so that the GPU and the CPU produce the same bytes.
//
// A refit keeps the tree (imask, meta, child_base, tri_base, the order of the records, the
// records' w lanes) and recomputes what follows from the positions.  Every step is exact:
//   record         A, B - A, C - A with the builder's fp32 subtractions
//   triangle box   min / max of the three vertices per axis, then lo - pad, hi + pad in fp32
//   leaf slot      union of its triangles' boxes; internal slot: the child node's exact box
//   node box       union of the non-empty slots; p = its lo
//   exponent       per axis the smallest e in [-126, 127] with 255 * 2^e >= hi - lo; byte e + 127
//   slot bounds    qlo = clamp(floor((lo - p) / 2^e), 0, 255), qhi = clamp(ceil((hi - p) / 2^e), 0, 255)
// The differences are differences of floats, taken in double with their rounding error kept
// (two_diff), so that the comparisons and the floor / ceil decide on the exact value; the scales
// are powers of two.  The exact node boxes are kept beside the nodes (6 floats each): a refit
// never reads de-quantised bytes, so repeated refits cannot inflate boxes.
#ifndef MPT_REFIT_H
#define MPT_REFIT_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bvh8.h"

#if defined(__HIPCC__)
#define REFIT_FN __host__ __device__ static inline
#else
#define REFIT_FN static inline
#endif

namespace mptrefit {

constexpr float BOX_EMPTY_LO = 3.4028234663852886e38f, BOX_EMPTY_HI = -3.4028234663852886e38f;

struct Box {
    float lo[3], hi[3];
};

REFIT_FN Box box_empty() {
    Box b;
    for (int a = 0; a < 3; a++) { b.lo[a] = BOX_EMPTY_LO; b.hi[a] = BOX_EMPTY_HI; }
    return b;
}
REFIT_FN void box_grow(Box& b, const Box& o) {
    for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], o.lo[a]); b.hi[a] = fmaxf(b.hi[a], o.hi[a]); }
}

// The record of a triangle (its w lanes untouched) and its padded box.
REFIT_FN Box refit_tri(const float* A, const float* B, const float* C, float pad, mpt::TriRec& tr) {
    tr.ax = A[0]; tr.ay = A[1]; tr.az = A[2];
    tr.e1x = B[0] - A[0]; tr.e1y = B[1] - A[1]; tr.e1z = B[2] - A[2];
    tr.e2x = C[0] - A[0]; tr.e2y = C[1] - A[1]; tr.e2z = C[2] - A[2];
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fminf(fminf(A[a], B[a]), C[a]) - pad;
        b.hi[a] = fmaxf(fmaxf(A[a], B[a]), C[a]) + pad;
    }
    return b;
}

// hi - lo of two floats: s the rounded double, err the rest (s + err is the exact difference).
REFIT_FN double two_diff(float hi, float lo, double* err) {
    const double a = (double)hi, c = -(double)lo;
    const double s = a + c;
    const double a1 = s - c, c1 = s - a1;
    *err = (a - a1) + (c - c1);
    return s;
}

// The smallest e in [-126, 127] with 255 * 2^e >= hi - lo (hi >= lo).
REFIT_FN int quant_exp_exact(float hi, float lo) {
    double err;
    const double s = two_diff(hi, lo, &err);
    if (!(s > 0.0)) return -126;
    uint64_t bits;
    memcpy(&bits, &s, 8);
    const int x = (int)((bits >> 52) & 0x7ff) - 1023;        // s = m * 2^x, 1 <= m < 2
    int e = x - 7;                                            // 255 * 2^(x - 7) = 1.9921875 * 2^x
    const double T = ldexp(255.0, e);
    if (s > T || (s == T && err > 0.0)) e++;
    return e < -126 ? -126 : (e > 127 ? 127 : e);
}

// floor / ceil of (v - p) / 2^e on the exact difference, clamped to a byte (v >= p).
REFIT_FN uint8_t quant_lo(float v, float p, int e) {
    double err;
    const double s = two_diff(v, p, &err);
    const double q = ldexp(s, -e);
    double f = floor(q);
    if (f == q && err < 0.0) f -= 1.0;
    f = fmin(fmax(f, 0.0), 255.0);
    return (uint8_t)(int)f;
}
REFIT_FN uint8_t quant_hi(float v, float p, int e) {
    double err;
    const double s = two_diff(v, p, &err);
    const double q = ldexp(s, -e);
    double f = ceil(q);
    if (f == q && err > 0.0) f += 1.0;
    f = fmin(fmax(f, 0.0), 255.0);
    return (uint8_t)(int)f;
}

// Slot kinds of a node.
REFIT_FN bool slot_internal(const mpt::Node8& n, int s) { return (n.imask >> s) & 1; }
REFIT_FN bool slot_empty(const mpt::Node8& n, int s) { return !slot_internal(n, s) && n.meta[s] == 0; }

}  // namespace mptrefit

namespace mpt {
// The host loop: records, exact node boxes (6 floats per node, lo then hi) and nodes of `bvh`
// refitted to `pos` (the records' prim lanes index `idx`, three vertex indices per primitive).
void refit_host(BVH8& bvh, const int32_t* idx, const float* pos, float pad, std::vector<float>& node_box);
// sum over nodes of the surface area of the exact boxes, in double, in node order
double node_box_area_sum(const float* node_box, size_t nodes);
}  // namespace mpt

#undef REFIT_FN
#endif
