// morph.h -- the arithmetic of morph targets (mpt_update_morph), shared verbatim by the kernel
// (morph.hip: k_morph) and the host loop (morph_host, behind mpt_morph_host), the way skin.h and
// xform.h are: compiled with -ffp-contract=off on both sides, so that the GPU and the CPU produce
// the same bytes.
//
// A morph is T >= 1 targets.  Both sides read it transposed BY VERTEX, in CSR form (to_csr below
// makes it from the caller's by-target form): row[V + 1] offsets; per entry the target index, a
// position delta (3 floats) and, when the morph has normal deltas, a normal delta (3 floats).  The
// entries of a vertex are in ascending target order.  A gather: a scatter with atomics would have
// no fixed order of additions.
//
// One vertex with rest position p, rest normal n and the weights w[0..T):
//   applied    the entries whose w[target] is not +0 / -0
//   pass       no applied entry: position and normal pass through byte for byte (p + 0*d would turn
//              a -0 into +0, renormalising would change a non-unit normal)
//   position   acc = p; per applied entry, in order: acc[r] = acc[r] + w*dp[r]   the product
//              rounded, then the sum; fp32, no fma
//   normal     with normal deltas: t = n; t[r] = t[r] + w*dn[r] in the same order; then
//              mptxform::nrm_tail(t, n): t / sqrtf((t0*t0 + t1*t1) + t2*t2) when that squared
//              length is positive and finite, else the rest normal.  Without normal deltas the
//              normal passes through.
#ifndef MPT_MORPH_H
#define MPT_MORPH_H

#include <vector>

#include "xform.h"

#if defined(__HIPCC__)
#define MORPH_FN __host__ __device__ static inline
#else
#define MORPH_FN static inline
#endif

namespace mptmorph {

// One vertex: its entries [b, e) of tgt / dp / dn (dn NULL: no normal deltas), the weights w (by
// target), rest position p and normal n into po / no.
MORPH_FN void morph_vertex(const int32_t* tgt, const float* dp, const float* dn, int32_t b, int32_t e, const float* w,
                           const float* p, const float* n, float* po, float* no) {
    float acc[3] = {p[0], p[1], p[2]};
    float t[3] = {n[0], n[1], n[2]};
    bool applied = false;
    for (int32_t k = b; k < e; k++) {
        const float wk = w[tgt[k]];
        if (wk != 0.0f) {
            applied = true;
            for (int r = 0; r < 3; r++) acc[r] = acc[r] + wk * dp[3 * (size_t)k + r];
            if (dn)
                for (int r = 0; r < 3; r++) t[r] = t[r] + wk * dn[3 * (size_t)k + r];
        }
    }
    for (int r = 0; r < 3; r++) po[r] = acc[r];   // (untouched without an applied entry)
    if (applied && dn) {
        mptxform::nrm_tail(t, n, no);
    } else {
        for (int r = 0; r < 3; r++) no[r] = n[r];
    }
}

// The per-vertex CSR.  dnrm is empty for a morph without normal deltas.
struct Csr {
    std::vector<int32_t> row, tgt;
    std::vector<float> dpos, dnrm;
};

// The caller's form, sparse by target -- target t owns the entries [off[t], off[t + 1]) of ids /
// dpos / dnrm (dnrm NULL: none), its vertex ids strictly ascending in [0, V) -- checked and
// transposed by a stable counting sort, so that a vertex's entries come in ascending target order.
// Returns NULL, or what is wrong with the input (out is then unspecified).
static inline const char* to_csr(int32_t T, const int32_t* off, const int32_t* ids, const float* dpos, const float* dnrm, int32_t V,
                                 Csr& out) {
    if (T < 1) return "morph: bad target count";
    if (off[0] != 0) return "morph: target offsets do not start at 0";
    for (int32_t t = 0; t < T; t++)
        if (off[t + 1] < off[t]) return "morph: target offsets decrease";
    const size_t N = (size_t)off[T];
    if (N > 0 && (!ids || !dpos)) return "NULL argument";
    out.row.assign((size_t)V + 1, 0);
    for (int32_t t = 0; t < T; t++)
        for (int32_t k = off[t]; k < off[t + 1]; k++) {
            if (ids[k] < 0 || ids[k] >= V) return "morph: vertex id out of range";
            if (k > off[t] && ids[k] <= ids[k - 1]) return "morph: vertex ids of a target not strictly ascending";
            out.row[(size_t)ids[k] + 1]++;
        }
    for (size_t k = 0; k < 3 * N; k++)
        if (!(fabsf(dpos[k]) <= mptxform::F_MAX) || (dnrm && !(fabsf(dnrm[k]) <= mptxform::F_MAX))) return "non-finite morph delta";
    for (size_t v = 0; v < (size_t)V; v++) out.row[v + 1] += out.row[v];   // (the sum is off[T]: no overflow)
    out.tgt.resize(N);
    out.dpos.resize(3 * N);
    out.dnrm.resize(dnrm ? 3 * N : 0);
    std::vector<int32_t> at(out.row.begin(), out.row.end() - 1);
    for (int32_t t = 0; t < T; t++)
        for (int32_t k = off[t]; k < off[t + 1]; k++) {
            const size_t d = (size_t)at[ids[k]]++;
            out.tgt[d] = t;
            memcpy(&out.dpos[3 * d], dpos + 3 * (size_t)k, 3 * sizeof(float));
            if (dnrm) memcpy(&out.dnrm[3 * d], dnrm + 3 * (size_t)k, 3 * sizeof(float));
        }
    return nullptr;
}

}  // namespace mptmorph

#undef MORPH_FN
#endif
