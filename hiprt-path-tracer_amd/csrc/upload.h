// upload.h -- the per-primitive passes of mpt_upload_scene_mode (upload.hip; DESIGN.md §2 "Uploads
// with a build mode"): what mpt_upload_scene does in host loops over its host tree, done on the
// device before the trees exist, so that the build (lbvh.hip) writes the records' flag lanes itself.
//
// The host evaluates two predicates per material (mpt_api.cpp: upload_alpha_flags' and
// build_light_bvh_impl's) into one word per material, MF_* below; everything per primitive follows
// from that word, the material's class (mat_tex, k_resolve_materials) and mat_idx:
//   flag words   two per scene primitive, as emit_node (lbvh.h) reads them: word 0 the material's
//                alpha flag (TriRec::pad0), word 1 its class under a mask (TriRec::pad1)
//   light list   the primitives whose material can emit, ascending by primitive index: a mark per
//                primitive, an exclusive scan (scan_u64), a scatter
#ifndef MPT_UPLOAD_H
#define MPT_UPLOAD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpt {

enum : uint32_t {
    MF_ALPHA = 1u,   // the alpha test can reject a hit on the material (TriRec::pad0 = 1)
    MF_LIT = 2u,     // the material's emission can be non-black (the light-hit BVH's set)
};

// flags[2 i], flags[2 i + 1] for every primitive i < n: (mat_flags[m] & MF_ALPHA) != 0 and
// mat_tex[m] & class_keep of its material m = mat_idx[i] (zeros for an index outside [0, n_mats))
hipError_t launch_prim_flags(const int32_t* mat_idx, int n, const uint32_t* mat_flags, const int32_t* mat_tex, int n_mats,
                             int32_t class_keep, uint32_t* flags, hipStream_t st);
// words[i] = 1 where primitive i's material has MF_LIT, else 0 (i < n): the scan's input
hipError_t launch_light_mark(const int32_t* mat_idx, int n, const uint32_t* mat_flags, int n_mats, uint64_t* words, hipStream_t st);
// scanned: the exclusive scan of launch_light_mark's words.  out[scanned[i]] = i for every marked
// primitive whose position is below cap (the scan's total): ascending by primitive index
hipError_t launch_light_scatter(const int32_t* mat_idx, int n, const uint32_t* mat_flags, int n_mats, const uint64_t* scanned,
                                int32_t* out, int cap, hipStream_t st);

}  // namespace mpt

#endif
