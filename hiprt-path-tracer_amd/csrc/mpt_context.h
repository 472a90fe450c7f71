// mpt_context.h -- private to the library's host side: the context and what the translation units
// that work on it share.  mpt_api.cpp owns the context's life, the scene upload and rebuild and the
// render path; mpt_geometry.cpp owns the geometry updates.  The feature headers
// (refit.h, xform.h, skin.h, morph.h, anim.h, normals.h, temporal.h) do not include this one: their
// host halves build without the library (tests/cpp/*_host_main.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "mpt_internal.h"

using namespace mpt;   // (MptContext is the C ABI's, outside the namespace, and names mpt_internal.h's types)

namespace mpt {

int fail(int code, const std::string& msg);   // mpt_api.cpp: sets mpt_last_error, returns code

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return mpt::fail(MPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Status of a failed allocation / memset: MPT_ERR_OUT_OF_MEMORY for hipErrorOutOfMemory.
// Clears HIP's last error so that a later launch check does not report it again.
inline int alloc_fail(hipError_t e, const std::string& what) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? MPT_ERR_OUT_OF_MEMORY : MPT_ERR_HIP, what + ": " + hipGetErrorString(e));
}

// Device buffer owned by a context (freed by the context's destructor at the latest).
template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        if (count == n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const T* h, size_t count, hipStream_t s) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
    // The commit of "build into temporaries, take them when all are there": from's buffer adopted, from left empty.
    void take(DBuf& from) { release(); p = from.p; n = from.n; from.p = nullptr; from.n = 0; }
    void swap(DBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }   // both stay live: a buffer and its staging twin
};

template <typename... B>
void release_all(B&... b) { (b.release(), ...); }

// timing events per frame: one pair per timed launch, 10 per bounce (path, any-hit and two
// light-hit traversals, split, plain and generic shade, miss, compact, resolve) for up to 65
// bounces (validate_frame), + camera, ReSTIR, accumulate
// + the ReSTIR DI kernels (G-buffer, presampling, initial, temporal / spatiotemporal, 4 spatial)
// samples per batched ReSTIR DI wavefront (<= 50 timed scopes each): a partitioned context's
// band is 1/N of the frame, so its later bounces need up to 128 samples to reach the
// single-GPU wavefront size (MPT_RESTIR_MAX_BATCH lowers it, A/B)
constexpr int RESTIR_MAX_BATCH = 128;
// x2: the two halves of an overlapped batch
constexpr int EV_POOL = 2 * 2 * ((10 * 65 + 3 + 8) > 50 * RESTIR_MAX_BATCH ? (10 * 65 + 3 + 8) : 50 * RESTIR_MAX_BATCH);

}  // namespace mpt

struct MptContext {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // overlapped batches (MPT_OVERLAP at mpt_create): the second half of a sample batch runs
    // on stream2, one pipeline stage behind the first, so that shading waves of one half and
    // traversal waves of the other share the CUs
    // MPT_OVERLAP: a path-tracing batch's two halves on two streams: 1 always, 0
    // never, -1 (default) for wavefronts of at most OVERLAP_AUTO_PATHS paths -- a rank's share of
    // a split frame at the driver's 20 samples, where the launch tails are a larger part of each
    // launch (one rank of 2 / 4 / 8: -2.3 / -2.7 / -3.8 %); a whole 1080p frame's 33-41 M paths
    // keep one stream (+1.2 % only, and its per-kernel times stay unshared)
    int overlap = -1;
    hipStream_t stream2 = nullptr;
    // the third and fourth row parts of a one-sample frame (MptContext::pix_parts): streams,
    // traversal spill areas, join events
    hipStream_t streamx[2] = {nullptr, nullptr};
    hipEvent_t ev_joinx[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_first = nullptr, ev_acc = nullptr, ev_join = nullptr;
    // Overlapped ReSTIR DI batches (MPT_RESTIR_OVERLAP, default on): a batch's per-sample chain
    // (G-buffer, reuse passes, halo exchanges: many small dependent launches) runs on the
    // context's stream while the previous batch's shared later-bounce wavefront runs on stream2.
    // The two batches in flight use the two halves of the path state (restir_half), each with its
    // own counters; ev_half[h] marks the end of the last wavefront that used half h.
    int restir_overlap = 1;
    bool restir_overlap_ok = false;       // prepare_batch found room for both halves
    int restir_half = 0;
    hipEvent_t ev_chain = nullptr, ev_half[2] = {nullptr, nullptr}, ev_wave_join = nullptr;
    bool ev_half_used[2] = {false, false};
    bool wave_pending = false;            // a wavefront on stream2 not yet joined into the stream
    // One-sample launch sets as a HIP graph (MPT_GRAPHS, default on): mpt_render_frame's ~50
    // launches of a path-tracing sample captured once and replayed while the frame differs only in
    // what the kernels read from it (seeds, sample number, cameras, status flags); the graph reads
    // its frame from the extra ring slot d_frames[FRAME_RING].  Keyed by those frame fields that
    // steer the host's launch sequence and by the kernels' by-value arguments (buffer pointers).
    int graphs = 0;   // MPT_GRAPHS=1: one-sample launch sets replayed from a captured HIP graph (no gain measured, r05e)
    // one-sample frames of a whole-frame context as row parts on their own streams (MPT_PIX_PARTS:
    // 0 / 1 off, 2 .. PIX_PARTS_MAX parts)
    int pix_parts = 3;   // batch-1 C3 6.09 -> 5.44 (2 parts) -> 5.29 ms/spp (3); 4 parts 6.76 (past GPU_MAX_HW_QUEUES), r06d
    // staged ReSTIR DI stages: the generic-class kernel on a side stream beside the plain one
    // (MPT_RESTIR_SIDE: 1 for partitions of at most 2^20 pixels, 2 always, 0 never)
    int restir_side = 1;
    hipEvent_t ev_side[2] = {nullptr, nullptr};
    // trace-ahead (MPT_TRACE_AHEAD): the next bounce's path traversal beside this bounce's NEE
    // traversals and resolve, on streamx[1]
    int trace_ahead = 1;
    int ovl_ahead = 1;   // MPT_OVERLAP_AHEAD: trace-ahead in both halves of an overlapped batch
    hipEvent_t ev_ahead[2] = {nullptr, nullptr};
    hipEvent_t ev_ahead2[2] = {nullptr, nullptr};   // (the second half of an overlapped batch)
    uint32_t ahead_launches = 0;   // MptStats::trace_ahead_launches
    uint32_t pipelined_batches = 0;   // MptStats::pipelined_batches
    hipGraphExec_t graph_exec = nullptr;
    std::vector<uint8_t> graph_key;
    uint32_t graph_launches = 0;
    uint32_t graph_captures = 0, graph_replays = 0;   // since mpt_enable_stats (MptStats)
    uint32_t overlapped_batches = 0;
    int num_cus = 256;
    int grid = 1024;
    // scene
    bool has_scene = false;
    BVH8 bvh;
    DBuf<Node8> nodes;
    DBuf<TriRec> tris;
    DBuf<float4> tri_attr;               // 5 per triangle (launch_tri_attr)
    DBuf<float> srgb;                    // 256-entry sRGB decode table (launch_srgb_table)
    // light-hit BVH (k_trace TM_NEE_LIGHT): the triangles whose emission can be non-black
    BVH8 bvh_light;
    DBuf<Node8> nodes_light;
    DBuf<TriRec> tris_light;
    std::vector<int32_t> h_light_prims;
    std::vector<int32_t> h_idx;           // host copies for rebuilding the light BVH on material edits
    std::vector<float> h_pos;
    float box_pad = 0.0f;
    // mpt_update_vertices (refit.hip): the exact node boxes of both trees (6 floats per node) and
    // the records' padded boxes (scratch); the area sums of the builders' node boxes; whether the
    // host copies bvh.tris, bvh_light.tris and h_pos still hold the positions before an update
    // (refresh_mirrors); which vertices the triangles use (the pad is taken over these)
    DBuf<float> nbox, nbox_light, tbox;
    double area0 = 0.0, area0_light = 0.0;
    bool mirrors_stale = false;
    // mpt_rebuild_bvh (lbvh.hip) swapped in trees built on the device: the host copies' nodes,
    // records and node boxes follow with the next refresh_mirrors (level_begin and depth at once)
    bool topology_stale = false;
    std::vector<uint8_t> h_vert_used;
    // per-object motion (mpt_set_objects, xform.hip): the object id of every vertex (-1: static),
    // the rest pose captured when the objects were set, the staging arrays a transform writes
    // before they are swapped in for pos / nrm, the objects' 21-float records, h_vert_used on the
    // device (mpt_update_vertices_device reads it as well) and the two reduction words
    int num_objects = -1;                 // -1: no objects set
    DBuf<int32_t> vert_obj;
    DBuf<float> rest_pos, rest_nrm, stage_pos, stage_nrm, xf_recs;
    DBuf<uint8_t> vert_used;
    DBuf<uint32_t> xf_red;
    // skinning (mpt_set_skin, skin.hip): four joint indices and weights per vertex and the joints'
    // 16-word records.  A skin and an object table exclude each other and share rest_pos /
    // rest_nrm / stage_pos / stage_nrm: setting one drops the other.
    int num_joints = -1;                  // -1: no skin set
    DBuf<int32_t> skin_joints;
    DBuf<float> skin_weights;
    DBuf<float4> skin_recs;
    // morph targets (mpt_set_morph, morph.hip): the per-vertex CSR of morph.h.  A morph composes
    // with a skin and excludes an object table; morph and skin share the rest pose, captured by
    // whichever is set first and kept until both are gone.  Retained for the call that brings only
    // the other half: the last accepted weights (morph_w, padded to a multiple of four floats) and
    // the last accepted palette (skin_recs; skin_posed false: no skin step).  New weights and
    // records go to the *_stage buffers and are swapped in when the call is accepted.
    int num_targets = -1;                 // -1: no morph set
    DBuf<int32_t> morph_row, morph_tgt;
    DBuf<float> morph_dpos, morph_dnrm, morph_w, morph_w_stage;
    bool skin_posed = false;
    DBuf<float4> skin_recs_stage;
    // an animation clip (mpt_set_animation, anim.hip): the packed tables with their scratch on the
    // device (anim: counts and section offsets; its blob is not kept), and the kernel's flag word.
    // It drives the skin's joints, the morph's targets or both, and goes when either goes.
    bool has_anim = false;
    AnimPacked anim;
    DBuf<unsigned char> anim_blob;
    DBuf<uint32_t> anim_flag;
    int refit_host_loop = 0;              // test hook (MPT_REFIT_HOST): the refit by the host loop of refit.h
    int light_bvh = 1;                    // MPT_LIGHT_BVH at mpt_create: 0 = one closest-hit traversal per light-hit query
    bool light_bvh_ok = false;            // the light BVH matches the materials (else: the exact closest-hit path)
    int light_bvh_max_stack = 1 << 30;    // test hook (MPT_LIGHT_BVH_MAX_STACK): a lower traversal-stack limit
    DBuf<int32_t> idx, mat_idx, mat_prio, emissive, tex_dims;
    DBuf<float> pos, nrm, uv;
    DBuf<uint8_t> has_n, tex;
    DBuf<uint64_t> tex_off;
    DBuf<MptMaterial> mats;
    DBuf<MptMaterial> mats_res;   // untextured intersection-time resolution per material
    DBuf<int32_t> mat_tex;
    DBuf<float4> em_tab;
    bool any_tex = false;
    bool any_glass = false;   // a material of the glass class (MT_GLASS): k_shade<GLASS> is launched
    double tex_tri_frac = 0.0;            // triangles with a textured material / all (resolve_materials)
    int mat_private = -1;                 // MPT_MAT_PRIVATE: 1 / 0 force k_shade's MATP, -1 by tex_tri_frac
    // material-class shading (k_split / k_shade): 1 on (default), 0 off, 2 on with every
    // plain vertex deferred to the generic kernel (test hook); MPT_SHADE_CLASSES at mpt_create
    int shade_classes = 1;
    int restir_staged = 1;                // ReSTIR DI reuse passes staged around their rays (MPT_RESTIR_STAGED)
    int restir_mono_reuse = 0;            // MPT_RESTIR_MONO_REUSE: the reuse passes monolithic, the initial pass staged
    int restir_batch = 1;                 // ReSTIR DI samples batched after bounce 0 (MPT_RESTIR_BATCH)
    int adaptive_batch = 1;               // adaptive samples batched, gated in k_accumulate (MPT_ADAPTIVE_BATCH)
    int restir_max_batch = RESTIR_MAX_BATCH;   // MPT_RESTIR_MAX_BATCH
    int shade_glass = 1;                  // glass-class shading kernel (MPT_SHADE_GLASS)
    int shade_split = 0;                  // plain-class shading stages (MPT_SHADE_SPLIT, LaunchCfg::shade_split)
    int shade_texmetal = 1;               // MT_TEXMETAL materials through the plain list (MPT_SHADE_TEXMETAL)
    std::vector<MptMaterial> h_mats;
    std::vector<int32_t> h_mat_idx;       // per triangle (alpha flags of the triangle records)
    std::vector<uint8_t> h_tex_alpha;     // per texture: some texel has alpha < 255
    int n_tex = 0;
    // luts / envmap
    DBuf<float> lut_conductor, lut_glossy, lut_glass, lut_glass_inv, lut_thin, lut_sheen;
    DBuf<float4> env;
    DBuf<int2> alias;
    DBuf<float4> env_rich;                // alias entries with their radiance texels (launch_env_rich)
    DBuf<float> env_cdf;
    float env_cdf_sum = 0.0f;
    int env_w = 0, env_h = 0;
    float env_sum = 0.0f;
    // paths
    int res_x = 0, res_y = 0, band_h = 1, band_i = 0, band_c = 1, n_slots = 0;   // n_slots = pixels of the partition
    int batch_cap = 0;      // samples per pixel the path state is sized for (mpt_render_frames)
    int batch = 1;          // samples of the launch being set up
    DBuf<float4> ray_o, ray_d, hit, thr, col, alb, nrmv, nq_o, nq_d, nhit, s_gn;
    DBuf<uint8_t> hit_inside, hit_cls, occ, qmask;
    DBuf<uint32_t> rng, spill, spill2, spillx[2];
    DBuf<uint2> seeds;
    DBuf<uint4> vsA, vsB;
    DBuf<int32_t> q0, q1, qh, qm, qf, nq_light, counters, nq_tgt, fetch_raw;
    DBuf<float4> nthr, na, nb, ndir, nris, ne1, ne2;   // NEE record planes (mpt_internal.h)
    // bounce pipeline (LaunchCfg::pipe_alt): the odd bounces' NEE planes, staged queries and their
    // lists, shaded lists, and both parities' col additions (MPT_PIPELINE)
    DBuf<float4> nthr2, na2, nb2, ndir2, nris2, ne12, ne22, nq_o2, nq_d2, ce, ce2;
    DBuf<int32_t> nq_tgt2, qh2, qf2;
    int pipeline = 1;
    size_t pipe_n = 0;
    hipEvent_t ev_nee[4] = {nullptr, nullptr, nullptr, nullptr};   // fork / join per NEE stream
    int pix_pipe = 1;   // MPT_PIX_PIPE: a one-sample frame as 2 row parts, each pipelined
    DBuf<float> fb_color, fb_albedo, fb_normal;
    DBuf<int32_t> as_count, as_conv;
    DBuf<float> as_sqlum;
    DBuf<uint8_t> active;
    DBuf<uint32_t> status;
    // ReSTIR DI (allocated on the first LSS_RESTIR_DI frame)
    DBuf<float4> gb_pos, gb_sn, gb_gn, gb_view, pgb_pos, pgb_sn, pgb_gn, pgb_view;
    DBuf<int4> gb_meta, pgb_meta;
    DBuf<uint4> gb_vsA, gb_vsB, pgb_vsA, pgb_vsB;
    DBuf<MptMaterial> gb_mat, pgb_mat;
    DBuf<float4> gb_cs, pgb_cs;           // compact surface records (4 float4 per pixel)
    DBuf<float4> rs_init, rs_sp1, rs_sp2, rs_plights;
    DBuf<float4> rs_keep;                 // batched ReSTIR DI: the final reservoirs of each sample of a batch
    DBuf<int32_t> rs_conv;
    // staged ReSTIR DI passes (DevPaths::rq_*): RS_RPP ray positions per pixel slot
    DBuf<float4> rq_o, rq_d, rq_rec;
    DBuf<uint32_t> rq_key;
    DBuf<uint8_t> rq_occ;
    DBuf<int32_t> rq_list, rq_items;
    DBuf<int4> rq_meta;
    // chunked ReSTIR DI initial candidates (launch_frames_restir, LaunchCfg::ci_planes): the
    // G-buffer, initial reservoirs and presampled lights of up to restir_chunk samples
    int restir_chunk = -1;                // MPT_RESTIR_CHUNK: samples per chunk (-1: by the band's pixels)
    int ci_chunk = 1;                     // the chunk the planes below are sized for
    DBuf<float4> ci_pos, ci_sn, ci_gn, ci_view, ci_cs, ci_rs, ci_pl;
    DBuf<int4> ci_meta;
    DBuf<uint4> ci_vsA, ci_vsB;
    DBuf<MptMaterial> ci_mat;
    DevPaths ci_dp{};
    int restir_out_sp2 = 0;
    MptHaloExchangeFn halo_fn = nullptr;   // ReSTIR DI across a row partition
    void* halo_user = nullptr;
    int halo_prev = 0;                     // halo agreed in the previous frame
    int32_t* h_reproj = nullptr;           // pinned readback of the reprojection offset
    DBuf<MptMaterial> mat_slot;
    // extended light sampling (ensure_ext): x_per entries per path slot of the current batch
    DBuf<float4> xq_o, xq_d, xq_hit, xrec;
    DBuf<uint8_t> xq_occ, xq_flag;
    DBuf<int32_t> xl_any, xl_cl, xl_light;
    int x_per = 0, x_iter = 0;
    DBuf<uint64_t> stats;
    DBuf<uint64_t> ray_counts;
    // frames
    MptFrame* h_frames = nullptr;   // pinned ring
    MptFrame* d_frames = nullptr;
    int frame_slot = 0;
    // stats
    bool timing = false;
    bool instrumented = false;
    // two event pools used by alternate frames: a pool is read back when it is
    // reused two frames later, so collecting timings never stalls the stream
    hipEvent_t ev[2][EV_POOL];
    int ev_mode[2][EV_POOL / 2];
    hipEvent_t ev_frame[2][2];
    int ev_used[2] = {0, 0};
    bool ev_pending[2] = {false, false};
    uint32_t frames_submitted = 0;
    uint32_t trace_launches = 0;
    uint32_t frames = 0;
    double stage_ms[KT_COUNT] = {};
    uint32_t stage_launches[KT_COUNT] = {};
    double frame_ms = 0.0;
    // raw traces
    DBuf<float4> raw_o, raw_d, raw_hit;
    DBuf<uint8_t> raw_occ;
    // one process per GPU (mpt_comm_*): the RCCL communicator of the frame partition and the
    // padded staging rows of mpt_comm_gather (send: this rank's rows, recv: every rank's, root)
    void* comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    // the library's own halo exchange (mpt_set_halo_native): 1 RCCL send / receive over the
    // communicator, 2 the one-GPU rehearsal (the bytes moved locally, no peers)
    int halo_native = 0;
    DBuf<uint8_t> halo_scratch;           // rehearsal: where the bytes go
    DBuf<int32_t> halo_agree;             // device word of the halo agreement (ncclAllReduce max)
    std::vector<MptHaloOp> halo_plan_ops; // the exchange point's operations (native_halo)
    uint64_t halo_exchanges = 0, halo_agreements = 0, halo_bytes_sent = 0, halo_bytes_recv = 0;   // MptStats
    uint32_t restir_overlapped_batches = 0;
    // upper bound of pixel_sample_count over the partition's pixels (restir_gate_static): a reset
    // frame restarts it, every frame with the adaptive buffers adds at most one sample; unknown
    // (large) until a reset frame has been launched
    int as_bound = 1 << 30;
    // a converged count may be set since the last reset (note_conv_set): by a stop-noise frame, or
    // by an adaptive frame whose bound had passed that frame's minimum.  While it is set, as_bound
    // at most an adaptive frame's minimum no longer means that no pixel has converged
    // (restir_gate_static); cleared with the converged counts (a reset frame, a new partition)
    bool as_conv_set = false;
    // the last batch reset the adaptive buffers in its k_accumulate (which an overlapped next batch
    // would run beside): the next ReSTIR DI batch does not overlap it
    bool as_reset_pending = false;
    DBuf<uint8_t> comm_send, comm_recv;
    // mpt_display: a frame has been rendered into the current partition's buffers, whether the
    // last one had the adaptive-sampling buffers (has_adaptive), the staging of a host
    // destination and of a host second buffer
    bool rendered = false, last_adaptive = false;
    DBuf<uint32_t> disp_out;
    DBuf<float> disp_second;
    // mpt_denoise / mpt_denoise_device: the working planes (denoise.hip), the kept result, the
    // sample count it was made at (0: nothing denoised since the last resize)
    DBuf<float> den_scratch, den_out;
    int den_samples = 0;
    // recomputed normals (mpt_set_normals, normals.hip): every vertex's group id, the by-group CSR
    // of normals.h over the scene's indices, the groups' flip bytes and the face vectors' scratch
    // array.  Independent of objects, skin, morph and animation; a scene upload drops it.
    int num_groups = -1;                  // -1: normals are not recomputed
    DBuf<int32_t> nrm_group, nrm_row, nrm_tri;
    DBuf<uint8_t> nrm_flip;
    DBuf<float4> nrm_face;
    // temporal accumulation (mpt_set_temporal, temporal.hip): the pose at the last temporal call
    // (prev_pos, written by the head hook of the first geometry update after it: tmp_dirty), the
    // history's two ping-pong plane pairs (tmp_cur: the pair the last call wrote; tmp_valid: it
    // holds a frame of tmp_w x tmp_h), the last call's visibility, motion and output planes and
    // the camera it was given
    bool temporal = false, tmp_dirty = false, tmp_valid = false;
    bool tmp_stats = false;               // MPT_TEMPORAL_STATS at mpt_create: per-launch times of every call, printed
    int tmp_cur = 0, tmp_w = 0, tmp_h = 0;
    DBuf<float> prev_pos, tmp_out;
    DBuf<float4> tmp_ha[2], tmp_hb[2], tmp_vis, tmp_motion;
    MptCamera tmp_prev_cam{};
};

namespace mpt {

// mpt_api.cpp
DevScene dev_scene(MptContext* c);
hipError_t drain(MptContext* c);
int refresh_mirrors(MptContext* c);

// mpt_geometry.cpp: what a scene upload, mpt_resize and mpt_set_temporal free
void drop_objects(MptContext* c);
void drop_normals(MptContext* c);
void drop_temporal_history(MptContext* c);
void drop_temporal_pose(MptContext* c);

// The refusals every call on a scene starts with.
inline int need_scene(const MptContext* c) {
    if (!c) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->has_scene) return fail(MPT_ERR_NO_SCENE, "no scene uploaded");
    return MPT_OK;
}

// A HIP error once an update or a rebuild has begun: the scene is dropped (half updated: the caller uploads again).
inline int update_fail(MptContext* c, hipError_t e, const char* who) {
    (void)hipGetLastError();
    c->has_scene = false;
    return fail(MPT_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// The light-hit tree is there: a scene without lit triangles has none.
inline bool has_light_tree(const MptContext* c) { return c->nodes_light.p && c->tris_light.p && !c->h_light_prims.empty(); }

}  // namespace mpt
