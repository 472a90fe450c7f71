// mpt_geometry.cpp -- the geometry updates of the C ABI (include/mpt.h): new vertices from the
// host or the device, object transforms, skin, morph targets, animation clips and recomputed
// normals, each ending in the refit of both BVH8s.  It touches the renderer (mpt_api.cpp) only
// through drain, dev_scene, refresh_mirrors and the context fields it owns.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "morph.h"
#include "mpt_context.h"
#include "normals.h"
#include "refit.h"

namespace mpt {

// The temporal accumulation's history and planes freed (the switch stays): by mpt_resize and, with
// the previous pose, by a scene upload and mpt_set_temporal(0).
void drop_temporal_history(MptContext* c) {
    c->tmp_valid = false;
    c->tmp_cur = 0;
    c->tmp_w = c->tmp_h = 0;
    release_all(c->tmp_ha[0], c->tmp_ha[1], c->tmp_hb[0], c->tmp_hb[1], c->tmp_vis, c->tmp_motion, c->tmp_out);
}
void drop_temporal_pose(MptContext* c) {
    c->tmp_dirty = false;
    c->prev_pos.release();
}

// The state of mpt_set_normals freed: by mpt_set_normals(NULL) or a scene upload.
void drop_normals(MptContext* c) {
    c->num_groups = -1;
    release_all(c->nrm_group, c->nrm_row, c->nrm_tri, c->nrm_flip, c->nrm_face);
}

// The animation freed: with the skin or the morph it drives, or by mpt_set_animation(NULL).
static void drop_animation(MptContext* c) {
    c->has_anim = false;
    c->anim = AnimPacked();
    release_all(c->anim_blob, c->anim_flag);
}

// The skin's tables and its retained palette freed (the rest pose stays).
static void drop_skin_tables(MptContext* c) {
    drop_animation(c);
    c->num_joints = -1;
    c->skin_posed = false;
    release_all(c->skin_joints, c->skin_weights, c->skin_recs, c->skin_recs_stage);
}

// The morph's tables and its retained weights freed (the rest pose stays).
static void drop_morph_tables(MptContext* c) {
    drop_animation(c);
    c->num_targets = -1;
    release_all(c->morph_row, c->morph_tgt, c->morph_dpos, c->morph_dnrm, c->morph_w, c->morph_w_stage);
}

// The object table of mpt_set_objects, or the skin of mpt_set_skin and the morph of mpt_set_morph
// (a table excludes the other two), the rest pose and the staging arrays freed.
void drop_objects(MptContext* c) {
    c->num_objects = -1;
    release_all(c->vert_obj, c->rest_pos, c->rest_nrm, c->stage_pos, c->stage_nrm, c->xf_recs);
    drop_skin_tables(c);
    drop_morph_tables(c);
}

}  // namespace mpt

namespace {

// The head hook of every geometry update, before it touches pos (mpt_set_temporal): the first
// update since the last temporal call copies pos to prev_pos on the stream; later ones leave the
// older pose there.  Off: one branch.  MPT_OK, or the refusal the update returns.
int temporal_snapshot(MptContext* c) {
    if (!c->temporal || c->tmp_dirty) return MPT_OK;
    hipError_t e = c->prev_pos.alloc(c->pos.n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->prev_pos.p, c->pos.p, c->pos.n * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) { c->tmp_dirty = true; return MPT_OK; }
    (void)hipGetLastError();
    c->prev_pos.release();
    return alloc_fail(e, "temporal: previous pose");
}

// The switches below are read from the environment at the call, never cached: tools/*_time.py flip
// them between calls in one process.  Unset reads as "".
const char* env(const char* name) {
    const char* e = std::getenv(name);
    return e ? e : "";
}

// Which of normals.hip's two structures recomputes the normals: the two kernels by default, by the
// measurement of DESIGN.md §4; MPT_NORMALS_FUSED=1 in the environment at the call, the one kernel
// (tools/normals_time.py measures both)
bool normals_fused() { return std::atoi(env("MPT_NORMALS_FUSED")) == 1; }

// vertices per lane of the xform kernels: 4 (MPT_XFORM_GROUP=1 in the environment, read at the
// call: dword accesses, the same bytes -- tools/xform_time.py measures both)
int xform_group() { return std::atoi(env("MPT_XFORM_GROUP")) == 1 ? 1 : 4; }

// the same for k_skin (MPT_SKIN_GROUP=1), and whether it stages a palette that fits in LDS
// (MPT_SKIN_LDS=0: always the gather through the cache) -- tools/skin_time.py measures all four
int skin_group() { return std::atoi(env("MPT_SKIN_GROUP")) == 1 ? 1 : 4; }
bool skin_lds() { return std::strcmp(env("MPT_SKIN_LDS"), "0") != 0; }

// k_morph takes ONE vertex per lane by default: a lane walks its vertices' entries one after the
// other, and with four vertices that serial walk costs more than the 16-byte accesses save
// (339 against 1056 us on the dense 4-target city).  MPT_MORPH_GROUP=4 selects four,
// MPT_MORPH_LDS=0 the gather through the cache -- tools/morph_time.py measures all four
int morph_group() { return std::atoi(env("MPT_MORPH_GROUP")) == 4 ? 4 : 1; }
bool morph_lds() { return std::strcmp(env("MPT_MORPH_LDS"), "0") != 0; }

// k_anim keeps the world matrices in LDS when they fit (MPT_ANIM_LDS=0: always in memory) --
// tools/anim_time.py measures both
bool anim_lds() { return std::strcmp(env("MPT_ANIM_LDS"), "0") != 0; }

// The box pad of a pose whose largest coordinate in use is m (scene_box_pad's formula).
float box_pad_for(float m) { return std::ldexp(std::max(m, 1.0f), -20); }

// A caller's vertex count is the scene's.
bool count_fits(const MptContext* c, int32_t num_vertices) { return num_vertices > 0 && 3 * (size_t)num_vertices == c->pos.n; }

// The tail of every geometry update, once pos / nrm hold the new arrays on the device: the refit
// of both trees and the tables derived from the positions.  host_v: the same positions on the host
// for the MPT_REFIT_HOST test hook (NULL: always the kernels -- mpt_update_transforms and
// mpt_update_vertices_device have no host array).
hipError_t refit_and_tables(MptContext* c, float pad, const float* host_v) {
#define UV(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
    hipStream_t st = c->stream;
    const float* v = host_v;
    const bool light = has_light_tree(c);
    UV(c->nbox.alloc(6 * c->nodes.n));
    if (light) UV(c->nbox_light.alloc(6 * c->nodes_light.n));
    if (c->refit_host_loop && v) {
        // (the host copies' w lanes are always current; their positions are rewritten here; after
        // a rebuild on the device the copies first take the new trees)
        if (c->topology_stale && refresh_mirrors(c) != MPT_OK) return hipErrorUnknown;
        std::vector<float> hb;
        auto tree = [&](BVH8& h, DBuf<Node8>& dn, DBuf<TriRec>& dt, DBuf<float>& db) -> hipError_t {
            refit_host(h, c->h_idx.data(), v, pad, hb);
            UV(hipMemcpyAsync(dn.p, h.nodes.data(), dn.n * sizeof(Node8), hipMemcpyHostToDevice, st));
            UV(hipMemcpyAsync(dt.p, h.tris.data(), dt.n * sizeof(TriRec), hipMemcpyHostToDevice, st));
            UV(hipMemcpyAsync(db.p, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice, st));
            return hipStreamSynchronize(st);
        };
        UV(tree(c->bvh, c->nodes, c->tris, c->nbox));
        if (light) UV(tree(c->bvh_light, c->nodes_light, c->tris_light, c->nbox_light));
        c->h_pos.assign(v, v + c->pos.n);
        c->mirrors_stale = false;
    } else {
        UV(c->tbox.alloc(6 * std::max(c->tris.n, light ? c->tris_light.n : (size_t)0)));
        c->mirrors_stale = true;
        UV(launch_refit_tris(c->tris.p, (int)c->tris.n, c->idx.p, c->pos.p, pad, c->tbox.p, st));
        UV(launch_refit_levels(c->nodes.p, c->nbox.p, c->tbox.p, c->bvh.level_begin.data(), c->bvh.depth, st));
        if (light) {   // the records hold scene primitive ids: the same path; the scene's pad
            UV(launch_refit_tris(c->tris_light.p, (int)c->tris_light.n, c->idx.p, c->pos.p, pad, c->tbox.p, st));
            UV(launch_refit_levels(c->nodes_light.p, c->nbox_light.p, c->tbox.p, c->bvh_light.level_begin.data(),
                                   c->bvh_light.depth, st));
        }
    }
    // recomputed normals (mpt_set_normals): pos is read, nrm is rewritten in place for the grouped
    // vertices, on the stream, before the attribute records bake the normals in
    if (c->num_groups >= 0) {
        NormalsLaunch a{};
        a.idx = c->idx.p; a.pos = c->pos.p; a.num_tris = (int)(c->idx.n / 3);
        a.group = c->nrm_group.p; a.has_n = c->has_n.p; a.row = c->nrm_row.p; a.tri = c->nrm_tri.p; a.flip = c->nrm_flip.p;
        a.n = (int)c->nrm_group.n; a.nrm = c->nrm.p;
        const bool fused = normals_fused();
        if (!fused) UV(c->nrm_face.alloc(std::max(c->idx.n / 3, (size_t)1)));
        a.face = c->nrm_face.p;
        UV(launch_normals(a, fused, st));
    }
    UV(launch_tri_attr(dev_scene(c), c->tri_attr.p, st));
    // the emissive-triangle table holds positions (the materials' resolution comes out as it was)
    UV(launch_resolve_materials(dev_scene(c), c->mats_res.p, c->mat_tex.p, (int)c->h_mats.size(), c->em_tab.p, st));
    return hipStreamSynchronize(st);
#undef UV
}

// The end of every geometry update: e is what the device side returned.  On success the report
// (a download of the exact node boxes, only when asked for); on a HIP error the scene is dropped.
int finish_update(MptContext* c, hipError_t e, MptRefitInfo* info, const char* who) {
    const bool light = has_light_tree(c);
    std::vector<float> hb, hbl;
    if (e == hipSuccess && info) {
        hb.resize(c->nbox.n);
        e = hipMemcpy(hb.data(), c->nbox.p, hb.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess && light) {
            hbl.resize(c->nbox_light.n);
            e = hipMemcpy(hbl.data(), c->nbox_light.p, hbl.size() * sizeof(float), hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess) return update_fail(c, e, who);
    if (info) {
        MptRefitInfo r{};
        r.nodes = (int32_t)c->nodes.n;
        r.levels = c->bvh.depth;
        r.area_ratio = (float)(node_box_area_sum(hb.data(), c->nodes.n) / c->area0);
        if (light) {
            r.light_nodes = (int32_t)c->nodes_light.n;
            r.light_levels = c->bvh_light.depth;
            r.light_area_ratio = (float)(node_box_area_sum(hbl.data(), c->nodes_light.n) / c->area0_light);
        }
        *info = r;
    }
    return MPT_OK;
}

// The last step of mpt_update_vertices and mpt_update_vertices_device, the streams drained (e: what
// that returned) and box_pad set: the caller's arrays, on the host or on the device (kind), copied
// over the context's, then the refit and the report.  Any HIP error drops the scene.
int upload_vertices(MptContext* c, hipError_t e, const float* v, const float* nrm, hipMemcpyKind kind, MptRefitInfo* info, const char* who) {
    if (e == hipSuccess) e = hipMemcpyAsync(c->pos.p, v, c->pos.n * sizeof(float), kind, c->stream);
    if (e == hipSuccess && nrm) e = hipMemcpyAsync(c->nrm.p, nrm, c->nrm.n * sizeof(float), kind, c->stream);
    if (e == hipSuccess) e = refit_and_tables(c, c->box_pad, kind == hipMemcpyHostToDevice ? v : nullptr);
    return finish_update(c, e, info, who);
}

// h_vert_used on the device (the pad's maximum is taken over the vertices in use).
hipError_t ensure_used_mask(MptContext* c) {
    if (c->vert_used.p && c->vert_used.n == c->h_vert_used.size()) return hipSuccess;
    hipError_t e = c->vert_used.upload(c->h_vert_used.data(), c->h_vert_used.size(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) c->vert_used.release();
    return e;
}

// The two words a reduction of xform.hip left: the maximum's bits and the non-finite flag; with
// extra, that device word is read in the same synchronisation and ORed into the flag.
hipError_t read_reduction(MptContext* c, float* max_abs, bool* bad, const uint32_t* extra = nullptr) {
    uint32_t w[2] = {0, 0}, x = 0;
    hipError_t e = hipMemcpyAsync(w, c->xf_red.p, sizeof(w), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && extra) e = hipMemcpyAsync(&x, extra, sizeof(x), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    std::memcpy(max_abs, &w[0], 4);
    *bad = w[1] != 0 || x != 0;
    return e;
}

// A staged update (mpt_update_transforms, update_pose) has two halves around its kernel.  First: the
// streams drained, the used mask and the reduction words there and, with stage, the arrays the kernel
// writes (mpt_update_vertices_device checks the caller's arrays and needs none).  Everything up to
// the commit writes scratch only: a refusal or an error before it changes nothing.
hipError_t begin_staged(MptContext* c, bool stage = true) {
    hipError_t e = drain(c);
    if (e == hipSuccess) e = ensure_used_mask(c);
    if (e == hipSuccess && stage) e = c->stage_pos.alloc(c->pos.n);
    if (e == hipSuccess && stage) e = c->stage_nrm.alloc(c->nrm.n);
    if (e == hipSuccess) e = c->xf_red.alloc(2);
    return e;
}

// ... and the commit.  e is what the scratch half returned, m and bad what read_reduction gave: an
// error drops the scene, bad refuses with the scene untouched; otherwise the staging arrays change
// places with pos / nrm and both trees are refitted to them.
int commit_staged(MptContext* c, hipError_t e, float m, bool bad, const char* refusal, MptRefitInfo* info, const char* who) {
    if (e != hipSuccess) return update_fail(c, e, who);
    if (bad) return fail(MPT_ERR_INVALID_ARGUMENT, refusal);
    c->pos.swap(c->stage_pos);
    c->nrm.swap(c->stage_nrm);
    c->box_pad = box_pad_for(m);
    return finish_update(c, refit_and_tables(c, c->box_pad, nullptr), info, who);
}

// The rest pose of mpt_set_objects, mpt_set_skin and mpt_set_morph: pos / nrm as they are now,
// copied on the stream into new buffers (the caller synchronises) ...
hipError_t capture_rest_pose(MptContext* c, DBuf<float>& rp, DBuf<float>& rn) {
    hipStream_t st = c->stream;
    hipError_t e = rp.alloc(c->pos.n);
    if (e == hipSuccess) e = rn.alloc(c->nrm.n);
    if (e == hipSuccess) e = hipMemcpyAsync(rp.p, c->pos.p, c->pos.n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(rn.p, c->nrm.p, c->nrm.n * sizeof(float), hipMemcpyDeviceToDevice, st);
    return e;
}
// ... and taken once the call is accepted: whatever used the old rest pose goes first (an object
// table, or an earlier skin and morph)
void take_rest_pose(MptContext* c, DBuf<float>& rp, DBuf<float>& rn) {
    drop_objects(c);
    c->rest_pos.take(rp);
    c->rest_nrm.take(rn);
}

// The pose of a skin and / or a morph evaluated from the shared rest pose: what mpt_update_skin,
// mpt_update_morph, mpt_update_morph_skin and mpt_update_animation have in common once their
// arguments are checked.  weights (NULL: the retained ones) are the morph's num_targets weights,
// matrices (NULL: the retained palette, if the skin has been posed) the skin's num_joints matrices.
// anim_time (not NULL: both others NULL): the staged weights and records come from the device
// instead, written by k_anim for the context's animation -- those of the two that it drives -- and
// its flag is read with the reductions.  Everything up to the swap writes scratch only -- the new
// weights and records included -- so a refusal changes nothing, retained state included.
int update_pose(MptContext* c, const float* weights, const float* matrices, MptRefitInfo* info, const char* who,
                const float* anim_time = nullptr) {
    const bool new_w = weights || (anim_time && c->anim.T > 0);
    const bool new_m = matrices || (anim_time && c->anim.J > 0);
    const bool morph = c->num_targets >= 0;
    const bool skin = new_m || (c->num_joints >= 0 && c->skin_posed);
    const size_t nv = c->pos.n / 3;
    if (c->rest_pos.n != c->pos.n || c->rest_nrm.n != c->nrm.n) return fail(MPT_ERR_INVALID_ARGUMENT, "rest pose does not fit the scene");
    if (skin && (3 * c->skin_joints.n != 4 * c->pos.n || c->skin_weights.n != c->skin_joints.n))
        return fail(MPT_ERR_INVALID_ARGUMENT, "skin does not fit the scene");
    if (morph && c->morph_row.n != nv + 1) return fail(MPT_ERR_INVALID_ARGUMENT, "morph does not fit the scene");
    std::vector<float4> recs;
    if (matrices) make_skin_records(matrices, c->num_joints, recs);
    std::vector<float> wpad;
    if (weights) {
        wpad.assign(((size_t)c->num_targets + 3) / 4 * 4, 0.0f);
        std::memcpy(wpad.data(), weights, (size_t)c->num_targets * sizeof(float));
    }
    HIPCHK(hipSetDevice(c->device));
    if (const int r = temporal_snapshot(c)) return r;
    hipStream_t st = c->stream;
    float m = 0.0f;
    bool bad = false;
    hipError_t e = begin_staged(c);
    if (e == hipSuccess && matrices) e = c->skin_recs_stage.upload(recs.data(), recs.size(), st);
    if (e == hipSuccess && weights) e = c->morph_w_stage.upload(wpad.data(), wpad.size(), st);
    if (anim_time) {
        // (a buffer the animation does not drive is not touched: k_anim's loop over it is empty)
        if (e == hipSuccess && new_m) e = c->skin_recs_stage.alloc((size_t)(mptskin::REC / 4) * (size_t)c->anim.J);
        if (e == hipSuccess && new_w) e = c->morph_w_stage.alloc(((size_t)c->anim.T + 3) / 4 * 4);
        if (e == hipSuccess)
            e = launch_anim(anim_tables(c->anim, c->anim_blob.p), *anim_time, c->skin_recs_stage.p, (float4*)c->morph_w_stage.p,
                            c->anim_flag.p, anim_lds(), st);
    }
    const float4* d_recs = new_m ? c->skin_recs_stage.p : c->skin_recs.p;
    const float* d_w = new_w ? c->morph_w_stage.p : c->morph_w.p;
    if (e == hipSuccess && !morph)
        e = launch_skin(c->rest_pos.p, c->rest_nrm.p, c->skin_joints.p, c->skin_weights.p, c->vert_used.p, (const float*)d_recs,
                        c->num_joints, (int)nv, c->stage_pos.p, c->stage_nrm.p, c->xf_red.p, skin_group(), skin_lds(), st);
    if (e == hipSuccess && morph) {
        MorphLaunch a{};
        a.rest_pos = c->rest_pos.p; a.rest_nrm = c->rest_nrm.p;
        a.row = c->morph_row.p; a.tgt = c->morph_tgt.p; a.dpos = c->morph_dpos.p; a.dnrm = c->morph_dnrm.p;
        a.mweights = d_w; a.num_targets = c->num_targets;
        if (skin) { a.joints = c->skin_joints.p; a.sweights = c->skin_weights.p; a.recs = (const float*)d_recs; a.num_joints = c->num_joints; }
        a.used = c->vert_used.p; a.n = (int)nv;
        a.out_pos = c->stage_pos.p; a.out_nrm = c->stage_nrm.p; a.red = c->xf_red.p;
        e = launch_morph(a, morph_group(), morph_lds(), st);
    }
    if (e == hipSuccess) e = read_reduction(c, &m, &bad, anim_time ? c->anim_flag.p : nullptr);
    if (e == hipSuccess && !bad) {   // accepted: the staged records and weights become the retained ones
        if (new_m) { c->skin_recs.swap(c->skin_recs_stage); c->skin_posed = true; }
        if (new_w) c->morph_w.swap(c->morph_w_stage);
    }
    return commit_staged(c, e, m, bad, anim_time ? "non-finite animation value or vertex coordinate" : "non-finite vertex coordinate",
                         info, who);
}

}  // namespace

extern "C" {

int mpt_update_vertices(MptContext* c, const float* vertices, const float* vertex_normals, int32_t num_vertices,
                        MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!vertices) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    // one pass: every coordinate finite, and scene_box_pad's maximum over the vertices in use
    float m = 0.0f;
    for (size_t i = 0; i < (size_t)num_vertices; i++) {
        const float* p = vertices + 3 * i;
        const float a0 = std::fabs(p[0]), a1 = std::fabs(p[1]), a2 = std::fabs(p[2]);
        if (!(a0 <= FLT_MAX && a1 <= FLT_MAX && a2 <= FLT_MAX))   // (a NaN fails every comparison)
            return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
        if (c->h_vert_used[i]) m = std::max(m, std::max(a0, std::max(a1, a2)));
    }
    HIPCHK(hipSetDevice(c->device));
    if (const int r = temporal_snapshot(c)) return r;
    c->box_pad = box_pad_for(m);
    return upload_vertices(c, drain(c), vertices, vertex_normals, hipMemcpyHostToDevice, info, "mpt_update_vertices");
}

int mpt_set_objects(MptContext* c, const int32_t* vertex_object, int32_t num_vertices, int32_t num_objects) {
    if (const int r = need_scene(c)) return r;
    if (!vertex_object) {
        if (num_objects != 0) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
        HIPCHK(hipSetDevice(c->device));
        if (c->num_joints < 0 && c->num_targets < 0) drop_objects(c);   // (a skin or a morph is its own call's to free)
        return MPT_OK;
    }
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    if (num_objects <= 0) return fail(MPT_ERR_INVALID_ARGUMENT, "objects: bad object count");
    for (int32_t i = 0; i < num_vertices; i++)
        if (vertex_object[i] < -1 || vertex_object[i] >= num_objects) return fail(MPT_ERR_INVALID_ARGUMENT, "object id out of range");
    HIPCHK(hipSetDevice(c->device));
    // into new buffers, taken when all of them are there: a failure leaves the old objects
    DBuf<int32_t> ids;
    DBuf<float> rp, rn;
    hipStream_t st = c->stream;
    hipError_t e = drain(c);
    if (e == hipSuccess) e = ensure_used_mask(c);
    if (e == hipSuccess) e = ids.upload(vertex_object, (size_t)num_vertices, st);
    if (e == hipSuccess) e = capture_rest_pose(c, rp, rn);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return alloc_fail(e, "mpt_set_objects");
    take_rest_pose(c, rp, rn);
    c->vert_obj.take(ids);
    c->num_objects = num_objects;
    return MPT_OK;
}

int mpt_update_transforms(MptContext* c, const float* matrices, int32_t num_objects, MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!matrices) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->num_objects < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "no objects set");
    if (num_objects != c->num_objects) return fail(MPT_ERR_INVALID_ARGUMENT, "object count differs from the table's");
    if (!matrices_finite(matrices, num_objects)) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite matrix entry");
    if (c->rest_pos.n != c->pos.n || c->rest_nrm.n != c->nrm.n || 3 * c->vert_obj.n != c->pos.n)
        return fail(MPT_ERR_INVALID_ARGUMENT, "objects do not fit the scene");
    std::vector<float> recs;
    make_xform_records(matrices, num_objects, recs);
    HIPCHK(hipSetDevice(c->device));
    if (const int r = temporal_snapshot(c)) return r;
    hipStream_t st = c->stream;
    float m = 0.0f;
    bool bad = false;
    hipError_t e = begin_staged(c);
    if (e == hipSuccess) e = c->xf_recs.upload(recs.data(), recs.size(), st);
    if (e == hipSuccess)
        e = launch_xform(c->rest_pos.p, c->rest_nrm.p, c->vert_obj.p, c->vert_used.p, c->xf_recs.p, (int)c->vert_obj.n,
                         c->stage_pos.p, c->stage_nrm.p, c->xf_red.p, xform_group(), st);
    if (e == hipSuccess) e = read_reduction(c, &m, &bad);
    return commit_staged(c, e, m, bad, "non-finite vertex coordinate", info, "mpt_update_transforms");
}

int mpt_set_skin(MptContext* c, const int32_t* joints, const float* weights, int32_t num_vertices, int32_t num_joints) {
    if (const int r = need_scene(c)) return r;
    if (!joints && !weights) {
        if (num_joints != 0) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
        HIPCHK(hipSetDevice(c->device));
        // (an object table is mpt_set_objects' to free; with a morph set the rest pose stays)
        if (c->num_targets >= 0) drop_skin_tables(c);
        else if (c->num_objects < 0) drop_objects(c);
        return MPT_OK;
    }
    if (!joints || !weights) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    if (num_joints < 1) return fail(MPT_ERR_INVALID_ARGUMENT, "skin: bad joint count");
    if (const char* bad = check_skin_table(joints, weights, (size_t)num_vertices, num_joints)) return fail(MPT_ERR_INVALID_ARGUMENT, bad);
    HIPCHK(hipSetDevice(c->device));
    // into new buffers, taken when all of them are there: a failure leaves what was set
    const bool capture = c->num_targets < 0;   // a morph has captured the rest pose already
    DBuf<int32_t> dj;
    DBuf<float> dw, rp, rn;
    hipStream_t st = c->stream;
    hipError_t e = drain(c);
    if (e == hipSuccess) e = ensure_used_mask(c);
    if (e == hipSuccess) e = dj.upload(joints, 4 * (size_t)num_vertices, st);
    if (e == hipSuccess) e = dw.upload(weights, 4 * (size_t)num_vertices, st);
    if (e == hipSuccess && capture) e = capture_rest_pose(c, rp, rn);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return alloc_fail(e, "mpt_set_skin");
    if (capture) take_rest_pose(c, rp, rn);
    else drop_skin_tables(c);      // (the new skin is not posed)
    c->skin_joints.take(dj);
    c->skin_weights.take(dw);
    c->num_joints = num_joints;
    return MPT_OK;
}

int mpt_update_skin(MptContext* c, const float* joint_matrices, int32_t num_joints, MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!joint_matrices) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->num_joints < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "no skin set");
    if (num_joints != c->num_joints) return fail(MPT_ERR_INVALID_ARGUMENT, "joint count differs from the table's");
    if (!matrices_finite(joint_matrices, num_joints)) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite matrix entry");
    return update_pose(c, nullptr, joint_matrices, info, "mpt_update_skin");
}

int mpt_set_morph(MptContext* c, int32_t num_targets, const int32_t* target_offsets, const int32_t* vertex_ids,
                  const float* pos_deltas, const float* nrm_deltas, int32_t num_vertices) {
    if (const int r = need_scene(c)) return r;
    if (!target_offsets && !vertex_ids && !pos_deltas && !nrm_deltas) {
        if (num_targets != 0) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
        HIPCHK(hipSetDevice(c->device));
        // (an object table is mpt_set_objects' to free; with a skin set the rest pose stays)
        if (c->num_joints >= 0) drop_morph_tables(c);
        else if (c->num_objects < 0) drop_objects(c);
        return MPT_OK;
    }
    if (!target_offsets) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    mptmorph::Csr csr;
    if (const char* bad = mptmorph::to_csr(num_targets, target_offsets, vertex_ids, pos_deltas, nrm_deltas, num_vertices, csr))
        return fail(MPT_ERR_INVALID_ARGUMENT, bad);
    HIPCHK(hipSetDevice(c->device));
    // into new buffers, taken when all of them are there: a failure leaves what was set
    const bool capture = c->num_joints < 0;   // a skin has captured the rest pose already
    const std::vector<float> zeros(((size_t)num_targets + 3) / 4 * 4, 0.0f);
    const size_t N = csr.tgt.size();
    DBuf<int32_t> dr, dt;
    DBuf<float> dp, dn, dw, rp, rn;
    hipStream_t st = c->stream;
    hipError_t e = drain(c);
    if (e == hipSuccess) e = ensure_used_mask(c);
    if (e == hipSuccess) e = dr.upload(csr.row.data(), csr.row.size(), st);
    // (a kernel is never handed a NULL table: a morph without entries keeps one unread entry)
    if (e == hipSuccess) e = dt.alloc(std::max(N, (size_t)1));
    if (e == hipSuccess) e = dp.alloc(3 * std::max(N, (size_t)1));
    if (e == hipSuccess && nrm_deltas) e = dn.alloc(3 * std::max(N, (size_t)1));
    if (e == hipSuccess && N) e = hipMemcpyAsync(dt.p, csr.tgt.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && N) e = hipMemcpyAsync(dp.p, csr.dpos.data(), 3 * N * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && N && nrm_deltas) e = hipMemcpyAsync(dn.p, csr.dnrm.data(), 3 * N * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = dw.upload(zeros.data(), zeros.size(), st);
    if (e == hipSuccess && capture) e = capture_rest_pose(c, rp, rn);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return alloc_fail(e, "mpt_set_morph");
    if (capture) take_rest_pose(c, rp, rn);   // (with an object table, or an earlier morph and its rest pose)
    else drop_morph_tables(c);
    c->morph_row.take(dr);
    c->morph_tgt.take(dt);
    c->morph_dpos.take(dp);
    c->morph_dnrm.take(dn);
    c->morph_w.take(dw);
    c->num_targets = num_targets;
    return MPT_OK;
}

int mpt_set_normals(MptContext* c, const int32_t* vertex_group, const uint8_t* group_flip, int32_t num_vertices, int32_t num_groups) {
    if (const int r = need_scene(c)) return r;
    if (!vertex_group) {
        if (num_groups != 0 || group_flip) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(drain(c));
        drop_normals(c);
        return MPT_OK;
    }
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    // (the indices: the context's own copy, taken at the upload -- no update, rebuild or material
    // edit changes them, so the copy is current also where the other host mirrors are stale)
    if (3 * (c->h_idx.size() / 3) != c->h_idx.size() || c->h_idx.size() != c->idx.n)
        return fail(MPT_ERR_HIP, "mpt_set_normals: index mirror differs from the scene's");
    mptnormals::Csr csr;
    if (const char* bad = mptnormals::to_csr(vertex_group, num_vertices, num_groups, c->h_idx.data(), (int32_t)(c->h_idx.size() / 3), csr))
        return fail(MPT_ERR_INVALID_ARGUMENT, bad);
    const std::vector<uint8_t> zeros(group_flip ? 0 : (size_t)num_groups, 0);
    HIPCHK(hipSetDevice(c->device));
    // into new buffers, taken when all of them are there: a failure leaves what was set
    const size_t N = csr.tri.size();
    DBuf<int32_t> dg, dr, dt;
    DBuf<uint8_t> df;
    hipStream_t st = c->stream;
    hipError_t e = drain(c);
    if (e == hipSuccess) e = dg.upload(vertex_group, (size_t)num_vertices, st);
    if (e == hipSuccess) e = dr.upload(csr.row.data(), csr.row.size(), st);
    // (a kernel is never handed a NULL table: groups without entries keep one unread entry)
    if (e == hipSuccess) e = dt.alloc(std::max(N, (size_t)1));
    if (e == hipSuccess && N) e = hipMemcpyAsync(dt.p, csr.tri.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = df.upload(group_flip ? group_flip : zeros.data(), (size_t)num_groups, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return alloc_fail(e, "mpt_set_normals");
    drop_normals(c);
    c->nrm_group.take(dg);
    c->nrm_row.take(dr);
    c->nrm_tri.take(dt);
    c->nrm_flip.take(df);
    c->num_groups = num_groups;
    return MPT_OK;
}

int mpt_get_vertices(MptContext* c, float* out_vertices, float* out_normals, int32_t num_vertices) {
    if (const int r = need_scene(c)) return r;
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(drain(c));
    if (out_vertices) HIPCHK(hipMemcpy(out_vertices, c->pos.p, c->pos.n * sizeof(float), hipMemcpyDeviceToHost));
    if (out_normals) HIPCHK(hipMemcpy(out_normals, c->nrm.p, c->nrm.n * sizeof(float), hipMemcpyDeviceToHost));
    return MPT_OK;
}

int mpt_update_morph(MptContext* c, const float* weights, int32_t num_targets, MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!weights) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->num_targets < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "no morph set");
    if (num_targets != c->num_targets) return fail(MPT_ERR_INVALID_ARGUMENT, "target count differs from the tables'");
    if (!weights_finite(weights, num_targets)) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite morph weight");
    return update_pose(c, weights, nullptr, info, "mpt_update_morph");
}

int mpt_update_morph_skin(MptContext* c, const float* weights, int32_t num_targets, const float* joint_matrices, int32_t num_joints,
                          MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!weights || !joint_matrices) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->num_targets < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "no morph set");
    if (c->num_joints < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "no skin set");
    if (num_targets != c->num_targets) return fail(MPT_ERR_INVALID_ARGUMENT, "target count differs from the tables'");
    if (num_joints != c->num_joints) return fail(MPT_ERR_INVALID_ARGUMENT, "joint count differs from the table's");
    if (!weights_finite(weights, num_targets)) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite morph weight");
    if (!matrices_finite(joint_matrices, num_joints)) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite matrix entry");
    return update_pose(c, weights, joint_matrices, info, "mpt_update_morph_skin");
}

int mpt_set_animation(MptContext* c, const MptAnimation* anim) {
    if (const int r = need_scene(c)) return r;
    if (!anim) {
        HIPCHK(hipSetDevice(c->device));
        drop_animation(c);
        return MPT_OK;
    }
    AnimPacked p;
    if (const char* bad = pack_animation(*anim, p)) return fail(MPT_ERR_INVALID_ARGUMENT, bad);
    if (p.J > 0 && c->num_joints < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "animation: joints without a skin set");
    if (p.J > 0 && p.J != c->num_joints) return fail(MPT_ERR_INVALID_ARGUMENT, "animation: joint count differs from the skin's");
    if (p.T > 0 && c->num_targets < 0) return fail(MPT_ERR_INVALID_ARGUMENT, "animation: targets without a morph set");
    if (p.T > 0 && p.T != c->num_targets) return fail(MPT_ERR_INVALID_ARGUMENT, "animation: target count differs from the morph's");
    HIPCHK(hipSetDevice(c->device));
    // into new buffers, taken when they are there: a failure leaves what was set
    DBuf<unsigned char> db;
    DBuf<uint32_t> df;
    hipStream_t st = c->stream;
    hipError_t e = drain(c);
    if (e == hipSuccess) e = db.upload(p.blob.data(), p.blob.size(), st);
    if (e == hipSuccess) e = df.alloc(1);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return alloc_fail(e, "mpt_set_animation");
    drop_animation(c);
    c->anim_blob.take(db);
    c->anim_flag.take(df);
    p.blob = std::vector<unsigned char>();   // (only the counts and the offsets are kept)
    c->anim = std::move(p);
    c->has_anim = true;
    return MPT_OK;
}

int mpt_update_animation(MptContext* c, float time, MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!c->has_anim) return fail(MPT_ERR_INVALID_ARGUMENT, "no animation set");
    if (!(std::fabs(time) <= FLT_MAX)) return fail(MPT_ERR_INVALID_ARGUMENT, "animation: time not finite");
    // (the animation goes with the skin and the morph it drives: the counts still fit)
    return update_pose(c, nullptr, nullptr, info, "mpt_update_animation", &time);
}

int mpt_update_vertices_device(MptContext* c, const float* d_vertices, const float* d_normals, int32_t num_vertices,
                               MptRefitInfo* info) {
    if (const int r = need_scene(c)) return r;
    if (!d_vertices) return fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!count_fits(c, num_vertices)) return fail(MPT_ERR_INVALID_ARGUMENT, "vertex count differs from the scene's");
    HIPCHK(hipSetDevice(c->device));
    for (const float* p : {d_vertices, d_normals}) {   // a host pointer must not reach a kernel
        if (!p) continue;
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->device) {
            (void)hipGetLastError();
            return fail(MPT_ERR_INVALID_ARGUMENT, "not memory of the context's device");
        }
    }
    if (const int r = temporal_snapshot(c)) return r;
    hipStream_t st = c->stream;
    float m = 0.0f;
    bool bad = false;
    // the caller's arrays are checked where they lie and copied over pos / nrm once accepted
    hipError_t e = begin_staged(c, false);
    if (e == hipSuccess) e = launch_xform_check(d_vertices, c->vert_used.p, num_vertices, c->xf_red.p, xform_group(), st);
    if (e == hipSuccess) e = read_reduction(c, &m, &bad);
    if (e != hipSuccess) return update_fail(c, e, "mpt_update_vertices_device");
    if (bad) return fail(MPT_ERR_INVALID_ARGUMENT, "non-finite vertex coordinate");
    c->box_pad = box_pad_for(m);
    return upload_vertices(c, e, d_vertices, d_normals, hipMemcpyDeviceToDevice, info, "mpt_update_vertices_device");
}

}  // extern "C"
