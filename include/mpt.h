/*
 * mpt.h -- C ABI of the MI355X-native path-tracing hot path ("libmpt").
 *
 * This is the drop-in boundary described in SURVEY.md §8(b).  Every entry point
 * replaces one piece of the reference's GPU launch API (wuyakuma/HIPRT-Path-Tracer,
 * src/Renderer/GPURenderer.h) or of the HIPRT/Orochi glue it sits on:
 *
 *   mpt_create / mpt_destroy      <- GPURenderer::GPURenderer (GPURenderer.h:75,
 *                                    GPURenderer.cpp:48-86) + HIPRTOrochiCtx (HIPRTOrochiCtx.h:20-66)
 *   mpt_upload_scene              <- GPURenderer::set_scene -> set_hiprt_scene_from_scene
 *                                    (GPURenderer.h:220, GPURenderer.cpp:1041-1134) and
 *                                    HIPRTGeometry::build_bvh (HIPRTScene.h:60-87)
 *   mpt_upload_scene_mode         <- the same, with both BVH8s built on the GPU in a build mode
 *                                    (HIPRT builds its geometry on the device as well)
 *   mpt_update_materials          <- GPURenderer::update_materials (GPURenderer.h:228)
 *   mpt_update_vertices           <- (no counterpart: the reference rebuilds its HIPRT geometry) moved
 *                                    vertices with a GPU refit of both BVH8s
 *   mpt_rebuild_bvh               <- (no counterpart: HIPRT rebuilds with the geometry) both BVH8s
 *   mpt_rebuild_bvh_mode             rebuilt on the GPU from the positions on the device: an LBVH
 *                                    (mode 0, the default), PLOC (mode 1) or binned SAH (mode 3; the
 *                                    reference builds with hiprtBuildFlagBitPreferHighQualityBuild)
 *   mpt_set_envmap                <- GPURenderer::set_envmap (GPURenderer.h:222, .cpp:1136-1174)
 *   mpt_set_luts                  <- GPURenderer::setup_brdfs_data (GPURenderer.h:76, .cpp:88-175)
 *   mpt_resize                    <- GPURenderer::resize (GPURenderer.h:172)
 *   mpt_render_frame              <- GPURenderer::render -> launch_camera_rays +
 *                                    launch_path_tracing (GPURenderer.h:139-143,
 *                                    .cpp:408-486), i.e. the CameraRays and FullPathTracer
 *                                    kernels (Device/kernels/CameraRays.h:45,
 *                                    Device/kernels/FullPathTracer.h:99)
 *   mpt_render_frames             <- GPURenderer::render's samples_per_frame loop
 *                                    (GPURenderer.cpp:424-449) as one batched wavefront
 *   mpt_synchronize / mpt_query_done <- GPURenderer::synchronize_kernel / frame_render_done
 *                                    (GPURenderer.h:149-156)
 *   mpt_get_framebuffer           <- the 'pixels' / denoiser AOV interop buffers
 *                                    (GPURenderer.h:193-197, RenderData.h:32-36)
 *   mpt_trace_closest / mpt_trace_any <- hiprtGeomTraversalClosest/AnyHit as called by
 *                                    trace_ray / evaluate_shadow_ray (Device/includes/Intersect.h:114-286)
 *   mpt_display / mpt_write_png   <- DisplayViewSystem::display + the display shaders (src/Shaders) and
 *                                    Screenshoter::write_to_png (Screenshoter.cpp:129-166)
 *   mpt_denoise / mpt_denoised_buffer <- RenderWindow::denoise (RenderWindow.cpp:881-972) and
 *                                    OpenImageDenoiser::denoise / get_denoised_framebuffer, with an
 *                                    a-trous filter in OIDN's place (no parity claimed)
 *   mpt_bake_lut                  <- GPUBaker::bake_* (Renderer/Baker/GPUBaker.cpp:35-97) and the
 *                                    Device/kernels/Baking/ headers kernels
 *
 * Conventions: every function returns MPT_OK (0) or a negative error code; the
 * message of the last error of the calling thread is in mpt_last_error().  The
 * library never exits the process (the reference logs and calls exit(),
 * HIPRT-Orochi/HIPRTOrochiUtils.cpp:15-47).  All device memory is owned by the
 * context; host arrays passed in are copied before the call returns.  Calls on one
 * context must be externally serialised.  All GPU work of a context is enqueued on
 * the stream given to mpt_create (or the context's own stream).
 *
 * The POD structs below are byte-identical mirrors of the reference's
 * HostDeviceCommon structs (sizes are static_assert-ed in the implementation):
 *   MptMaterial       == RendererMaterial        (HostDeviceCommon/Material.h:29-268), 332 B
 *   MptRenderSettings == HIPRTRenderSettings     (HostDeviceCommon/RenderSettings.h:26-252), 304 B
 *   MptWorldSettings  == WorldSettings           (HostDeviceCommon/WorldSettings.h:18-52), 200 B
 *   MptCamera         == HIPRTCamera             (HostDeviceCommon/HIPRTCamera.h:16-49), 196 B
 */
#ifndef MPT_H
#define MPT_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Status codes                                                               */
/* ------------------------------------------------------------------------- */
#define MPT_OK 0
#define MPT_ERR_INVALID_ARGUMENT (-1)
#define MPT_ERR_HIP (-2)
#define MPT_ERR_NO_SCENE (-3)
#define MPT_ERR_UNSUPPORTED (-4)
#define MPT_ERR_OUT_OF_MEMORY (-5)

/* ------------------------------------------------------------------------- */
/* Compile-time kernel options of the reference (HostDeviceCommon/KernelOptions.h) */
/* become runtime selections of pre-instantiated kernel variants.             */
/* ------------------------------------------------------------------------- */
#define MPT_BSDF_NONE 0        /* BSDF_NONE: Principled BSDF  (KernelOptions.h:21) */
#define MPT_BSDF_LAMBERTIAN 1  /* BSDF_LAMBERTIAN                                   */
#define MPT_BSDF_OREN_NAYAR 2  /* BSDF_OREN_NAYAR (OrenNayar.h; see dev_bsdf.h bsdf_eval) */

#define MPT_LSS_NO_DIRECT_LIGHT_SAMPLING 0 /* KernelOptions.h:50-56 */
#define MPT_LSS_UNIFORM_ONE_LIGHT 1
#define MPT_LSS_BSDF 2
#define MPT_LSS_MIS_LIGHT_BSDF 3
#define MPT_LSS_RIS_BSDF_AND_LIGHT 4
#define MPT_LSS_RESTIR_DI 5

#define MPT_ESS_NO_SAMPLING 0 /* KernelOptions.h:58-60 */
#define MPT_ESS_BINARY_SEARCH 1
#define MPT_ESS_ALIAS_TABLE 2

#define MPT_AMBIENT_NONE 0 /* WorldSettings.h:11-16 */
#define MPT_AMBIENT_UNIFORM 1
#define MPT_AMBIENT_ENVMAP 2

#define MPT_NO_TEXTURE (-1)
#define MPT_CONSTANT_EMISSIVE_TEXTURE (-2)

/* ------------------------------------------------------------------------- */
/* Byte-identical mirrors of the reference PODs                               */
/* ------------------------------------------------------------------------- */
typedef struct MptColor { float r, g, b; } MptColor;           /* ColorRGB32F, Color.h:61 */
typedef struct MptFloat4x4 { float m[4][4]; } MptFloat4x4;      /* float4x4, Math.h:43 */

/* RendererMaterial (HostDeviceCommon/Material.h:29-268).  Field order is the
 * reference's; 'emission' is the (private) last field of SimplifiedRendererMaterial. */
typedef struct MptMaterial {
    bool emissive_texture_used;
    float emission_strength;
    MptColor base_color;
    float roughness;
    float oren_nayar_sigma;
    float metallic;
    float metallic_F90_falloff_exponent;
    MptColor metallic_F82;
    MptColor metallic_F90;
    float anisotropy;
    float anisotropy_rotation;
    float second_roughness_weight;
    float second_roughness;
    float specular;
    float specular_tint;
    MptColor specular_color;
    float specular_darkening;
    float coat;
    MptColor coat_medium_absorption;
    float coat_medium_thickness;
    float coat_roughness;
    float coat_roughening;
    float coat_darkening;
    float coat_anisotropy;
    float coat_anisotropy_rotation;
    float coat_ior;
    float sheen;
    float sheen_roughness;
    MptColor sheen_color;
    float ior;
    float specular_transmission;
    float absorption_at_distance;
    MptColor absorption_color;
    float dispersion_scale;
    float dispersion_abbe_number;
    bool thin_walled;
    float thin_film;
    float thin_film_ior;
    float thin_film_thickness;
    float thin_film_kappa_3;
    float thin_film_hue_shift_degrees;
    float thin_film_base_ior_override;
    bool thin_film_do_ior_override;
    bool srgb;
    float alpha_opacity;
    int32_t dielectric_priority;
    int32_t energy_preservation_monte_carlo_samples;
    bool enforce_strong_energy_conservation;
    MptColor emission;
    /* RendererMaterial texture indices (Material.h:217-266) */
    int32_t normal_map_texture_index;
    int32_t emission_texture_index;
    int32_t base_color_texture_index;
    int32_t roughness_metallic_texture_index;
    int32_t roughness_texture_index;
    int32_t oren_sigma_texture_index;
    int32_t metallic_texture_index;
    int32_t specular_texture_index;
    int32_t specular_tint_texture_index;
    int32_t specular_color_texture_index;
    int32_t anisotropic_texture_index;
    int32_t anisotropic_rotation_texture_index;
    int32_t coat_texture_index;
    int32_t coat_roughness_texture_index;
    int32_t coat_ior_texture_index;
    int32_t sheen_texture_index;
    int32_t sheen_roughness_texture_index;
    int32_t sheen_color_texture_index;
    int32_t specular_transmission_texture_index;
} MptMaterial;

/* ReSTIRDISettings (HostDeviceCommon/ReSTIRDISettings.h:12-195) */
typedef struct MptReSTIRDISettings {
    /* InitialCandidatesSettings */
    int32_t number_of_initial_light_candidates;
    int32_t number_of_initial_bsdf_candidates;
    float envmap_candidate_probability;
    void* ic_output_reservoirs;
    /* TemporalPassSettings */
    bool do_temporal_reuse_pass;
    bool use_permutation_sampling;
    int32_t permutation_sampling_random_bits;
    int32_t max_neighbor_search_count;
    int32_t neighbor_search_radius;
    bool temporal_buffer_clear_requested;
    void* tp_input_reservoirs;
    void* tp_output_reservoirs;
    /* SpatialPassSettings */
    bool do_spatial_reuse_pass;
    int32_t spatial_pass_index;
    int32_t number_of_passes;
    int32_t reuse_radius;
    int32_t reuse_neighbor_count;
    bool do_disocclusion_reuse_boost;
    int32_t disocclusion_reuse_count;
    bool debug_neighbor_location;
    bool do_neighbor_rotation;
    bool allow_converged_neighbors_reuse;
    float converged_neighbor_reuse_probability;
    bool do_visibility_only_last_pass;
    int32_t neighbor_visibility_count;
    void* sp_input_reservoirs;
    void* sp_output_reservoirs;
    /* LightPresamplingSettings */
    int32_t number_of_subsets;
    int32_t subset_size;
    int32_t tile_size;
    void* light_samples;
    /* ReSTIRDISettings */
    bool do_fused_spatiotemporal;
    int32_t m_cap;
    bool use_confidence_weights;
    bool use_normal_similarity_heuristic;
    float normal_similarity_angle_degrees;
    float normal_similarity_angle_precomp;
    bool use_plane_distance_heuristic;
    float plane_distance_threshold;
    bool use_roughness_similarity_heuristic;
    float roughness_similarity_threshold;
    bool do_final_shading_visibility;
    void* restir_output_reservoirs;
} MptReSTIRDISettings;

/* HIPRTRenderSettings (HostDeviceCommon/RenderSettings.h:26-252) */
typedef struct MptRenderSettings {
    bool need_to_reset;
    bool do_update_status_buffers;
    bool accumulate;
    int32_t denoiser_AOV_accumulation_counter;
    int32_t sample_number;
    int32_t samples_per_frame;
    int32_t nb_bounces;
    bool use_russian_roulette;
    int32_t russian_roulette_min_depth;
    float russian_roulette_throughput_clamp;
    int32_t path_russian_roulette_method; /* PathRussianRoulette: 0 MAX_THROUGHPUT, 1 ARNOLD_2014 */
    int32_t freeze_random;
    bool display_NaNs;
    bool allow_render_low_resolution;
    bool wants_render_low_resolution;
    int32_t render_low_resolution_scaling;
    bool enable_adaptive_sampling;
    int32_t adaptive_sampling_min_samples;
    float adaptive_sampling_noise_threshold;
    bool enable_pixel_stop_noise_threshold;
    float stop_pixel_percentage_converged;
    float stop_pixel_noise_threshold;
    float direct_contribution_clamp;
    float envmap_contribution_clamp;
    float indirect_contribution_clamp;
    float minimum_light_contribution;
    int32_t number_of_light_samples;
    bool do_alpha_testing;
    int32_t ris_number_of_light_candidates; /* RISSettings (RenderSettings.h:17-24) */
    int32_t ris_number_of_bsdf_candidates;
    MptReSTIRDISettings restir_di_settings;
} MptRenderSettings;

/* WorldSettings (HostDeviceCommon/WorldSettings.h:18-52).  The pointer fields are
 * ignored by mpt_render_frame: the envmap lives in the context (mpt_set_envmap). */
typedef struct MptWorldSettings {
    int32_t ambient_light_type;
    MptColor uniform_light_color;
    uint32_t envmap_width, envmap_height;
    float envmap_intensity;
    int32_t envmap_scale_background_intensity;
    void* envmap;
    float envmap_total_sum;
    float* envmap_cdf;
    int32_t* alias_table_alias;
    float* alias_table_probas;
    MptFloat4x4 envmap_to_world_matrix;
    MptFloat4x4 world_to_envmap_matrix;
} MptWorldSettings;

/* HIPRTCamera (HostDeviceCommon/HIPRTCamera.h:16-49) */
typedef struct MptCamera {
    MptFloat4x4 inverse_view;
    MptFloat4x4 inverse_projection;
    MptFloat4x4 view_projection;
    bool do_jittering;
} MptCamera;

/* The compile-time options of KernelOptions.h that select code paths on the hot
 * path.  Defaults of the reference: bsdf_override NONE, light_sampling RIS,
 * envmap_sampling ALIAS_TABLE, envmap_bsdf_mis 1, ggx multiple scattering 1. */
typedef struct MptKernelOptions {
    int32_t bsdf_override;                 /* BSDFOverride (KernelOptions.h:116) */
    int32_t direct_light_sampling;         /* DirectLightSamplingStrategy (KernelOptions.h:218) */
    int32_t envmap_sampling;               /* EnvmapSamplingStrategy (KernelOptions.h:231) */
    int32_t envmap_bsdf_mis;               /* EnvmapSamplingDoBSDFMIS (KernelOptions.h:242) */
    int32_t ris_use_visibility;            /* RISUseVisiblityTargetFunction (KernelOptions.h:252) */
    int32_t restir_di_bias_correction_weights;        /* ReSTIR_DI_BiasCorrectionWeights (KernelOptions.h:335),
                                                         MPT_RESTIR_DI_BIAS_* */
    int32_t restir_di_bias_correction_use_visibility; /* ReSTIR_DI_BiasCorrectionUseVisibility (KernelOptions.h:304) */
    int32_t restir_di_later_bounces_sampling_strategy; /* ReSTIR_DI_LaterBouncesSamplingStrategy (KernelOptions.h:355),
                                                          MPT_RESTIR_DI_LATER_BOUNCES_* */
    int32_t restir_di_initial_target_visibility; /* ReSTIR_DI_InitialTargetFunctionVisibility (KernelOptions.h:270), 0 */
    int32_t restir_di_spatial_target_visibility; /* ReSTIR_DI_SpatialTargetFunctionVisibility (KernelOptions.h:279), 1 */
    int32_t restir_di_do_visibility_reuse;       /* ReSTIR_DI_DoVisibilityReuse (KernelOptions.h:289), 1 */
    int32_t restir_di_do_lights_presampling;     /* ReSTIR_DI_DoLightsPresampling (KernelOptions.h:366), 1; 0: no
                                                    presampling pass and no seed drawn for it (restir_di_seeds[0] unused) */
} MptKernelOptions;

#define MPT_RESTIR_DI_LATER_BOUNCES_UNIFORM_ONE_LIGHT 0 /* KernelOptions.h:73-76 */
#define MPT_RESTIR_DI_LATER_BOUNCES_BSDF 1
#define MPT_RESTIR_DI_LATER_BOUNCES_MIS_LIGHT_BSDF 2
#define MPT_RESTIR_DI_LATER_BOUNCES_RIS_BSDF_AND_LIGHT 3

#define MPT_RESTIR_DI_BIAS_1_OVER_M 0 /* KernelOptions.h:66-71 */
#define MPT_RESTIR_DI_BIAS_1_OVER_Z 1
#define MPT_RESTIR_DI_BIAS_MIS_LIKE 2
#define MPT_RESTIR_DI_BIAS_MIS_GBH 3
#define MPT_RESTIR_DI_BIAS_PAIRWISE_MIS 4
#define MPT_RESTIR_DI_BIAS_PAIRWISE_MIS_DEFENSIVE 5

/* BRDFsData flags (HostDeviceCommon/BSDFsData.h:24-62), the LUTs themselves are
 * uploaded once with mpt_set_luts. */
typedef struct MptBSDFFlags {
    bool white_furnace_mode;
    bool white_furnace_mode_turn_off_emissives;
    bool clearcoat_compensation_approximation;
    int32_t ggx_masking_shadowing; /* 0 HeightCorrelated, 1 HeightUncorrelated */
} MptBSDFFlags;

/* Everything one sample-per-pixel pass needs (the by-value HIPRTRenderData of
 * the reference, minus device pointers which the library owns). */
typedef struct MptFrame {
    MptRenderSettings render_settings;
    MptWorldSettings world_settings;
    MptCamera current_camera;
    MptCamera prev_camera;
    MptKernelOptions options;
    MptBSDFFlags bsdf_flags;
    uint32_t random_seed;   /* HIPRTRenderData::random_seed (RenderData.h:146) */
    int32_t res_x, res_y;   /* int2 res kernel argument */
    /* Framebuffer row partition for multi-GPU tiling: this context renders the
     * rows y with (y / band_height) % band_count == band_index.  (1, 0, 1) renders
     * the whole frame.  Per-pixel RNG seeds use the global pixel index so a
     * partitioned render is bit-identical to a single-device one. */
    int32_t band_height, band_index, band_count;
    /* Seed of the CameraRays launch (GPURenderer::launch_camera_rays draws a new
     * m_rng.xorshift32() per launch, GPURenderer.cpp:468-474); 0 = use random_seed for
     * the camera rays too (CPURenderer: one seed per sample, CPURenderer.cpp:271-287). */
    uint32_t camera_random_seed;
    /* LSS_RESTIR_DI: the seeds ReSTIRDIRenderPass::launch draws from the renderer's RNG
     * (ReSTIRDIRenderPass.cpp:233-264, 298-431) that its kernels see as random_seed:
     * [0] lights presampling, [1] initial candidates, [2] the fused spatiotemporal pass
     * (the draw of configure_spatial_pass_for_fused_spatiotemporal(0), after the temporal
     * seed and the permutation bits) or, unfused, the temporal pass, [3] the
     * permutation-sampling bits (the kernels read them from
     * render_settings.restir_di_settings, where the caller stores them as the reference
     * does), [4 + i] spatial pass i (unfused: i >= 0; fused: i >= 1).  Hence
     * number_of_passes <= 4. */
    uint32_t restir_di_seeds[8];
} MptFrame;

/* Scene arrays as produced by the reference's SceneParser (Scene/SceneParser.h:80-131). */
typedef struct MptScene {
    const int32_t* triangle_indices;   /* 3 * num_triangles */
    int32_t num_triangles;
    const float* vertices;             /* 3 * num_vertices  (float3) */
    const float* vertex_normals;       /* 3 * num_vertices */
    const uint8_t* has_vertex_normals; /* num_vertices */
    const float* texcoords;            /* 2 * num_vertices  (float2) */
    int32_t num_vertices;
    const int32_t* material_indices;   /* num_triangles */
    const MptMaterial* materials;
    int32_t num_materials;
    const int32_t* emissive_triangle_indices;
    int32_t num_emissive_triangles;
    /* 8-bit textures, tightly packed one after the other, RGBA8 per texel */
    int32_t num_textures;
    const uint8_t* const* texture_data; /* num_textures pointers, RGBA8 (4 channels) */
    const int32_t* texture_dims;        /* 2 * num_textures (width, height) */
} MptScene;

/* Energy-compensation LUTs (data/BRDFsData, GPUBakerConstants.h:15-32), float32,
 * x fastest (cos_theta_o), then y (roughness), then z (ior / layer); already flipped
 * vertically as Image32Bit::read_image_hdr(..., flipY=true) does (CPURenderer.cpp:93-132). */
typedef struct MptLuts {
    const float* ggx_conductor_ess;        /* 128 x 128 */
    const float* glossy_dielectric_ess;    /* 128 x 64 x 128 */
    const float* ggx_glass_ess;            /* 256 x 16 x 128 */
    const float* ggx_glass_inverse_ess;    /* 256 x 16 x 128 */
    const float* ggx_thin_glass_ess;       /* 32 x 32 x 96 */
    const float* sheen_ltc_params;         /* 32 x 32 x 3 */
} MptLuts;

/* Counters and timings, cumulative since the last mpt_enable_stats call.
 * Ray counts are always collected; node/triangle counts only with the instrumented
 * traversal; times only when timing is enabled (hipEvents around every traversal launch
 * and around every frame, read back without stalling the stream). */
typedef struct MptStats {
    uint64_t rays_closest;      /* closest-hit queries (camera/continuation + NEE BSDF/light rays) */
    uint64_t rays_any;          /* any-hit (shadow) queries */
    uint64_t node_visits;       /* BVH8 node fetches, all stages (instrumented) */
    uint64_t triangle_tests;    /* triangle record fetches, all stages (instrumented) */
    uint32_t trace_launches;    /* traversal kernel launches */
    uint32_t frames;            /* samples rendered (one per mpt_render_frame, count per mpt_render_frames) */
    double trace_ms;            /* summed traversal kernel time */
    double frame_ms;            /* summed whole-frame time */
    /* per traversal stage: 0 = path rays (camera / continuation, closest hit),
     * 1 = NEE shadow rays (any hit), 2 = NEE BSDF / light rays (closest hit) */
    uint64_t stage_rays[3];         /* queries, always counted */
    uint64_t stage_traversals[3];   /* BVH traversals (instrumented; >= queries: boundary skips retrace) */
    uint64_t stage_nodes[3];
    uint64_t stage_tris[3];
    double stage_ms[3];
    uint32_t stage_launches[3];
    uint32_t shade_launches;
    /* summed time of the other kernels (timing enabled) */
    double camera_ms;
    double shade_ms;
    double resolve_ms;
    double accumulate_ms;
    double compact_ms;
    double restir_ms;           /* ReSTIR DI passes (presampling .. spatial reuse) */
    /* instrumented traversal, per stage: wave-level node / triangle iterations x 64 (the
     * lane slots they occupied); stage_nodes / stage_node_slots = SIMD utilisation */
    uint64_t stage_node_slots[3];
    uint64_t stage_tri_slots[3];
    /* path rays that hit a surface (shaded by the shade stage; the rest by the miss stage) */
    uint64_t path_hits;
    double split_ms;            /* hit / miss partition of the path queue */
    double miss_ms;             /* miss shading (sky / envmap) */
    /* material-class shading: shade_ms / shade_launches time the plain-dielectric kernel
     * (the Lambert override and MPT_SHADE_CLASSES=0: the one shading kernel), these the
     * generic-material kernel and the vertices it shaded */
    double shade_generic_ms;
    uint64_t shade_generic_vertices;
    /* the ReSTIR DI kernels one by one (timing enabled): 0 G-buffer (k_gbuffer), 1 lights
     * presampling, 2 initial candidates, 3 temporal or fused spatiotemporal reuse, 4 spatial
     * reuse passes; summed time and launches */
    double restir_kernel_ms[5];
    uint32_t restir_kernel_launches[5];
    /* the staged reuse passes' plain-class target-function evaluations (k_rsp_eval, Principled
     * BSDF): summed time, launches and evaluation items */
    double restir_eval_ms;
    uint32_t restir_eval_launches;
    uint64_t restir_eval_items;
    /* one-sample launch sets (MPT_GRAPHS): captured HIP graphs and replays of them */
    uint32_t graph_captures;
    uint32_t graph_replays;
    /* path-tracing batches launched as two overlapped halves on two streams (MPT_OVERLAP): their
     * kernels share the GPU, so the per-kernel times above overlap */
    uint32_t overlapped_batches;
    /* the library's halo exchange (mpt_set_halo_native): exchange points served, halo
     * agreements run (the all-reduce of a moving camera), bytes sent to / received from peers
     * (mode 2: the bytes a rank would move; mpt_halo_plan's operations) */
    uint64_t halo_exchanges;
    uint64_t halo_agreements;
    uint64_t halo_bytes_sent;
    uint64_t halo_bytes_received;
    /* batched ReSTIR DI wavefronts whose later bounces ran on the second stream beside the next
     * batch's per-sample chain (MPT_RESTIR_OVERLAP) */
    uint32_t restir_overlapped_batches;
    /* path traversals launched ahead, beside the previous bounce's NEE traversals and resolve
     * (MPT_TRACE_AHEAD): their times and those of the NEE traversals overlap */
    uint32_t trace_ahead_launches;
    /* wavefronts whose bounces ran pipelined (MPT_PIPELINE: a bounce's NEE traversals and resolve
     * beside the next bounce's split and shading): their kernels' times overlap */
    uint32_t pipelined_batches;
} MptStats;

#define MPT_FB_COLOR 0        /* 'pixels': running SUM of samples (RenderData.h:34-36) */
#define MPT_FB_ALBEDO 1       /* denoiser_albedo */
#define MPT_FB_NORMALS 2      /* denoiser_normals */

/* Adaptive-sampling buffers (AuxiliaryBuffers, RenderData.h:62-84), 4 bytes per pixel */
#define MPT_AUX_SAMPLE_COUNT 0            /* pixel_sample_count (int32) */
#define MPT_AUX_CONVERGED_SAMPLE_COUNT 1  /* pixel_converged_sample_count (int32, -1 = not converged) */
#define MPT_AUX_SQUARED_LUMINANCE 2       /* pixel_squared_luminance (float) */
/* ReSTIR DI reservoirs of the whole frame (3 float4 per pixel: {M, weight_sum, UCW, triangle},
 * {point, target_function}, {flags}): the last frame's output, the other spatial buffer (the
 * fused pass's output when a spatial pass followed it) and the initial candidates */
#define MPT_AUX_RESTIR_OUTPUT 3
#define MPT_AUX_RESTIR_OTHER 4
#define MPT_AUX_RESTIR_INITIAL 5

/* StatusBuffersValues (Renderer/StatusBuffersValues.h:9-21) */
typedef struct MptStatus {
    bool one_ray_active;              /* at least one pixel still sampled in the last frame */
    uint32_t pixel_converged_count;   /* pixels converged (adaptive sampling / stop noise threshold) */
} MptStatus;

typedef struct MptContext MptContext;

/* ReSTIR DI across a row partition (the C4 configuration on 1-8 GPUs).
 * The spatial / spatiotemporal reuse passes read neighbouring pixels' G-buffer entries and
 * reservoirs (FusedSpatiotemporalReuse.h:112-586, SpatialReuse.h:52-348), and the temporal
 * reuse reads the previous frame's data around each pixel's reprojection (Utils.h:371-421),
 * so a context that renders one contiguous band of rows (band_count > 1,
 * band_height * band_count >= res_y) keeps its ReSTIR buffers frame-sized and asks the host
 * to fill the rows around its band from the contexts that own them.  The result is
 * bit-identical to a single-context render.
 *
 * Each buffer is a frame-sized, row-major array of per-pixel records on the context's device
 * (pixel (x, y) at byte (y * res_x + x) * bytes_per_pixel).  The callback is invoked from
 * mpt_render_frame after the producing kernels were enqueued on `stream` (not necessarily
 * finished).  Before it returns it must have arranged (enqueued on `stream`, or completed)
 * that rows [max(0, own_y0 - halo_rows), own_y0) and [own_y1, min(res_y, own_y1 + halo_rows))
 * of every buffer hold the owning contexts' values, and must provide its own rows to its
 * neighbours' callbacks of the same phase.  Returns 0, or non-zero to fail the frame.
 *
 * Phases, in order, per frame:
 *  MPT_HALO_GBUFFER       after the G-buffer pass.  On entry halo_rows is what THIS context
 *                         needs (measured: the largest reprojection offset of its pixels
 *                         plus the reuse radius and temporal search extent -- the
 *                         reference's reprojection is not confined to a pixel's
 *                         neighbourhood).  The callback agrees on the maximum over all
 *                         contexts, exchanges with it and stores it back in halo_rows --
 *                         unless halo_agreed is set: the frame's camera did not move, so every
 *                         context derived the same halo from the frame alone (a pixel
 *                         reprojects onto itself) without waiting for its G-buffer, and the
 *                         callback may skip the agreement (and any host synchronisation).
 *  MPT_HALO_PREV_GBUFFER  only when the agreed halo grew since the previous frame: the
 *                         previous frame's G-buffer rows the context did not maintain.
 *  MPT_HALO_RESERVOIRS    the temporal input before the fused pass (pass 0), then the
 *                         output of pass i - 1 before spatial pass i. */
#define MPT_HALO_GBUFFER 0
#define MPT_HALO_RESERVOIRS 1
#define MPT_HALO_PREV_GBUFFER 2
#define MPT_HALO_MAX_BUFFERS 12
typedef struct MptHaloExchange {
    int32_t phase;        /* MPT_HALO_* */
    int32_t pass;         /* reservoirs: the reuse pass about to read them (0 = fused spatiotemporal) */
    int32_t res_x, res_y;
    int32_t own_y0, own_y1;
    int32_t halo_rows;    /* MPT_HALO_GBUFFER: in = needed here, out = agreed maximum */
    int32_t n_buffers;
    void* buffers[MPT_HALO_MAX_BUFFERS];
    int64_t bytes_per_pixel[MPT_HALO_MAX_BUFFERS];
    void* stream;         /* hipStream_t */
    int32_t halo_agreed;  /* MPT_HALO_GBUFFER: halo_rows is already the same in every context */
} MptHaloExchange;
typedef int (*MptHaloExchangeFn)(void* user, MptHaloExchange* x);

const char* mpt_last_error(void);
int mpt_version(void);
/* sizes of the mirrored structs as compiled into the library (ABI check): MptMaterial,
 * MptRenderSettings, MptWorldSettings, MptCamera, MptFrame, MptScene, MptStats, MptDisplaySettings */
int mpt_abi_sizes(int32_t* out_sizes, int n);
/* The HIP device's marketing name, its gfx architecture string and compute-unit count (the
 * bench line's device identity); any output may be NULL. */
int mpt_device_info(int device, char* name, int32_t name_cap, char* arch, int32_t arch_cap, int32_t* out_cus);

int mpt_create(int device, void* hip_stream, MptContext** out_ctx);
int mpt_destroy(MptContext* ctx);
int mpt_upload_scene(MptContext* ctx, const MptScene* scene);
int mpt_update_materials(MptContext* ctx, const MptMaterial* materials, int32_t count);

/* Geometry updates (DESIGN.md §2 "Geometry updates").  What mpt_update_vertices reports; filling it
 * costs a download of the exact node boxes, so it is only done when asked for.  area_ratio: the
 * sum over the scene BVH's nodes of the surface area of the node's exact box after the refit,
 * divided by the same sum at the last mpt_upload_scene (host, double, node order): 1 after an
 * identity update; the host decides from it when a real rebuild (mpt_upload_scene) is due.
 * light_*: the same of the light-hit BVH, against its last build (a material edit that changes
 * the light set rebuilds it); zeros when no light BVH is in use. */
typedef struct MptRefitInfo {
    int32_t nodes, levels, light_nodes, light_levels;
    float area_ratio, light_area_ratio;
} MptRefitInfo;
/* Replaces the vertex positions of the uploaded scene (and its vertex normals when given);
 * topology, indices, materials, textures, has_vertex_normals and the emissive list stay.  The
 * context's streams are drained, the arrays uploaded, and everything derived from positions is
 * brought up to date on the GPU: the triangle records and node boxes of the scene BVH and of the
 * light-hit BVH (a refit: the trees keep their topology and depth), the per-triangle attributes,
 * the emissive-triangle table, the box pad.  Traversal results never depend on the BVH, so they
 * equal those of a fresh upload of the new scene bit for bit; a tree refitted far from its build
 * traverses more slowly (MptRefitInfo::area_ratio).
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT for NULL vertices, a vertex count
 * that differs from the scene's or a non-finite coordinate -- a refused call changes nothing.
 * MPT_ERR_HIP part-way through leaves the context without a scene: upload again.
 * The caller's next frame must carry render_settings.need_to_reset (sample_number 0), as the
 * reference's does when its scene changes: accumulated samples, ReSTIR DI reservoirs, G-buffers
 * and adaptive-sampling counters of the old geometry are stale.  The library checks nothing
 * about it. */
int mpt_update_vertices(MptContext* ctx, const float* vertices, const float* vertex_normals_or_NULL,
                        int32_t num_vertices, MptRefitInfo* info_or_NULL);
/* Per-object motion (DESIGN.md §2 "Geometry updates", Transforms): the scene stays one flat triangle
 * soup; an object is a set of its vertices that moves by one 3x4 matrix.  mpt_set_objects sets the
 * table once: vertex_object[i] in [-1, num_objects) is vertex i's object (-1: static), num_vertices
 * the scene's count, num_objects >= 1.  The ids and a mask of the vertices the triangles use go to
 * the device, and the REST POSE is captured: a device-to-device copy of the positions and vertex
 * normals the context holds at that moment (after any earlier update).  Every later
 * mpt_update_transforms moves the rest pose, never the previous call's result.
 * mpt_update_vertices, mpt_update_vertices_device and rebuilds leave the rest pose as captured;
 * mpt_upload_scene and mpt_upload_scene_mode drop the objects (a new scene).  NULL with
 * num_objects 0 frees the table, the rest pose and the staging arrays.  A skin (mpt_set_skin)
 * and an object table exclude each other: setting the table drops a skin, and a morph
 * (mpt_set_morph) with it.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, for a vertex count
 * other than the scene's, num_objects < 1 with a table, or an id out of range. */
int mpt_set_objects(MptContext* ctx, const int32_t* vertex_object, int32_t num_vertices, int32_t num_objects);
/* Moves the objects: matrices is num_objects x 12 floats on the host, per object a row-major 3x4
 * matrix m applied to the rest pose by a kernel (csrc/xform.h has the arithmetic, shared with
 * mpt_transform_host byte for byte):
 *   position  p'[r] = ((m[r][0]*x + m[r][1]*y) + m[r][2]*z) + m[r][3]      (fp32, no fma)
 *   normal    N n / |N n| with N the cofactor matrix of m's linear part times the sign of its
 *             determinant (made on the host in double, rounded to float); a normal whose N n has
 *             a zero or non-finite squared length passes through (the zero normals of vertices
 *             without has_vertex_normals)
 * An object whose 12 floats are exactly the identity (1 and +0) and the vertices of object -1 pass
 * through byte for byte, so an all-identity call changes no bit and reports area_ratio 1.
 * The context's streams are drained as by mpt_update_vertices; the kernel writes staging arrays
 * and reduces the largest |coordinate| over the vertices in use and a non-finite flag on the
 * device; two words are read back; the staging arrays are then swapped in for the positions and
 * normals, and the refit, the per-triangle attributes, the emissive table and the box pad follow
 * as in mpt_update_vertices -- with the same bytes as mpt_update_vertices of mpt_transform_host's
 * output.  No vertex array crosses the bus and the host makes no pass over the vertices.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, when no objects are
 * set, num_objects differs from the table's, a matrix entry is not finite (checked on the host) or
 * a transformed coordinate of any vertex is not finite (the device's flag).  MPT_ERR_HIP part-way
 * leaves the context without a scene.  The reset rule and info are those of mpt_update_vertices.
 * The MPT_REFIT_HOST test hook does not apply to this call or to mpt_update_vertices_device: they
 * always refit on the GPU.  MPT_XFORM_GROUP=1 in the environment (read at the call) makes the
 * kernels take one vertex per lane instead of four: the same bytes, a measuring aid. */
int mpt_update_transforms(MptContext* ctx, const float* matrices, int32_t num_objects, MptRefitInfo* info_or_NULL);
/* mpt_update_vertices for arrays that already live in the memory of the context's device
 * (3 floats per vertex, any alignment): a kernel first checks the caller's positions (finite, and
 * the maximum over the vertices in use), so a refusal changes nothing; then device-to-device copies
 * and the same refit and tables.  The same refusals, and the same bytes afterwards, as
 * mpt_update_vertices of the same values; a pointer that is not memory of the context's device is
 * refused with MPT_ERR_INVALID_ARGUMENT.  The reads are enqueued on the context's stream: THE CALLER
 * GUARANTEES that the arrays are complete with respect to that stream (e.g. by synchronising the
 * stream that wrote them).  The call returns after the stream is synchronised, so the arrays may
 * be reused at once. */
int mpt_update_vertices_device(MptContext* ctx, const float* d_vertices, const float* d_normals_or_NULL,
                               int32_t num_vertices, MptRefitInfo* info_or_NULL);
/* No device needed: the host loop of csrc/xform.h -- what mpt_update_transforms writes for a rest
 * pose, a table and matrices (rest_normals NULL: positions only, out_normals must then be NULL).
 * MPT_ERR_INVALID_ARGUMENT for a NULL array, an id out of [-1, num_objects), a non-finite matrix
 * entry or a non-finite output coordinate; the outputs are then unspecified, the inputs untouched. */
int mpt_transform_host(const float* rest_vertices, const float* rest_normals_or_NULL, const int32_t* vertex_object,
                       int32_t num_vertices, const float* matrices, int32_t num_objects, float* out_vertices,
                       float* out_normals_or_NULL);
/* Skinning (DESIGN.md §2 "Geometry updates", Skinning): linear-blend skinning of the flat scene, the
 * general case of which an object of mpt_set_objects is the one-joint, weight-1 instance.
 * mpt_set_skin sets the table once: joints and weights hold num_vertices x 4 entries, per vertex
 * four indices into a palette of num_joints >= 1 joints and their four weights (all four zero: the
 * vertex is not skinned).  The tables and a mask of the vertices the triangles use go to the
 * device, and the REST POSE is captured exactly as by mpt_set_objects.  Every later
 * mpt_update_skin skins the rest pose, never the previous call's result.
 * A skin and an object table exclude each other and share the rest pose and the staging arrays:
 * mpt_set_skin drops an object table and mpt_set_objects drops a skin; mpt_upload_scene and
 * mpt_upload_scene_mode drop either.  mpt_update_vertices, mpt_update_vertices_device and rebuilds
 * leave the rest pose as captured.  NULL tables with num_joints 0 free the skin, the rest pose and
 * the staging arrays (and leave an object table alone, as mpt_set_objects(NULL) leaves a skin).
 * A morph (mpt_set_morph, below) composes with the skin and shares its rest pose: with a morph set,
 * mpt_set_skin does not capture the rest pose again, and NULL tables free only the skin's tables.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, for a vertex count
 * other than the scene's, num_joints < 1 with a table, an index outside [0, num_joints) in any slot
 * (whatever its weight) or a weight that is not finite. */
int mpt_set_skin(MptContext* ctx, const int32_t* joints, const float* weights, int32_t num_vertices, int32_t num_joints);
/* The most joints whose records (64 bytes each) mpt_update_skin's kernel stages in LDS; a larger
 * palette is gathered through the cache.  Both give the same bytes. */
#define MPT_SKIN_LDS_JOINTS 256
/* Poses the skin: joint_matrices is num_joints x 12 floats on the host, per joint a row-major 3x4
 * matrix M_j relative to the pose at mpt_set_skin, applied to the rest pose by a kernel
 * (csrc/skin.h has the arithmetic, shared with mpt_skin_host byte for byte; fp32, no fma):
 *   blend     B[e] = ((w0*M_j0[e] + w1*M_j1[e]) + w2*M_j2[e]) + w3*M_j3[e], the 12 entries e
 *   position  p'[r] = ((B[r][0]*x + B[r][1]*y) + B[r][2]*z) + B[r][3]
 *   normal    N n / |N n| with N the cofactor matrix of B's linear part times the sign of its
 *             determinant, computed per vertex in fp32 (each cofactor a*b - c*d with two rounded
 *             products, the determinant (a00*c00 + a01*c01) + a02*c02); a zero or non-finite
 *             squared length passes the rest normal through
 * A vertex passes through byte for byte when its four weights are all zero or when every joint with
 * a non-zero weight has exactly the identity matrix (1 and +0), so an all-identity pose changes no
 * bit and reports area_ratio 1, whatever the weights sum to.
 * The flow is mpt_update_transforms': streams drained, 64 bytes per joint uploaded, the kernel
 * writes staging arrays and reduces the largest |coordinate| over the vertices in use and a
 * non-finite flag, two words are read back, the staging arrays are swapped in, and the refit, the
 * per-triangle attributes, the emissive table and the box pad follow -- with the same bytes as
 * mpt_update_vertices of mpt_skin_host's output.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, when no skin is
 * set, num_joints differs from the table's, a matrix entry is not finite (checked on the host) or a
 * skinned coordinate of any vertex is not finite (the device's flag); the joint records are
 * uploaded into a staging buffer and kept only when the call is accepted.  With a morph set the call
 * evaluates the retained morph weights first, in the fused kernel (below).  MPT_ERR_HIP part-way leaves
 * the context without a scene.  The reset rule and info are those of mpt_update_vertices; the refit
 * is always the GPU's.  Measuring aids, read from the environment at the call, the same bytes:
 * MPT_SKIN_GROUP=1 takes one vertex per lane instead of four, MPT_SKIN_LDS=0 gathers the palette
 * through the cache whatever its size. */
int mpt_update_skin(MptContext* ctx, const float* joint_matrices, int32_t num_joints, MptRefitInfo* info_or_NULL);
/* No device needed: the host loop of csrc/skin.h -- what mpt_update_skin writes for a rest pose,
 * tables and matrices (rest_normals NULL: positions only, out_normals must then be NULL).
 * MPT_ERR_INVALID_ARGUMENT for a NULL array, num_joints < 1, an index outside [0, num_joints) in
 * any slot, a non-finite weight or matrix entry, or a non-finite output coordinate; the outputs are
 * then unspecified, the inputs untouched. */
int mpt_skin_host(const float* rest_vertices, const float* rest_normals_or_NULL, const int32_t* joints, const float* weights,
                  int32_t num_vertices, const float* joint_matrices, int32_t num_joints, float* out_vertices,
                  float* out_normals_or_NULL);
/* Morph targets (DESIGN.md §2 "Geometry updates", Morph targets): blend shapes of the flat scene,
 * applied BEFORE the skin as glTF does: pose = skin(morph(rest pose)).
 * mpt_set_morph sets the tables once, sparse by target: target t of num_targets >= 1 owns the
 * entries [target_offsets[t], target_offsets[t + 1]) of vertex_ids / pos_deltas / nrm_deltas (3
 * floats per entry; nrm_deltas NULL: the morph has no normal deltas).  target_offsets starts at 0
 * and never decreases (a target may be empty); the ids of a target are strictly ascending in
 * [0, num_vertices), so a vertex appears at most once per target.  The library transposes the
 * tables by vertex on the host (a stable counting sort, shared with mpt_morph_host: a vertex's
 * entries end up in ascending target order) and uploads that form.
 * STATE.  A morph composes with a skin and excludes an object table: mpt_set_morph drops an object
 * table, mpt_set_objects drops a morph as it drops a skin (a rigid object is a one-joint skin).  A
 * morph and a skin share one REST POSE and the staging arrays: whichever of the two is set first
 * captures it as mpt_set_objects does, setting the second does not capture again, and it lives
 * until both are gone -- mpt_set_skin(NULL) with a morph set frees only the skin's tables,
 * mpt_set_morph(NULL tables, num_targets 0) with a skin set frees only the morph's; without the
 * other, either frees the rest pose and the staging arrays too.  With no morph ever set every call
 * behaves as it did before morphs existed.
 * The context retains the last ACCEPTED morph weights (all zero after mpt_set_morph) and the last
 * ACCEPTED joint palette ("not posed", i.e. no skin step, after mpt_set_skin).  mpt_update_morph
 * evaluates new weights with the retained palette; mpt_update_skin with a morph set evaluates the
 * retained weights with the new palette through the fused kernel; mpt_update_morph_skin sets both:
 * one kernel, one refit.  A refused call changes nothing, the retained weights and palette
 * included: new weights and records are uploaded into staging buffers and swapped in on acceptance.
 * mpt_update_vertices, mpt_update_vertices_device and rebuilds leave rest pose, weights and palette
 * alone; mpt_upload_scene and mpt_upload_scene_mode drop everything.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, for a vertex count
 * other than the scene's, num_targets < 1 with tables, offsets that do not start at 0 or that
 * decrease, an id outside [0, num_vertices) or out of order, or a delta that is not finite. */
int mpt_set_morph(MptContext* ctx, int32_t num_targets, const int32_t* target_offsets /* [T+1] */,
                  const int32_t* vertex_ids /* [N] */, const float* pos_deltas /* [3N] */,
                  const float* nrm_deltas_or_NULL /* [3N] */, int32_t num_vertices);
/* The most targets whose weights the morph kernel stages in LDS (16 KiB); more are gathered through
 * the cache.  Both give the same bytes. */
#define MPT_MORPH_LDS_TARGETS 4096
/* Evaluates the morph: weights is num_targets floats on the host, applied to the rest pose by a
 * kernel (csrc/morph.h has the arithmetic, shared with mpt_morph_host byte for byte; fp32, no fma).
 * Per vertex, over its entries in ascending target order, those whose weight is not +0 / -0:
 *   position  acc = p; acc[r] = acc[r] + w*dp[r]          (the product rounded, then the sum)
 *   normal    with normal deltas: t = n; t[r] = t[r] + w*dn[r]; t / |t| when (t0*t0 + t1*t1) + t2*t2
 *             is positive and finite, else the rest normal.  Without normal deltas it passes through.
 * A vertex without such an entry passes through byte for byte, so all-zero weights change no bit
 * and report area_ratio 1.  When the skin has been posed, mptskin's skin_vertex (mpt_update_skin)
 * follows in the same kernel on the morphed position and normal in registers: the morphed pose is
 * never written to memory.
 * The flow is mpt_update_skin's: streams drained, 4 bytes per target uploaded (plus 64 per joint),
 * the kernel writes the staging arrays and reduces the largest |coordinate| over the vertices in
 * use and a non-finite flag, two words are read back, the arrays are swapped in, and the refit and
 * the tables follow -- with the same bytes as mpt_update_vertices of
 * mpt_skin_host(mpt_morph_host(rest pose)), or of mpt_morph_host(rest pose) alone without a posed
 * skin.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing (retained weights
 * and palette included), when no morph is set, num_targets differs from the tables', a weight is
 * not finite, or an output coordinate is not finite (the device's flag); mpt_update_morph_skin
 * also when no skin is set, num_joints differs or a matrix entry is not finite.  MPT_ERR_HIP
 * part-way leaves the context without a scene.  Measuring aids, read from the environment at the
 * call, the same bytes: the kernel takes one vertex per lane, the faster of the two as measured
 * (DESIGN.md §4), MPT_MORPH_GROUP=4 takes four with 16-byte accesses (MPT_MORPH_GROUP=1 names the
 * default); MPT_MORPH_LDS=0 stages nothing in LDS. */
int mpt_update_morph(MptContext* ctx, const float* weights, int32_t num_targets, MptRefitInfo* info_or_NULL);
int mpt_update_morph_skin(MptContext* ctx, const float* weights, int32_t num_targets,
                          const float* joint_matrices, int32_t num_joints, MptRefitInfo* info_or_NULL);
/* No device needed: the host loop of csrc/morph.h -- what mpt_update_morph writes for a rest pose,
 * tables (in mpt_set_morph's form) and weights (rest_normals NULL: positions only, out_normals must
 * then be NULL).  MPT_ERR_INVALID_ARGUMENT for a NULL array, num_vertices < 1, what mpt_set_morph
 * refuses, a non-finite weight or a non-finite output coordinate; the outputs are then
 * unspecified, the inputs untouched. */
int mpt_morph_host(const float* rest_vertices, const float* rest_normals_or_NULL, int32_t num_vertices,
                   int32_t num_targets, const int32_t* target_offsets, const int32_t* vertex_ids,
                   const float* pos_deltas, const float* nrm_deltas_or_NULL, const float* weights,
                   float* out_vertices, float* out_normals_or_NULL);
/* Recomputed normals (DESIGN.md §2 "Geometry updates", Normals): an opt-in state of the context.
 * Once set, EVERY geometry update -- mpt_update_vertices, mpt_update_vertices_device,
 * mpt_update_transforms, mpt_update_skin, mpt_update_morph, mpt_update_morph_skin and
 * mpt_update_animation -- ends with the smooth normals of the chosen vertices recomputed from the
 * new positions on the device, before the per-triangle attribute records are made.  The call itself
 * changes no normal; the next update does.  A context that never sets it behaves as before.
 *   vertex_group [V]  values in [-1, num_groups): the vertices with one id form a smoothing group
 *                     and receive one common normal; -1: the vertex is never touched
 *   group_flip [G]    optional, one byte per group: non-zero negates the group's sum (a mesh whose
 *                     winding was mirrored)
 * csrc/normals.h has the arithmetic, shared with mpt_normals_host byte for byte (fp32, no fma):
 *   table   by group, one entry (the triangle id p) for every corner (p, k) of the scene's index
 *           buffer whose vertex lies in the group, in ascending p, then k (a stable counting sort on
 *           the host; a triangle with two corners in one group appears twice)
 *   face    e1 = b - a, e2 = c - a, f = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),
 *           every product rounded before the difference
 *   sum     s = +0; s[r] = s[r] + f[r] over the group's entries in table order (area weighting);
 *           s = -s when the group's flip byte is set
 *   output  for every vertex v of the group with has_vertex_normals[v] != 0: s / sqrtf(l2) when
 *           l2 = (s0*s0 + s1*s1) + s2*s2 is positive and finite, else the normal the update itself
 *           left at v (the uploaded or deformed one): an empty group, a group of degenerate
 *           triangles and an overflowing cross product pass through, and no update is refused
 *           because of the recompute
 * Vertices of group -1 and vertices without has_vertex_normals keep their bytes (the renderer shades
 * the latter with the geometric normal).  Normals passed to mpt_update_vertices are uploaded first and
 * then overwritten for the grouped vertices.
 * The indices are the context's own copy of the scene's.  The tables are uploaded into new buffers
 * and swapped in on success.  vertex_group NULL with num_groups 0 (and group_flip NULL) frees the
 * state.  It is independent of objects, skin, morph and animation: none of them drops it and it drops
 * none of them; rebuilds and material edits leave it; mpt_upload_scene and mpt_upload_scene_mode drop
 * it.  MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, for a vertex
 * count other than the scene's, num_groups < 1 with a table, or an id outside [-1, num_groups).
 * Measuring aid, read from the environment at each update, the same bytes: by default one kernel
 * writes the face vectors (16 bytes per triangle) and a second gathers them per vertex;
 * MPT_NORMALS_FUSED=1 forms them in registers in one kernel. */
int mpt_set_normals(MptContext* ctx, const int32_t* vertex_group, const uint8_t* group_flip_or_NULL,
                    int32_t num_vertices, int32_t num_groups);
/* No device needed: the host loop of csrc/normals.h -- the normals that an update leaves on the
 * device after mpt_set_normals, for these positions, indices and groups, written over inout_normals
 * (has_vertex_normals NULL: every vertex has one).  MPT_ERR_INVALID_ARGUMENT, the arrays untouched,
 * for a NULL array, num_vertices < 1, num_triangles < 0, a vertex index outside [0, num_vertices),
 * and what mpt_set_normals refuses. */
int mpt_normals_host(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                     const int32_t* vertex_group, const uint8_t* group_flip_or_NULL, int32_t num_groups,
                     const uint8_t* has_vertex_normals_or_NULL, float* inout_normals);
/* Downloads the context's current positions and normals ([3V] floats each; either may be NULL),
 * with the streams drained: what the last update left on the device.  MPT_ERR_NO_SCENE without a
 * scene, MPT_ERR_INVALID_ARGUMENT for a vertex count other than the scene's. */
int mpt_get_vertices(MptContext* ctx, float* out_vertices_or_NULL, float* out_normals_or_NULL, int32_t num_vertices);
/* Animation clips (DESIGN.md §2 "Geometry updates", Animation): one glTF clip sampled, the node
 * hierarchy composed and the joint palette and morph weights produced ON THE DEVICE, straight into
 * the staging buffers the skin and morph kernels read: a frame of playback is one float.
 * MptAnimation is counts and host pointers (csrc/anim.h's top comment is the specification):
 *   nodes     node_parents [N] (-1: a root; a child may come before its parent), node_trs [10N]
 *             (translation 3, rotation x y z w, scale 3), node_is_trs [N] (1: the node was given as
 *             TRS and its local matrix is made from the sampled TRS; 0: given as a matrix, its
 *             node_locals entry is used and no channel may drive it), node_locals [12N] row-major
 *             3x4 float64
 *   joints    joint_nodes [J], joint_bind [12J] row-major 3x4 float64; joint j's matrix is
 *             world[joint_nodes[j]] * joint_bind[j] (two joints may share a node)
 *   targets   base_weights [T]: what an undriven target keeps
 *   samplers  sampler s owns the key times [sampler_key_offsets[s], sampler_key_offsets[s + 1]) of
 *             key_times (at least one, finite, strictly ascending) and the floats
 *             [sampler_value_offsets[s], sampler_value_offsets[s + 1]) of values: keys x width, x 3
 *             for MPT_ANIM_CUBICSPLINE (in-tangent, value, out-tangent per key); both offset arrays
 *             start at 0
 *   channels  channel_sampler, channel_node, channel_path (MPT_ANIM_PATH_*), and for a weights
 *             channel the stretch [channel_first_target, + channel_num_targets) of the weight
 *             vector (the width of its values); no two channels write the same component
 * mpt_set_animation checks the tables (check_animation), uploads them into a new buffer and swaps
 * it in when it is there; NULL frees the animation.  num_joints > 0 needs a skin with as many
 * joints, num_targets > 0 a morph with as many targets; one of the two must be driven.  It changes
 * no geometry and no retained state.  The animation is dropped wherever a skin or a morph is
 * dropped: mpt_set_objects, mpt_upload_scene*, mpt_set_skin / mpt_set_morph with new tables or NULL.
 * One clip is set at a time.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing, for a count that
 * does not fit the skin or the morph, a parent index out of range or a cycle, a joint or channel
 * node out of range, offsets that decrease, key times that are not finite or not strictly
 * ascending, a non-finite value, a stored rotation of zero length, a weights channel outside
 * [0, T), a channel on a node given as a matrix, a value count that does not match the key count,
 * or two channels that write the same component. */
#define MPT_ANIM_STEP 0
#define MPT_ANIM_LINEAR 1
#define MPT_ANIM_CUBICSPLINE 2
#define MPT_ANIM_PATH_TRANSLATION 0
#define MPT_ANIM_PATH_ROTATION 1
#define MPT_ANIM_PATH_SCALE 2
#define MPT_ANIM_PATH_WEIGHTS 3
typedef struct MptAnimation {
    int32_t num_nodes;
    int32_t num_joints;
    int32_t num_targets;
    int32_t num_samplers;
    int32_t num_channels;
    int32_t reserved;
    const int32_t* node_parents;
    const float* node_trs;
    const uint8_t* node_is_trs;
    const double* node_locals;
    const int32_t* joint_nodes;
    const double* joint_bind;
    const float* base_weights;
    const int32_t* sampler_key_offsets;
    const float* key_times;
    const int32_t* sampler_value_offsets;
    const float* values;
    const int32_t* sampler_interp;
    const int32_t* channel_sampler;
    const int32_t* channel_node;
    const int32_t* channel_path;
    const int32_t* channel_first_target;
    const int32_t* channel_num_targets;
} MptAnimation;
int mpt_set_animation(MptContext* ctx, const MptAnimation* anim_or_NULL);
/* The most nodes whose float64 world matrices the animation kernel keeps in LDS (96 bytes each,
 * 48 KiB); more live in a scratch array in memory.  Both give the same bytes. */
#define MPT_ANIM_LDS_NODES 512
/* Evaluates the clip at `time` (seconds, clamped to every sampler's key range) with one workgroup
 * (csrc/anim.hip: k_anim) -- channels sampled, local matrices made, world matrices composed level
 * by level in float64, joint records and padded weights written to the staging buffers -- and then
 * follows mpt_update_morph_skin's path with those buffers: the morph or skin kernel, ONE read of
 * the reductions (the animation's non-finite flag in the same synchronisation), the swaps, the
 * refit.  Nothing but `time` crosses the bus.  The result has the bytes mpt_update_morph_skin
 * leaves for mpt_animation_host's output (mpt_update_skin / mpt_update_morph when only one of the
 * two is driven).  On success the retained weights and palette are the evaluated ones.
 * MPT_ERR_NO_SCENE without a scene; MPT_ERR_INVALID_ARGUMENT, changing nothing (retained weights
 * and palette included), when no animation is set, `time` is not finite, a sampled value, weight or
 * matrix entry is not finite (the device's flag), or an output coordinate is not finite.
 * Measuring aid, read from the environment at the call, the same bytes: MPT_ANIM_LDS=0 keeps the
 * world matrices in memory whatever the node count. */
int mpt_update_animation(MptContext* ctx, float time, MptRefitInfo* info_or_NULL);
/* No device needed: the host loop of csrc/anim.h -- the joint matrices (num_joints x 12 floats) and
 * weights (num_targets floats) mpt_update_animation evaluates for these tables at `time`; either
 * output may be NULL.  MPT_ERR_INVALID_ARGUMENT for what mpt_set_animation refuses of the tables, a
 * non-finite time or a non-finite result; the outputs are then unspecified. */
int mpt_animation_host(const MptAnimation* anim, float time, float* out_matrices_or_NULL, float* out_weights_or_NULL);
/* Downloads a BVH of the context as the kernels read it: which 0 the scene's, 1 the light-hit
 * BVH's (counts of 0 when none is in use).  nodes: 80-byte Node8, tris: 48-byte TriRec records
 * (csrc/bvh8.h; mpt.abi.NODE8_DTYPE / TRIREC_DTYPE).  out_counts (optional): nodes, records,
 * levels.  With both caps 0 only the counts are returned. */
int mpt_get_bvh(MptContext* ctx, int which, void* nodes, int64_t nodes_cap_bytes, void* tris, int64_t tris_cap_bytes,
                int32_t* out_counts);
/* No device needed: builds the BVH8 over build_vertices as mpt_upload_scene does, refits it to
 * new_vertices with the host loop of csrc/refit.h (NULL: the builder's output unchanged) and
 * returns the bytes mpt_get_bvh(ctx, 0, ...) returns after mpt_update_vertices -- except the
 * records' two flag lanes (alpha test, material class), which a context stamps from its
 * materials and which are 0 here. */
int mpt_bvh_refit_host(const float* build_vertices, const float* new_vertices_or_NULL, int32_t num_vertices,
                       const int32_t* indices, int32_t num_triangles, void* nodes, int64_t nodes_cap_bytes,
                       void* tris, int64_t tris_cap_bytes, int32_t* out_counts);
/* Rebuilds (DESIGN.md §2 "Rebuilds").  What mpt_rebuild_bvh reports: whether each tree was replaced
 * (0 / 1) and the new tree's nodes, records and levels; light_*: the light-hit BVH (zeros when none
 * is in use or it was left as it was). */
typedef struct MptRebuildInfo {
    int32_t rebuilt, nodes, records, levels;
    int32_t light_rebuilt, light_nodes, light_records, light_levels;
} MptRebuildInfo;
/* Rebuilds the scene BVH, and the light-hit BVH when one is in use, on the GPU from the positions
 * already on the device (after any mpt_update_vertices): Morton keys, a radix sort, Karras' radix
 * tree, a greedy collapse to 8-wide nodes, then the refit's arithmetic on the new topology
 * (csrc/lbvh.h).  The context's streams are drained; no vertices are uploaded and the host makes
 * no pass over triangles or vertices.  A tree is built into new buffers and replaces the old one
 * only when complete and when 2 * levels + 2 fits the traversal stack bound mpt_upload_scene uses;
 * there is no shallower fallback.  A light-hit tree that does not fit is left as it was (refits
 * kept it valid); when the scene tree does not fit the call returns MPT_ERR_UNSUPPORTED and changes
 * nothing.  MPT_ERR_NO_SCENE without a scene.  MPT_ERR_HIP part-way through leaves the context
 * without a scene: upload again.  Afterwards MptRefitInfo's area ratios are taken against the new
 * trees (an identity update reports exactly 1), and mpt_get_bvh, mpt_update_vertices and
 * mpt_update_materials work on the new trees.
 * No frame reset is needed: traversal results never depend on the tree, so accumulation simply
 * continues across a rebuild, bit for bit as without it. */
int mpt_rebuild_bvh(MptContext* ctx, MptRebuildInfo* info_or_NULL);
/* The build modes of a rebuild.  MPT_BUILD_LBVH: Karras' radix tree as above (what mpt_rebuild_bvh
 * builds).  MPT_BUILD_PLOC: the binary tree comes from parallel locally-ordered clustering over the
 * same Morton order instead (csrc/ploc.h: radius 8, mutual nearest neighbours by the fp32 area of
 * the union merge, iterated until one cluster is left); keys, sort, collapse, slots, layout, flag
 * lanes and refit are the same code.  A lower-area tree for more build time.
 * MPT_BUILD_SAH: the binary tree comes from a top-down build with 32 bins per axis over the same
 * Morton order (csrc/sah.h: the algorithm of mpt_upload_scene's host builder, level by level, with a
 * stable partition); everything else is again the same code.  Its value is 3: 2 is not a mode and
 * stays refused with MPT_ERR_INVALID_ARGUMENT, as it always was. */
#define MPT_BUILD_LBVH 0
#define MPT_BUILD_PLOC 1
#define MPT_BUILD_SAH 3
/* mpt_rebuild_bvh with a build mode for both trees; mode 0 is mpt_rebuild_bvh, byte for byte.  An
 * unknown mode returns MPT_ERR_INVALID_ARGUMENT and changes nothing.  Every other rule of
 * mpt_rebuild_bvh holds as stated there.  MPT_PLOC_TAIL=0 in the environment (read at the call)
 * keeps mode 1 from finishing its last 1024 clusters in one workgroup: the same bytes, slower.
 * MPT_SAH_TAIL=0 sends every node of mode 3 down the path of nodes above 1024 triangles (bins in
 * global memory) instead of one wave per node: the same bytes.  MPT_SAH_DEPTH=d (both entry points)
 * lowers the depth below which mode 3 splits by count only, 40: a test hook. */
int mpt_rebuild_bvh_mode(MptContext* ctx, int32_t mode, MptRebuildInfo* info_or_NULL);
/* mpt_upload_scene with both BVH8s built on the GPU in a build mode (DESIGN.md §2 "Uploads with a
 * build mode"): the way to change topology -- an object added or removed, another index list,
 * another emissive list, a new scene -- without the host builder.  The call takes over the context
 * as mpt_upload_scene does: the same argument checks and messages, the same device arrays, box pad,
 * per-triangle attributes, resolved materials and emissive table.  No tree is built on the host:
 * the scene tree is built over all primitives as mpt_rebuild_bvh_mode builds it; the light-hit
 * tree's primitives (those whose material can emit, ascending) are selected on the device and the
 * tree built over them in the same mode; the records' flag lanes (alpha test, material class) are
 * written by the build from per-primitive words made on the device.  The trees' bytes are those of
 * mpt_bvh_build_host_mode, the flag lanes those after mpt_upload_scene.
 * The scene tree must fit the traversal stack bound as in mpt_rebuild_bvh (2 * levels + 2; no
 * shallower fallback): else MPT_ERR_UNSUPPORTED.  A light-hit tree that does not fit is dropped as
 * mpt_upload_scene drops it; one that cannot be allocated is an optimisation lost, not an error.
 * A NULL argument, a scene that mpt_upload_scene refuses or an unknown mode (2 among them) returns
 * MPT_ERR_INVALID_ARGUMENT and changes nothing.  MPT_ERR_UNSUPPORTED or MPT_ERR_HIP leaves the context WITHOUT a scene (its arrays are already the new
 * scene's): upload again.  info is filled as by mpt_rebuild_bvh_mode.  Afterwards
 * mpt_update_materials, mpt_update_vertices (area ratios against these trees), mpt_rebuild_bvh_mode
 * and mpt_get_bvh work as after a rebuild.  As after any upload, the next frame must carry
 * need_to_reset.  MPT_UPLOAD_STATS in the environment (read at the call) prints the wall time of
 * the call's phases to stderr: a measuring aid. */
int mpt_upload_scene_mode(MptContext* ctx, const MptScene* scene, int32_t mode, MptRebuildInfo* info_or_NULL);
/* No device needed: the host loop of the same definition over the list prims (NULL: all
 * num_triangles primitives in order; else num_prims > 0 scene primitive indices) -- the bytes
 * mpt_get_bvh returns after mpt_rebuild_bvh, except the records' two flag lanes, which are 0 here
 * as in mpt_bvh_refit_host.  The box pad is the whole scene's.  With both caps 0 only the counts. */
int mpt_bvh_build_host(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                       const int32_t* prims_or_NULL, int32_t num_prims, void* nodes, int64_t nodes_cap_bytes, void* tris,
                       int64_t tris_cap_bytes, int32_t* out_counts);
/* mpt_bvh_build_host with a build mode: the bytes after mpt_rebuild_bvh_mode(ctx, mode, ...). */
int mpt_bvh_build_host_mode(const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_triangles,
                            const int32_t* prims_or_NULL, int32_t num_prims, int32_t mode, void* nodes,
                            int64_t nodes_cap_bytes, void* tris, int64_t tris_cap_bytes, int32_t* out_counts);
int mpt_set_envmap(MptContext* ctx, const float* rgba, int32_t width, int32_t height,
                   const float* alias_probas, const int32_t* alias_indices, float luminance_total_sum);
/* Vose alias table in double precision, Image32Bit::compute_alias_table (Image/Image.cpp:579-659) */
int mpt_build_alias_table(const float* rgba, int32_t width, int32_t height,
                          float* out_probas, int32_t* out_alias, float* out_luminance_sum);
/* ESS_BINARY_SEARCH: the envmap luminance CDF, Image32Bit::compute_cdf (Image/Image.cpp:553-574),
 * and its upload (GPURenderer::set_envmap / RendererEnvmap.cpp:119-125; total = last element) */
int mpt_build_envmap_cdf(const float* rgba, int32_t width, int32_t height, float* out_cdf, float* out_total_sum);
int mpt_set_envmap_cdf(MptContext* ctx, const float* cdf, float total_sum);
int mpt_set_luts(MptContext* ctx, const MptLuts* luts);
int mpt_resize(MptContext* ctx, int32_t width, int32_t height);
/* Renders one sample per pixel of the context's partition, accumulating into the
 * sum framebuffer (assign when render_settings.sample_number == 0). Asynchronous. */
int mpt_render_frame(MptContext* ctx, const MptFrame* frame);
/* Renders count consecutive samples (GPURenderer::render's samples_per_frame loop,
 * GPURenderer.cpp:424-449): frames[k] is the frame of the k-th sample, each with its own
 * sample_number / seeds.  Runs of frames that differ only in sample_number, random_seed,
 * camera_random_seed, denoiser_AOV_accumulation_counter, need_to_reset and
 * do_update_status_buffers (and, for ReSTIR DI, restir_di_seeds, the permutation bits and
 * temporal_buffer_clear_requested), and need no per-sample feedback (no adaptive sampling or
 * stop-noise threshold), are traced as ONE wavefront of up to max_batch
 * (<= MPT_MAX_BATCH; <= 0: see MPT_DEFAULT_WAVEFRONT_PATHS) samples per pixel -- ReSTIR DI
 * samples (at most 32, not across a partition) run their camera rays, reuse passes and
 * first bounce one after the other and share the later bounces; the result is bit-identical
 * to count mpt_render_frame calls (samples are added to the sums in order).  Other frames
 * are rendered one by one.  Asynchronous. */
#define MPT_MAX_BATCH 128
/* max_batch <= 0 picks the wavefront size: MPT_DEFAULT_WAVEFRONT_PATHS paths (samples x pixels of
 * the partition) per launch, at most MPT_MAX_BATCH samples, and at most half of the device
 * memory that is free or already held by the context's path state (~460 B per path, +332 B in
 * textured scenes).  Whatever max_batch is, a wavefront whose path state cannot be allocated
 * is halved (the result is bit-identical) before MPT_ERR_OUT_OF_MEMORY is returned. */
#define MPT_DEFAULT_WAVEFRONT_PATHS (1 << 25)
/* paths of one wavefront (and pixels of one frame) are limited to 2^29 */
#define MPT_MAX_WAVEFRONT_PATHS (1 << 29)
int mpt_render_frames(MptContext* ctx, const MptFrame* frames, int32_t count, int32_t max_batch);
/* Installs the halo exchange of a partitioned ReSTIR DI context (see MptHaloExchange);
 * fn = NULL removes it.  Required before rendering LSS_RESTIR_DI with band_count > 1. */
int mpt_set_halo_exchange(MptContext* ctx, MptHaloExchangeFn fn, void* user);
int mpt_synchronize(MptContext* ctx);
int mpt_query_done(MptContext* ctx, int* out_done);
/* Copies the partition's rows of a framebuffer (band-major compact layout: the
 * rows owned by this context in increasing y) to dst; dst may be host or device. */
int mpt_get_framebuffer(MptContext* ctx, int kind, float* dst, int dst_is_device);
int mpt_partition_rows(int32_t res_y, int32_t band_height, int32_t band_index, int32_t band_count);
/* Multi-GPU output (SURVEY.md §8b Outputs row; GPURenderer.cpp:583-598 hands the one device's
 * 'pixels' to the display).  n contexts render the n row partitions of one frame (MptFrame
 * band_count == n, band_index 0..n-1, one band_height, same resolution; each on its own GPU or
 * several on one).  mpt_gather assembles buffer `kind` of the whole frame, row-major
 * (res_y x res_x), into dst on ctxs[root]'s device (dst_is_device) or in host memory: every
 * context's compact rows go out on its own stream (after its frames) as strided 2D copies --
 * peer copies over xGMI when the devices differ.  One host process drives all contexts.
 * Synchronous.  kind: MPT_FB_* (3 floats per pixel) or MPT_GATHER_AUX + MPT_AUX_SAMPLE_COUNT /
 * _CONVERGED_SAMPLE_COUNT / _SQUARED_LUMINANCE (4 bytes per pixel). */
#define MPT_GATHER_AUX 16
int mpt_gather(MptContext* const* ctxs, int32_t n, int32_t root, int kind, void* dst, int dst_is_device);
/* One process per GPU: an RCCL communicator over the ranks of the partition (loaded from
 * librccl.so.1 on first use).  Rank 0 calls mpt_comm_unique_id and shares the id out of band;
 * every rank then calls mpt_comm_init on its context (ncclCommInitRank, collective).
 * mpt_comm_gather is collective over the ranks: rank k's frames must carry band_count = ranks,
 * band_index = k; each rank's compact rows (padded to the largest band) travel with one
 * ncclGather over xGMI to the root, which re-interleaves them into dst (row-major frame; device
 * or host).  dst is ignored on the other ranks.  The communicator is destroyed with the
 * context.  Synchronous. */
#define MPT_COMM_ID_BYTES 128
int mpt_comm_unique_id(uint8_t* out_id, int32_t cap);
int mpt_comm_init(MptContext* ctx, int32_t nranks, int32_t rank, const uint8_t* id);
int mpt_comm_gather(MptContext* ctx, int32_t root, int kind, void* dst, int dst_is_device);
/* ReSTIR DI across the ranks of the communicator without a host callback: rank k's frames carry
 * the contiguous band (band_height = ceil(res_y / ranks), band_index = k, band_count = ranks) and
 * the library exchanges the halo rows itself -- one ncclGroupStart / ncclSend / ncclRecv group per
 * exchange point on the context's stream, the halo agreement an ncclAllReduce (max), skipped when
 * the camera did not move (MptHaloExchange.halo_agreed).  mode: 1 RCCL (after mpt_comm_init),
 * 2 the one-GPU rehearsal (the bytes a rank would receive moved by one local device copy; the
 * rows keep what the buffers held -- timing only), 0 off.  Replaces mpt_set_halo_exchange's
 * callback. */
int mpt_set_halo_native(MptContext* ctx, int32_t mode);
/* The bounce pipeline of single-stream path-tracing wavefronts (default 1, or MPT_PIPELINE at
 * mpt_create): 1 a bounce's NEE traversals and resolve beside the next bounce's split and shading,
 * 0 in line.  Images are identical either way; 0 gives every kernel the GPU to itself (the bench's
 * solo roofline).  Takes effect at the next launch; no reference counterpart (a launch schedule). */
int mpt_set_pipeline(MptContext* ctx, int32_t mode);
/* One point-to-point operation of a halo exchange point: `buffer`'s rows [row_lo, row_hi)
 * sent to (recv = 0) or received from (recv = 1) band `peer`. */
typedef struct MptHaloOp {
    int32_t peer;
    int32_t recv;
    int32_t buffer;
    int32_t row_lo, row_hi;
} MptHaloOp;
/* The operations mpt_set_halo_native's exchange issues, in issue order, for band band_index of
 * band_count contiguous bands of band_height rows (res_y rows in all), the agreed halo_rows and
 * n_buffers buffers: per peer in increasing order, per buffer, the sends of this band's rows in
 * the peer's upper and lower halo, then the receives of the peer's rows in this band's upper and
 * lower halo.  Writes at most cap entries to out, returns the count (< 0: error).  Host only. */
int mpt_halo_plan(int32_t res_y, int32_t band_height, int32_t band_count, int32_t band_index, int32_t halo_rows,
                  int32_t n_buffers, MptHaloOp* out, int32_t cap);
/* Status buffers: mpt_clear_status <- GPURenderer::internal_update_clear_device_status_buffers
 * (GPURenderer.cpp:275-283, once per displayed frame); the last sample of the frame sets
 * render_settings.do_update_status_buffers; mpt_query_status <- copy_status_buffers (.cpp:269-273). */
int mpt_clear_status(MptContext* ctx);
int mpt_query_status(MptContext* ctx, MptStatus* out);
/* Copies an MPT_AUX_* buffer of the partition (n_slots * 4 bytes; the ReSTIR DI kinds: frame pixels * 48 bytes) to dst (host or device). */
int mpt_get_aux_buffer(MptContext* ctx, int kind, void* dst, int dst_is_device);
int mpt_enable_stats(MptContext* ctx, int enable, int instrumented);
int mpt_get_stats(MptContext* ctx, MptStats* out);
/* Energy-compensation LUT baker, GPUBaker::bake_* (Renderer/Baker/GPUBaker.cpp:35-97,
 * GPUBakerKernel.cpp:22-151, Device/kernels/Baking/ headers): Monte-Carlo directional albedo of
 * a GGX lobe per texel, x = cos(theta_o) fastest, then y = roughness, then z = IOR (F0^4
 * parameterisation), with the reference's launch structure and seeds (so the table is
 * deterministic), integration_sample_count samples per texel.  The output is the baked
 * buffer as the reference writes it to its .hdr files (rows not flipped; the renderer's
 * MptLuts hold each slice flipped vertically, as read_image_hdr(flipY=true) loads them).
 * Reference sizes / sample counts (GPUBakerConstants.h:15-32, *Settings.h):
 *   GGX_CONDUCTOR       128 x 128 x 1,  65536        GGX_FRESNEL 256 x 256 x 256, 65536
 *   GLOSSY_DIELECTRIC   128 x 64 x 128, 131072       GGX_GLASS(_INVERSE) 256 x 16 x 128, 65536
 *   GGX_THIN_GLASS      32 x 32 x 96,   65536
 * Synchronous; out may be host or device memory. */
#define MPT_BAKE_GGX_CONDUCTOR 0
#define MPT_BAKE_GGX_FRESNEL 1
#define MPT_BAKE_GLOSSY_DIELECTRIC 2
#define MPT_BAKE_GGX_GLASS 3
#define MPT_BAKE_GGX_GLASS_INVERSE 4
#define MPT_BAKE_GGX_THIN_GLASS 5
int mpt_bake_lut(MptContext* ctx, int kind, int32_t width, int32_t height, int32_t depth, int32_t sample_count,
                 float* out, int out_is_device);
/* Raw ray queries against the uploaded BVH8 (parity / microbenchmarks).
 * rays: n * 8 floats (ox, oy, oz, tmin_unused, dx, dy, dz, tmax); last_hit: n ints (-1 = none).
 * Outputs (may be NULL): prim (n ints, -1 on miss), t, u, v (n floats).  Host or device pointers. */
int mpt_trace_closest(MptContext* ctx, const float* rays, const int32_t* last_hit, int32_t n,
                      int32_t* out_prim, float* out_t, float* out_u, float* out_v, int pointers_are_device);
int mpt_trace_any(MptContext* ctx, const float* rays, const int32_t* last_hit, int32_t n,
                  uint8_t* out_occluded, int pointers_are_device);

/* Host helper of the glTF texture loader (mpt/image.py; the reference decodes textures with
 * stb_image in Image8Bit::read_image, Image.cpp:33-61): reverses the PNG scanline filters
 * (None / Sub / Up / Average / Paeth) of `rows` inflated rows, each a filter-type byte
 * followed by row_bytes bytes, into out (rows * row_bytes).  bpp = bytes per complete pixel
 * (rounded up to 1).  No context, no GPU. */
int mpt_png_unfilter(const uint8_t* filtered, int64_t filtered_size, uint8_t* out, int32_t rows, int32_t row_bytes,
                     int32_t bpp);
/* JPEG decode with stb_image's semantics (stbi_load in Image8Bit::read_image, Image.cpp:33-61: the
 * reference's textured scene ships JPEG textures): baseline / extended / progressive Huffman,
 * 1 / 3 / 4 components, any integer sampling ratio; the islow integer IDCT, the 2:1 triangle
 * upsampling and fixed-point YCbCr conversion of stb_image's x86-64 build, bit for bit.
 * req_comp 0 = the file's own (3 for colour, 1 for grey), else 1..4.  out = NULL: only the
 * header is read (w, h, the file's component count); else out_cap >= w * h * n bytes, rows top
 * to bottom.  No context, no GPU. */
int mpt_jpeg_decode(const uint8_t* data, int64_t size, int32_t req_comp, uint8_t* out, int64_t out_cap,
                    int32_t* out_w, int32_t* out_h, int32_t* out_comp);
/* Radiance .hdr (RGBE, flat or RLE scanlines) decode with stbi_loadf's semantics
 * (Image32Bit::read_image_hdr, Image.cpp:342-370: envmaps, RendererEnvmap.cpp:39-48, and the
 * baked LUTs, GPURenderer.cpp:122-170): float = mantissa * 2^(e - 136), req_comp 1 / 2 average the
 * three channels, alpha 1.  out = NULL: dimensions only.  Rows top to bottom (the caller flips). */
int mpt_hdr_decode(const uint8_t* data, int64_t size, int32_t req_comp, float* out, int64_t out_cap,
                   int32_t* out_w, int32_t* out_h);

/* ------------------------------------------------------------------------- */
/* Display views and screenshots: the sums as 8-bit RGBA                      */
/* ------------------------------------------------------------------------- */
/* The reference turns its buffers into an image with seven display shaders (src/Shaders/ *.frag),
 * which DisplayViewSystem::display runs once per displayed frame and Screenshoter::write_to_png
 * (Screenshoter.cpp:129-166) runs as compute shaders writing RGBA8.  Here the same arithmetic, in
 * fp32 and in the order written, is one kernel on the context's stream (csrc/display.hip) and one
 * host loop (the same pixel functions, csrc/display.h); the two agree bit for bit.
 * Views, numbered as DisplayViewType (DisplayViewEnum.h; the two denoised-AOV views, which the
 * reference has disabled, are not offered): */
#define MPT_VIEW_DEFAULT 0                    /* default_display.frag: 'pixels' / sample_number, tonemapped */
#define MPT_VIEW_BLEND 1                      /* blend_2_display.frag (DENOISED_BLEND): 'pixels' and a second RGB sum */
#define MPT_VIEW_NORMALS 2                    /* normal_display.frag: the normals AOV */
#define MPT_VIEW_ALBEDO 4                     /* albedo_display.frag: the albedo AOV */
#define MPT_VIEW_PIXEL_CONVERGENCE_HEATMAP 6  /* heatmap_int.frag: pixel_converged_sample_count */
#define MPT_VIEW_PIXEL_CONVERGED_MAP 7        /* boolmap_int.frag: pixel_converged_sample_count */
#define MPT_VIEW_WHITE_FURNACE_THRESHOLD 8    /* white_furnace_threshold.frag: 'pixels' */
#define MPT_DISPLAY_MAX_STOPS 16

/* The shaders' uniforms (DisplaySettings.h and what update_display_program_uniforms derives,
 * DisplayViewSystem.cpp:198-329).  Every component v of a shader's output becomes the byte
 * trunc(v * 255) (uvec4(v * 255)), saturated to [0, 255], NaN -> 0 (GLSL leaves those undefined). */
typedef struct MptDisplaySettings {
    int32_t view;               /* MPT_VIEW_* */
    int32_t sample_number;      /* u_sample_number / u_sample_number_1 */
    int32_t sample_number_2;    /* BLEND: u_sample_number_2, the second buffer's sample count */
    int32_t resolution_scaling; /* u_resolution_scaling s >= 1: output (x, y) reads source (x / s, y / s) */
    int32_t do_tonemapping;     /* 1: 1 - exp(-c * exposure), then pow(., 1 / gamma) */
    float gamma;
    float exposure;
    float blend_factor;         /* BLEND: 0 = the first buffer, 1 = the second */
    int32_t use_low_threshold;  /* WHITE_FURNACE_THRESHOLD: green below 0.49 */
    int32_t use_high_threshold; /* WHITE_FURNACE_THRESHOLD: red above 0.51 */
    float min_val;              /* heat map: the count of the first colour stop ... */
    float max_val;              /* ... and of the last; min_val <= max_val */
    float threshold_val;        /* converged map: white where 0 <= count < threshold_val */
    int32_t nb_stops;           /* heat map: 1..MPT_DISPLAY_MAX_STOPS */
    MptColor color_stops[MPT_DISPLAY_MAX_STOPS];
} MptDisplaySettings;

/* DisplaySettings.h's defaults (tonemapping on, gamma 2.2, exposure 1.8, blend 1, low threshold
 * off, high on), view DEFAULT, one sample, no scaling, the heat map's blue / green / red stops
 * (DisplayViewSystem.cpp:294) over [1, 1].  Host only. */
int mpt_display_settings_default(MptDisplaySettings* out);
/* What update_display_program_uniforms (DisplayViewSystem.cpp:203-324) derives from the render
 * settings of the last frame for `view`, written into inout (its other fields stay):
 * sample_number = max(1, render_settings->sample_number) -- the reference's count of samples
 * rendered so far, i.e. the last MptFrame's sample_number + 1; resolution_scaling =
 * render_low_resolution_scaling when low_resolution_displayed, else 1; min_val =
 * adaptive_sampling_min_samples under enable_adaptive_sampling, else 1; max_val = threshold_val =
 * max(sample_number, min_val).  Host only. */
int mpt_display_uniforms(const MptRenderSettings* render_settings, int32_t view, int32_t low_resolution_displayed,
                         MptDisplaySettings* inout);
/* RGBA8 (bytes r, g, b, a) of the partition's rows, in the compact row order of
 * mpt_get_framebuffer: one kernel on the context's stream, after the frames enqueued so far,
 * reading the context's sums in place.  dst: rows * res_x * 4 bytes, device (asynchronous: no
 * host synchronisation) or host memory (synchronous).  second_rgb (BLEND only): 3 floats per
 * pixel in the partition's layout, device or host memory (a host array is copied before the call
 * returns).  resolution_scaling > 1 shows the top-left ceil(W / s) x ceil(H / s) block a
 * low-resolution frame renders, scaled up; a context of a row partition (band_count > 1) holds
 * only its own rows of that block: MPT_ERR_UNSUPPORTED.  The heat map and the converged map need
 * the last frame to have had the adaptive-sampling buffers (adaptive sampling or the stop-noise
 * threshold, while accumulating). */
int mpt_display(MptContext* ctx, const MptDisplaySettings* settings, const float* second_rgb, int second_is_device,
                uint8_t* dst_rgba8, int dst_is_device);
/* The same pixel functions on host arrays, no GPU: src is width * height float3 (int32 counts
 * for the heat map and the converged map), src2 the second float3 buffer of BLEND (else NULL). */
int mpt_display_host(const MptDisplaySettings* settings, const void* src, const float* src2, int32_t width,
                     int32_t height, uint8_t* dst_rgba8);
/* 8-bit RGBA PNG of width x height pixels (rows top to bottom), stored (uncompressed) deflate
 * blocks.  flip_y = 1 writes the last row first, as stbi_flip_vertically_on_write(true) does for
 * the reference's screenshots (Screenshoter.cpp:162-163).  Host only. */
int mpt_write_png(const char* path, const uint8_t* rgba8, int32_t width, int32_t height, int32_t flip_y);

/* ------------------------------------------------------------------------- */
/* Denoiser: an edge-avoiding a-trous filter guided by the AOVs               */
/* ------------------------------------------------------------------------- */
/* The reference denoises with OIDN (RenderWindow::denoise, RenderWindow.cpp:881-972;
 * OpenImageDenoiser::denoise / get_denoised_framebuffer) and blends the result in with the BLEND
 * view.  OIDN is not available here; in its place stands a self-contained, deterministic filter
 * that claims no parity with it: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
 * albedo-demodulated radiance, its edge stopping taken from the normals AOV, the albedo AOV and
 * the colour itself (the definition: DESIGN.md §2).  Inputs: three planes of float3 per pixel --
 * the colour sums over sample_number samples (MPT_FB_COLOR) and the albedo and normals averages
 * (MPT_FB_ALBEDO, MPT_FB_NORMALS; 0 where the camera ray missed).  Output: float3 sums over
 * sample_number samples, i.e. in the units of the input; the BLEND view takes it as its second
 * buffer with sample_number_2 = sample_number.  All arithmetic is fp32 in a fixed order; the
 * kernels (csrc/denoise.hip) and the host loop share the pixel functions (csrc/denoise.h) and
 * agree bit for bit. */
#define MPT_DENOISE_MAX_ITERATIONS 8
typedef struct MptDenoiseSettings {
    int32_t sample_number;      /* samples in the colour sums, >= 1 */
    int32_t iterations;         /* 1..MPT_DENOISE_MAX_ITERATIONS; iteration i has its taps 1 << i pixels apart */
    int32_t use_albedo;         /* demodulate by max(albedo, 0.01) and stop at albedo edges */
    int32_t use_normals;        /* stop at normal edges: weight max(0, n_p . n_q) ^ (2 ^ normal_power_log2) */
    float sigma_color;          /* colour edge stopping, halved at every iteration; finite, > 0 */
    float sigma_albedo;         /* albedo edge stopping; finite, > 0 */
    int32_t normal_power_log2;  /* 0..10 */
} MptDenoiseSettings;

/* One sample, 5 iterations, albedo and normals on, sigma_color 4, sigma_albedo 0.1,
 * normal_power_log2 6.  Host only. */
int mpt_denoise_settings_default(MptDenoiseSettings* out);
/* Denoises the context's own colour sums with its AOV buffers: 1 + iterations kernels on the
 * context's stream, after the frames enqueued so far, reading the buffers in place.  The result
 * stays in a context-owned device buffer (mpt_denoised_buffer) and is also copied to
 * dst_rgb_or_NULL (rows * res_x float3): a device destination is asynchronous (no host
 * synchronisation), a host destination makes the call synchronous.  The working planes (40 B per
 * pixel) and the result live in the context, allocated at the first call and dropped by
 * mpt_resize.  MPT_ERR_INVALID_ARGUMENT before any frame was rendered; MPT_ERR_UNSUPPORTED on a
 * context of a row partition (band_count > 1), whose stencil would need other bands' rows:
 * mpt_gather the three planes and use mpt_denoise_device. */
int mpt_denoise(MptContext* ctx, const MptDenoiseSettings* settings, float* dst_rgb_or_NULL, int dst_is_device);
/* The result mpt_denoise kept (device pointer, valid until the next mpt_denoise, mpt_resize or a
 * frame of another partition) and the sample_number it was made at: the reference's
 * get_denoised_framebuffer and last_denoised_sample_count.  The pointer is what mpt_display takes
 * as a device second buffer, with sample_number_2 = *sample_number.  Either output may be NULL.
 * MPT_ERR_INVALID_ARGUMENT when nothing was denoised since the last resize. */
int mpt_denoised_buffer(MptContext* ctx, const float** dev, int32_t* sample_number);
/* The same kernels on caller-owned device planes of width x height float3 (on the context's
 * device), with the context's stream and working planes; dst (device, width * height float3) may
 * be one of the inputs.  Asynchronous.  The multi-GPU route: mpt_gather the three planes to the
 * root's device, then denoise there. */
int mpt_denoise_device(MptContext* ctx, const MptDenoiseSettings* settings, const float* color, const float* albedo,
                       const float* normals, int32_t width, int32_t height, float* dst);
/* The same pixel functions in a host loop, no GPU: host arrays of width * height float3. */
int mpt_denoise_host(const MptDenoiseSettings* settings, const float* color, const float* albedo, const float* normals,
                     int32_t width, int32_t height, float* dst);

/* ------------------------------------------------------------------------- */
/* Temporal accumulation: motion-vector history for moving scenes              */
/* ------------------------------------------------------------------------- */
/* Every geometry update restarts the sample accumulation, so a playing animation shows a few
 * samples per pose.  With mpt_set_temporal on, the context keeps the pose before the updates since
 * the last temporal call (prev_pos, 12 B per vertex) and mpt_temporal_accumulate blends the frame
 * just rendered into a reprojected history: the closest hit of each pixel's centre ray gives a
 * primitive and barycentrics, the same combination of the triangle's previous vertices the point
 * the surface came from, the previous call's camera where it was seen.  Exact for skinned,
 * morphed, animated and transformed geometry and for a moving camera; the definition is DESIGN.md
 * §2, the arithmetic csrc/temporal.h, shared by the kernels and the host path bit for bit.  The
 * visibility query does not alpha-test; reflections and refractions move with the surface they
 * are seen on. */
#define MPT_TEMPORAL_MAX_HISTORY 1024
typedef struct MptTemporalSettings {
    int32_t sample_number;    /* samples in the colour sums, >= 1 (as MptDenoiseSettings) */
    int32_t max_history;      /* cap of the history length, 1..MPT_TEMPORAL_MAX_HISTORY */
    float   alpha;            /* floor of the current frame's blend weight, (0, 1] */
    float   depth_tolerance;  /* relative, finite, > 0 */
    float   normal_threshold; /* least cosine between the current and a tap's normal, [-1, 1] */
    int32_t use_albedo;       /* demodulate exactly as the denoiser does */
} MptTemporalSettings;

/* The planes of mpt_get_temporal: the accumulated colour (float3, sums over sample_number samples
 * like MPT_FB_COLOR), and four float4 planes: motion {fx, fy, expected depth, prim bits} -- the
 * previous call's pixel coordinates of the pixel's surface point ((-1, -1): behind the previous
 * camera), its distance from the previous camera (-1: a miss) --, visibility {t, u, v, prim bits}
 * (prim -1: a miss), and the history's two planes {e.r, e.g, e.b, depth} (the demodulated mean,
 * the distance from the camera or -1) and {n.x, n.y, n.z, length}. */
#define MPT_TEMPORAL_OUTPUT 0
#define MPT_TEMPORAL_MOTION 1
#define MPT_TEMPORAL_VISIBILITY 2
#define MPT_TEMPORAL_HISTORY_A 3
#define MPT_TEMPORAL_HISTORY_B 4

/* One sample, max_history 32, alpha 0.1, depth_tolerance 0.02, normal_threshold 0.9, albedo on:
 * the values the quality test of tests/test_temporal_host.py was run with.  Host only. */
int mpt_temporal_settings_default(MptTemporalSettings* out);
/* enable != 0: from now on every geometry update (mpt_update_vertices, _vertices_device,
 * _transforms, _skin, _morph, _morph_skin, _animation) first copies the positions to prev_pos on
 * the stream unless an update since the last temporal call has done so already -- two updates
 * between two temporal calls leave the older pose.  mpt_rebuild_bvh* keeps the previous pose and
 * the history (the primitive ids are the scene's); mpt_upload_scene* and mpt_resize drop both.
 * enable == 0 frees everything; a context that never enabled it pays one branch per update. */
int mpt_set_temporal(MptContext* ctx, int enable);
/* Accumulates the context's colour sums: k_primary_rays, the raw closest-hit traversal and
 * k_temporal on the context's stream, after the frames enqueued so far.  camera: the camera the
 * sums were rendered with; the previous camera is the one given to the previous call (the first
 * call after a reset: this one).  The result stays in the context (mpt_get_temporal) and is also
 * copied to dst_rgb_or_NULL (rows * res_x float3): a device destination is asynchronous, a host
 * destination makes the call synchronous.  The working planes (108 B per pixel and two ray planes
 * shared with mpt_trace_*) are allocated at the first call.  MPT_ERR_INVALID_ARGUMENT when
 * mpt_set_temporal is off, before any frame was rendered, without a scene, or on bad settings;
 * MPT_ERR_UNSUPPORTED on a row partition (band_count > 1).  A refusal changes nothing; a HIP error
 * drops the history. */
int mpt_temporal_accumulate(MptContext* ctx, const MptTemporalSettings* settings, const MptCamera* camera,
                            float* dst_rgb_or_NULL, int dst_is_device);
/* Forgets the history (not the previous pose): the next call starts at length 1. */
int mpt_temporal_reset(MptContext* ctx);
/* A plane of the last mpt_temporal_accumulate (kind: MPT_TEMPORAL_*), rows * res_x elements of the
 * current partition, copied on the stream; a host destination synchronises.
 * MPT_ERR_INVALID_ARGUMENT when there is none, and when a frame of another size or of a row
 * partition has been rendered since that call: the planes keep the size of the call (the history
 * goes on once a frame of that size is rendered again) and are not handed out meanwhile.
 * MPT_TEMPORAL_STATS in the environment at mpt_create (tools/temporal_time.py) makes every
 * mpt_temporal_accumulate of the context synchronise and print the GPU times of its three launches
 * to stderr; unset, nothing is timed. */
int mpt_get_temporal(MptContext* ctx, int kind, void* dst, int dst_is_device);
/* mpt_temporal_accumulate, then the a-trous filter over the accumulated plane with the context's
 * albedo and normals into the kept denoise buffer: mpt_denoised_buffer and the BLEND view then
 * show it.  The two settings must carry the same sample_number. */
int mpt_denoise_temporal(MptContext* ctx, const MptTemporalSettings* settings, const MptCamera* camera,
                         const MptDenoiseSettings* denoise_settings, float* dst_rgb_or_NULL, int dst_is_device);
/* The centre rays of a width x height frame as the call traces them, width * height * 8 floats in
 * mpt_trace_closest's layout (origin, 0, direction, tmax inf).  Host only. */
int mpt_primary_rays_host(const MptCamera* camera, int32_t width, int32_t height, float* out_rays);
/* The same pixel functions in a host loop, no GPU.  The host has no traversal: visibility is an
 * input (width * height float4 {t, u, v, prim bits}, e.g. from mpt_trace_closest on the rays
 * above).  history_in_a NULL: no history.  history planes, visibility and motion: float4; color,
 * albedo, normals and output: float3. */
typedef struct MptTemporalHostArgs {
    MptTemporalSettings settings;
    MptCamera camera, prev_camera;
    int32_t width, height;
    int32_t num_vertices, num_triangles;
    const float* visibility;
    const int32_t* indices;
    const float* positions;
    const float* prev_positions;
    const float* color;
    const float* albedo;
    const float* normals;
    const float* history_in_a;
    const float* history_in_b;
    float* history_out_a;
    float* history_out_b;
    float* output;
    float* motion;
} MptTemporalHostArgs;
int mpt_temporal_host(const MptTemporalHostArgs* args);

#ifdef __cplusplus
}
#endif

#endif /* MPT_H */
