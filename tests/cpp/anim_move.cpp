// Test driver (tests/test_anim_host_cpp.py): GPURenderer::set_animation / update_animation /
// animation_host of the C++ mirror (hiprt-path-tracer_amd/host).
// usage: anim_move host <anim.blob> <out.bin>          (no device)
//        anim_move <in.blob> <anim.blob> <out.bin>     (over N_SPLIT contexts)
//   anim.blob = uint32 magic 0x4d494e41, int32 N, J, T, S, C, K (key times), V (values), then the
//   arrays of MptAnimation in the struct's order (the two offset arrays only when S > 0), then int32
//   n_times and the times (floats).
//   host: GPURenderer::animation_host at every time; out.bin = per time J x 12 floats, then T floats.
//   Tables or a time that the library refuses: "refused: <message>" on stdout, exit status 3.
//   Otherwise in.blob is the blob of morph_move (tests/test_morph_host_cpp.py; its weights, matrices
//   and `fused` are read and not used).  The driver sets morph, skin and animation, renders
//   n_updates displayed frames of the uploaded scene, calls update_animation(times[0]), checks the
//   report and the refusals, and renders n_updates more: the accumulation must have restarted on
//   the posed scene.
//   out.bin = int32 n_frames, MptFrame[n_frames] (the frames enqueued after the update),
//             float sums[W*H*3], int32 pixel_sample_count[W*H]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "gpu_renderer.h"

namespace {
struct Reader {
    FILE* f;
    template <typename T> T get() { T v; if (fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short blob"); return v; }
    template <typename T> std::vector<T> arr(size_t n) {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short blob");
        return v;
    }
};

// The tables of an anim.blob and the MptAnimation over them.
struct Clip {
    std::vector<int32_t> parents, jnodes, koff, voff, interp, csamp, cnode, cpath, ctgt0, ctgtn;
    std::vector<float> trs, basew, key_times, values, times;
    std::vector<uint8_t> is_trs;
    std::vector<double> locals, bind;
    MptAnimation a{};
};

void read_clip(const char* path, Clip& c) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error("cannot open the animation blob");
    Reader r{f};
    if (r.get<uint32_t>() != 0x4d494e41u) throw std::runtime_error("bad animation magic");
    const int N = r.get<int32_t>(), J = r.get<int32_t>(), T = r.get<int32_t>(), S = r.get<int32_t>(), C = r.get<int32_t>();
    const int K = r.get<int32_t>(), V = r.get<int32_t>();
    if (N < 0 || J < 0 || T < 0 || S < 0 || C < 0 || K < 0 || V < 0) throw std::runtime_error("bad animation counts");
    c.parents = r.arr<int32_t>((size_t)N);
    c.trs = r.arr<float>(10 * (size_t)N);
    c.is_trs = r.arr<uint8_t>((size_t)N);
    c.locals = r.arr<double>(12 * (size_t)N);
    c.jnodes = r.arr<int32_t>((size_t)J);
    c.bind = r.arr<double>(12 * (size_t)J);
    c.basew = r.arr<float>((size_t)T);
    c.koff = r.arr<int32_t>(S ? (size_t)S + 1 : 0);
    c.key_times = r.arr<float>((size_t)K);
    c.voff = r.arr<int32_t>(S ? (size_t)S + 1 : 0);
    c.values = r.arr<float>((size_t)V);
    c.interp = r.arr<int32_t>((size_t)S);
    c.csamp = r.arr<int32_t>((size_t)C);
    c.cnode = r.arr<int32_t>((size_t)C);
    c.cpath = r.arr<int32_t>((size_t)C);
    c.ctgt0 = r.arr<int32_t>((size_t)C);
    c.ctgtn = r.arr<int32_t>((size_t)C);
    const int n_times = r.get<int32_t>();
    c.times = r.arr<float>((size_t)(n_times > 0 ? n_times : 0));
    fclose(f);
    MptAnimation& a = c.a;
    a.num_nodes = N; a.num_joints = J; a.num_targets = T; a.num_samplers = S; a.num_channels = C;
    a.node_parents = c.parents.data(); a.node_trs = c.trs.data(); a.node_is_trs = c.is_trs.data(); a.node_locals = c.locals.data();
    a.joint_nodes = c.jnodes.data(); a.joint_bind = c.bind.data(); a.base_weights = c.basew.data();
    a.sampler_key_offsets = c.koff.data(); a.key_times = c.key_times.data(); a.sampler_value_offsets = c.voff.data();
    a.values = c.values.data(); a.sampler_interp = c.interp.data();
    a.channel_sampler = c.csamp.data(); a.channel_node = c.cnode.data(); a.channel_path = c.cpath.data();
    a.channel_first_target = c.ctgt0.data(); a.channel_num_targets = c.ctgtn.data();
}

int host_mode(const char* clip_path, const char* out_path) {
    Clip c;
    read_clip(clip_path, c);
    std::vector<float> out;
    std::vector<float> m(12 * (size_t)c.a.num_joints), w((size_t)c.a.num_targets);
    for (float t : c.times) {
        try {
            mpt_host::GPURenderer::animation_host(c.a, t, m.empty() ? nullptr : m.data(), w.empty() ? nullptr : w.data());
        } catch (const std::exception& e) {
            printf("refused: %s\n", e.what());
            return 3;
        }
        out.insert(out.end(), m.begin(), m.end());
        out.insert(out.end(), w.begin(), w.end());
    }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) throw std::runtime_error("cannot open output");
    fwrite(out.data(), sizeof(float), out.size(), fo);
    fclose(fo);
    printf("ok %d times\n", (int)c.times.size());
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s host anim.blob out.bin | in.blob anim.blob out.bin\n", argv[0]); return 2; }
    try {
        if (!strcmp(argv[1], "host")) return host_mode(argv[2], argv[3]);
        Clip clip;
        read_clip(argv[2], clip);
        if (clip.times.empty()) throw std::runtime_error("no time");
        FILE* fin = fopen(argv[1], "rb");
        if (!fin) throw std::runtime_error("cannot open blob");
        Reader r{fin};
        if (r.get<uint32_t>() != 0x4254504du) throw std::runtime_error("bad magic");
        const auto settings = r.get<MptRenderSettings>();
        const auto world = r.get<MptWorldSettings>();
        const auto options = r.get<MptKernelOptions>();
        const auto flags = r.get<MptBSDFFlags>();
        const auto camera = r.get<MptCamera>();
        const int W = r.get<int32_t>(), H = r.get<int32_t>(), n_updates = r.get<int32_t>();
        const int T = r.get<int32_t>(), V = r.get<int32_t>(), M = r.get<int32_t>(), E = r.get<int32_t>();
        const int mode = r.get<int32_t>(), M2 = r.get<int32_t>(), n_split = r.get<int32_t>();
        (void)mode;
        auto idx = r.arr<int32_t>(3 * (size_t)T);
        auto pos = r.arr<float>(3 * (size_t)V);
        auto nrm = r.arr<float>(3 * (size_t)V);
        auto has_n = r.arr<uint8_t>((size_t)V);
        auto uv = r.arr<float>(2 * (size_t)V);
        auto mat_idx = r.arr<int32_t>((size_t)T);
        auto mats = r.arr<MptMaterial>((size_t)M);
        auto emissive = r.arr<int32_t>((size_t)(E > 0 ? E : 1));
        const size_t lut_n[6] = {128 * 128, 128 * 64 * 128, 256 * 16 * 128, 256 * 16 * 128, 32 * 32 * 96, 32 * 32 * 3};
        std::vector<float> lut[6];
        for (int k = 0; k < 6; k++) lut[k] = r.arr<float>(lut_n[k]);
        (void)r.arr<MptMaterial>((size_t)M2);
        auto joints = r.arr<int32_t>(4 * (size_t)V);
        auto weights = r.arr<float>(4 * (size_t)V);
        const int K = r.get<int32_t>();
        (void)r.arr<float>(12 * (size_t)K);
        const int NT = r.get<int32_t>();
        auto toff = r.arr<int32_t>((size_t)NT + 1);
        const size_t NE = (size_t)toff[NT];
        auto tids = r.arr<int32_t>(NE);
        auto dpos = r.arr<float>(3 * NE);
        auto dnrm = r.arr<float>(3 * NE);
        (void)r.arr<float>((size_t)NT);
        (void)r.get<int32_t>();
        fclose(fin);

        mpt_host::GPURenderer gr(std::vector<int>(n_split > 1 ? n_split : 1, 0));
        MptScene s{};
        s.triangle_indices = idx.data(); s.num_triangles = T;
        s.vertices = pos.data(); s.vertex_normals = nrm.data(); s.has_vertex_normals = has_n.data();
        s.texcoords = uv.data(); s.num_vertices = V;
        s.material_indices = mat_idx.data(); s.materials = mats.data(); s.num_materials = M;
        s.emissive_triangle_indices = emissive.data(); s.num_emissive_triangles = E;
        gr.set_scene(s);
        bool early = false;   // refused: the clip drives joints and no skin is set yet
        try { gr.set_animation(&clip.a); } catch (const std::exception&) { early = true; }
        if (!early) throw std::runtime_error("set_animation without a skin was accepted");
        gr.set_morph(NT, toff.data(), tids.data(), dpos.data(), dnrm.data(), V);
        gr.set_skin(joints.data(), weights.data(), V, K);
        early = false;        // refused: no animation set yet
        try { gr.update_animation(clip.times[0]); } catch (const std::exception&) { early = true; }
        if (!early) throw std::runtime_error("update_animation without an animation was accepted");
        gr.set_animation(&clip.a);
        MptLuts L{};
        L.ggx_conductor_ess = lut[0].data(); L.glossy_dielectric_ess = lut[1].data(); L.ggx_glass_ess = lut[2].data();
        L.ggx_glass_inverse_ess = lut[3].data(); L.ggx_thin_glass_ess = lut[4].data(); L.sheen_ltc_params = lut[5].data();
        gr.setup_brdfs_data(L);
        gr.resize(W, H);
        gr.get_render_settings() = settings;
        gr.get_world_settings() = world;
        gr.get_kernel_options() = options;
        gr.get_bsdf_flags() = flags;
        gr.set_camera(camera);
        gr.reset();
        std::vector<MptFrame> frames;
        for (int phase = 0; phase < 2; phase++) {
            if (phase == 1) {
                MptRefitInfo info{};
                gr.update_animation(clip.times[0], &info);
                if (info.nodes <= 0 || info.levels <= 0 || !(info.area_ratio > 0.0f)) throw std::runtime_error("refit info");
                if (gr.get_render_settings().sample_number != 0 || !gr.get_render_settings().need_to_reset)
                    throw std::runtime_error("the update did not restart the accumulation");
                bool thrown = false;   // a refused update: a time that is not finite
                try { gr.update_animation(std::numeric_limits<float>::quiet_NaN()); } catch (const std::exception&) { thrown = true; }
                if (!thrown) throw std::runtime_error("a time that is not finite was accepted");
            }
            for (int u = 0; u < n_updates; u++) {
                gr.update();
                gr.render();
                gr.unmap_buffers();
                if (phase == 1) frames.insert(frames.end(), gr.last_frames().begin(), gr.last_frames().end());
            }
        }
        gr.synchronize_kernel();
        const size_t px = (size_t)W * H;
        std::vector<float> img(px * 3);
        gr.get_framebuffer(MPT_FB_COLOR, img.data());
        std::vector<int32_t> cnt(px);
        gr.get_aux_buffer(MPT_AUX_SAMPLE_COUNT, cnt.data());
        FILE* fo = fopen(argv[3], "wb");
        if (!fo) throw std::runtime_error("cannot open output");
        int32_t nf = (int32_t)frames.size();
        fwrite(&nf, sizeof(nf), 1, fo);
        fwrite(frames.data(), sizeof(MptFrame), frames.size(), fo);
        fwrite(img.data(), sizeof(float), img.size(), fo);
        fwrite(cnt.data(), sizeof(int32_t), cnt.size(), fo);
        fclose(fo);
        printf("ok %d frames over %d contexts\n", nf, gr.device_count());
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
