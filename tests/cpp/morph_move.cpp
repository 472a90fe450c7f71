// Test driver (tests/test_morph_host_cpp.py): GPURenderer::set_morph / update_morph /
// update_morph_skin of the C++ mirror (hiprt-path-tracer_amd/host) over N_SPLIT contexts.
// usage: morph_move <in.blob> <out.bin>
//   The blob is the one of skin_move (tests/test_skin_host_cpp.py: the scene, then joint indices,
//   weights, num_joints and the joints' matrices) followed by int32 num_targets, the target offsets
//   (num_targets + 1 int32), the entries' vertex ids (int32), position deltas and normal deltas (3
//   floats each), the weights (num_targets floats) and int32 fused.  The driver sets morph and skin,
//   renders n_updates displayed frames of the uploaded scene, poses both -- fused: one
//   update_morph_skin; else update_skin, then update_morph -- checks the report, and renders
//   n_updates more: the accumulation must have restarted on the posed scene.
//   out.bin = int32 n_frames, MptFrame[n_frames] (the frames enqueued after the update),
//             float sums[W*H*3], int32 pixel_sample_count[W*H]
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.blob out.bin\n", argv[0]); return 2; }
    try {
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
        auto mats12 = r.arr<float>(12 * (size_t)K);
        const int NT = r.get<int32_t>();
        auto toff = r.arr<int32_t>((size_t)NT + 1);
        const size_t NE = (size_t)toff[NT];
        auto tids = r.arr<int32_t>(NE);
        auto dpos = r.arr<float>(3 * NE);
        auto dnrm = r.arr<float>(3 * NE);
        auto mw = r.arr<float>((size_t)NT);
        const int fused = r.get<int32_t>();
        fclose(fin);

        mpt_host::GPURenderer gr(std::vector<int>(n_split > 1 ? n_split : 1, 0));
        MptScene s{};
        s.triangle_indices = idx.data(); s.num_triangles = T;
        s.vertices = pos.data(); s.vertex_normals = nrm.data(); s.has_vertex_normals = has_n.data();
        s.texcoords = uv.data(); s.num_vertices = V;
        s.material_indices = mat_idx.data(); s.materials = mats.data(); s.num_materials = M;
        s.emissive_triangle_indices = emissive.data(); s.num_emissive_triangles = E;
        gr.set_scene(s);
        bool early = false;   // refused: no morph set yet
        try { gr.update_morph(mw.data(), NT); } catch (const std::exception&) { early = true; }
        if (!early) throw std::runtime_error("update_morph without a morph was accepted");
        gr.set_morph(NT, toff.data(), tids.data(), dpos.data(), dnrm.data(), V);
        early = false;        // refused: no skin set yet
        try { gr.update_morph_skin(mw.data(), NT, mats12.data(), K); } catch (const std::exception&) { early = true; }
        if (!early) throw std::runtime_error("update_morph_skin without a skin was accepted");
        gr.set_skin(joints.data(), weights.data(), V, K);
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
                if (fused) {
                    gr.update_morph_skin(mw.data(), NT, mats12.data(), K, &info);
                } else {
                    gr.update_skin(mats12.data(), K);
                    gr.update_morph(mw.data(), NT, &info);
                }
                if (info.nodes <= 0 || info.levels <= 0 || !(info.area_ratio > 0.0f)) throw std::runtime_error("refit info");
                if (gr.get_render_settings().sample_number != 0 || !gr.get_render_settings().need_to_reset)
                    throw std::runtime_error("the update did not restart the accumulation");
                bool thrown = false;   // a refused update: the wrong target count
                try { gr.update_morph(mw.data(), NT - 1); } catch (const std::exception&) { thrown = true; }
                if (!thrown) throw std::runtime_error("a wrong target count was accepted");
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
        FILE* fo = fopen(argv[2], "wb");
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
