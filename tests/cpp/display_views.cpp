// Test driver (tests/test_display_host_cpp.py): the display step of the C++ GPURenderer mirror
// (hiprt-path-tracer_amd/host) -- set_display_view / display / write_to_png over mpt_display and
// mpt_write_png -- on a scene handed over as the raw blob of tests/test_host_cpp.py.
// usage: display_views <in.blob> <out.png> <out.bin> <view>
//   Runs RenderWindow's loop (update() then render() per displayed frame), writes a screenshot of
//   MPT_VIEW_* `view` to out.png (Screenshoter::write_to_png: bottom row first) and displays the
//   same view into host memory and into a hipMalloc'd buffer (as a front-end's mapped texture
//   would be), which must agree.
//   out.bin = int32 n_frames, MptFrame[n_frames] (every frame enqueued), uint8 rgba[W*H*4]
#include <hip/hip_runtime_api.h>

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
    if (argc != 5) { fprintf(stderr, "usage: %s in.blob out.png out.bin view\n", argv[0]); return 2; }
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
        (void)r.get<int32_t>();   // mode: always RenderWindow's loop here
        const int M2 = r.get<int32_t>(), n_split = r.get<int32_t>();
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
        fclose(fin);

        mpt_host::GPURenderer gr(std::vector<int>(n_split > 1 ? n_split : 1, 0));
        MptScene s{};
        s.triangle_indices = idx.data(); s.num_triangles = T;
        s.vertices = pos.data(); s.vertex_normals = nrm.data(); s.has_vertex_normals = has_n.data();
        s.texcoords = uv.data(); s.num_vertices = V;
        s.material_indices = mat_idx.data(); s.materials = mats.data(); s.num_materials = M;
        s.emissive_triangle_indices = emissive.data(); s.num_emissive_triangles = E;
        gr.set_scene(s);
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
        for (int u = 0; u < n_updates; u++) {
            gr.update();
            gr.render();
            frames.insert(frames.end(), gr.last_frames().begin(), gr.last_frames().end());
        }
        const size_t bytes = (size_t)W * H * 4;
        gr.set_display_view(atoi(argv[4]));
        // the device destination first, straight after render(): ordered on the renderer's stream
        std::vector<uint8_t> from_device;
        if (gr.device_count() == 1) {
            uint8_t* d = nullptr;
            if (hipMalloc(&d, bytes) != hipSuccess) throw std::runtime_error("hipMalloc");
            gr.display(d, true);
            gr.synchronize_kernel();
            from_device.resize(bytes);
            if (hipMemcpy(from_device.data(), d, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
            (void)hipFree(d);
        }
        gr.write_to_png(argv[2]);
        std::vector<uint8_t> rgba(bytes);
        gr.display(rgba.data(), false);
        if (!from_device.empty() && std::memcmp(from_device.data(), rgba.data(), bytes) != 0)
            throw std::runtime_error("device and host destinations differ");
        FILE* fo = fopen(argv[3], "wb");
        if (!fo) throw std::runtime_error("cannot open output");
        int32_t nf = (int32_t)frames.size();
        fwrite(&nf, sizeof(nf), 1, fo);
        fwrite(frames.data(), sizeof(MptFrame), frames.size(), fo);
        fwrite(rgba.data(), 1, rgba.size(), fo);
        fclose(fo);
        printf("ok %d frames, view %d\n", nf, gr.get_display_view());
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
