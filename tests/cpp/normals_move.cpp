// Test driver (tests/test_normals_host_cpp.py): GPURenderer::set_normals / get_vertices of the C++
// mirror (hiprt-path-tracer_amd/host) over n_split contexts.
// usage: normals_move <in.blob> <out.bin>
//   The blob: uint32 magic 0x4d524e4d, int32 T, V, M, E, G, n_split, has_flips; the scene's indices
//   (3T int32), positions and normals (3V floats each), normal flags (V bytes), texture coordinates
//   (2V floats), material indices (T int32), materials (M), emissive triangles (max(E, 1) int32);
//   then the group id of every vertex (V int32), the flip bytes (G, when has_flips) and the new
//   positions (3V floats).  The driver uploads the scene, checks that set_normals alone changes no
//   normal, moves the geometry with update_vertices (no normals given) and downloads every
//   context's arrays; then removes the groups and updates again.
//   out.bin = int32 n_split, then per context positions and normals (3V floats each) after the
//             update with the groups set, then the same after the update without them
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
        if (r.get<uint32_t>() != 0x4d524e4du) throw std::runtime_error("bad magic");
        const int T = r.get<int32_t>(), V = r.get<int32_t>(), M = r.get<int32_t>(), E = r.get<int32_t>();
        const int G = r.get<int32_t>(), n_split = r.get<int32_t>(), has_flips = r.get<int32_t>();
        auto idx = r.arr<int32_t>(3 * (size_t)T);
        auto pos = r.arr<float>(3 * (size_t)V);
        auto nrm = r.arr<float>(3 * (size_t)V);
        auto has_n = r.arr<uint8_t>((size_t)V);
        auto uv = r.arr<float>(2 * (size_t)V);
        auto mat_idx = r.arr<int32_t>((size_t)T);
        auto mats = r.arr<MptMaterial>((size_t)M);
        auto emissive = r.arr<int32_t>((size_t)(E > 0 ? E : 1));
        auto group = r.arr<int32_t>((size_t)V);
        auto flips = r.arr<uint8_t>(has_flips ? (size_t)G : 0);
        auto moved = r.arr<float>(3 * (size_t)V);
        fclose(fin);

        mpt_host::GPURenderer gr(std::vector<int>(n_split > 1 ? n_split : 1, 0));
        bool early = false;   // refused: no scene yet
        try { gr.set_normals(group.data(), nullptr, V, G); } catch (const std::exception&) { early = true; }
        if (!early) throw std::runtime_error("set_normals without a scene was accepted");
        MptScene s{};
        s.triangle_indices = idx.data(); s.num_triangles = T;
        s.vertices = pos.data(); s.vertex_normals = nrm.data(); s.has_vertex_normals = has_n.data();
        s.texcoords = uv.data(); s.num_vertices = V;
        s.material_indices = mat_idx.data(); s.materials = mats.data(); s.num_materials = M;
        s.emissive_triangle_indices = emissive.data(); s.num_emissive_triangles = E;
        gr.set_scene(s);
        gr.set_normals(group.data(), has_flips ? flips.data() : nullptr, V, G);
        bool thrown = false;   // a refused table: the wrong vertex count
        try { gr.set_normals(group.data(), nullptr, V - 1, G); } catch (const std::exception&) { thrown = true; }
        if (!thrown) throw std::runtime_error("a wrong vertex count was accepted");
        std::vector<float> gp(3 * (size_t)V), gn(3 * (size_t)V);
        for (int k = 0; k < gr.device_count(); k++) {   // the call itself changes nothing
            gr.get_vertices(gp.data(), gn.data(), V, k);
            if (memcmp(gp.data(), pos.data(), gp.size() * sizeof(float)) || memcmp(gn.data(), nrm.data(), gn.size() * sizeof(float)))
                throw std::runtime_error("set_normals alone changed the arrays");
        }
        FILE* fo = fopen(argv[2], "wb");
        if (!fo) throw std::runtime_error("cannot open output");
        const int32_t nc = gr.device_count();
        fwrite(&nc, sizeof(nc), 1, fo);
        for (int phase = 0; phase < 2; phase++) {
            if (phase == 1) gr.set_normals(nullptr, nullptr, 0, 0);
            MptRefitInfo info{};
            gr.update_vertices(moved.data(), nullptr, V, &info);
            if (info.nodes <= 0 || info.levels <= 0 || !(info.area_ratio > 0.0f)) throw std::runtime_error("refit info");
            for (int k = 0; k < nc; k++) {
                gr.get_vertices(gp.data(), gn.data(), V, k);
                fwrite(gp.data(), sizeof(float), gp.size(), fo);
                fwrite(gn.data(), sizeof(float), gn.size(), fo);
            }
        }
        fclose(fo);
        printf("ok %d vertices over %d contexts\n", V, nc);
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
