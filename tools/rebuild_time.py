"""Times mpt_rebuild_bvh (the GPU BVH8 rebuild: Morton keys, radix sort, radix tree, collapse,
refit) on the C3 city, procedural_city(1234), against the other route to a fresh tree, a second
mpt_upload_scene, and the render cost of the rebuilt (LBVH) tree against the host builder's
(binned SAH) and against a tree that was only refitted (DESIGN.md §4 "Rebuilds").

Method (that of tools/refit_time.py): one MI355X; a warm-up of every variant; `--repeats` repeats
with the variants alternating inside every repeat; medians with minimum and maximum.  A rebuild is
timed as the wall time of the whole call and as GPU time between two events on the context's
stream around it (the call drains and synchronises the stream itself); an upload as the wall time
of the mpt_upload_scene call alone.  Render cost: C3 (1920x1080, RIS, HDR sky, alpha testing on)
wall ms per sample over `--samples` samples in batches of `--batch`, for the identity and the 1 %
jitter vertex sets (`--sets`; jitter_x10: ten successive jitters), on three contexts holding the
same vertices: updated and rebuilt on the GPU, uploaded afresh (host builder), updated only
(refitted).  Node visits and triangle tests per ray come from one instrumented pass per column
after the timed repeats.  Writes one JSON document (--out) and prints it.

--upload-only times just the uploads: the run to make at a commit without mpt_rebuild_bvh, with
--pkg naming that commit's package directory.
--variant rebuild runs `--calls` rebuilds and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for per-kernel times.
--mode 1 adds the PLOC build mode (mpt_rebuild_bvh_mode, MPT_BUILD_PLOC): its rebuild is timed next
to the LBVH's inside every repeat, a fourth context `rebuilt_ploc` joins the render columns, and
the iteration counts of both trees (and how many ran in the single-workgroup tail) are taken from
the library's MPT_PLOC_STATS line of one extra call.  With --variant rebuild the calls use the mode.
--mode 3 adds the binned-SAH build mode (MPT_BUILD_SAH) on top of --mode 1: its rebuild is timed
next to the LBVH's and PLOC's inside every repeat, a fifth context `rebuilt_sah` joins the render
columns, and its level counts come from the library's MPT_SAH_STATS line.
--rebuild-only times just the rebuilds (of --mode 0, and of the modes --mode adds): the run to make
with --pkg at a commit that lacks the newest mode, to show that the older modes have not moved."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--sets", default="identity,jitter_1pct", help="vertex sets of the render columns (also: jitter_x10)")
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--rebuild-only", action="store_true")
    ap.add_argument("--mode", type=int, default=0, help="1: also the PLOC build mode; 3: PLOC and the binned-SAH mode")
    ap.add_argument("--variant", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "hiprt-path-tracer_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import numpy as np
    import torch

    import mpt
    from mpt import abi, scene, synthetic

    sd0 = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    ext = float((v0.max(0) - v0.min(0)).max())

    def jitter(v, seed):
        rng = np.random.default_rng(seed)
        return (v + (2 * rng.random(v.shape, np.float32) - 1) * np.float32(0.01 * ext)).astype(np.float32)

    v1 = jitter(v0, 1)
    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd0.num_triangles,
           "vertices": len(v0), "repeats": a.repeats}
    stream = torch.cuda.Stream()

    def with_vertices(v):
        s = copy.copy(sd0)
        s.vertices = v
        return s

    def upload_ms(r, sd):
        s = sd.to_abi()
        r.synchronize_kernel()
        t0 = time.perf_counter()
        rc = mpt.lib().mpt_upload_scene(r.h, C.byref(s))
        t = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return t

    if a.upload_only:
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            ts = {"upload_build": [], "upload_jittered": []}
            upload_ms(r, sd0)
            for _ in range(a.repeats):
                ts["upload_jittered"].append(upload_ms(r, with_vertices(v1)))
                ts["upload_build"].append(upload_ms(r, sd0))
        out["upload_wall_ms"] = {k: stats(t) for k, t in ts.items()}
        return finish(a, out)

    def rebuild_ms(r, mode=0):
        kw = {"mode": mode} if mode else {}                # (a package without build modes takes none)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r.synchronize_kernel()
        e0.record(stream)
        t0 = time.perf_counter()
        ri = r.rebuild_bvh(info=True, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return wall, e0.elapsed_time(e1), ri

    if a.variant == "rebuild":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0)
            r.update_vertices(v1)
            for k in range(a.calls):
                r.rebuild_bvh(**({"mode": a.mode} if a.mode else {}))
        return

    def ploc_stats(r, mode=1):
        """The library's report of one mode-1 (mode-3) rebuild (a line on stderr under MPT_PLOC_STATS,
        MPT_SAH_STATS)."""
        import re
        var = "MPT_SAH_STATS" if mode == 3 else "MPT_PLOC_STATS"
        import tempfile
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            os.environ[var] = "1"
            try:
                r.rebuild_bvh(mode=mode)
            finally:
                del os.environ[var]
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode()
            if mode == 3:
                m = re.search(r"scene levels (\d+) small-only (\d+), light levels (\d+) small-only (\d+)", text)
                return dict(zip(("levels", "small_only_levels", "light_levels", "light_small_only_levels"), map(int, m.groups())))
            m = re.search(r"scene iterations (\d+) tail (\d+), light iterations (\d+) tail (\d+)", text)
        return dict(zip(("iterations", "tail_iterations", "light_iterations", "light_tail_iterations"), map(int, m.groups())))

    modes = {0: (0,), 1: (0, 1), 3: (0, 1, 3)}[a.mode]
    KEY = {0: "rebuild", 1: "rebuild_ploc", 3: "rebuild_sah"}
    sah = a.mode == 3
    if a.rebuild_only:
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0)
            r.update_vertices(v1)
            ts = {m: ([], []) for m in modes}
            for m in modes:
                rebuild_ms(r, m)                           # warm-up
            for _ in range(a.repeats):
                for m in modes:
                    w, g, info = rebuild_ms(r, m)
                    ts[m][0].append(w)
                    ts[m][1].append(g)
            for m in modes:
                key = KEY[m]
                out[key + "_wall_ms"], out[key + "_gpu_ms"] = stats(ts[m][0]), stats(ts[m][1])
            if a.mode:
                out["ploc"] = ploc_stats(r)
            if sah:
                out["sah"] = ploc_stats(r, 3)
        return finish(a, out)

    W, H = 1920, 1080
    luts = scene.load_luts()
    env = mpt.build_envmap(scene.procedural_sky(2048, 1024, seed=7))
    cam = scene.make_camera(sd0.camera_info, W, H)
    opt = abi.KernelOptions.default()
    opt.direct_light_sampling = abi.LSS_RIS_BSDF_AND_LIGHT
    frames = []
    for s, seed in scene.cpu_seed_schedule(a.samples):
        st = scene.parity_settings(3)
        st.do_alpha_testing = True
        frames.append(scene.make_frame(cam, W, H, options=opt, settings=st, world=scene.envmap_world(1.0), sample_number=s,
                                       random_seed=seed))

    def render_ms(r):
        r.synchronize_kernel()
        t0 = time.perf_counter()
        r.render_samples(frames, max_batch=a.batch)
        r.synchronize_kernel()
        return (time.perf_counter() - t0) * 1e3 / a.samples

    def per_ray(r):
        r.enable_stats(timing=False, instrumented=True)
        r.render_samples(frames[:a.batch], max_batch=a.batch)
        r.synchronize_kernel()
        s = r.stats()
        r.enable_stats(timing=False, instrumented=False)
        rays = max(1, s.rays_closest + s.rays_any)
        return {"nodes_per_ray": round(s.node_visits / rays, 3), "triangle_tests_per_ray": round(s.triangle_tests / rays, 3)}

    sets = {}
    for name in a.sets.split(","):
        if name == "jitter_x10":                           # ten successive jitters (a refit depends on the final positions only)
            v10 = v0
            for k in range(10):
                v10 = jitter(v10, 100 + k)
            sets[name] = v10
        else:
            sets[name] = {"identity": v0, "jitter_1pct": v1}[name]
    cols = ("rebuilt_gpu", "fresh_upload", "refitted") + (("rebuilt_ploc",) if a.mode else ()) + (("rebuilt_sah",) if sah else ())
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as rb, mpt.GPURenderer(0, stream=stream.cuda_stream) as rf, \
            mpt.GPURenderer(0, stream=stream.cuda_stream) as rr, mpt.GPURenderer(0, stream=stream.cuda_stream) as rp, \
            mpt.GPURenderer(0, stream=stream.cuda_stream) as rs:
        ctx = dict(zip(cols, (rb, rf, rr, rp, rs)))
        for r in ctx.values():
            r.set_scene(sd0)
            r.set_luts(luts)
            r.set_envmap(env)
            render_ms(r)                                   # warm-up: path state allocated, kernels loaded
        rb.update_vertices(v1)
        rebuild_ms(rb)                                     # warm-up
        t_wall_p, t_gpu_p, info_p = [], [], None
        if a.mode:
            rp.update_vertices(v1)
            rebuild_ms(rp, 1)
        t_wall_s, t_gpu_s, info_s = [], [], None
        if sah:
            rs.update_vertices(v1)
            rebuild_ms(rs, 3)
        t_wall, t_gpu, t_upload = [], [], []
        t_render = {name: {c: [] for c in cols} for name in sets}
        info = None
        for rep in range(a.repeats):
            rb.update_vertices(v1)
            w, g, info = rebuild_ms(rb)
            t_wall.append(w)
            t_gpu.append(g)
            if a.mode:
                rp.update_vertices(v1)
                w, g, info_p = rebuild_ms(rp, 1)
                t_wall_p.append(w)
                t_gpu_p.append(g)
            if sah:
                rs.update_vertices(v1)
                w, g, info_s = rebuild_ms(rs, 3)
                t_wall_s.append(w)
                t_gpu_s.append(g)
            t_upload.append(upload_ms(rf, with_vertices(v1)))
            for name, v in sets.items():
                rb.update_vertices(v)
                rb.rebuild_bvh()
                if a.mode:
                    rp.update_vertices(v)
                    rp.rebuild_bvh(mode=1)
                if sah:
                    rs.update_vertices(v)
                    rs.rebuild_bvh(mode=3)
                upload_ms(rf, with_vertices(v))
                rr.update_vertices(v)
                for c in cols:
                    t_render[name][c].append(render_ms(ctx[c]))
        out.update(nodes=info.nodes, records=info.records, levels=info.levels, light_nodes=info.light_nodes,
                   light_records=info.light_records, light_levels=info.light_levels)
        hn, _, hl = rf.get_bvh(0)
        out["host_builder"] = {"nodes": len(hn), "levels": hl}
        out["rebuild_wall_ms"] = stats(t_wall)
        out["rebuild_gpu_ms"] = stats(t_gpu)
        out["upload_wall_ms"] = stats(t_upload)
        out["upload_over_rebuild"] = round(out["upload_wall_ms"]["median"] / out["rebuild_wall_ms"]["median"], 1)
        if a.mode:
            rp.update_vertices(v1)
            out["ploc"] = dict(ploc_stats(rp), nodes=info_p.nodes, levels=info_p.levels, light_nodes=info_p.light_nodes,
                               light_levels=info_p.light_levels)
            out["rebuild_ploc_wall_ms"] = stats(t_wall_p)
            out["rebuild_ploc_gpu_ms"] = stats(t_gpu_p)
        if sah:
            rs.update_vertices(v1)
            out["sah"] = dict(ploc_stats(rs, 3), nodes=info_s.nodes, tree_levels=info_s.levels, light_nodes=info_s.light_nodes,
                              light_tree_levels=info_s.light_levels)
            out["rebuild_sah_wall_ms"] = stats(t_wall_s)
            out["rebuild_sah_gpu_ms"] = stats(t_gpu_s)
        out["render"] = {"width": W, "height": H, "samples": a.samples, "batch": a.batch, "unit": "wall ms per sample"}
        for name, v in sets.items():
            rb.update_vertices(v)
            rb.rebuild_bvh()
            if a.mode:
                rp.update_vertices(v)
                rp.rebuild_bvh(mode=1)
            if sah:
                rs.update_vertices(v)
                rs.rebuild_bvh(mode=3)
            upload_ms(rf, with_vertices(v))
            ri = rr.update_vertices(v, info=True)
            out["render"][name] = {c: dict(stats(t_render[name][c]), **per_ray(ctx[c])) for c in cols}
            out["render"][name]["refitted_area_ratio"] = round(ri.area_ratio, 4)
    finish(a, out)


def finish(a, out):
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
