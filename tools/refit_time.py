"""Times mpt_update_vertices (the GPU BVH8 refit) on the C3 city, procedural_city(1234), against
the only other route to moved geometry, a second mpt_upload_scene, and the render cost of a
refitted (stale) tree against a freshly built one (DESIGN.md §4 "Geometry updates").

Method: one MI355X; a warm-up of every variant; `--repeats` repeats with the variants alternating
inside every repeat; medians with minimum and maximum.  An update is timed as the wall time of the
whole call and as GPU time between two events on the context's stream around it (the call drains
and synchronises the stream itself, so the events bracket its copies and kernels); an upload as
the wall time of the mpt_upload_scene call alone (the scene struct is prepared before).  Render
cost: C3 (1920x1080, RIS, HDR sky, alpha testing on) wall ms per sample over `--samples` samples
in batches of `--batch`, on the refitted context after an identity update, after a 1 % jitter of
every vertex and after ten successive jitters (MptRefitInfo::area_ratio with each), and on a
context that uploaded the same vertices afresh.  Writes one JSON document (--out) and prints it.

--upload-only times just the uploads (of the scene and of its jittered copy): the run to make at
a commit without mpt_update_vertices, with --pkg naming that commit's package directory.
--variant update runs `--calls` updates and nothing else: the run to put under
`rocprofv3 --kernel-trace --memory-copy-trace --stats` for per-kernel and per-copy times."""
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
    ap.add_argument("--upload-only", action="store_true")
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
    v10 = v0
    for k in range(10):
        v10 = jitter(v10, 100 + k)
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

    def update_ms(r, v, info=False):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r.synchronize_kernel()
        e0.record(stream)
        t0 = time.perf_counter()
        ri = r.update_vertices(v, info=info)
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return wall, e0.elapsed_time(e1), ri

    if a.variant == "update":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0)
            for k in range(a.calls):
                r.update_vertices(v1 if k % 2 == 0 else v0)
        return

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

    sets = {"identity": v0, "jitter_1pct": v1, "jitter_x10": v10}
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as rr, mpt.GPURenderer(0, stream=stream.cuda_stream) as rf:
        for r in (rr, rf):
            r.set_scene(sd0)
            r.set_luts(luts)
            r.set_envmap(env)
            render_ms(r)                                   # warm-up: path state allocated, kernels loaded
        update_ms(rr, v1)
        update_ms(rr, v0)
        nodes, tris, levels = rr.get_bvh(0)
        ln, lt, llevels = rr.get_bvh(1)
        out.update(nodes=len(nodes), records=len(tris), levels=levels, light_nodes=len(ln), light_records=len(lt),
                   light_levels=llevels)
        t_upd_wall, t_upd_gpu, t_info_wall, t_upload = [], [], [], []
        t_refit = {k: [] for k in sets}
        t_fresh = {k: [] for k in sets}
        ratios = {}
        for rep in range(a.repeats):
            # update against re-upload, alternating
            w, g, _ = update_ms(rr, v1)
            t_upd_wall.append(w)
            t_upd_gpu.append(g)
            t_upload.append(upload_ms(rf, with_vertices(v1)))
            t_info_wall.append(update_ms(rr, v0, info=True)[0])
            # render cost: refitted tree against a fresh upload of the same vertices
            for name, v in sets.items():
                if name == "jitter_x10" and rep == 0:       # ten updates in a row, as a front-end would make them
                    vk = v0
                    for k in range(10):
                        vk = jitter(vk, 100 + k)
                        ri = rr.update_vertices(vk, info=True)
                else:
                    ri = rr.update_vertices(v, info=True)
                ratios[name] = {"area_ratio": round(ri.area_ratio, 4), "light_area_ratio": round(ri.light_area_ratio, 4)}
                t_refit[name].append(render_ms(rr))
                upload_ms(rf, with_vertices(v))
                t_fresh[name].append(render_ms(rf))
        out["update_wall_ms"] = stats(t_upd_wall)
        out["update_gpu_ms"] = stats(t_upd_gpu)
        out["update_with_info_wall_ms"] = stats(t_info_wall)
        out["upload_wall_ms"] = stats(t_upload)
        out["upload_over_update"] = round(out["upload_wall_ms"]["median"] / out["update_wall_ms"]["median"], 1)
        out["render"] = {"width": W, "height": H, "samples": a.samples, "batch": a.batch, "unit": "wall ms per sample"}
        for name in sets:
            out["render"][name] = dict(ratios[name], refitted=stats(t_refit[name]), fresh_upload=stats(t_fresh[name]))
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
