"""Times a scene upload on the C3 city, procedural_city(1234): mpt_upload_scene (both BVH8s by the
host builder) against mpt_upload_scene_mode in each build mode (both BVH8s built on the GPU), and
the render cost of the SAH-uploaded context against the host-uploaded one (DESIGN.md §4 "Uploads
with a build mode").

Method (that of tools/rebuild_time.py): one MI355X; one context; a warm-up of every variant;
`--repeats` repeats with the variants alternating inside every repeat; median, minimum and maximum
of the wall time of the whole call.  A mode counts as faster than the host upload when its maximum
is below the host upload's minimum (`faster_than_host`).  The phases of the new call (host checks,
copies into the mirrors, host-to-device copies with the texture pass and the attributes, materials
and flag words, the scene build, the light selection with its download, the light build, the
downloads of the node boxes) are the library's own wall-clock marks, printed under
MPT_UPLOAD_STATS and collected here over the same repeats (medians).  Render cost: C3 (1920x1080,
RIS, HDR sky, alpha testing on) wall ms per sample over `--samples` samples in batches of `--batch`
on two contexts, one uploaded by each route, alternating; node visits and triangle tests per ray
from one instrumented pass per column.  Writes one JSON document (--out) and prints it.

--variant upload runs `--calls` uploads in --mode and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for per-kernel times (--kernel-stats CSV merges that run's
kernel table into the document, by kernel name)."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"lbvh": 0, "ploc": 1, "sah": 3}
PHASES = ("check", "mirrors", "arrays", "materials", "build", "select", "build_light", "download")


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "n": len(ts)}


def kernel_groups(path):
    """rocprofv3's kernel_stats CSV as {kernel: {calls, total_ms}} for the kernels of an upload."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            short = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).split("::")[-1].strip()
            calls = int(float(row.get("Calls", 0) or 0))
            ns = float(row.get("TotalDurationNs", 0) or 0)
            e = out.setdefault(short, {"calls": 0, "total_ms": 0.0})
            e["calls"] += calls
            e["total_ms"] = round(e["total_ms"] + ns / 1e6, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["total_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--mode", type=int, default=3, help="--variant upload: the build mode of the calls")
    ap.add_argument("--variant", default=None)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a --variant upload run under rocprofv3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np  # noqa: F401
    import torch

    import mpt
    from mpt import abi, scene, synthetic

    sd = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    s_abi = sd.to_abi()
    L = mpt.lib()
    stream = torch.cuda.Stream()

    if a.variant == "upload":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            for _ in range(a.calls):
                rc = L.mpt_upload_scene_mode(r.h, C.byref(s_abi), a.mode, None)
                assert rc == 0, (rc, L.mpt_last_error())
        return

    def host_ms(r):
        r.synchronize_kernel()
        t0 = time.perf_counter()
        rc = L.mpt_upload_scene(r.h, C.byref(s_abi))
        t = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, L.mpt_last_error())
        return t

    def mode_ms(r, mode):
        """(wall ms, the library's phase marks, RebuildInfo) of one mpt_upload_scene_mode call."""
        info = abi.RebuildInfo()
        r.synchronize_kernel()
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            os.environ["MPT_UPLOAD_STATS"] = "1"
            try:
                t0 = time.perf_counter()
                rc = L.mpt_upload_scene_mode(r.h, C.byref(s_abi), mode, C.byref(info))
                t = (time.perf_counter() - t0) * 1e3
            finally:
                del os.environ["MPT_UPLOAD_STATS"]
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode()
        assert rc == 0, (rc, L.mpt_last_error())
        m = re.search(r"mpt upload: " + " ".join(p + r" ([0-9.]+)" for p in PHASES) + " ms", text)
        return t, dict(zip(PHASES, map(float, m.groups()))), info

    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd.num_triangles,
           "vertices": len(sd.vertices), "materials": len(sd.materials), "textures": len(sd.textures), "repeats": a.repeats}
    t_host, t_mode = [], {k: [] for k in MODES}
    ph = {k: {p: [] for p in PHASES} for k in MODES}
    infos = {}
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        host_ms(r)                                             # warm-up of every variant
        for k, m in MODES.items():
            mode_ms(r, m)
        for _ in range(a.repeats):
            t_host.append(host_ms(r))
            for k, m in MODES.items():
                t, p, infos[k] = mode_ms(r, m)
                t_mode[k].append(t)
                for name, v in p.items():
                    ph[k][name].append(v)
        host_ms(r)
        hn, _, hl = r.get_bvh(0)
        out["host_builder"] = {"nodes": len(hn), "levels": hl}
    out["upload_scene_wall_ms"] = stats(t_host)
    out["upload_scene_mode_wall_ms"] = {k: stats(t) for k, t in t_mode.items()}
    out["faster_than_host"] = {k: out["upload_scene_mode_wall_ms"][k]["max"] < out["upload_scene_wall_ms"]["min"] for k in MODES}
    out["host_over_mode"] = {k: round(out["upload_scene_wall_ms"]["median"] / out["upload_scene_mode_wall_ms"][k]["median"], 2)
                             for k in MODES}
    out["phases_wall_ms"] = {k: {p: round(sorted(v)[len(v) // 2], 3) for p, v in ph[k].items()} for k in MODES}
    out["trees"] = {k: {"nodes": i.nodes, "levels": i.levels, "light_nodes": i.light_nodes, "light_records": i.light_records,
                        "light_levels": i.light_levels} for k, i in infos.items()}
    if a.kernel_stats:
        out["kernels_of_one_profiled_run"] = kernel_groups(a.kernel_stats)

    if not a.no_render:
        W, H = 1920, 1080
        luts = scene.load_luts()
        env = mpt.build_envmap(scene.procedural_sky(2048, 1024, seed=7))
        cam = scene.make_camera(sd.camera_info, W, H)
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

        cols = {"host_upload": None, "sah_upload": abi.BUILD_SAH}
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as rh, mpt.GPURenderer(0, stream=stream.cuda_stream) as rs:
            ctx = dict(zip(cols, (rh, rs)))
            for c, r in ctx.items():
                r.set_scene(sd, build=cols[c])
                r.set_luts(luts)
                r.set_envmap(env)
                render_ms(r)                                   # warm-up: path state allocated, kernels loaded
            t_render = {c: [] for c in cols}
            for _ in range(a.repeats):
                for c in cols:
                    t_render[c].append(render_ms(ctx[c]))
            out["render"] = {"width": W, "height": H, "samples": a.samples, "batch": a.batch, "unit": "wall ms per sample"}
            for c in cols:
                out["render"][c] = dict(stats(t_render[c]), **per_ray(ctx[c]))
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
