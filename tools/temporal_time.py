"""Times the temporal accumulation of mpt_temporal_accumulate on the C3 city, procedural_city(1234),
at 1920 x 1080, under update_skin with tools/skin_time.py's 16 x 16 palette (DESIGN.md §4 "Temporal
accumulation").

Measured:
  call         mpt_temporal_accumulate with a device destination: wall time of the call and GPU time
               between two events on the context's stream around it
  rays, trace, temporal
               k_primary_rays, the raw closest-hit traversal and k_temporal inside such a call, from
               the events MPT_TEMPORAL_STATS makes the library record between its launches.  The
               variable is read at mpt_create and makes every call of that context synchronise, so
               these come from a second context, created with it set, after the other timings
  denoise_temporal
               mpt_denoise_temporal: the same plus the a-trous filter's six kernels
  skin_on, skin_off
               update_skin with mpt_set_temporal on, straight after a temporal call (the update
               takes the snapshot of the previous pose: one device-to-device copy of the positions,
               24 B per vertex read and written) and once more after that (the pose is marked: the
               hook is one branch, the library's cost before the feature): what the snapshot adds.

Method: one MI355X, no profiler; a warm-up of everything; `--repeats` repeats, skin_on and skin_off
alternating inside every repeat; medians with minimum and maximum.  One sample
per pose is rendered before every temporal call (not timed).  Writes one JSON document (--out) and
prints it."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np
    import torch

    import mpt
    from mpt import abi, scene, synthetic

    sd = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd.vertices, np.float32)
    nv, nt = len(v0), len(sd.triangle_indices) // 3
    lo, hi = v0.min(0).astype(np.float64), v0.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    g = 16
    fx = (v0[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
    fz = (v0[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
    ix, iz = np.minimum(fx.astype(np.int32), g - 2), np.minimum(fz.astype(np.int32), g - 2)
    tx, tz = (fx - ix).astype(np.float32), (fz - iz).astype(np.float32)
    J = np.stack([ix * g + iz, (ix + 1) * g + iz, ix * g + iz + 1, (ix + 1) * g + iz + 1], 1).astype(np.int32)
    Wt = np.stack([(1 - tx) * (1 - tz), tx * (1 - tz), (1 - tx) * tz, tx * tz], 1).astype(np.float32)
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], g), np.linspace(lo[2], hi[2], g), indexing="ij")
    cen = np.stack([gx.ravel(), np.full(g * g, lo[1]), gz.ravel()], 1)

    def pose(seed):
        rng = np.random.default_rng(seed)
        K = len(cen)
        ang = np.radians(rng.uniform(-2, 2, K))
        R = np.zeros((K, 3, 3))
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
        M = np.zeros((K, 3, 4), np.float32)
        M[:, :, :3] = R
        M[:, :, 3] = cen - np.einsum("krc,kc->kr", R, cen) + rng.uniform(-0.0005, 0.0005, (K, 3)) * ext
        return M

    Ms = [pose(1), pose(2)]
    W, H = a.width, a.height
    cam = scene.make_camera(sd.camera_info, W, H)
    opt = abi.KernelOptions.default()
    opt.direct_light_sampling = abi.LSS_MIS_LIGHT_BSDF
    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": nt, "vertices": nv,
           "width": W, "height": H, "joints": g * g, "repeats": a.repeats}
    stream = torch.cuda.Stream()

    def timed(r, fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r.synchronize_kernel()
        ev0.record(stream)
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        ev1.record(stream)
        ev1.synchronize()
        return wall, ev0.elapsed_time(ev1)

    def with_stats(fn):
        """fn() on the context created with MPT_TEMPORAL_STATS, the library's line parsed: (rays,
        trace, temporal) in us."""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                fn()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode()
        m = re.search(r"mpt temporal: rays ([0-9.]+) trace ([0-9.]+) temporal ([0-9.]+) us", text)
        assert m, text
        return tuple(float(x) for x in m.groups())

    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd, build=abi.BUILD_LBVH)
        r.set_skin(J, Wt, g * g)
        dst = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        seeds = [s for _, s in scene.cpu_seed_schedule(2 * a.repeats + 8)]
        count = [0]

        def render():
            f = scene.make_frame(cam, W, H, options=opt, settings=scene.parity_settings(3), sample_number=0,
                                 random_seed=seeds[count[0] % len(seeds)])
            count[0] += 1
            r.render(f)

        wall = {k: [] for k in ("call", "denoise_temporal", "skin_off", "skin_on")}
        gpu = {k: [] for k in wall}
        parts = {"rays": [], "trace": [], "temporal": []}
        r.set_temporal(True)
        r.update_skin(Ms[0])
        render()
        r.temporal_to_device(dst.data_ptr(), camera=cam)
        for rep in range(a.repeats + 1):                      # (the first repeat is the warm-up)
            r.temporal_to_device(dst.data_ptr(), camera=cam)  # (clears the mark: the next update takes the snapshot)
            for k, name in enumerate(["skin_on", "skin_off"]):
                w, t = timed(r, lambda: r.update_skin(Ms[(rep + k) % 2]))
                if rep:
                    wall[name].append(w)
                    gpu[name].append(t)
            render()
            w, t = timed(r, lambda: r.temporal_to_device(dst.data_ptr(), camera=cam))
            r.update_skin(Ms[(rep + 1) % 2])
            render()
            wd, td = timed(r, lambda: r.denoise_temporal(camera=cam, to_host=False))
            if rep:
                wall["call"].append(w)
                gpu["call"].append(t)
                wall["denoise_temporal"].append(wd)
                gpu["denoise_temporal"].append(td)
        lens = r.temporal_planes(abi.TEMPORAL_HISTORY_B)[..., 3]
        out["history_length"] = {"median": float(np.median(lens)), "max": float(lens.max()), "without_history": float((lens == 1).mean())}
    os.environ["MPT_TEMPORAL_STATS"] = "1"
    try:
        r = mpt.GPURenderer(0, stream=stream.cuda_stream)
    finally:
        del os.environ["MPT_TEMPORAL_STATS"]
    with r:
        r.set_scene(sd, build=abi.BUILD_LBVH)
        r.set_skin(J, Wt, g * g)
        r.set_temporal(True)
        for rep in range(a.repeats + 1):
            r.update_skin(Ms[rep % 2])
            render()
            p = with_stats(lambda: r.temporal_to_device(dst.data_ptr(), camera=cam))
            if rep:
                for k, x in zip(("rays", "trace", "temporal"), p):
                    parts[k].append(x)
    out["wall_ms"] = {n: stats(t) for n, t in wall.items()}
    out["gpu_ms"] = {n: stats(t) for n, t in gpu.items()}
    out["kernel_us"] = {n: stats(t) for n, t in parts.items()}
    # the algorithmic traffic of k_temporal per pixel: the hit, three float3 planes, indices and two
    # poses of three vertices, four taps of two float4 history planes, two history elements, motion
    # and output written; the snapshot reads and writes every position once
    px = 16 + 36 + 12 + 72 + 4 * 32 + 32 + 16 + 12
    out["traffic_bytes"] = {"k_temporal_per_pixel": px, "k_temporal": px * W * H, "snapshot": 24 * nv}
    out["bound_us_at_8TBps"] = {"k_temporal": round(px * W * H / 8e12 * 1e6, 1), "snapshot": round(24 * nv / 8e12 * 1e6, 1)}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
