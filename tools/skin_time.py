"""Times linear-blend skinning on the C3 city, procedural_city(1234), with synthetic weights: joints
on a g x g grid over the ground plan, every vertex blending the four corners of its grid cell
bilinearly (DESIGN.md §4 "Geometry updates", Skinning).  Palettes: 16 joints (4 x 4), 256 (16 x 16,
exactly MPT_SKIN_LDS_JOINTS) and 1024 (32 x 32, past the LDS budget: always gathered).

Variants, all ending in the same refit of both trees:
  a  skin_host_then_update   the only route without mpt_update_skin: mpt.skin_host on the host
                             (the loop of csrc/skin.h, one thread), then update_vertices
  b  update_vertices         update_vertices alone, the arrays already prepared
  c  update_skin             64 bytes per joint cross the bus; the kernel of csrc/skin.hip, in its
                             four configurations: 4 or 1 vertices per lane (MPT_SKIN_GROUP), the
                             palette staged in LDS or gathered through the cache (MPT_SKIN_LDS)

Method: one MI355X, no profiler; a warm-up of every variant; `--repeats` repeats with the variants
in a new random order inside every repeat; medians with minimum and maximum.  Each call is timed as the wall time
of the whole call and as GPU time between two events on the context's stream around it.  b and every
c are given the same values and must report the same MptRefitInfo: checked before anything is timed.
Writes one JSON document (--out) and prints it.

--variant skin runs `--calls` update_skin per palette and configuration and nothing else: the run to
put under `rocprofv3 --kernel-trace --output-format csv` for the times of k_skin alone (no counters
in that run).  --kernel-trace <kernel_trace.csv of that run> merges them into the document: the
dispatches of k_skin in order, `--calls` per palette and configuration, the first of each left out
as warm-up."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (4, 16, 32)
CONFIGS = (("g4_lds", "4", "1"), ("g4_gather", "4", "0"), ("g1_lds", "1", "1"), ("g1_gather", "1", "0"))


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4), "n": len(ts)}


def configure(group, lds):
    os.environ["MPT_SKIN_GROUP"] = group
    os.environ["MPT_SKIN_LDS"] = lds


def kernel_times(path, calls):
    """{palette: {config: stats in us}} from the k_skin rows of a kernel trace of --variant skin."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_skin" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(GRIDS) * len(CONFIGS) * calls, f"{len(rows)} k_skin dispatches"
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    out, k = {}, 0
    for g in GRIDS:
        out[str(g * g)] = {}
        for name, _, _ in CONFIGS:
            out[str(g * g)][name] = stats(us[k + 1:k + calls])
            k += calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--variant", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np
    import torch

    import mpt
    from mpt import abi, synthetic

    sd0 = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    n0 = np.ascontiguousarray(sd0.normals, np.float32)
    nv = len(v0)
    lo, hi = v0.min(0).astype(np.float64), v0.max(0).astype(np.float64)
    ext = float((hi - lo).max())

    def skin(g):
        """(joints [V, 4], weights [V, 4], joint centres [g * g, 3]) for a g x g grid of joints."""
        fx = (v0[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
        fz = (v0[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
        ix, iz = np.minimum(fx.astype(np.int32), g - 2), np.minimum(fz.astype(np.int32), g - 2)
        tx, tz = (fx - ix).astype(np.float32), (fz - iz).astype(np.float32)
        J = np.stack([ix * g + iz, (ix + 1) * g + iz, ix * g + iz + 1, (ix + 1) * g + iz + 1], 1).astype(np.int32)
        W = np.stack([(1 - tx) * (1 - tz), tx * (1 - tz), (1 - tx) * tz, tx * tz], 1).astype(np.float32)
        gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], g), np.linspace(lo[2], hi[2], g), indexing="ij")
        return J, W, np.stack([gx.ravel(), np.full(g * g, lo[1]), gz.ravel()], 1)

    def pose(cen, seed):
        """[J, 3, 4]: every joint turned a little about the vertical through its centre and moved."""
        rng = np.random.default_rng(seed)
        K = len(cen)
        ang = np.radians(rng.uniform(-10, 10, K))
        R = np.zeros((K, 3, 3))
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
        M = np.zeros((K, 3, 4), np.float32)
        M[:, :, :3] = R
        M[:, :, 3] = cen - np.einsum("krc,kc->kr", R, cen) + rng.uniform(-0.002, 0.002, (K, 3)) * ext
        return M

    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd0.num_triangles,
           "vertices": nv, "repeats": a.repeats, "lds_joints": mpt.SKIN_LDS_JOINTS, "palettes": {}}
    stream = torch.cuda.Stream()

    if a.variant == "skin":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0, build=abi.BUILD_LBVH)
            for g in GRIDS:
                J, W, cen = skin(g)
                Ms = [pose(cen, 1), pose(cen, 2)]
                r.set_skin(J, W, g * g)
                for _, group, lds in CONFIGS:
                    configure(group, lds)
                    for k in range(a.calls):
                        r.update_skin(Ms[k % 2])
        return

    def timed(r, fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r.synchronize_kernel()
        ev0.record(stream)
        t0 = time.perf_counter()
        ri = fn()
        wall = (time.perf_counter() - t0) * 1e3
        ev1.record(stream)
        ev1.synchronize()
        return wall, ev0.elapsed_time(ev1), ri

    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd0)
        for g in GRIDS:
            J, W, cen = skin(g)
            Ms = [pose(cen, 1), pose(cen, 2)]
            r.update_vertices(v0, n0)             # the rest pose is captured from the undisturbed city
            r.set_skin(J, W, g * g)
            pre = [mpt.skin_host(v0, n0, J, W, M) for M in Ms]

            def c(group, lds):
                return lambda k, info=False: (configure(group, lds), r.update_skin(Ms[k], info=info))[1]

            variants = {"a_skin_host_then_update": lambda k, info=False: r.update_vertices(*mpt.skin_host(v0, n0, J, W, Ms[k]), info=info),
                        "b_update_vertices": lambda k, info=False: r.update_vertices(*pre[k], info=info)}
            for name, group, lds in CONFIGS:
                variants["c_update_skin_" + name] = c(group, lds)
            res = {"joints": g * g, "palette": "LDS or gather" if g * g <= mpt.SKIN_LDS_JOINTS else "past the LDS budget: gathered whatever MPT_SKIN_LDS says"}
            for k in (0, 1):
                reps = {name: fn(k, True) for name, fn in variants.items()}
                tup = {name: (i.nodes, i.levels, i.light_nodes, i.light_levels, i.area_ratio, i.light_area_ratio) for name, i in reps.items()}
                assert all(t == tup["b_update_vertices"] for t in tup.values()), tup
                res[f"area_ratio_pose{k + 1}"] = round(tup["b_update_vertices"][4], 4)
            wall = {n: [] for n in variants}
            gpu = {n: [] for n in variants}
            names = list(variants)
            order = np.random.default_rng(g)
            for rep in range(a.repeats):
                # a new order in every repeat: what a call finds in the host's caches and on the bus
                # depends on the call before it (a and b move 130 MB), so no variant keeps one predecessor
                for name in order.permutation(names):
                    w, t, _ = timed(r, lambda: variants[name](rep % 2))
                    wall[name].append(w)
                    gpu[name].append(t)
            res["wall_ms"] = {n: stats(t) for n, t in wall.items()}
            res["gpu_ms"] = {n: stats(t) for n, t in gpu.items()}
            res["record_upload_bytes"] = 64 * g * g
            out["palettes"][str(g * g)] = res
    # the kernel's traffic without the palette: the rest pose read and the staging written (48 B), the
    # indices and weights (32 B) and the mask
    out["k_skin_bytes"] = 81 * nv
    out["k_skin_bound_us_at_8TBps"] = round(81 * nv / 8e12 * 1e6, 2)
    if a.kernel_trace:
        out["k_skin_us"] = kernel_times(a.kernel_trace, a.calls)
        out["k_skin_us_method"] = f"rocprofv3 --kernel-trace in a run of its own (--variant skin --calls {a.calls}), the first dispatch of each configuration left out"
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
