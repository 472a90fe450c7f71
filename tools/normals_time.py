"""Times the recomputed normals of mpt_set_normals on the C3 city, procedural_city(1234), with welded
groups over all vertices and every vertex flagged as having a normal (the city's own flags leave most
of its vertices to the geometric normal: flagged, every vertex is recomputed, the worst case), under
update_skin with tools/skin_time.py's 16 x 16 palette (DESIGN.md §4 "Geometry updates", Normals).

Variants, all ending in the same refit of both trees:
  off          update_skin with no groups set: the code path of the library before the feature
  two_kernels  update_skin with the groups set, the default structure of csrc/normals.hip: one kernel
               writes the face vectors, a second gathers them per vertex
  fused        the same with MPT_NORMALS_FUSED=1: one kernel, the face vectors formed in registers
  host         what the same normals cost without the feature: the skinned positions taken as given,
               area-weighted normals in numpy on the host (bincount per component over the welded
               groups), then update_vertices(v, n)

Method: one MI355X, no profiler; a warm-up of every variant; `--repeats` repeats, the variants in a
new random order inside every repeat (two_kernels and fused so alternate); medians with minimum and
maximum.  Each call is timed as the wall time of the whole call and as GPU time between two events
on the context's stream around it.  The two structures must leave the same bytes: checked through
get_vertices before anything is timed.  Writes one JSON document (--out) and prints it."""
import argparse
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
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import copy

    import numpy as np
    import torch

    import mpt
    from mpt import abi, synthetic

    sd_city = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    sd0 = copy.copy(sd_city)
    sd0.has_normals = np.ones(len(sd_city.vertices), np.uint8)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    n0 = np.ascontiguousarray(sd0.normals, np.float32)
    idx = np.ascontiguousarray(sd0.triangle_indices, np.int32).reshape(-1, 3)
    nv, nt = len(v0), len(idx)
    lo, hi = v0.min(0).astype(np.float64), v0.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    g = 16

    fx = (v0[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
    fz = (v0[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
    ix, iz = np.minimum(fx.astype(np.int32), g - 2), np.minimum(fz.astype(np.int32), g - 2)
    tx, tz = (fx - ix).astype(np.float32), (fz - iz).astype(np.float32)
    J = np.stack([ix * g + iz, (ix + 1) * g + iz, ix * g + iz + 1, (ix + 1) * g + iz + 1], 1).astype(np.int32)
    W = np.stack([(1 - tx) * (1 - tz), tx * (1 - tz), (1 - tx) * tz, tx * tz], 1).astype(np.float32)
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], g), np.linspace(lo[2], hi[2], g), indexing="ij")
    cen = np.stack([gx.ravel(), np.full(g * g, lo[1]), gz.ravel()], 1)

    def pose(seed):
        rng = np.random.default_rng(seed)
        K = len(cen)
        ang = np.radians(rng.uniform(-10, 10, K))
        R = np.zeros((K, 3, 3))
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
        M = np.zeros((K, 3, 4), np.float32)
        M[:, :, :3] = R
        M[:, :, 3] = cen - np.einsum("krc,kc->kr", R, cen) + rng.uniform(-0.002, 0.002, (K, 3)) * ext
        return M

    Ms = [pose(1), pose(2)]
    t0 = time.perf_counter()
    grp, G = mpt.normal_groups(v0, n0)
    t_groups = time.perf_counter() - t0
    corner_group = grp[idx]                                   # [T, 3]
    row_len = np.bincount(corner_group.ravel(), minlength=G)
    walked = int(row_len[grp].sum())                          # entries read by the per-vertex kernel
    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''}), every vertex flagged",
           "triangles": nt, "vertices": nv, "vertices_flagged_in_the_city": int(np.count_nonzero(sd_city.has_normals)),
           "groups": G, "table_entries": int(row_len.sum()), "row_length": {"median": int(np.median(row_len)), "max": int(row_len.max())},
           "entries_walked": walked, "normal_groups_seconds": round(t_groups, 2), "joints": g * g, "repeats": a.repeats}

    def numpy_normals(v):
        """Area-weighted normals per welded group, float32 sums by bincount (not the library's order)."""
        e1, e2 = v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]]
        f = np.cross(e1, e2)
        s = np.stack([np.bincount(corner_group.ravel(), np.repeat(f[:, r], 3), G) for r in range(3)], 1)
        l = np.linalg.norm(s, axis=1, keepdims=True)
        return (s / np.where(l > 0, l, 1.0)).astype(np.float32)[grp]

    stream = torch.cuda.Stream()

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
        r.set_scene(sd0, build=abi.BUILD_LBVH)
        r.set_skin(J, W, g * g)
        posed = [mpt.skin_host(v0, n0, J, W, M)[0] for M in Ms]

        # set_normals is part of no timed call: the state is switched before the clock starts
        def switch(groups):
            r.set_normals(grp if groups else None, None, G if groups else None)

        variants = {"off": (False, "0"), "two_kernels": (True, "0"), "fused": (True, "1")}
        got = {}
        for name, (groups, fused) in variants.items():
            os.environ["MPT_NORMALS_FUSED"] = fused
            switch(groups)
            r.update_skin(Ms[0])
            got[name] = r.get_vertices()
        assert got["two_kernels"][1].tobytes() == got["fused"][1].tobytes(), "the two structures differ"
        assert got["two_kernels"][0].tobytes() == got["off"][0].tobytes()
        out["normals_changed_by_the_recompute"] = int((got["two_kernels"][1] != got["off"][1]).any(1).sum())
        wall = {n: [] for n in list(variants) + ["host"]}
        gpu = {n: [] for n in wall}
        order = np.random.default_rng(5)
        names = list(variants)
        for rep in range(a.repeats + 1):                      # (the first repeat is the warm-up)
            for name in order.permutation(names):
                groups, fused = variants[name]
                os.environ["MPT_NORMALS_FUSED"] = fused
                switch(groups)
                w, t, _ = timed(r, lambda: r.update_skin(Ms[rep % 2]))
                if rep:
                    wall[name].append(w)
                    gpu[name].append(t)
        switch(False)
        for rep in range(a.host_repeats + 1):
            w, t, _ = timed(r, lambda: r.update_vertices(posed[rep % 2], numpy_normals(posed[rep % 2])))
            if rep:
                wall["host"].append(w)
                gpu["host"].append(t)
    out["wall_ms"] = {n: stats(t) for n, t in wall.items()}
    out["gpu_ms"] = {n: stats(t) for n, t in gpu.items()}
    # the algorithmic traffic of the two-kernel structure: indices, gathered positions and face
    # vectors written per triangle; group id, normal flag, two row offsets, flip byte and the normal
    # read and written per vertex; the triangle id and the face vector per entry walked
    face = (12 + 36 + 16) * nt
    gather = (4 + 1 + 8 + 1 + 24) * nv + (4 + 16) * walked
    fused = (4 + 1 + 8 + 1 + 24) * nv + (4 + 12 + 36) * walked
    out["traffic_bytes"] = {"k_face": face, "k_vertex": gather, "two_kernels": face + gather, "fused": fused}
    out["bound_us_at_8TBps"] = {"two_kernels": round((face + gather) / 8e12 * 1e6, 1), "fused": round(fused / 8e12 * 1e6, 1)}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
