"""Times per-object motion on the C3 city, procedural_city(1234): a tenth of its connected components
are objects, each turned about its centroid and moved (DESIGN.md §4 "Geometry updates", Transforms).

Variants, all ending in the same refit of both trees:
  a  numpy_then_update     the only route without mpt_update_transforms: the motion applied with
                           numpy on the host (positions and normals of the moving vertices), then
                           update_vertices of both arrays
  b  update_vertices       update_vertices alone, the arrays already prepared
  c  update_transforms     48 bytes per object cross the bus; the kernel of csrc/xform.hip
  c1 update_transforms, MPT_XFORM_GROUP=1   the same with one vertex per lane (dword accesses)
  d  update_vertices_device  update_vertices from torch tensors already on the device

Method: one MI355X; a warm-up of every variant; `--repeats` repeats with the variants alternating
inside every repeat; medians with minimum and maximum.  Each call is timed as the wall time of the
whole call and as GPU time between two events on the context's stream around it (the calls drain
and synchronise the stream themselves, so the events bracket their copies and kernels).  b, c, c1
and d are given the same values (mpt.transform_host's) and must report the same MptRefitInfo: that
is checked before anything is timed.  Writes one JSON document (--out) and prints it.

--variant xform runs `--calls` update_transforms and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the per-kernel times of k_xform (no counters in that run):
`--calls` calls with four vertices per lane, then as many with one."""
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--variant", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    import mpt
    from mpt import abi, synthetic

    sd0 = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    n0 = np.ascontiguousarray(sd0.normals, np.float32)
    nv = len(v0)
    I = sd0.triangle_indices.reshape(-1, 3)
    e0, e1 = np.concatenate([I[:, 0], I[:, 1]]), np.concatenate([I[:, 1], I[:, 2]])
    ncomp, lab = connected_components(coo_matrix((np.ones(len(e0), np.int8), (e0, e1)), shape=(nv, nv)), directed=False)
    parts = np.arange(ncomp)[::10]                                   # a tenth of the components are objects
    remap = np.full(ncomp, -1, np.int32)
    remap[parts] = np.arange(len(parts), dtype=np.int32)
    ids = remap[lab]
    K = len(parts)
    moving = ids >= 0
    cnt = np.bincount(ids[moving], minlength=K).astype(np.float64)
    cen = np.stack([np.bincount(ids[moving], weights=v0[moving, k].astype(np.float64), minlength=K) / np.maximum(cnt, 1) for k in range(3)], 1)
    ext = float((v0.max(0) - v0.min(0)).max())

    def motion(seed):
        """[K, 3, 4]: every object turned about the vertical through its centroid and moved."""
        rng = np.random.default_rng(seed)
        ang = np.radians(rng.uniform(-45, 45, K))
        R = np.zeros((K, 3, 3))
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
        t = rng.uniform(-0.005, 0.005, (K, 3)) * ext
        M = np.zeros((K, 3, 4), np.float32)
        M[:, :, :3] = R
        M[:, :, 3] = cen - np.einsum("krc,kc->kr", R, cen) + t
        return M

    def numpy_motion(M):
        """Variant a's host work: the moving vertices' positions and normals, float32 numpy."""
        v, n = v0.copy(), n0.copy()
        m = M[ids[moving]]
        v[moving] = np.einsum("vrc,vc->vr", m[:, :, :3], v0[moving]) + m[:, :, 3]
        t = np.einsum("vrc,vc->vr", m[:, :, :3], n0[moving])               # (rigid: the linear part is its own normal matrix)
        l = np.linalg.norm(t, axis=1, keepdims=True)
        n[moving] = np.where(l > 0, t / np.maximum(l, 1e-30), n0[moving])
        return v, n

    Ms = [motion(1), motion(2)]
    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd0.num_triangles,
           "vertices": nv, "components": int(ncomp), "objects": int(K), "moving_vertices": int(moving.sum()), "repeats": a.repeats}
    stream = torch.cuda.Stream()

    if a.variant == "xform":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0, build=abi.BUILD_LBVH)
            r.set_objects(ids, K)
            for g in (4, 1):                   # k_xform<4> and k_xform<1> are told apart by name in the trace
                os.environ["MPT_XFORM_GROUP"] = str(g)
                for k in range(a.calls):
                    r.update_transforms(Ms[k % 2])
        return

    pre = [mpt.transform_host(v0, n0, ids, M) for M in Ms]              # b and d: the arrays already prepared
    dev = torch.device("cuda", 0)
    pre_dev = [(torch.from_numpy(v).to(dev), torch.from_numpy(n).to(dev)) for v, n in pre]
    torch.cuda.synchronize()

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

    def group(g):
        os.environ["MPT_XFORM_GROUP"] = str(g)

    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd0)
        r.set_objects(ids, K)
        variants = {
            "a_numpy_then_update": lambda k, info=False: r.update_vertices(*numpy_motion(Ms[k]), info=info),
            "b_update_vertices": lambda k, info=False: r.update_vertices(*pre[k], info=info),
            "c_update_transforms": lambda k, info=False: (group(4), r.update_transforms(Ms[k], info=info))[1],
            "c1_update_transforms_group1": lambda k, info=False: (group(1), r.update_transforms(Ms[k], info=info))[1],
            "d_update_vertices_device": lambda k, info=False: (group(4), r.update_vertices(*pre_dev[k], info=info))[1],
        }
        # the same values must give the same report (and every variant is warmed up on both motions)
        for k in (0, 1):
            reps = {name: fn(k, True) for name, fn in variants.items()}
            tup = {name: (i.nodes, i.levels, i.light_nodes, i.light_levels, i.area_ratio, i.light_area_ratio) for name, i in reps.items()}
            same = [tup[n] for n in tup if n != "a_numpy_then_update"]
            assert all(t == same[0] for t in same), tup
            out[f"area_ratio_motion{k + 1}"] = round(same[0][4], 4)
        wall = {n: [] for n in variants}
        gpu = {n: [] for n in variants}
        names = list(variants)
        for rep in range(a.repeats):
            # the order rotates with the repeat: what a call finds in the host's caches depends on the
            # call before it (a and b stream 130 MB through them), so no variant keeps one predecessor
            for name in names[rep % len(names):] + names[:rep % len(names)]:
                w, g, _ = timed(r, lambda: variants[name](rep % 2))
                wall[name].append(w)
                gpu[name].append(g)
        out["wall_ms"] = {n: stats(t) for n, t in wall.items()}
        out["gpu_ms"] = {n: stats(t) for n, t in gpu.items()}
        out["record_upload_bytes"] = 21 * 4 * K
        # the common case, a handful of rigid objects: the same moving vertices as 16 objects (the rest
        # pose is captured anew from the undisturbed city), each turned about the city's centre
        r.update_vertices(v0, n0)
        few = np.where(moving, ids % 16, -1).astype(np.int32)
        r.set_objects(few, 16)
        c0 = (v0.min(0) + v0.max(0)).astype(np.float64) / 2

        def few_motion(seed):
            rng = np.random.default_rng(seed)
            ang = np.radians(rng.uniform(-2, 2, 16))
            R = np.zeros((16, 3, 3))
            R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
            M = np.zeros((16, 3, 4), np.float32)
            M[:, :, :3] = R
            M[:, :, 3] = c0 - R @ c0 + rng.uniform(-0.005, 0.005, (16, 3)) * ext
            return M

        Mf = [few_motion(3), few_motion(4)]
        fv = {"c_update_transforms": lambda k: (group(4), r.update_transforms(Mf[k]))[1],
              "c1_update_transforms_group1": lambda k: (group(1), r.update_transforms(Mf[k]))[1]}
        for k in (0, 1):
            for fn in fv.values():
                fn(k)
        fw = {n: [] for n in fv}
        fg = {n: [] for n in fv}
        for rep in range(a.repeats):
            for name in (list(fv) if rep % 2 == 0 else list(fv)[::-1]):
                w, g, _ = timed(r, lambda: fv[name](rep % 2))
                fw[name].append(w)
                fg[name].append(g)
        out["few_objects"] = {"objects": 16, "wall_ms": {n: stats(t) for n, t in fw.items()}, "gpu_ms": {n: stats(t) for n, t in fg.items()}}
    # the kernel's traffic bound: 52 B per vertex (rest pose read, staging written, ids) and the mask
    out["k_xform_bytes"] = 53 * nv
    out["k_xform_bound_us_at_8TBps"] = round(53 * nv / 8e12 * 1e6, 2)
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
