"""Times morph targets on the C3 city, procedural_city(1234), with synthetic morphs (DESIGN.md §4
"Geometry updates", Morph targets): dense4 (4 targets, every vertex in each, with normal deltas),
dense32 (32 targets, every vertex in each, positions only) and sparse32 (32 targets, each touching a
random 10 % of the vertices, positions only).

Variants, all ending in the same refit of both trees:
  a  morph_host_then_update  the only route without mpt_update_morph: mpt.morph_host on the host
                             (the loop of csrc/morph.h, one thread), then update_vertices
  b  update_vertices         update_vertices alone, the arrays already prepared
  c  update_morph            4 bytes per target cross the bus; the kernel of csrc/morph.hip in its
                             four configurations: 4 or 1 vertices per lane (MPT_MORPH_GROUP), the
                             weights staged in LDS or gathered through the cache (MPT_MORPH_LDS)
  d  (dense4 and sparse32, with skin_time.py's 16-joint skin) update_morph_skin as one call, with
     one and with four vertices per lane, against update_morph followed by update_skin

Method: skin_time.py's -- one MI355X, no profiler; a warm-up of every variant; `--repeats` repeats
with the variants in a new random order inside every repeat; medians with minimum and maximum; wall
time of the whole call and GPU time between two events on the context's stream.  b and every c are
given the same values and must report the same MptRefitInfo: checked before anything is timed.
c is to be read against a and b of the same run, never against itself.

--variant morph runs `--calls` update_morph per morph and configuration and nothing else: the run to
put under `rocprofv3 --kernel-trace --output-format csv` for the times of k_morph alone (no counters
in that run).  --kernel-trace <kernel_trace.csv of that run> merges them into the document."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skin_time import stats  # noqa: E402

MORPHS = ("dense4", "dense32", "sparse32")
CONFIGS = (("g4_lds", "4", "1"), ("g4_gather", "4", "0"), ("g1_lds", "1", "1"), ("g1_gather", "1", "0"))


def configure(group, lds):
    os.environ["MPT_MORPH_GROUP"] = group
    os.environ["MPT_MORPH_LDS"] = lds


def kernel_times(path, calls, morphs):
    """{morph: {config: stats in us}} from the k_morph rows of a kernel trace of --variant morph."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_morph" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(morphs) * len(CONFIGS) * calls, f"{len(rows)} k_morph dispatches"
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    out, k = {}, 0
    for m in morphs:
        out[m] = {}
        for name, _, _ in CONFIGS:
            out[m][name] = stats(us[k + 1:k + calls])
            k += calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--morphs", default=",".join(MORPHS))
    ap.add_argument("--variant", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    morphs = [m for m in a.morphs.split(",") if m]
    assert all(m in MORPHS for m in morphs), morphs
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np
    import torch

    import mpt
    from mpt import abi, scene, synthetic

    sd0 = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    n0 = np.ascontiguousarray(sd0.normals, np.float32)
    nv = len(v0)
    lo, hi = v0.min(0).astype(np.float64), v0.max(0).astype(np.float64)
    ext = float((hi - lo).max())

    def morph(name):
        """(scene.MorphData, two weight vectors) -- built as MorphData so that set_morph does not sort again."""
        T = 4 if name == "dense4" else 32
        rng = np.random.default_rng(T + len(name))
        md = scene.MorphData()
        if name == "sparse32":
            ids = [np.flatnonzero(rng.random(nv) < 0.1).astype(np.int32) for _ in range(T)]
        else:
            ids = [np.arange(nv, dtype=np.int32)] * T
        md.target_offsets = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int32)
        md.vertex_ids = np.concatenate(ids)
        N = len(md.vertex_ids)
        md.pos_deltas = rng.standard_normal((N, 3), dtype=np.float32) * np.float32(0.0005 * ext)
        md.nrm_deltas = rng.standard_normal((N, 3), dtype=np.float32) * np.float32(0.2) if name == "dense4" else None
        md.target_node, md.target_index = np.zeros(T, np.int32), np.arange(T, dtype=np.int32)
        ws = [rng.uniform(-1, 1, T).astype(np.float32) for _ in range(2)]
        return md, ws

    def skin16():
        g = 4
        fx = (v0[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
        fz = (v0[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
        ix, iz = np.minimum(fx.astype(np.int32), g - 2), np.minimum(fz.astype(np.int32), g - 2)
        tx, tz = (fx - ix).astype(np.float32), (fz - iz).astype(np.float32)
        J = np.stack([ix * g + iz, (ix + 1) * g + iz, ix * g + iz + 1, (ix + 1) * g + iz + 1], 1).astype(np.int32)
        W = np.stack([(1 - tx) * (1 - tz), tx * (1 - tz), (1 - tx) * tz, tx * tz], 1).astype(np.float32)
        rng = np.random.default_rng(3)
        Ms = []
        for _ in range(2):
            ang = np.radians(rng.uniform(-10, 10, g * g))
            M = np.zeros((g * g, 3, 4), np.float32)
            M[:, 0, 0], M[:, 0, 2], M[:, 1, 1], M[:, 2, 0], M[:, 2, 2] = np.cos(ang), np.sin(ang), 1.0, -np.sin(ang), np.cos(ang)
            M[:, :, 3] = rng.uniform(-0.002, 0.002, (g * g, 3)) * ext
            Ms.append(M)
        return J, W, Ms

    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd0.num_triangles,
           "vertices": nv, "repeats": a.repeats, "lds_targets": mpt.MORPH_LDS_TARGETS, "morphs": {}}
    stream = torch.cuda.Stream()

    if a.variant == "morph":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0, build=abi.BUILD_LBVH)
            for name in morphs:
                md, ws = morph(name)
                r.set_morph(md)
                for _, group, lds in CONFIGS:
                    configure(group, lds)
                    for k in range(a.calls):
                        r.update_morph(ws[k % 2])
                r.set_morph(None)
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

    def measure(r, variants, seed):
        wall = {n: [] for n in variants}
        gpu = {n: [] for n in variants}
        names = list(variants)
        order = np.random.default_rng(seed)
        for name in names:                                    # warm-up
            variants[name](0)
        for rep in range(a.repeats):
            for name in order.permutation(names):            # a new order in every repeat
                w, t, _ = timed(r, lambda: variants[name](rep % 2))
                wall[name].append(w)
                gpu[name].append(t)
        return {n: stats(t) for n, t in wall.items()}, {n: stats(t) for n, t in gpu.items()}

    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd0)
        for name in morphs:
            md, ws = morph(name)
            r.update_vertices(v0, n0)             # the rest pose is captured from the undisturbed city
            r.set_morph(md)
            T, off, ids, dp, dn = mpt._morph_tables(md, "morph_time")      # once: a times the library's call alone

            def host(w):
                ov, on = np.empty_like(v0), np.empty_like(n0)
                p = lambda x: None if x is None else x.ctypes.data
                rc = mpt.lib().mpt_morph_host(p(v0), p(n0), nv, T, p(off), p(ids), p(dp), p(dn), p(w), p(ov), p(on))
                assert rc == 0, rc
                return ov, on

            pre = [host(w) for w in ws]

            def c(group, lds):
                return lambda k, info=False: (configure(group, lds), r.update_morph(ws[k], info=info))[1]

            variants = {"a_morph_host_then_update": lambda k, info=False: r.update_vertices(*host(ws[k]), info=info),
                        "b_update_vertices": lambda k, info=False: r.update_vertices(*pre[k], info=info)}
            for cname, group, lds in CONFIGS:
                variants["c_update_morph_" + cname] = c(group, lds)
            N = len(md.vertex_ids)
            res = {"targets": md.num_targets, "entries": N, "normal_deltas": md.nrm_deltas is not None}
            for k in (0, 1):
                reps = {vn: fn(k, True) for vn, fn in variants.items()}
                tup = {vn: (i.nodes, i.levels, i.light_nodes, i.light_levels, i.area_ratio, i.light_area_ratio) for vn, i in reps.items()}
                assert all(t == tup["b_update_vertices"] for t in tup.values()), tup
                res[f"area_ratio_pose{k + 1}"] = round(tup["b_update_vertices"][4], 4)
            res["wall_ms"], res["gpu_ms"] = measure(r, variants, len(name))
            # the kernel's traffic: rest pose read and staging written (48 B), a row offset (4 B) and the
            # mask per vertex; target index and deltas per entry
            per_entry = 4 + 12 + (12 if md.nrm_deltas is not None else 0)
            res["k_morph_bytes"] = 53 * nv + per_entry * N
            res["k_morph_bound_us_at_8TBps"] = round(res["k_morph_bytes"] / 8e12 * 1e6, 2)
            if name != "dense32":
                J, W, Ms = skin16()
                r.set_skin(J, W, 16)
                two = lambda k: (configure("1", "1"), r.update_morph(ws[k]), r.update_skin(Ms[k]))
                one1 = lambda k: (configure("1", "1"), r.update_morph_skin(ws[k], Ms[k]))
                one4 = lambda k: (configure("4", "1"), r.update_morph_skin(ws[k], Ms[k]))
                dw, dg = measure(r, {"d_update_morph_skin_g1_lds": one1, "d_update_morph_skin_g4_lds": one4,
                                     "d_update_morph_then_update_skin_g1_lds": two}, 99)
                res["wall_ms"].update(dw)
                res["gpu_ms"].update(dg)
                r.set_skin(None)
            r.set_morph(None)
            out["morphs"][name] = res
            del md, pre, off, ids, dp, dn
    if a.kernel_trace:
        out["k_morph_us"] = kernel_times(a.kernel_trace, a.calls, morphs)
        out["k_morph_us_method"] = f"rocprofv3 --kernel-trace in a run of its own (--variant morph --calls {a.calls}), the first dispatch of each configuration left out"
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
