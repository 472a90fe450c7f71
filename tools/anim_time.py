"""Times animation playback on the C3 city, procedural_city(1234), with a synthetic skin over a
g x g grid of joints, morph_time.py's dense 4-target morph, and a synthetic clip: the joints are one
chain of J nodes, each with a LINEAR rotation channel of 8 keys, and one LINEAR weights channel
drives the 4 targets (DESIGN.md §4 "Geometry updates", Animation).  J is 16 and 1024.

Variants, all ending in the same fused morph + skin kernel and the same refit of both trees:
  a  update_animation           one float crosses the bus; k_anim (csrc/anim.hip) evaluates the clip
  b  update_morph_skin          the weights and matrices of mpt.animation_host, evaluated outside
                                the timer: for the same arguments this is the path before
                                mpt_update_animation existed
  c  host_then_update           the same with mpt.animation_host inside the timer
  d  python_then_update         the caller samples the clip in numpy, scene.skin_matrices walks the
                                hierarchy, then update_morph_skin: the route the documentation
                                described before

Method: skin_time.py's -- one MI355X, no profiler; a warm-up of every variant; `--repeats` repeats
with the variants in a new random order inside every repeat; medians with minimum and maximum; wall
time of the whole call and GPU time between two events on the context's stream.  a and b must
report the same MptRefitInfo: checked before anything is timed.  a is to be read against b of the
same run.

--variant anim runs `--calls` update_animation per joint count, with the world matrices in LDS and
with MPT_ANIM_LDS=0, and nothing else: the run to put under `rocprofv3 --kernel-trace
--output-format csv` for the times of k_anim alone (no counters in that run).  --kernel-trace
<kernel_trace.csv of that run> merges them into the document."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skin_time import stats  # noqa: E402

JOINTS = (16, 1024)
LDS = (("lds", "1"), ("memory", "0"))


def kernel_times(path, calls, joints):
    """{joints: {lds | memory: stats in us}} from the k_anim rows of a kernel trace of --variant anim."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_anim" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(joints) * len(LDS) * calls, f"{len(rows)} k_anim dispatches"
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    out, k = {}, 0
    for j in joints:
        out[str(j)] = {}
        for name, _ in LDS:
            out[str(j)][name] = stats(us[k + 1:k + calls])
            k += calls
    return out


def clip_tables(np, J, ext, seed=5):
    """The chain of J joint nodes with its clip, as mpt.animation_tables would give it."""
    rng = np.random.default_rng(seed)
    K = 8
    trs = np.zeros((J, 10), np.float32)
    trs[:, 0:3] = rng.uniform(-1, 1, (J, 3)) * (0.5 * ext / J)
    trs[:, 6] = 1.0
    trs[:, 7:10] = 1.0
    world = np.tile(np.eye(4), (J, 1, 1))
    for n in range(J):
        world[n, :3, 3] = trs[:n + 1, 0:3].astype(np.float64).sum(0)      # identity rotations: the translations add up
    loc = np.tile(np.eye(4), (J, 1, 1))
    loc[:, :3, 3] = trs[:, 0:3]
    bind = np.linalg.inv(world)[:, :3, :]
    times = np.linspace(0.0, 2.0, K).astype(np.float32)
    half = np.radians(rng.uniform(-20.0 / J, 20.0 / J, (J, K))) / 2         # the chain adds up to 20 degrees at most
    axis = rng.normal(size=(J, 1, 3))
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    q = np.concatenate([axis * np.sin(half)[..., None], np.cos(half)[..., None]], 2).astype(np.float32)   # [J, K, 4]
    wv = rng.uniform(-1, 1, (K, 4)).astype(np.float32)
    S = J + 1
    return {
        "node_parents": np.arange(-1, J - 1), "node_trs": trs, "node_is_trs": np.ones(J, np.uint8), "node_locals": loc[:, :3, :],
        "joint_nodes": np.arange(J), "joint_bind": bind, "base_weights": np.zeros(4, np.float32),
        "sampler_key_offsets": np.arange(S + 1) * K, "key_times": np.tile(times, S),
        "sampler_value_offsets": np.concatenate([np.arange(J + 1) * 4 * K, [4 * K * J + 4 * K]]),
        "values": np.concatenate([q.reshape(-1), wv.reshape(-1)]), "sampler_interp": np.ones(S, np.int32),
        "channel_sampler": np.arange(S), "channel_node": np.concatenate([np.arange(J), [0]]),
        "channel_path": np.concatenate([np.ones(J, np.int32), [3]]), "channel_first_target": np.zeros(S, np.int32),
        "channel_num_targets": np.concatenate([np.zeros(J, np.int32), [4]]),
    }


def python_route(np, scene, tb, t):
    """What a caller without mpt_update_animation does: the channels sampled in numpy (slerp and
    lerp, float64), scene.skin_matrices over the node hierarchy.  Returns (weights, matrices)."""
    J = len(tb["joint_nodes"])
    times = np.asarray(tb["key_times"][:8], np.float64)
    t = min(max(float(t), times[0]), times[-1])
    k = min(int(np.searchsorted(times, t, side="right")) - 1, len(times) - 2)
    u = (t - times[k]) / (times[k + 1] - times[k])
    locals_ = {}
    q = np.asarray(tb["values"][:32 * J], np.float64).reshape(J, 8, 4)
    for n in range(J):
        a, b = q[n, k], q[n, k + 1]
        d = float(a @ b)
        if d < 0:
            b, d = -b, -d
        if d > 0.9995:
            r = a + u * (b - a)
        else:
            th = np.arccos(d)
            r = (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)
        r = r / np.linalg.norm(r)
        m = np.eye(4)
        m[:3, :3] = scene._quat_to_mat(r)
        m[:3, 3] = tb["node_trs"][n, 0:3]
        locals_[n] = m
    wv = np.asarray(tb["values"][32 * J:], np.float64).reshape(8, 4)
    w = (wv[k] + u * (wv[k + 1] - wv[k])).astype(np.float32)

    class SD:
        pass
    sd = SD()
    sd.skin = scene.SkinData()
    sd.skin.joint_nodes, sd.skin.node_parents = np.asarray(tb["joint_nodes"]), np.asarray(tb["node_parents"])
    sd.skin.bind = np.concatenate([np.asarray(tb["joint_bind"]), np.tile([[[0, 0, 0, 1.0]]], (J, 1, 1))], 1)
    sd.skin.node_locals = np.tile(np.eye(4), (J, 1, 1))
    return w, scene.skin_matrices(sd, locals_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=0, help="0: the C3 city; else a smaller city of that many blocks")
    ap.add_argument("--joints", default=",".join(map(str, JOINTS)))
    ap.add_argument("--variant", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    joints = [int(j) for j in a.joints.split(",") if j]
    sys.setrecursionlimit(10000)          # scene.skin_matrices recurses once per level of the chain
    sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))
    import numpy as np
    import torch

    import mpt
    from mpt import abi, scene, synthetic

    sd0 = synthetic.procedural_city(1234, blocks=a.blocks) if a.blocks else synthetic.procedural_city(1234)
    v0 = np.ascontiguousarray(sd0.vertices, np.float32)
    nv = len(v0)
    lo, hi = v0.min(0).astype(np.float64), v0.max(0).astype(np.float64)
    ext = float((hi - lo).max())

    def morph4():
        rng = np.random.default_rng(4 + len("dense4"))
        md = scene.MorphData()
        md.target_offsets = (np.arange(5) * nv).astype(np.int32)
        md.vertex_ids = np.tile(np.arange(nv, dtype=np.int32), 4)
        md.pos_deltas = rng.standard_normal((4 * nv, 3), dtype=np.float32) * np.float32(0.0005 * ext)
        md.nrm_deltas = rng.standard_normal((4 * nv, 3), dtype=np.float32) * np.float32(0.2)
        md.target_node, md.target_index = np.zeros(4, np.int32), np.arange(4, dtype=np.int32)
        return md

    def grid_skin(J):
        g = int(round(J ** 0.5))
        assert g * g == J
        fx = (v0[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
        fz = (v0[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
        ix, iz = np.minimum(fx.astype(np.int32), g - 2), np.minimum(fz.astype(np.int32), g - 2)
        tx, tz = (fx - ix).astype(np.float32), (fz - iz).astype(np.float32)
        Jn = np.stack([ix * g + iz, (ix + 1) * g + iz, ix * g + iz + 1, (ix + 1) * g + iz + 1], 1).astype(np.int32)
        W = np.stack([(1 - tx) * (1 - tz), tx * (1 - tz), (1 - tx) * tz, tx * tz], 1).astype(np.float32)
        return Jn, W

    out = {"scene": f"procedural_city(1234{', blocks=%d' % a.blocks if a.blocks else ''})", "triangles": sd0.num_triangles,
           "vertices": nv, "repeats": a.repeats, "lds_nodes": mpt.ANIM_LDS_NODES, "joints": {}}
    stream = torch.cuda.Stream()
    T2 = (0.37, 1.61)

    if a.variant == "anim":
        with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
            r.set_scene(sd0, build=abi.BUILD_LBVH)
            r.set_morph(morph4())
            for J in joints:
                r.set_skin(*grid_skin(J), J)
                r.set_animation(clip_tables(np, J, ext))
                for _, lds in LDS:
                    os.environ["MPT_ANIM_LDS"] = lds
                    for k in range(a.calls):
                        r.update_animation(T2[k % 2])
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

    os.environ.pop("MPT_ANIM_LDS", None)
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd0)
        r.set_morph(morph4())
        for J in joints:
            tb = clip_tables(np, J, ext)
            r.set_skin(*grid_skin(J), J)
            r.set_animation(tb)
            pre = [mpt.animation_host(tb, t) for t in T2]
            py = [python_route(np, scene, tb, t) for t in T2]
            res = {"nodes": J, "channels": J + 1, "keys": 8,
                   "python_route_max_abs_diff": float(max(np.abs(py[k][1] - pre[k][1]).max() for k in (0, 1)))}
            variants = {
                "a_update_animation": lambda k, info=False: r.update_animation(T2[k], info=info),
                "b_update_morph_skin": lambda k, info=False: r.update_morph_skin(*pre[k], info=info),
                "c_host_then_update": lambda k, info=False: r.update_morph_skin(*mpt.animation_host(tb, T2[k]), info=info),
                "d_python_then_update": lambda k, info=False: r.update_morph_skin(*python_route(np, scene, tb, T2[k]), info=info),
            }
            for k in (0, 1):
                reps = {vn: variants[vn](k, True) for vn in ("a_update_animation", "b_update_morph_skin")}
                tup = {vn: (i.nodes, i.levels, i.light_nodes, i.light_levels, i.area_ratio, i.light_area_ratio) for vn, i in reps.items()}
                assert tup["a_update_animation"] == tup["b_update_morph_skin"], tup
                res[f"area_ratio_time{k + 1}"] = round(tup["b_update_morph_skin"][4], 4)
            res["wall_ms"], res["gpu_ms"] = measure(r, variants, J)
            out["joints"][str(J)] = res
    if a.kernel_trace:
        out["k_anim_us"] = kernel_times(a.kernel_trace, a.calls, joints)
        out["k_anim_us_method"] = f"rocprofv3 --kernel-trace in a run of its own (--variant anim --calls {a.calls}), the first dispatch of each configuration left out"
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
