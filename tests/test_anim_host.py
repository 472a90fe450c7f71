"""mpt_animation_host: the host loop of csrc/anim.h, which mpt_update_animation's kernel shares byte
for byte (tests/test_anim.py compares the two on the GPU); check_animation's refusals; the glTF
loader's SceneData.animations and SceneData.nodes; synthetic.write_animated_gltf.  No GPU.

The reference of the numeric comparison is gltf_eval below: numpy float64 straight from the glTF
formulas (slerp by np.arccos / np.sin at every angle, the cubic spline's Hermite basis, matrices by
@), reading the file itself; it shares no code with csrc/anim.h or mpt.scene.

BOUND.  Measured on the CPU over both clips of the tube file and all the times below, the largest
absolute difference between mpt.animation_host and gltf_eval is 2.70e-7 for the matrix entries
(largest entry 1.243) and 1.33e-7 for the weights (the cubic spline's): fp32 key arithmetic, slerp
and spline (a few ulp of 1), and one rounding of each matrix entry to float.  The test's bounds are
four times that, 1.08e-6 and 5.33e-7; both are below 1e-4 times the largest matrix entry.
"""
import base64
import copy
import json
import os

import numpy as np
import pytest

import mpt
from mpt import abi, scene, synthetic

F = np.float32
BOUND_M = 1.08e-6    # 4 x the measured 2.70e-7 (matrix entries)
BOUND_W = 5.33e-7    # 4 x the measured 1.33e-7 (weights)

_cache = {}


def tube():
    """(path, SceneData) of synthetic.write_animated_gltf, kept for the session."""
    if "tube" not in _cache:
        import tempfile
        d = tempfile.mkdtemp(prefix="mpt_anim_")
        p = synthetic.write_animated_gltf(os.path.join(d, "tube_anim.gltf"))
        _cache["tube"] = (p, scene.load_gltf(p))
    return _cache["tube"]


# ------------------------------------------------------------------------------------
# The independent evaluation
# ------------------------------------------------------------------------------------
_DT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_NC = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def _read(path):
    g = json.load(open(path))
    buf = base64.b64decode(g["buffers"][0]["uri"].split(",", 1)[1])

    def acc(i):
        a = g["accessors"][i]
        bv = g["bufferViews"][a["bufferView"]]
        dt = np.dtype(_DT[a["componentType"]])
        raw = np.frombuffer(buf, dt, a["count"] * _NC[a["type"]], bv.get("byteOffset", 0) + a.get("byteOffset", 0))
        v = raw.astype(np.float64).reshape(a["count"], _NC[a["type"]])
        if a.get("normalized"):
            v = {1: lambda c: np.maximum(c / 127.0, -1.0), 2: lambda c: np.maximum(c / 32767.0, -1.0)}[dt.itemsize](v) \
                if dt.kind == "i" else v / (255.0 if dt.itemsize == 1 else 65535.0)
        return v
    return g, acc


def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _sample64(times, vals, interp, rot, t):
    """glTF 2.0 appendix C in float64.  vals: [K, W] or [3K, W]."""
    K = len(times)
    v = (lambda k: vals[3 * k + 1]) if interp == "CUBICSPLINE" else (lambda k: vals[k])
    t = min(max(t, times[0]), times[-1])
    if K == 1 or t >= times[-1]:
        return v(K - 1)
    k = int(np.searchsorted(times, t, side="right")) - 1
    td = times[k + 1] - times[k]
    u = (t - times[k]) / td
    if interp == "STEP" or u == 0:      # on a key every formula below gives the stored value
        return v(k)
    if interp == "LINEAR" and rot:
        a, b = v(k), v(k + 1)
        d = float(a @ b)
        if d < 0:
            b, d = -b, -d
        th = np.arccos(min(d, 1.0))
        q = (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th) if np.sin(th) > 1e-9 else a + u * (b - a)
        return q / np.linalg.norm(q)
    if interp == "LINEAR":
        return (1 - u) * v(k) + u * v(k + 1)
    u2, u3 = u * u, u * u * u
    p = (2 * u3 - 3 * u2 + 1) * v(k) + td * (u3 - 2 * u2 + u) * vals[3 * k + 2] + (-2 * u3 + 3 * u2) * v(k + 1) \
        + td * (u3 - u2) * vals[3 * (k + 1)]
    return p / np.linalg.norm(p) if rot else p


def gltf_eval(path, clip, t):
    """(weights float64 [T], joint matrices float64 [J, 3, 4]) of the tube file at time t: the file's
    skin on node 0 and its mesh's weights, in the loader's convention (vertices in world space, so
    the joint matrix is world_j @ inverse_bind_j @ inverse(world of the mesh node at rest))."""
    g, acc = _read(path)
    nodes = g["nodes"]
    T_ = {i: np.array(n.get("translation", [0, 0, 0]), np.float64) for i, n in enumerate(nodes)}
    R_ = {i: np.array(n.get("rotation", [0, 0, 0, 1]), np.float64) for i, n in enumerate(nodes)}
    S_ = {i: np.array(n.get("scale", [1, 1, 1]), np.float64) for i, n in enumerate(nodes)}
    mesh_node = next(i for i, n in enumerate(nodes) if "skin" in n)
    w = np.array(g["meshes"][nodes[mesh_node]["mesh"]]["weights"], np.float64)

    def local(i, pose):
        n = nodes[i]
        if "matrix" in n:
            return np.array(n["matrix"], np.float64).reshape(4, 4).T
        tr, ro, sc = pose[i] if pose else (np.array(n.get("translation", [0, 0, 0.0])), np.array(n.get("rotation", [0, 0, 0, 1.0])),
                                           np.array(n.get("scale", [1, 1, 1.0])))
        m = np.eye(4)
        m[:3, :3] = _qmat(ro) @ np.diag(sc)
        m[:3, 3] = tr
        return m

    parent = {c: i for i, n in enumerate(nodes) for c in n.get("children", [])}

    def world(i, pose):
        m = local(i, pose)
        while i in parent:
            i = parent[i]
            m = local(i, pose) @ m
        return m

    an = g["animations"][clip]
    for ch in an["channels"]:
        sm = an["samplers"][ch["sampler"]]
        times = acc(sm["input"]).reshape(-1)
        ni, pth = ch["target"]["node"], ch["target"]["path"]
        wd = {"translation": 3, "rotation": 4, "scale": 3, "weights": len(w)}[pth]
        val = _sample64(times, acc(sm["output"]).reshape(-1, wd), sm.get("interpolation", "LINEAR"), pth == "rotation", float(t))
        if pth == "weights":
            w = val
        else:
            {"translation": T_, "rotation": R_, "scale": S_}[pth][ni] = val
    pose = {i: (T_[i], R_[i], S_[i]) for i in range(len(nodes))}
    sk = g["skins"][nodes[mesh_node]["skin"]]
    ibm = acc(sk["inverseBindMatrices"]).reshape(-1, 4, 4).transpose(0, 2, 1)
    Minv = np.linalg.inv(world(mesh_node, None))
    return w, np.stack([(world(j, pose) @ ibm[k] @ Minv)[:3] for k, j in enumerate(sk["joints"])])


def key_times(path, clip):
    g, acc = _read(path)
    return [acc(s["input"]).reshape(-1) for s in g["animations"][clip]["samplers"]]


def sample_times(path, clip):
    """Before the first key, every key, after the last, 50 random times in between (fixed seed); the
    negative-dot pair (keys at 0.5 and 1.0 s) and the pair above the lerp threshold (1.0 and 1.5 s)
    on and between their keys."""
    ks = np.unique(np.concatenate(key_times(path, clip)))
    rng = np.random.default_rng(7)
    ts = [float(ks[0]) - 0.5] + [float(k) for k in ks] + [float(ks[-1]) + 0.5] + list(rng.uniform(ks[0], ks[-1], 50))
    return ts + [0.5, 0.625, 0.75, 0.875, 1.0, 1.125, 1.25, 1.375, 1.5]


# ------------------------------------------------------------------------------------
# Loader
# ------------------------------------------------------------------------------------
def test_loader_reads_the_clips():
    path, sd = tube()
    assert [a.name for a in sd.animations] == ["bend", "face"]
    a0, a1 = sd.animations
    assert [(c.sampler, c.node, c.path) for c in a0.channels] == [(0, 2, "rotation"), (1, 3, "rotation"), (2, 2, "translation"),
                                                                   (3, 3, "scale"), (4, 0, "weights")]
    assert [(s.interpolation, len(s.times), s.values.shape) for s in a0.samplers] == [
        ("LINEAR", 4, (4, 4)), ("CUBICSPLINE", 3, (9, 4)), ("STEP", 3, (3, 3)), ("LINEAR", 2, (2, 3)), ("LINEAR", 3, (3, 2))]
    assert [(c.sampler, c.node, c.path) for c in a1.channels] == [(0, 0, "weights"), (1, 3, "translation")]
    assert [(s.interpolation, len(s.times), s.values.shape) for s in a1.samplers] == [("CUBICSPLINE", 3, (9, 2)), ("LINEAR", 1, (1, 3))]
    assert a0.duration == 1.5 and a1.duration == 2.0
    for s in a0.samplers + a1.samplers:
        assert s.times.dtype == np.float32 and s.values.dtype == np.float32
    # the rotation stored as normalised signed shorts: max(c / 32767, -1)
    g = json.load(open(path))
    out = g["accessors"][g["animations"][0]["samplers"][0]["output"]]
    assert out["componentType"] == 5122 and out["normalized"]
    bv = g["bufferViews"][out["bufferView"]]
    raw = np.frombuffer(base64.b64decode(g["buffers"][0]["uri"].split(",", 1)[1]), np.int16, 16, bv["byteOffset"]).reshape(4, 4)
    want = np.maximum(raw.astype(np.float64) / 32767.0, -1.0)
    assert np.array_equal(a0.samplers[0].values, want.astype(F))
    assert a0.samplers[0].values[1] @ a0.samplers[0].values[2] < 0          # the negative-dot pair
    assert a0.samplers[0].values[2] @ a0.samplers[0].values[3] > 0.9995     # the pair above the lerp threshold
    # the node table
    nt = sd.nodes
    assert nt.is_trs.tolist() == [1, 0, 1, 1, 1, 1] and nt.parents.tolist() == [-1, -1, 1, 2, -1, -1]
    assert np.array_equal(nt.locals, sd.skin.node_locals) and np.array_equal(nt.parents, sd.skin.node_parents)
    assert np.array_equal(nt.trs[2], np.array([0, 0.6, 0, 0, 0, 0, 1, 1, 1, 1], F))
    assert nt.trs.dtype == np.float32 and nt.locals.dtype == np.float64


def _broken(tmp_path, edit):
    path, _ = tube()
    g = json.load(open(path))
    edit(g)
    p = str(tmp_path / "broken.gltf")
    json.dump(g, open(p, "w"))
    return p


def _dup(g):
    g["animations"][0]["channels"].append(copy.deepcopy(g["animations"][0]["channels"][0]))


@pytest.mark.parametrize("edit,what", [
    (lambda g: g["animations"][0]["channels"][0]["target"].update(node=1), "matrix"),
    (lambda g: g["animations"][1]["channels"][0]["target"].update(node=2), "no morph targets"),
    (lambda g: g["animations"][0]["samplers"][3].update(input=g["animations"][0]["samplers"][2]["input"]), "output components"),
    (_dup, "two channels"),
], ids=["matrix_node", "weights_without_targets", "count_mismatch", "duplicate_channel"])
def test_loader_refuses_malformed_animations(tmp_path, edit, what):
    with pytest.raises(ValueError, match=what) as e:
        scene.load_gltf(_broken(tmp_path, edit))
    assert "broken.gltf" in str(e.value) and "animation" in str(e.value)


def test_files_without_animations_load_as_before(tmp_path):
    a = scene.load_gltf(synthetic.write_morphed_gltf(str(tmp_path / "m.gltf")))
    _, b = tube()
    assert a.animations == []
    for f in ("joints", "weights", "joint_nodes", "bind", "node_parents", "node_locals"):
        assert np.array_equal(getattr(a.skin, f), getattr(b.skin, f)), f
    for f in ("target_offsets", "vertex_ids", "pos_deltas", "nrm_deltas", "target_node", "target_index", "default_weights"):
        assert np.array_equal(getattr(a.morph, f), getattr(b.morph, f)), f
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.normals, b.normals)
    c = scene.load_gltf(synthetic.write_morphed_gltf(str(tmp_path / "u.gltf"), skinned=False))
    assert c.animations == [] and c.nodes is None and c.skin is None


# ------------------------------------------------------------------------------------
# Against the independent evaluation
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0, 1])
def test_host_equals_the_gltf_formulas(clip):
    path, sd = tube()
    worst_m = worst_w = biggest = 0.0
    for t in sample_times(path, clip):
        w, m = mpt.animation_host(sd, t, clip)
        rw, rm = gltf_eval(path, clip, F(t))
        worst_m = max(worst_m, float(np.abs(m - rm).max()))
        worst_w = max(worst_w, float(np.abs(w - rw).max()))
        biggest = max(biggest, float(np.abs(rm).max()))
    print(f"clip {clip}: matrices {worst_m:.3e} (largest entry {biggest:.3f}), weights {worst_w:.3e}")
    assert BOUND_M < 1e-4 * biggest
    assert worst_m <= BOUND_M and worst_w <= BOUND_W


def test_the_pose_moves():
    path, sd = tube()
    rest = scene.skin_matrices(sd)
    w, m = mpt.animation_host(sd, 0.75, 0)
    assert np.abs(m - rest).max() > 0.05 and np.abs(w - sd.morph.default_weights).max() > 0.1


def no_channels(tb):
    tb = dict(tb)
    for k in tb:
        if k.startswith("channel"):
            tb[k] = tb[k][:0]
    return tb


def test_rest_pose():
    _, sd = tube()
    w, m = mpt.animation_host(no_channels(mpt.animation_tables(sd, 0)), 0.3)
    assert np.abs(m - scene.skin_matrices(sd)).max() <= BOUND_M
    assert w.tobytes() == sd.morph.default_weights.tobytes()


# ------------------------------------------------------------------------------------
# Synthetic tables (tests/test_anim.py uses them on the GPU)
# ------------------------------------------------------------------------------------
def _rand_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


def rest_world(parents, trs):
    """World matrices [N, 4, 4] float64 of the base TRS (the test's own composition)."""
    N = len(parents)
    loc = np.tile(np.eye(4), (N, 1, 1))
    for n in range(N):
        loc[n, :3, :3] = _qmat(trs[n, 3:7].astype(np.float64)) @ np.diag(trs[n, 7:10].astype(np.float64))
        loc[n, :3, 3] = trs[n, 0:3]
    done = {}
    for n in range(N):
        chain = []
        m = n
        while m >= 0 and m not in done:
            chain.append(m)
            m = int(parents[m])
        for c in reversed(chain):
            done[c] = loc[c] if parents[c] < 0 else done[int(parents[c])] @ loc[c]
    return np.stack([done[n] for n in range(N)]), loc


def make_tables(parents, joint_nodes, T=0, channels=0, keys=3, seed=0, weight_channels=(), interps=(1, 2, 0)):
    """Random tables: every node TRS with a small random base pose; bind = inverse of the rest world,
    so the rest pose is the identity up to rounding.  `channels` TRS channels over distinct (node,
    path) pairs in a shuffled order, each with its own sampler of `keys` keys (an int, or a list
    cycled over the channels) and the interpolations cycled from interps; weight_channels: (first
    target, count) stretches, each a weights channel of its own."""
    rng = np.random.default_rng(seed)
    parents = np.asarray(parents, np.int32)
    N = len(parents)
    trs = np.zeros((N, 10), F)
    trs[:, 0:3] = rng.normal(size=(N, 3)) * 0.05
    trs[:, 3:7] = _rand_quat(rng, N)
    trs[:, 7:10] = rng.uniform(0.97, 1.03, (N, 3))
    world, loc = rest_world(parents, trs)
    jn = np.asarray(joint_nodes, np.int32)
    bind = np.stack([np.linalg.inv(world[j]) for j in jn])[:, :3, :] if len(jn) else np.zeros((0, 3, 4))
    pairs = [(n, p) for n in range(N) for p in range(3)]
    order = rng.permutation(len(pairs))[:channels]
    assert len(order) == channels, "more channels than (node, path) pairs"
    klist = [keys] if isinstance(keys, int) else list(keys)
    koff, voff, times, vals, interp = [0], [0], [], [], []
    cs, cn, cp, c0, ck = [], [], [], [], []

    def add_sampler(K, width, ip, rot):
        t = np.cumsum(rng.uniform(0.05, 0.3, K)).astype(F)
        rows = K * (3 if ip == 2 else 1)
        if rot:
            v = _rand_quat(rng, rows)
            if ip == 2:
                v[0::3] *= F(0.3)
                v[2::3] *= F(0.3)
        elif width == 3:
            v = rng.normal(size=(rows, width)).astype(F) * F(0.1)
        else:
            v = rng.uniform(-1, 1, (rows, width)).astype(F)
        times.append(t)
        vals.append(v.reshape(-1))
        koff.append(koff[-1] + K)
        voff.append(voff[-1] + v.size)
        interp.append(ip)
        return len(interp) - 1

    for i, o in enumerate(order):
        n, p = pairs[int(o)]
        s = add_sampler(klist[i % len(klist)], 4 if p == 1 else 3, interps[i % len(interps)], p == 1)
        if p == 2:       # scales near 1, so that a deep chain stays finite
            vals[-1] = (F(1.0) + vals[-1] * F(0.3)).astype(F)
        cs.append(s); cn.append(n); cp.append(p); c0.append(0); ck.append(0)
    for i, (first, count) in enumerate(weight_channels):
        s = add_sampler(klist[i % len(klist)], count, interps[i % len(interps)], False)
        cs.append(s); cn.append(0); cp.append(3); c0.append(first); ck.append(count)
    tb = {"node_parents": parents, "node_trs": trs, "node_is_trs": np.ones(N, np.uint8), "node_locals": loc[:, :3, :],
          "joint_nodes": jn, "joint_bind": bind, "base_weights": rng.uniform(-0.5, 0.5, T).astype(F),
          "sampler_key_offsets": koff if interp else [], "key_times": np.concatenate(times) if times else [],
          "sampler_value_offsets": voff if interp else [], "values": np.concatenate(vals) if vals else [], "sampler_interp": interp,
          "channel_sampler": cs, "channel_node": cn, "channel_path": cp, "channel_first_target": c0, "channel_num_targets": ck}
    return {k: np.ascontiguousarray(tb[k], dt) for k, dt in mpt._ANIM_FIELDS}


def chain(n):
    return np.arange(-1, n - 1)


def permuted(tb, seed=3):
    """The same animation with the nodes renumbered so that every child precedes its parent."""
    N = len(tb["node_parents"])
    world, _ = rest_world(tb["node_parents"], tb["node_trs"])
    depth = np.zeros(N, int)
    for n in range(N):
        m = n
        while tb["node_parents"][m] >= 0:
            m = tb["node_parents"][m]
            depth[n] += 1
    rng = np.random.default_rng(seed)
    old_of_new = np.lexsort((rng.random(N), -depth))      # deepest first
    new_of_old = np.empty(N, np.int64)
    new_of_old[old_of_new] = np.arange(N)
    out = dict(tb)
    out["node_parents"] = np.where(tb["node_parents"][old_of_new] >= 0, new_of_old[tb["node_parents"][old_of_new]], -1).astype(np.int32)
    for k in ("node_trs", "node_is_trs", "node_locals"):
        out[k] = np.ascontiguousarray(tb[k][old_of_new])
    out["joint_nodes"] = new_of_old[tb["joint_nodes"]].astype(np.int32)
    out["channel_node"] = new_of_old[tb["channel_node"]].astype(np.int32)
    return out


# ------------------------------------------------------------------------------------
# Exact cases
# ------------------------------------------------------------------------------------
def one_channel(interp, times, values, path=0, T=0):
    """One root node (one joint on it, bind the identity) and one channel."""
    tb = make_tables([-1], [0], T=T, channels=0)
    tb["node_trs"][:] = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    tb["joint_bind"][:] = np.eye(4)[:3]
    v = np.asarray(values, F)
    tb.update(sampler_key_offsets=np.array([0, len(times)], np.int32), key_times=np.asarray(times, F),
              sampler_value_offsets=np.array([0, v.size], np.int32), values=v.reshape(-1), sampler_interp=np.array([interp], np.int32),
              channel_sampler=np.array([0], np.int32), channel_node=np.array([0], np.int32), channel_path=np.array([path], np.int32),
              channel_first_target=np.array([0], np.int32), channel_num_targets=np.array([T if path == 3 else 0], np.int32))
    return tb


def test_stored_values_come_back_exactly():
    vals = np.array([[0.1, 0.0, 0.3], [1e-3, 7.7, -2.5], [3.25, 0.2, 0.7]], F)
    wvals = np.array([[0.1, -0.0, 0.3], [-0.0, 7.7, -2.5], [3.25, 0.2, -0.0]], F)   # (a matrix product would lose the sign)
    # a one-key sampler at any time
    for t in (-1.0, 0.5, 9.0):
        _, m = mpt.animation_host(one_channel(abi.ANIM_LINEAR, [0.5], vals[:1]), t)
        assert m[0, :, 3].tobytes() == vals[0].tobytes()
    # STEP: the key at or before t
    tb = one_channel(abi.ANIM_STEP, [0.0, 1.0, 2.0], vals)
    for t, k in ((-1, 0), (0, 0), (0.99, 0), (1.0, 1), (1.5, 1), (2.0, 2), (5, 2)):
        assert mpt.animation_host(tb, t)[1][0, :, 3].tobytes() == vals[k].tobytes(), t
    # LINEAR on a key (a -0 keeps its sign); weights as well
    tb = one_channel(abi.ANIM_LINEAR, [0.25, 1.0, 2.0], vals)
    for t, k in ((0.25, 0), (1.0, 1), (2.0, 2), (0.0, 0), (3.0, 2)):
        assert mpt.animation_host(tb, t)[1][0, :, 3].tobytes() == vals[k].tobytes(), t
    tb = one_channel(abi.ANIM_LINEAR, [0.25, 1.0, 2.0], wvals, path=3, T=3)
    for t, k in ((0.25, 0), (1.0, 1), (2.0, 2)):
        assert mpt.animation_host(tb, t)[0].tobytes() == wvals[k].tobytes(), t
    # the one-key sampler of the tube file's second clip
    _, sd = tube()
    tbl = mpt.animation_tables(sd, 1)
    s = sd.animations[1].samplers[1]
    only = no_channels(tbl)
    for k in ("channel_sampler", "channel_node", "channel_path", "channel_first_target", "channel_num_targets"):
        only[k] = tbl[k][1:2]
    one = mpt.animation_host(only, 0.1)[1]
    moved = copy.deepcopy(only)
    moved["node_trs"][3, 0:3] = s.values[0]
    assert one.tobytes() == mpt.animation_host(no_channels(moved), 0.1)[1].tobytes()


def test_linear_between_keys_is_a_plus_u_times_b_minus_a():
    vals = np.array([[0.1, 0.2, 0.3], [1.5, 7.7, -2.5]], F)
    tb = one_channel(abi.ANIM_LINEAR, [0.25, 1.0], vals)
    t = F(0.6)
    u = F(F(t - F(0.25)) / F(F(1.0) - F(0.25)))
    want = (vals[0] + (u * (vals[1] - vals[0])).astype(F)).astype(F)
    assert mpt.animation_host(tb, t)[1][0, :, 3].tobytes() == want.tobytes()


def test_identity_pose_has_the_identity_word():
    """One joint whose world times bind is exactly the identity: the matrix is the identity's bytes,
    which is what sets the record's identity word (mptxform::is_identity on these floats; the GPU
    test shows that no bit of the geometry changes)."""
    tb = one_channel(abi.ANIM_STEP, [0.0, 1.0], [[0, 0, 0, 1], [0, 0, 0, 1]], path=1)
    _, m = mpt.animation_host(tb, 0.5)
    assert m.tobytes() == np.eye(4, dtype=F)[:3][None].tobytes()


def test_children_before_parents_give_the_same_bytes():
    parents = np.array([-1, 0, 0, 1, 1, 2, 3, 3, 6, -1, 9, 10])
    tb = make_tables(parents, [11, 8, 4, 4, 0, 7], T=5, channels=20, keys=[1, 2, 3, 5], seed=5, weight_channels=[(1, 3)])
    pb = permuted(tb)
    assert (pb["node_parents"] > np.arange(len(parents))).any()
    for t in (0.0, 0.21, 0.4, 0.77, 2.0):
        w, m = mpt.animation_host(tb, t)
        pw, pm = mpt.animation_host(pb, t)
        assert m.tobytes() == pm.tobytes() and w.tobytes() == pw.tobytes()
    _, sd = tube()
    tube_tb = mpt.animation_tables(sd, 0)
    a, b = mpt.animation_host(tube_tb, 0.8), mpt.animation_host(permuted(tube_tb), 0.8)
    assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes()


# ------------------------------------------------------------------------------------
# check_animation
# ------------------------------------------------------------------------------------
def _base():
    return make_tables([-1, 0, 1], [2, 1], T=4, channels=9, keys=3, seed=9, weight_channels=[(0, 2)])


def _set(key, index, value):
    def edit(tb):
        tb[key] = tb[key].copy()
        tb[key][index] = value
    return edit


def _rot_channel(tb):
    return int(np.flatnonzero(tb["channel_path"] == 1)[0])


def _zero_rotation(tb):
    c = _rot_channel(tb)
    s = tb["channel_sampler"][c]
    o = tb["sampler_value_offsets"][s] + (4 if tb["sampler_interp"][s] == 2 else 0)
    tb["values"] = tb["values"].copy()
    tb["values"][o:o + 4] = 0


def _same_component(tb):
    for k in ("channel_sampler", "channel_node", "channel_path", "channel_first_target", "channel_num_targets"):
        tb[k] = np.concatenate([tb[k], tb[k][:1]])


def _overlap(tb):
    for k in ("channel_sampler", "channel_node", "channel_path", "channel_first_target", "channel_num_targets"):
        tb[k] = np.concatenate([tb[k], tb[k][-1:]])
    tb["channel_first_target"][-1] = 1


REFUSALS = {
    "parent_out_of_range": (_set("node_parents", 1, 3), "parent index"),
    "parent_cycle": (_set("node_parents", 0, 2), "cycle"),
    "joint_node_out_of_range": (_set("joint_nodes", 0, 3), "joint node"),
    "channel_node_out_of_range": (_set("channel_node", 0, -1), "channel node"),
    "offsets_decrease": (_set("sampler_key_offsets", 2, 2), "offsets decrease"),
    "key_time_not_finite": (_set("key_times", 1, np.inf), "key time not finite"),
    "key_times_not_ascending": (_set("key_times", 1, 0.0), "strictly ascending"),
    "non_finite_value": (_set("values", 5, np.nan), "non-finite value"),
    "zero_rotation": (_zero_rotation, "zero length"),
    "weights_outside_targets": (_set("channel_first_target", -1, 3), "outside the targets"),
    "same_component_trs": (_same_component, "same component"),
    "same_component_weights": (_overlap, "same component"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_check_animation_refuses(name):
    tb = _base()
    assert (tb["channel_path"] == 1).any()
    mpt.animation_host(tb, 0.2)                  # the base tables are accepted
    edit, what = REFUSALS[name]
    edit(tb)
    with pytest.raises(mpt.MptError, match=what) as e:
        mpt.animation_host(tb, 0.2)
    assert e.value.code == abi.ERR_INVALID_ARGUMENT


def test_host_refuses_a_time_that_is_not_finite():
    for t in (np.nan, np.inf):
        with pytest.raises(mpt.MptError, match="time not finite"):
            mpt.animation_host(_base(), t)


def zero_quaternion_clip():
    """A CUBICSPLINE rotation from q to -q with zero tangents: the spline passes through the zero
    quaternion at u = 1/2 exactly (h00 = h01 = 1/2), so the normalisation divides 0 by 0."""
    q = [0.0, 0.0, 0.0, 1.0]
    z = [0.0] * 4
    return one_channel(abi.ANIM_CUBICSPLINE, [0.0, 1.0], [z, q, z, z, [-x for x in q], z], path=1)


def test_a_spline_through_the_zero_quaternion_is_refused():
    tb = zero_quaternion_clip()
    mpt.animation_host(tb, 0.25)
    with pytest.raises(mpt.MptError, match="non-finite"):
        mpt.animation_host(tb, 0.5)
