"""mpt_set_animation / mpt_update_animation on the GPU (csrc/anim.hip: k_anim).

Renderer A sets skin, morph and animation and calls update_animation(t): the clip is sampled, the
hierarchy composed and the palette and weights written on the device.  Renderer B gets
mpt.animation_host(t)'s weights and matrices through update_morph_skin (update_skin / update_morph
when only one of the two is driven), which is the path tests/test_morph.py and tests/test_skin.py
pin to the host mirrors.  Both must leave the same bytes: both trees (nodes and records hold every
position), the report, and -- through a render against the oracle -- the normals.  The shapes are
the ones at which k_anim can go wrong: tails of its strided loops, both homes of the world
matrices, deep and wide hierarchies, node numberings, padding of the weights.
"""
import copy

import numpy as np
import pytest

import mpt
from mpt import abi

from test_anim_host import chain, make_tables, one_channel, permuted, tube, zero_quaternion_clip
from test_gpu_parity import assert_same, frames, gpu_render, oracle_for
from test_morph import case as morph_case, many_targets
from test_refit import fresh
from test_shade_classes import _assert_modes_equal
from test_skin import cornell_skin, random_skin
from test_xform import assert_trees_equal, edge_scene, info_tuple, soup_scene, trees

pytestmark = pytest.mark.gpu

F = np.float32


def device_path(luts, sd, tb, times, skin=None, morph=None, clip=0):
    """[(info, trees)] after update_animation(t) for every t, one renderer."""
    r = fresh(sd, luts)
    try:
        if skin is not None:
            r.set_skin(skin[0], skin[1], num_joints=skin[2])
        if morph is not None:
            r.set_morph(morph)
        r.set_animation(tb, clip)
        return [(info_tuple(r.update_animation(t, info=True)), trees(r)) for t in times]
    finally:
        r.close()


def host_path(luts, sd, tb, times, skin=None, morph=None, clip=0):
    """The same through mpt.animation_host and update_morph_skin / update_skin / update_morph."""
    r = fresh(sd, luts)
    try:
        if skin is not None:
            r.set_skin(skin[0], skin[1], num_joints=skin[2])
        if morph is not None:
            r.set_morph(morph)
        out = []
        for t in times:
            w, m = mpt.animation_host(tb, t, clip)
            if w is not None and m is not None:
                i = r.update_morph_skin(w, m, info=True)
            elif m is not None:
                i = r.update_skin(m, info=True)
            else:
                i = r.update_morph(w, info=True)
            out.append((info_tuple(i), trees(r)))
        return out
    finally:
        r.close()


def assert_paths_equal(dev, host, what):
    assert len(dev) == len(host)
    for k, (d, h) in enumerate(zip(dev, host)):
        assert d[0] == h[0], f"{what}, time {k}: report"
        assert_trees_equal(d[1], h[1], f"{what}, time {k}")


# ------------------------------------------------------------------------------------
# The tube file
# ------------------------------------------------------------------------------------
TUBE_TIMES = {0: [-0.5, 0.5, 0.8, 1.5, 2.5], 1: [-0.5, 1.0, 1.4, 2.0, 3.0]}   # before, a key, between, the last key, after


@pytest.mark.parametrize("clip", [0, 1])
def test_tube_bytes_equal_host_path(luts, clip):
    _, sd = tube()
    skin = (sd.skin.joints, sd.skin.weights, sd.skin.num_joints)
    dev = device_path(luts, sd, sd, TUBE_TIMES[clip], skin, sd.morph, clip)
    host = host_path(luts, sd, sd, TUBE_TIMES[clip], skin, sd.morph, clip)
    assert_paths_equal(dev, host, f"tube clip {clip}")
    assert all(d[0][4] != 1.0 for d in dev)          # area_ratio: no time leaves the upload's pose


def test_tube_only_the_skin_or_only_the_morph_driven(luts):
    _, sd = tube()
    tb = mpt.animation_tables(sd, 0)
    skin = (sd.skin.joints, sd.skin.weights, sd.skin.num_joints)
    only_skin = dict(tb)
    keep = tb["channel_path"] != abi.ANIM_PATH_WEIGHTS
    for k in tb:
        if k.startswith("channel"):
            only_skin[k] = tb[k][keep]
    only_skin["base_weights"] = tb["base_weights"][:0]
    dev = device_path(luts, sd, only_skin, TUBE_TIMES[0], skin=skin)
    assert_paths_equal(dev, host_path(luts, sd, only_skin, TUBE_TIMES[0], skin=skin), "only the skin")
    assert dev[2][0][4] != 1.0
    only_morph = dict(tb)
    only_morph["joint_nodes"], only_morph["joint_bind"] = tb["joint_nodes"][:0], tb["joint_bind"][:0]
    dev = device_path(luts, sd, only_morph, TUBE_TIMES[0], morph=sd.morph)
    assert_paths_equal(dev, host_path(luts, sd, only_morph, TUBE_TIMES[0], morph=sd.morph), "only the morph")
    assert dev[2][0][4] != 1.0
    # with the skin set as well and never posed, the morph alone is still what is evaluated
    dev2 = device_path(luts, sd, only_morph, TUBE_TIMES[0][2:3], skin=skin, morph=sd.morph)
    assert_trees_equal(dev2[0][1], dev[2][1], "only the morph driven, an unposed skin set")


def test_render_after_update_animation(luts):
    """The tube at t mid-clip: the oracle of a fresh upload of skin_host(morph_host(rest)) for
    animation_host(t)."""
    _, sd0 = tube()
    t = 0.8
    w, m = mpt.animation_host(sd0, t, 0)
    sd = copy.copy(sd0)
    sd.vertices, sd.normals = mpt.skin_host(*mpt.morph_host(sd0.vertices, sd0.normals, sd0.morph, w), sd0.skin.joints, sd0.skin.weights, m)
    frs = frames(sd, 40, 24, 3, lss=abi.LSS_MIS_LIGHT_BSDF)
    r = fresh(sd0, luts)
    try:
        r.set_skin(sd0.skin.joints, sd0.skin.weights, num_joints=sd0.skin.num_joints)
        r.set_morph(sd0.morph)
        r.set_animation(sd0, 0)
        r.update_animation(t)
        out = {1: gpu_render(r, frs)}
    finally:
        r.close()
    ref = oracle_for(sd, luts).render(frs, aov=True)
    _assert_modes_equal(out, ref, "tube mid-clip")
    assert out[1][0].mean() > 0
    assert not np.array_equal(ref[0], oracle_for(sd0, luts).render(frs, aov=True)[0])   # the pose shows


# ------------------------------------------------------------------------------------
# Shapes
# ------------------------------------------------------------------------------------
NV = 129


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return np.array([-1] + [int(rng.integers(max(0, i - 40), i)) for i in range(1, n)])


def star(n):
    return np.array([-1] + [0] * n)


L, SJ = mpt.ANIM_LDS_NODES, mpt.SKIN_LDS_JOINTS
# name: (parents, joint nodes, targets, TRS channels, keys, weights channels)
SHAPES = {
    "keys_1_2_3_64_65": (random_tree(9, 1), [8, 3, 0], 3, 15, [1, 2, 3, 64, 65], [(0, 3)]),
    "channels_0": (random_tree(400, 2), [399, 7], 2, 0, 3, []),
    "channels_1": (random_tree(400, 2), [399, 7], 2, 1, 3, []),
    "channels_1023": (random_tree(400, 2), [399, 7, 200], 2, 1022, [2, 3], [(0, 2)]),
    "channels_1025": (random_tree(400, 2), [399, 7, 200], 2, 1024, [2, 3], [(0, 2)]),
    "node_1": ([-1], [0], 0, 3, 3, []),
    "nodes_budget": (random_tree(L, 3), [L - 1, 0, L // 2], 1, 40, 3, [(0, 1)]),
    "nodes_past_budget": (random_tree(L + 1, 3), [L, 0, L // 2], 1, 40, 3, [(0, 1)]),
    "chain_70": (chain(70), [69, 35, 0, 64], 0, 100, 2, []),
    "star_1025": (star(1025), [1025, 1, 256, 257, 0], 0, 300, 2, []),
    "joint_1": (random_tree(5, 4), [4], 0, 6, 3, []),
    "joints_budget": (random_tree(300, 5), list(np.arange(SJ) + 40), 0, 60, 3, []),
    "joints_past_budget": (random_tree(300, 5), list(np.arange(SJ + 1) + 40), 0, 60, 3, []),
    "two_joints_on_one_node": (random_tree(6, 6), [5, 5, 2], 0, 8, 3, []),
    "targets_1": (random_tree(4, 7), [3], 1, 4, 3, [(0, 1)]),
    "targets_3": (random_tree(4, 7), [3], 3, 4, 3, [(0, 3)]),
    "targets_5": (random_tree(4, 7), [3], 5, 4, 3, [(0, 5)]),
    "two_weight_stretches": (random_tree(4, 7), [3], 5, 4, [3, 2], [(0, 2), (3, 2)]),   # target 2 keeps its base weight
}


def shape_case(name):
    parents, jn, T, C, keys, wch = SHAPES[name]
    tb = make_tables(parents, jn, T=T, channels=C, keys=keys, seed=len(name), weight_channels=wch)
    v, idx = edge_scene(NV)
    sd = soup_scene(v, idx)
    J, W = random_skin(NV, len(jn), 11)
    J[-1, 0], W[-1, 0] = len(jn) - 1, 0.5                      # the last joint is used
    morph = many_targets(NV, T, 5)[0] if T else None
    return sd, tb, (J, W, len(jn)), morph


def mid_time(tb):
    """A time between two keys of most samplers, and one after every last key."""
    return [0.21, 1e3] if len(tb["key_times"]) else [0.0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(monkeypatch, luts, name):
    monkeypatch.delenv("MPT_ANIM_LDS", raising=False)
    sd, tb, skin, morph = shape_case(name)
    times = mid_time(tb)
    dev = device_path(luts, sd, tb, times, skin, morph)
    assert_paths_equal(dev, host_path(luts, sd, tb, times, skin, morph), name)
    if name == "two_weight_stretches":
        w, _ = mpt.animation_host(tb, times[0])
        assert w[2] == tb["base_weights"][2] and not np.array_equal(w, tb["base_weights"])


@pytest.mark.parametrize("name", ["nodes_budget", "nodes_past_budget"])
def test_world_matrices_in_memory_give_the_same_bytes(monkeypatch, luts, name):
    sd, tb, skin, morph = shape_case(name)
    monkeypatch.delenv("MPT_ANIM_LDS", raising=False)
    dev = device_path(luts, sd, tb, [0.21], skin, morph)
    monkeypatch.setenv("MPT_ANIM_LDS", "0")
    assert_paths_equal(device_path(luts, sd, tb, [0.21], skin, morph), dev, f"{name}: MPT_ANIM_LDS=0")


@pytest.mark.parametrize("name", ["keys_1_2_3_64_65", "chain_70", "nodes_past_budget"])
def test_children_before_parents(luts, name):
    sd, tb, skin, morph = shape_case(name)
    pb = permuted(tb)
    assert (pb["node_parents"] > np.arange(len(pb["node_parents"]))).any()
    assert_paths_equal(device_path(luts, sd, pb, [0.21], skin, morph), device_path(luts, sd, tb, [0.21], skin, morph), name)


def test_identity_pose_changes_nothing(luts):
    """One joint whose world times bind is exactly the identity, the weights all zero: every vertex
    passes through (the record's identity word, made on the device), so no bit changes."""
    v, idx = edge_scene(NV)
    sd = soup_scene(v, idx)
    tb = one_channel(abi.ANIM_STEP, [0.0, 1.0], [[0, 0, 0, 1], [0, 0, 0, 1]], path=1, T=2)
    tb["base_weights"][:] = 0
    J, W = random_skin(NV, 1, 3)
    frs = frames(sd, 40, 24, 2)
    a, b = fresh(sd, luts), fresh(sd, luts)
    try:
        a.set_skin(J, W, num_joints=1)
        a.set_morph(many_targets(NV, 2, 5)[0])
        a.set_animation(tb)
        before = trees(a)
        i = a.update_animation(0.5, info=True)
        assert i.area_ratio == 1.0
        assert_trees_equal(trees(a), before, "an identity pose")
        ga, gb = gpu_render(a, frs), gpu_render(b, frs)
        for k, what in enumerate(["color", "albedo", "normals"]):
            assert_same(ga[k], gb[k], f"an identity pose, {what}")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# State
# ------------------------------------------------------------------------------------
def cornell_anim(seed=2):
    """cornell_skin's four joints as a chain of three and a root, cornell_morph's targets 0..2
    driven by one weights channel, target 3 (the overflow's handle) left at its base weight 0."""
    tb = make_tables([-1, 0, 1, -1], [0, 1, 2, 3], T=4, channels=8, keys=3, seed=seed, weight_channels=[(0, 3)])
    tb["base_weights"][3] = 0.0
    return tb


def cornell_setup(r, tb=None):
    sd0, targets = morph_case("cornell")[:2]
    J, W, _, _ = cornell_skin()
    r.set_skin(J, W, 4)
    r.set_morph(targets)
    if tb is not None:
        r.set_animation(tb)


def test_poses_start_from_the_rest_pose(luts):
    sd0 = morph_case("cornell")[0]
    tb = cornell_anim()
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        cornell_setup(a, tb)
        cornell_setup(b, tb)
        a.update_animation(0.15)
        ia = a.update_animation(0.33, info=True)
        ib = b.update_animation(0.33, info=True)
        assert info_tuple(ia) == info_tuple(ib) and ia.area_ratio != 1.0
        assert_trees_equal(trees(a), trees(b), "the second of two times")
    finally:
        a.close()
        b.close()


def test_update_morph_composes_with_the_animated_palette(luts):
    sd0, _, w, _, _, _ = morph_case("cornell")
    tb = cornell_anim()
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        cornell_setup(a, tb)
        cornell_setup(b)
        a.update_animation(0.33)
        a.update_morph(w)
        b.update_morph_skin(w, mpt.animation_host(tb, 0.33)[1])
        assert_trees_equal(trees(a), trees(b), "update_animation, then update_morph")
        # and the retained weights are the animation's: update_skin alone keeps them
        m2 = mpt.animation_host(tb, 0.1)[1]
        a.update_animation(0.33)
        a.update_skin(m2)
        b.update_morph_skin(mpt.animation_host(tb, 0.33)[0], m2)
        assert_trees_equal(trees(a), trees(b), "update_animation, then update_skin")
    finally:
        a.close()
        b.close()


def test_refusals_change_nothing(luts):
    sd0, targets, w, _, _, _ = morph_case("cornell")
    tb = cornell_anim()
    # a clip whose spline passes through the zero quaternion at t = 0.5 (the device's flag)
    zq = zero_quaternion_clip()
    bad = cornell_anim()
    c = int(np.flatnonzero(bad["channel_path"] == abi.ANIM_PATH_ROTATION)[0])
    for k in ("sampler_key_offsets", "key_times", "sampler_value_offsets", "values", "sampler_interp"):
        bad[k] = zq[k]
    for k in bad:
        if k.startswith("channel"):
            bad[k] = bad[k][c:c + 1].copy()
    bad["channel_sampler"][:] = 0
    with pytest.raises(mpt.MptError):
        mpt.animation_host(bad, 0.5)                             # (the host mirror agrees)
    r, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        with mpt.GPURenderer(0) as empty:
            assert mpt.lib().mpt_update_animation(empty.h, 0.0, None) == abi.ERR_NO_SCENE
        cornell_setup(r)
        cornell_setup(b)

        def refused(call, word, what):
            before = trees(r)
            with pytest.raises(mpt.MptError) as e:
                call()
            assert e.value.code == abi.ERR_INVALID_ARGUMENT and word in str(e.value), what
            assert_trees_equal(trees(r), before, what)

        refused(lambda: r.update_animation(0.2), "no animation set", "no animation set")
        r.set_animation(tb)
        r.update_animation(0.2)
        for t in (np.nan, np.inf, -np.inf):
            refused(lambda: r.update_animation(t), "time not finite", f"t = {t}")
        r.set_animation(bad)                                     # (setting an animation changes no geometry)
        r.update_animation(0.25)
        r.update_animation(0.2)
        r.set_animation(tb)
        r.update_animation(0.2)
        r.set_animation(bad)
        refused(lambda: r.update_animation(0.5), "non-finite", "a spline through the zero quaternion")
        # the retained state is the last accepted call's: tb at 0.2
        r.update_morph(w)
        b.update_morph_skin(w, mpt.animation_host(tb, 0.2)[1])
        assert_trees_equal(trees(r), trees(b), "update_morph after the refusals: the palette of the last accepted time")
        r.update_skin(mpt.animation_host(tb, 0.1)[1])
        b.update_skin(mpt.animation_host(tb, 0.1)[1])
        assert_trees_equal(trees(r), trees(b), "update_skin after the refusals")
        # tables that do not fit what is set
        for edit, word in ((dict(joint_nodes=tb["joint_nodes"][:3], joint_bind=tb["joint_bind"][:3]), "joint count"),
                           (dict(base_weights=np.zeros(5, F)), "target count")):
            t2 = dict(tb)
            t2.update(edit)
            refused(lambda: r.set_animation(t2), word, word)
        r.update_animation(0.5 + 1.0)                            # the refused set_animation left the one that was set
    finally:
        r.close()
        b.close()


def test_what_drops_a_skin_or_a_morph_drops_the_animation(luts):
    sd0, targets = morph_case("cornell")[:2]
    J, W, _, _ = cornell_skin()
    tb = cornell_anim()
    drops = {
        "set_scene": lambda r: (r.set_scene(sd0), cornell_setup(r)),
        "set_objects": lambda r: (r.set_objects(np.zeros(len(sd0.vertices), np.int32), 1), r.set_objects(None), cornell_setup(r)),
        "set_skin": lambda r: r.set_skin(J, W, 4),
        "set_morph": lambda r: r.set_morph(targets),
        "set_skin(None)": lambda r: (r.set_skin(None), r.set_skin(J, W, 4)),
        "set_morph(None)": lambda r: (r.set_morph(None), r.set_morph(targets)),
        "set_animation(None)": lambda r: r.set_animation(None),
    }
    r = fresh(sd0, luts)
    try:
        for what, drop in drops.items():
            cornell_setup(r, tb)
            r.update_animation(0.2)
            drop(r)
            with pytest.raises(mpt.MptError) as e:
                r.update_animation(0.2)
            assert e.value.code == abi.ERR_INVALID_ARGUMENT and "no animation set" in str(e.value), what
    finally:
        r.close()


def test_rebuild_then_update_animation(luts):
    sd0 = morph_case("cornell")[0]
    tb = cornell_anim()
    a, b = fresh(sd0, luts), fresh(sd0, luts)
    try:
        cornell_setup(a, tb)
        cornell_setup(b)
        a.update_animation(0.15)
        a.rebuild_bvh(mode=abi.BUILD_LBVH)
        ia = a.update_animation(0.33, info=True)
        ta = trees(a)
        b.update_morph_skin(*mpt.animation_host(tb, 0.15))
        b.rebuild_bvh(mode=abi.BUILD_LBVH)
        ib = b.update_morph_skin(*mpt.animation_host(tb, 0.33), info=True)
        tb_ = trees(b)
    finally:
        a.close()
        b.close()
    assert_trees_equal(ta, tb_, "update_animation vs update_morph_skin after the rebuild")
    assert info_tuple(ia) == info_tuple(ib)
