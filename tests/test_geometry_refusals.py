"""Every refusal of the geometry entry points (csrc/mpt_geometry.cpp), by its exact text.

The other tests of these calls mostly look at the code or at a word of the message.  Here a table
holds one row per refusal string of mpt_update_vertices, mpt_set_objects, mpt_update_transforms,
mpt_set_skin, mpt_update_skin, mpt_set_morph, mpt_update_morph, mpt_update_morph_skin,
mpt_set_normals, mpt_get_vertices, mpt_set_animation, mpt_update_animation and
mpt_update_vertices_device, with the text as the entry points' source had it before they moved out
of mpt_api.cpp.  Every row asserts the code, the exact mpt_last_error, that mpt_get_vertices gives
the same bytes as before the refused call, and that a valid update afterwards succeeds and gives
the bytes it gave before any refusal (so retained weights and palettes are untouched as well).
Non-finite inputs count: a NaN matrix entry, an infinite weight, a NaN time, and finite inputs
whose result overflows on the device.  No row provokes a device fault.

Not reachable from outside, so without a row: "objects do not fit the scene", "rest pose does not
fit the scene", "skin does not fit the scene", "morph does not fit the scene" and
"mpt_set_normals: index mirror differs from the scene's" guard the context's own bookkeeping, and
the HIP and out-of-memory tails need a failing runtime.

The scene: two triangles over vertices 0, 1, 2 and a fourth vertex that no triangle uses.
Contexts, one per state a row needs: "empty" (no scene), "plain" (the scene), "objects" (an object
table), "morph" (a morph of one target), "rig" (a skin of two joints, the morph, an animation of
the morph's weight).
"""
import ctypes as C

import numpy as np
import pytest

import mpt
from mpt import abi

from test_xform import IDENT, soup_scene

pytestmark = pytest.mark.gpu

F = np.float32
ARG, NOSCENE = abi.ERR_INVALID_ARGUMENT, abi.ERR_NO_SCENE
V0 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], F)
IDX = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
NV = len(V0)
NAN, INF, BIG = F(np.nan), F(np.inf), F(3e38)


_alive = []   # ctypes sees addresses only: whatever a call was handed stays until the module goes


def p(a):
    if a is None:
        return None
    _alive.append(a)
    return C.c_void_p(a.ctypes.data)


def arr(x, dt=F):
    return np.ascontiguousarray(x, dt)


def mats(k, *edits):
    """k identity 3x4 matrices; every edit is (matrix, row, column, value)."""
    m = np.tile(IDENT, (k, 1, 1)).astype(F)
    for i, r, c, v in edits:
        m[i, r, c] = v
    return m


# finite entries whose product is not: x' = 3e38 * x + 3e38 in every matrix (vertex 1 has x = 1)
def overflowing(k):
    return mats(k, *[(i, 0, c, BIG) for i in range(k) for c in (0, 3)])


def anim_tables(J=0, T=1, values=(0.5, 0.5)):
    """One TRS root; J joints on it; T targets whose weights one LINEAR sampler drives from
    values[0] at t = 0 to values[1] at t = 1."""
    t = {"node_parents": [-1], "node_trs": [0, 0, 0, 0, 0, 0, 1, 1, 1, 1], "node_is_trs": [1],
         "node_locals": np.eye(4)[:3].ravel()}
    if J:
        t["joint_nodes"], t["joint_bind"] = [0] * J, np.tile(np.eye(4)[:3].ravel(), J)
    if T:
        t["base_weights"] = [0.0] * T
        t["sampler_key_offsets"], t["sampler_value_offsets"] = [0, 2], [0, 2 * T]
        t["key_times"], t["values"] = [0.0, 1.0], np.repeat(arr(values), T)
        t["sampler_interp"] = [abi.ANIM_LINEAR]
        t["channel_sampler"], t["channel_node"], t["channel_path"] = [0], [0], [abi.ANIM_PATH_WEIGHTS]
        t["channel_first_target"], t["channel_num_targets"] = [0], [T]
    st, arrays = mpt._animation_struct(t, 0, "anim_tables")
    _alive.append(arrays)
    return st


# the morph: one target that moves vertex 0 by (2, 0, 0) and the unused vertex 3 by (0, 2, 0)
M_OFF, M_IDS, M_DP = arr([0, 2], np.int32), arr([0, 3], np.int32), arr([[2, 0, 0], [0, 2, 0]])
SKIN_J = arr(np.tile([0, 1, 0, 0], (NV, 1)), np.int32)
SKIN_W = arr(np.tile([0.5, 0.5, 0, 0], (NV, 1)))
OBJ_IDS = arr([0, 0, 1, -1], np.int32)

# the valid update that follows every row, per state
MOVE_OBJ = mats(2, (1, 0, 3, F(0.25)))
MOVE_SKIN = mats(2, (0, 1, 3, F(-0.5)))
MOVE_PLAIN = V0 + F(0.125)
MOVE_MORPH = arr([0.25])


class Ctx:
    def __init__(self, state, r):
        self.state, self.r, self.h, self.L = state, r, r.h, mpt.lib()
        self.want = None

    def vertices(self):
        v, n = np.empty((NV, 3), F), np.empty((NV, 3), F)
        assert self.L.mpt_get_vertices(self.h, p(v), p(n), NV) == 0, self.L.mpt_last_error()
        return v.tobytes() + n.tobytes()

    def valid_update(self):
        L, h = self.L, self.h
        if self.state == "objects":
            return L.mpt_update_transforms(h, p(MOVE_OBJ), 2, None)
        if self.state == "morph":
            return L.mpt_update_morph(h, p(MOVE_MORPH), 1, None)
        if self.state == "rig":   # the skin alone: the morph's retained weight composes with it
            return L.mpt_update_skin(h, p(MOVE_SKIN), 2, None)
        return L.mpt_update_vertices(h, p(MOVE_PLAIN), None, NV, None)


@pytest.fixture(scope="module")
def ctxs():
    L = mpt.lib()
    sd = soup_scene(V0.copy(), IDX)
    out = {}
    try:
        for state in ("empty", "plain", "objects", "morph", "rig"):
            r = mpt.GPURenderer(0)
            c = out[state] = Ctx(state, r)
            if state == "empty":
                continue
            r.set_scene(sd)
            if state == "objects":
                assert L.mpt_set_objects(r.h, p(OBJ_IDS), NV, 2) == 0
            if state in ("morph", "rig"):
                assert L.mpt_set_morph(r.h, 1, p(M_OFF), p(M_IDS), p(M_DP), None, NV) == 0
            if state == "rig":
                assert L.mpt_set_skin(r.h, p(SKIN_J), p(SKIN_W), NV, 2) == 0
                assert L.mpt_update_morph(r.h, p(arr([0.5])), 1, None) == 0
                assert L.mpt_set_animation(r.h, C.byref(anim_tables())) == 0, L.mpt_last_error()
            assert c.valid_update() == 0, L.mpt_last_error()
            c.want = c.vertices()
        out["empty"].want = out["plain"].want
        yield out
    finally:
        for c in out.values():
            c.r.close()


def device(x):
    import torch
    t = torch.tensor(np.asarray(x, F), device="cuda:0")
    torch.cuda.synchronize()
    return t


def dptr(t):
    _alive.append(t)
    return C.c_void_p(t.data_ptr())


# (id, state, call -> rc given (L, context handle), expected code, expected text).  A call that
# needs arrays builds them itself (p, dptr and anim_tables keep them alive).
NULLARG, COUNT, NONFINITE_V = "NULL argument", "vertex count differs from the scene's", "non-finite vertex coordinate"
V_NAN = V0.copy(); V_NAN[1, 2] = NAN
V_INF_UNUSED = V0.copy(); V_INF_UNUSED[3, 0] = INF
J_BAD = SKIN_J.copy(); J_BAD[2, 3] = 2
W_INF = SKIN_W.copy(); W_INF[1, 0] = INF
G_OK = arr([0, 0, 0, -1], np.int32)
ROWS = []


def row(name, state, call, code, text):
    ROWS.append(pytest.param(state, call, code, text, id=f"{name}-{state}"))


# --- the two refusals every call starts with
ENTRY = {
    "update_vertices": lambda L, h: L.mpt_update_vertices(h, p(V0), None, NV, None),
    "set_objects": lambda L, h: L.mpt_set_objects(h, p(OBJ_IDS), NV, 2),
    "update_transforms": lambda L, h: L.mpt_update_transforms(h, p(mats(2)), 2, None),
    "set_skin": lambda L, h: L.mpt_set_skin(h, p(SKIN_J), p(SKIN_W), NV, 2),
    "update_skin": lambda L, h: L.mpt_update_skin(h, p(mats(2)), 2, None),
    "set_morph": lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), p(M_IDS), p(M_DP), None, NV),
    "update_morph": lambda L, h: L.mpt_update_morph(h, p(arr([0.5])), 1, None),
    "update_morph_skin": lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5])), 1, p(mats(2)), 2, None),
    "set_normals": lambda L, h: L.mpt_set_normals(h, p(G_OK), None, NV, 1),
    "get_vertices": lambda L, h: L.mpt_get_vertices(h, p(np.empty((NV, 3), F)), None, NV),
    "set_animation": lambda L, h: L.mpt_set_animation(h, C.byref(anim_tables())),
    "update_animation": lambda L, h: L.mpt_update_animation(h, 0.0, None),
    "update_vertices_device": lambda L, h: L.mpt_update_vertices_device(h, dptr(device(V0)), None, NV, None),
}
for _name, _call in ENTRY.items():
    row(f"{_name}-null-context", "plain", (lambda call: lambda L, h: call(L, None))(_call), ARG, NULLARG)
    row(f"{_name}-no-scene", "empty", _call, NOSCENE, "no scene uploaded")

# --- mpt_update_vertices
row("update_vertices-null", "plain", lambda L, h: L.mpt_update_vertices(h, None, None, NV, None), ARG, NULLARG)
row("update_vertices-count", "plain", lambda L, h: L.mpt_update_vertices(h, p(V0), None, NV - 1, None), ARG, COUNT)
row("update_vertices-zero", "plain", lambda L, h: L.mpt_update_vertices(h, p(V0), None, 0, None), ARG, COUNT)
row("update_vertices-nan", "plain", lambda L, h: L.mpt_update_vertices(h, p(V_NAN), None, NV, None), ARG, NONFINITE_V)
row("update_vertices-inf-unused", "plain", lambda L, h: L.mpt_update_vertices(h, p(V_INF_UNUSED), None, NV, None), ARG, NONFINITE_V)
row("update_vertices-nan", "rig", lambda L, h: L.mpt_update_vertices(h, p(V_NAN), None, NV, None), ARG, NONFINITE_V)

# --- mpt_set_objects
row("set_objects-null-count", "objects", lambda L, h: L.mpt_set_objects(h, None, 0, 2), ARG, NULLARG)
row("set_objects-count", "objects", lambda L, h: L.mpt_set_objects(h, p(OBJ_IDS), NV + 1, 2), ARG, COUNT)
row("set_objects-no-objects", "objects", lambda L, h: L.mpt_set_objects(h, p(OBJ_IDS), NV, 0), ARG, "objects: bad object count")
row("set_objects-id-high", "objects", lambda L, h: L.mpt_set_objects(h, p(OBJ_IDS), NV, 1), ARG, "object id out of range")
row("set_objects-id-low", "plain", lambda L, h: L.mpt_set_objects(h, p(arr([0, -2, 0, 0], np.int32)), NV, 1), ARG, "object id out of range")

# --- mpt_update_transforms
row("update_transforms-null", "objects", lambda L, h: L.mpt_update_transforms(h, None, 2, None), ARG, NULLARG)
row("update_transforms-none-set", "plain", lambda L, h: L.mpt_update_transforms(h, p(mats(2)), 2, None), ARG, "no objects set")
row("update_transforms-none-set", "rig", lambda L, h: L.mpt_update_transforms(h, p(mats(2)), 2, None), ARG, "no objects set")
row("update_transforms-count", "objects", lambda L, h: L.mpt_update_transforms(h, p(mats(3)), 3, None), ARG, "object count differs from the table's")
row("update_transforms-nan", "objects", lambda L, h: L.mpt_update_transforms(h, p(mats(2, (1, 2, 1, NAN))), 2, None), ARG, "non-finite matrix entry")
row("update_transforms-inf", "objects", lambda L, h: L.mpt_update_transforms(h, p(mats(2, (0, 0, 3, INF))), 2, None), ARG, "non-finite matrix entry")
# (finite entries, an infinite product in vertex 1, found by the kernel's reduction)
row("update_transforms-overflow", "objects", lambda L, h: L.mpt_update_transforms(h, p(overflowing(2)), 2, None), ARG, NONFINITE_V)

# --- mpt_set_skin
row("set_skin-null-count", "rig", lambda L, h: L.mpt_set_skin(h, None, None, 0, 2), ARG, NULLARG)
row("set_skin-null-joints", "rig", lambda L, h: L.mpt_set_skin(h, None, p(SKIN_W), NV, 2), ARG, NULLARG)
row("set_skin-null-weights", "plain", lambda L, h: L.mpt_set_skin(h, p(SKIN_J), None, NV, 2), ARG, NULLARG)
row("set_skin-count", "rig", lambda L, h: L.mpt_set_skin(h, p(SKIN_J), p(SKIN_W), NV - 1, 2), ARG, COUNT)
row("set_skin-no-joints", "rig", lambda L, h: L.mpt_set_skin(h, p(SKIN_J), p(SKIN_W), NV, 0), ARG, "skin: bad joint count")
row("set_skin-joint-range", "rig", lambda L, h: L.mpt_set_skin(h, p(J_BAD), p(SKIN_W), NV, 2), ARG, "joint index out of range")
row("set_skin-weight-inf", "objects", lambda L, h: L.mpt_set_skin(h, p(SKIN_J), p(W_INF), NV, 2), ARG, "non-finite weight")

# --- mpt_update_skin
row("update_skin-null", "rig", lambda L, h: L.mpt_update_skin(h, None, 2, None), ARG, NULLARG)
row("update_skin-none-set", "plain", lambda L, h: L.mpt_update_skin(h, p(mats(2)), 2, None), ARG, "no skin set")
row("update_skin-none-set", "morph", lambda L, h: L.mpt_update_skin(h, p(mats(2)), 2, None), ARG, "no skin set")
row("update_skin-count", "rig", lambda L, h: L.mpt_update_skin(h, p(mats(1)), 1, None), ARG, "joint count differs from the table's")
row("update_skin-nan", "rig", lambda L, h: L.mpt_update_skin(h, p(mats(2, (0, 1, 1, NAN))), 2, None), ARG, "non-finite matrix entry")
row("update_skin-overflow", "rig", lambda L, h: L.mpt_update_skin(h, p(overflowing(2)), 2, None), ARG, NONFINITE_V)

# --- mpt_set_morph
row("set_morph-null-count", "morph", lambda L, h: L.mpt_set_morph(h, 1, None, None, None, None, 0), ARG, NULLARG)
row("set_morph-null-offsets", "morph", lambda L, h: L.mpt_set_morph(h, 1, None, p(M_IDS), p(M_DP), None, NV), ARG, NULLARG)
row("set_morph-null-ids", "morph", lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), None, p(M_DP), None, NV), ARG, NULLARG)
row("set_morph-count", "rig", lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), p(M_IDS), p(M_DP), None, NV + 3), ARG, COUNT)
row("set_morph-no-targets", "morph", lambda L, h: L.mpt_set_morph(h, 0, p(M_OFF), p(M_IDS), p(M_DP), None, NV), ARG, "morph: bad target count")
row("set_morph-offset-start", "morph", lambda L, h: L.mpt_set_morph(h, 1, p(arr([1, 2], np.int32)), p(M_IDS), p(M_DP), None, NV), ARG,
    "morph: target offsets do not start at 0")
row("set_morph-offsets-decrease", "morph", lambda L, h: L.mpt_set_morph(h, 2, p(arr([0, 2, 1], np.int32)), p(M_IDS), p(M_DP), None, NV), ARG,
    "morph: target offsets decrease")
row("set_morph-id-range", "rig", lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), p(arr([0, NV], np.int32)), p(M_DP), None, NV), ARG,
    "morph: vertex id out of range")
row("set_morph-ids-order", "plain", lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), p(arr([3, 3], np.int32)), p(M_DP), None, NV), ARG,
    "morph: vertex ids of a target not strictly ascending")
row("set_morph-delta-nan", "rig", lambda L, h: L.mpt_set_morph(h, 1, p(M_OFF), p(M_IDS), p(arr([[1, NAN, 0], [0, 2, 0]])), None, NV), ARG,
    "non-finite morph delta")

# --- mpt_update_morph
row("update_morph-null", "morph", lambda L, h: L.mpt_update_morph(h, None, 1, None), ARG, NULLARG)
row("update_morph-none-set", "plain", lambda L, h: L.mpt_update_morph(h, p(arr([0.5])), 1, None), ARG, "no morph set")
row("update_morph-none-set", "objects", lambda L, h: L.mpt_update_morph(h, p(arr([0.5])), 1, None), ARG, "no morph set")
row("update_morph-count", "morph", lambda L, h: L.mpt_update_morph(h, p(arr([0.5, 0.5])), 2, None), ARG, "target count differs from the tables'")
row("update_morph-inf", "morph", lambda L, h: L.mpt_update_morph(h, p(arr([INF])), 1, None), ARG, "non-finite morph weight")
row("update_morph-nan", "rig", lambda L, h: L.mpt_update_morph(h, p(arr([NAN])), 1, None), ARG, "non-finite morph weight")
# (a finite weight, an infinite vertex: 3e38 * 2)
row("update_morph-overflow", "morph", lambda L, h: L.mpt_update_morph(h, p(arr([BIG])), 1, None), ARG, NONFINITE_V)
row("update_morph-overflow", "rig", lambda L, h: L.mpt_update_morph(h, p(arr([BIG])), 1, None), ARG, NONFINITE_V)

# --- mpt_update_morph_skin
row("update_morph_skin-null-weights", "rig", lambda L, h: L.mpt_update_morph_skin(h, None, 1, p(mats(2)), 2, None), ARG, NULLARG)
row("update_morph_skin-null-matrices", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5])), 1, None, 2, None), ARG, NULLARG)
row("update_morph_skin-no-morph", "plain", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5])), 1, p(mats(2)), 2, None), ARG, "no morph set")
row("update_morph_skin-no-skin", "morph", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5])), 1, p(mats(2)), 2, None), ARG, "no skin set")
row("update_morph_skin-targets", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5, 0.5])), 2, p(mats(2)), 2, None), ARG,
    "target count differs from the tables'")
row("update_morph_skin-joints", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.5])), 1, p(mats(3)), 3, None), ARG,
    "joint count differs from the table's")
row("update_morph_skin-weight-inf", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([-INF])), 1, p(mats(2)), 2, None), ARG,
    "non-finite morph weight")
row("update_morph_skin-matrix-nan", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.9])), 1, p(mats(2, (1, 2, 3, NAN))), 2, None), ARG,
    "non-finite matrix entry")
# (new weights and a new palette staged, then refused: neither may be retained)
row("update_morph_skin-overflow", "rig", lambda L, h: L.mpt_update_morph_skin(h, p(arr([0.9])), 1, p(overflowing(2)), 2, None), ARG,
    NONFINITE_V)

# --- mpt_set_normals
row("set_normals-null-count", "plain", lambda L, h: L.mpt_set_normals(h, None, None, 0, 1), ARG, NULLARG)
row("set_normals-null-flips", "plain", lambda L, h: L.mpt_set_normals(h, None, p(arr([0], np.uint8)), 0, 0), ARG, NULLARG)
row("set_normals-count", "plain", lambda L, h: L.mpt_set_normals(h, p(G_OK), None, NV - 1, 1), ARG, COUNT)
row("set_normals-no-groups", "rig", lambda L, h: L.mpt_set_normals(h, p(G_OK), None, NV, 0), ARG, "normals: bad group count")
row("set_normals-group-range", "objects", lambda L, h: L.mpt_set_normals(h, p(arr([0, 1, 0, -1], np.int32)), None, NV, 1), ARG,
    "normals: group id out of range")

# --- mpt_get_vertices
row("get_vertices-count", "plain", lambda L, h: L.mpt_get_vertices(h, p(np.empty((NV, 3), F)), None, NV + 1), ARG, COUNT)
row("get_vertices-zero", "rig", lambda L, h: L.mpt_get_vertices(h, p(np.empty((NV, 3), F)), None, 0), ARG, COUNT)


# --- mpt_set_animation
def set_anim(**kw):
    def call(L, h):
        st = anim_tables(**kw)
        return L.mpt_set_animation(h, C.byref(st))
    return call


def set_anim_edit(field, value):
    def call(L, h):
        st = anim_tables()
        setattr(st, field, value)
        return L.mpt_set_animation(h, C.byref(st))
    return call


row("set_animation-packing", "rig", set_anim(J=0, T=0), ARG, "animation: neither joints nor targets")
row("set_animation-null-table", "rig", set_anim_edit("node_parents", None), ARG, NULLARG)
row("set_animation-bad-count", "rig", set_anim_edit("num_nodes", 0), ARG, "animation: bad count")
row("set_animation-value-nan", "rig", set_anim(values=(0.5, NAN)), ARG, "animation: non-finite value")
row("set_animation-joints-no-skin", "morph", set_anim(J=2, T=1), ARG, "animation: joints without a skin set")
row("set_animation-joint-count", "rig", set_anim(J=3, T=1), ARG, "animation: joint count differs from the skin's")
row("set_animation-targets-no-morph", "plain", set_anim(J=0, T=1), ARG, "animation: targets without a morph set")
row("set_animation-targets-no-morph", "objects", set_anim(J=0, T=1), ARG, "animation: targets without a morph set")
row("set_animation-target-count", "rig", set_anim(J=0, T=2), ARG, "animation: target count differs from the morph's")

# --- mpt_update_animation
row("update_animation-none-set", "plain", lambda L, h: L.mpt_update_animation(h, 0.0, None), ARG, "no animation set")
row("update_animation-none-set", "morph", lambda L, h: L.mpt_update_animation(h, 0.0, None), ARG, "no animation set")
row("update_animation-nan", "rig", lambda L, h: L.mpt_update_animation(h, float("nan"), None), ARG, "animation: time not finite")
row("update_animation-inf", "rig", lambda L, h: L.mpt_update_animation(h, float("-inf"), None), ARG, "animation: time not finite")


# (a clip whose weight reaches 3e38 at t = 1: finite tables, an infinite vertex, found on the device
# after k_anim has staged the weight -- the retained one must stay)
def anim_overflow(L, h):
    st = anim_tables(values=(0.5, BIG))
    rc = L.mpt_set_animation(h, C.byref(st))
    assert rc == 0, L.mpt_last_error()
    return L.mpt_update_animation(h, 1.0, None)


row("update_animation-overflow", "rig", anim_overflow, ARG, "non-finite animation value or vertex coordinate")


# --- mpt_update_vertices_device
def dev_call(v, n=None, count=NV, host=False):
    def call(L, h):
        if host:   # host memory where device memory is asked for: refused before any kernel sees it
            return L.mpt_update_vertices_device(h, p(v), None, count, None)
        tv, tn = device(v), None if n is None else device(n)
        return L.mpt_update_vertices_device(h, dptr(tv), None if tn is None else dptr(tn), count, None)
    return call


row("update_vertices_device-null", "plain", lambda L, h: L.mpt_update_vertices_device(h, None, None, NV, None), ARG, NULLARG)
row("update_vertices_device-count", "plain", dev_call(V0, count=NV - 1), ARG, COUNT)
row("update_vertices_device-host-pointer", "plain", dev_call(V0, host=True), ARG, "not memory of the context's device")


def dev_host_normals(L, h):
    tv = device(V0)
    return L.mpt_update_vertices_device(h, dptr(tv), p(V0), NV, None)


row("update_vertices_device-host-normals", "objects", dev_host_normals, ARG, "not memory of the context's device")
row("update_vertices_device-nan", "plain", dev_call(V_NAN), ARG, NONFINITE_V)
row("update_vertices_device-nan", "rig", dev_call(V_NAN, n=V0), ARG, NONFINITE_V)


def test_the_table_names_every_entry_point_and_text():
    texts = {q.values[3] for q in ROWS}
    assert {
        NULLARG, "no scene uploaded", COUNT, NONFINITE_V, "objects: bad object count", "object id out of range", "no objects set",
        "object count differs from the table's", "non-finite matrix entry", "skin: bad joint count", "no skin set",
        "joint count differs from the table's", "no morph set", "target count differs from the tables'", "non-finite morph weight",
        "animation: joints without a skin set", "animation: joint count differs from the skin's",
        "animation: targets without a morph set", "animation: target count differs from the morph's", "no animation set",
        "animation: time not finite", "non-finite animation value or vertex coordinate", "not memory of the context's device",
    } <= texts
    assert len({q.id for q in ROWS}) == len(ROWS)


@pytest.mark.parametrize("state, call, code, text", ROWS)
def test_refusal(ctxs, state, call, code, text):
    c = ctxs[state]
    seen = ctxs["plain"] if state == "empty" else c   # (a context without a scene has no vertices to compare)
    L = c.L
    before = seen.vertices()
    rc = call(L, c.h)
    msg = L.mpt_last_error().decode()
    assert (rc, msg) == (code, text)
    assert seen.vertices() == before, "the refused call changed the vertices"
    assert seen.valid_update() == 0, L.mpt_last_error().decode()
    assert seen.vertices() == seen.want, "the update after the refusal gives other bytes than before it"
