"""The BVH8 rebuild on the host (mpt_bvh_build_host: the host loop of csrc/lbvh.h -- the definition
the kernels of mpt_rebuild_bvh share -- then the host loop of csrc/refit.h), no GPU.

For every input below: each list primitive sits in exactly one record; the layout is what the
traversal and the refit expect (breadth-first nodes, contiguous internal children in slot order,
contiguous records in slot order, 1 to 3 triangles per leaf slot); the bytes that follow from the
positions pass the refit's own checks (test_refit_host.check_refit: containment, tightness, the
smallest exponents, fp32 records).  An independent numpy restatement of the definition (keys,
order, split rule, collapse, slot choice), written top down where the library works per node,
reproduces the topology and the record order exactly.

That a refit of the result to the same vertices reproduces it byte for byte needs a refit of a
given topology, which only a context offers: tests/test_rebuild.py checks it there, through the
kernels and through the library's host loop.
"""
import numpy as np
import pytest

import mpt

from test_refit_host import EDITS, box_pad, check_refit, cornell_scene, level_ranges, slot_kinds, small_city, tiny

SORT_TILE = 2048   # csrc/lbvh.h: keys per workgroup of a radix-sort pass


def copies(n=1000):
    """n copies of one triangle: equal codes (ties go by index), a zero extent on every axis."""
    v = np.tile(np.array([[0.25, 0.5, -1.0], [1.25, 0.5, -1.0], [0.25, 1.5, -0.5]], np.float32), (n, 1))
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def _cornell():
    return cornell_scene().vertices.astype(np.float32), cornell_scene().triangle_indices.reshape(-1, 3)


def _city(edit=None):
    v, idx = small_city().vertices.astype(np.float32), small_city().triangle_indices.reshape(-1, 3)
    return (EDITS[edit](v, idx) if edit else v), idx


def _huge():
    v, idx = tiny(9)
    return (v * np.float32(1e37)).astype(np.float32), idx


INPUTS = {f"tiny{n}": (lambda n=n: tiny(n) + (None,)) for n in (1, 3, 4, 9, 25, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1)}
INPUTS.update({
    "copies1000": lambda: copies() + (None,),
    "cornell": lambda: _cornell() + (None,),
    "city": lambda: _city() + (None,),
    "city_plane": lambda: _city("plane") + (None,),
    "city_scale_up": lambda: _city("scale_up") + (None,),
    "tiny9_1e37": lambda: _huge() + (None,),
    "cornell_emissive": lambda: _cornell() + (np.asarray(cornell_scene().emissive, np.int32),),
})
_built = {}


def built(name):
    if name not in _built:
        v, idx, prims = INPUTS[name]()
        _built[name] = (v, idx, prims) + mpt.bvh_build_host(v, idx, prims)
    return _built[name]


def check_layout(nodes, tris, levels, prims_list, what):
    """The Layout bullet of the definition; returns the level ranges."""
    assert sorted(tris["prim"].tolist()) == sorted(np.asarray(prims_list).tolist()), f"{what}: records are not the list, once each"
    lr = level_ranges(nodes)
    assert levels == len(lr), what
    assert 2 * levels + 2 <= 64, what
    internal, leaf = slot_kinds(nodes)
    meta = nodes["meta"].astype(np.int64)
    n_int = internal.sum(1)
    cnt, off = meta >> 5, meta & 31
    n_rec = np.where(leaf, cnt, 0).sum(1)
    # ranks: 0, 1, 2 ... over the internal slots in slot order
    rank = np.cumsum(internal, 1) - 1
    assert np.array_equal(meta[internal], rank[internal]), f"{what}: ranks"
    # leaf slots: 1 to 3 triangles, offsets running in slot order from 0
    assert ((cnt[leaf] >= 1) & (cnt[leaf] <= 3)).all(), f"{what}: leaf counts"
    run = np.cumsum(np.where(leaf, cnt, 0), 1) - np.where(leaf, cnt, 0)
    assert np.array_equal(off[leaf], run[leaf]), f"{what}: offsets"
    # breadth first: children and records contiguous in node order
    assert np.array_equal(nodes["child_base"], 1 + np.cumsum(n_int) - n_int), f"{what}: child_base"
    assert np.array_equal(nodes["tri_base"], np.cumsum(n_rec) - n_rec), f"{what}: tri_base"
    assert n_rec.sum() == len(tris) and 1 + n_int.sum() == len(nodes), what
    # an inner node is full or has no internal child; only a root may hold fewer than 4 triangles
    assert ((n_int == 0) | ((internal | leaf).sum(1) == 8)).all(), f"{what}: a node stopped opening early"
    assert not (tris["alpha_flag"].any() or tris["mat_class"].any()), f"{what}: flag lanes"
    return lr


@pytest.mark.parametrize("name", list(INPUTS))
def test_build_host(name):
    v, idx, prims, nodes, tris, levels = built(name)
    lst = np.arange(len(idx)) if prims is None else prims
    check_layout(nodes, tris, levels, lst, name)
    with np.errstate(over="ignore", invalid="ignore"):
        check_refit(nodes, tris, nodes, tris, v, idx, name)
    if name in ("tiny1", "tiny3"):
        assert len(nodes) == 1 and nodes["imask"][0] == 0 and nodes["meta"][0].tolist() == [(len(idx) << 5)] + [0] * 7
    if name == "tiny4":
        assert len(nodes) == 1 and (nodes["meta"][0] != 0).sum() >= 2
    if name == "city_plane":
        assert (nodes["e"][:, 1] == nodes["e"][0, 1]).all()      # one degenerate axis: only the pad is left


# ------------------------------------------------------------------------------------
# The definition again, in numpy, top down
# ------------------------------------------------------------------------------------
def restate(v, idx, prims=None):
    """(imask, meta, child_base, tri_base) per node in breadth-first order and the records' prims."""
    f32, f64 = np.float32, np.float64
    P = np.arange(len(idx)) if prims is None else np.asarray(prims)
    M = len(P)
    pad = box_pad(v, idx)
    tri = v[idx[P]]
    lo, hi = (tri.min(1) - pad).astype(f32), (tri.max(1) + pad).astype(f32)
    c = 0.5 * lo.astype(f64) + 0.5 * hi.astype(f64)
    cmin, cmax = c.min(0), c.max(0)
    q = np.zeros((M, 3), np.int64)
    for a in range(3):
        if cmax[a] - cmin[a] > 0:
            q[:, a] = np.clip(np.floor((c[:, a] - cmin[a]) / (cmax[a] - cmin[a]) * 1024.0), 0, 1023).astype(np.int64)
    code = np.zeros(M, np.int64)
    for bit in range(10):
        for a in range(3):
            code |= ((q[:, a] >> bit) & 1) << (3 * bit + 2 - a)
    key = (code << 32) | np.arange(M, dtype=np.int64)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    slo, shi = lo[order], hi[order]

    # binary tree: node = (l, r, left, right) over sorted positions, split at the highest differing bit
    tree = {}

    def box(l, r):
        return slo[l:r + 1].min(0), shi[l:r + 1].max(0)

    def area(l, r):
        blo, bhi = box(l, r)
        d = np.maximum(f32(0), bhi - blo)
        return f32(2) * ((d[0] * d[1] + d[1] * d[2]) + d[2] * d[0])

    def children(l, r):
        if (l, r) not in tree:
            hb = int(sk[l] ^ sk[r]).bit_length() - 1
            first_one = ((int(sk[l]) >> hb) | 1) << hb
            s = l + int(np.searchsorted(sk[l:r + 1], first_one))      # the first key with that bit set
            tree[(l, r)] = ((l, s - 1), (s, r))
        return tree[(l, r)]

    size = lambda n: n[1] - n[0] + 1
    out_nodes, out_prims = [], []
    level = [(0, M - 1)]
    n_alloc = 1
    with np.errstate(over="ignore", invalid="ignore"):
        while level:
            nxt = []
            for nd in level:
                if size(nd) <= 3:
                    ch = [nd]
                else:
                    ch = list(children(*nd))
                    while len(ch) < 8:
                        best, ba = -1, None
                        for i, x in enumerate(ch):
                            if size(x) <= 3:
                                continue
                            a = area(*x)
                            if best < 0 or a > ba:
                                best, ba = i, a
                        if best < 0:
                            break
                        l_, r_ = children(*ch[best])
                        ch[best] = l_
                        ch.append(r_)
                boxes = [box(*x) for x in ch]
                nlo, nhi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
                pc = 0.5 * nlo.astype(f64) + 0.5 * nhi.astype(f64)
                vv = [0.5 * b[0].astype(f64) + 0.5 * b[1].astype(f64) - pc for b in boxes]
                in_slot, used = [-1] * 8, [False] * len(ch)
                for _ in ch:
                    best, bi, bs = None, -1, -1
                    for i in range(len(ch)):
                        if used[i]:
                            continue
                        for s in range(8):
                            if in_slot[s] >= 0:
                                continue
                            x = vv[i][0] if s & 1 else -vv[i][0]
                            y = vv[i][1] if s & 2 else -vv[i][1]
                            z = vv[i][2] if s & 4 else -vv[i][2]
                            cost = -((x + y) + z)
                            if bi < 0 or cost < best:
                                best, bi, bs = cost, i, s
                    used[bi] = True
                    in_slot[bs] = bi
                imask, meta, rank, off = 0, [0] * 8, 0, 0
                child_base, tri_base = n_alloc, len(out_prims)
                for s in range(8):
                    if in_slot[s] < 0:
                        continue
                    x = ch[in_slot[s]]
                    if size(x) > 3:
                        imask |= 1 << s
                        meta[s] = rank
                        rank += 1
                        nxt.append(x)
                        n_alloc += 1
                    else:
                        meta[s] = (size(x) << 5) | off
                        off += size(x)
                        out_prims.extend(P[order[x[0]:x[1] + 1]].tolist())
                out_nodes.append((imask, meta, child_base, tri_base))
            level = nxt
    return out_nodes, out_prims


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "tiny4", "tiny9", "tiny25", "tiny257", "copies1000", "cornell",
                                  "cornell_emissive", "tiny9_1e37"])
def test_numpy_restatement(name):
    v, idx, prims, nodes, tris, levels = built(name)
    ref_nodes, ref_prims = restate(v, idx, prims)
    assert len(ref_nodes) == len(nodes), name
    assert tris["prim"].tolist() == ref_prims, f"{name}: record order"
    assert nodes["imask"].tolist() == [n[0] for n in ref_nodes], f"{name}: imask"
    assert nodes["meta"].tolist() == [n[1] for n in ref_nodes], f"{name}: meta"
    assert nodes["child_base"].tolist() == [n[2] for n in ref_nodes], f"{name}: child_base"
    assert nodes["tri_base"].tolist() == [n[3] for n in ref_nodes], f"{name}: tri_base"


def test_copies_order_by_index():
    v, idx, prims, nodes, tris, levels = built("copies1000")
    # equal codes: the radix tree splits on the bits of the list position, and every leaf slot's
    # triangles ascend
    internal, leaf = slot_kinds(nodes)
    first = (nodes["tri_base"][:, None] + (nodes["meta"] & 31))[leaf]
    cnt = (nodes["meta"] >> 5)[leaf]
    for f, c in zip(first.tolist(), cnt.tolist()):
        p = tris["prim"][f:f + c]
        assert (np.diff(p) == 1).all()


def test_build_host_errors():
    v, idx = tiny(3)
    L = mpt.lib()
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[4, 1] = bad
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(w, idx)
        assert e.value.code == -1
    with pytest.raises(mpt.MptError) as e:
        mpt.bvh_build_host(v, idx + 7)                         # an index past the vertices
    assert e.value.code == -1
    for prims in ([3], [-1], [0, 1, 5]):
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(v, idx, np.array(prims, np.int32))
        assert e.value.code == -1
    counts = np.zeros(3, np.int32)
    args = (v.ctypes.data, len(v), idx.ctypes.data, len(idx))
    assert L.mpt_bvh_build_host(None, len(v), idx.ctypes.data, len(idx), None, 0, None, 0, None, 0, counts.ctypes.data) == -1
    assert L.mpt_bvh_build_host(v.ctypes.data, len(v), None, len(idx), None, 0, None, 0, None, 0, counts.ctypes.data) == -1
    one = np.zeros(1, np.int32)
    assert L.mpt_bvh_build_host(*args, one.ctypes.data, 0, None, 0, None, 0, counts.ctypes.data) == -1   # an empty list
    assert L.mpt_bvh_build_host(*args, None, 0, None, 0, None, 0, counts.ctypes.data) == 0               # counts only
    assert counts.tolist() == [1, 3, 1]
    assert L.mpt_bvh_build_host(*args, one.ctypes.data, 1, None, 0, None, 0, counts.ctypes.data) == 0
    assert counts.tolist() == [1, 1, 1]
    small = np.zeros(10, np.uint8)
    assert L.mpt_bvh_build_host(*args, None, 0, small.ctypes.data, 10, small.ctypes.data, 10, None) == -1
