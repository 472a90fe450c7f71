"""The PLOC build mode on the host (mpt_bvh_build_host_mode: the host loop of csrc/ploc.h -- the
definition the kernels of mpt_rebuild_bvh_mode share -- between the keys and the collapse of
csrc/lbvh.h), no GPU.

Mode 0 through the new entry point is mpt_bvh_build_host byte for byte.  Mode 1 passes the layout
and refit checks of tests/test_build_host.py on every input there and on chain40 (the slow-merge
case: every triangle 1.5 times the size of the one before).  An independent numpy restatement of
the definition, written per list (every position's keys at once) where the library works per
position, and with subtrees as leaf lists where the library assigns ranges, reproduces topology
and record order exactly.  The quality proxy -- the sum over nodes of the fp32 area of the exact
node box, over the root's -- is strictly lower in mode 1 than in mode 0 on cornell, on the city
and on the city with a part moved.
"""
import numpy as np
import pytest

import mpt
from mpt import abi

from test_build_host import INPUTS, _city, check_layout
from test_refit_host import box_pad, check_refit, exact_boxes

R = 8   # csrc/ploc.h PLOC_RADIUS


def chain(n=40):
    """n triangles, each 1.5 times the one before: merges run one after another."""
    x = (np.float32(1.5) ** np.arange(n, dtype=np.float32)).astype(np.float32)
    z = np.zeros(n, np.float32)
    a = np.stack([x, z, z], 1)
    b = np.stack([np.float32(1.01) * x, np.float32(0.01) * x, z], 1)
    c = np.stack([x, z, np.float32(0.01) * x], 1)
    v = np.stack([a, b, c], 1).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


PLOC_INPUTS = dict(INPUTS)
PLOC_INPUTS["chain40"] = lambda: chain(40) + (None,)
PLOC_INPUTS["city_move"] = lambda: _city("move") + (None,)
_built = {}


def built(name, mode):
    if (name, mode) not in _built:
        v, idx, prims = PLOC_INPUTS[name]()
        _built[(name, mode)] = (v, idx, prims) + mpt.bvh_build_host(v, idx, prims, mode=mode)
    return _built[(name, mode)]


@pytest.mark.parametrize("name", list(INPUTS))
def test_mode0_is_build_host(name):
    v, idx, prims, nodes, tris, levels = built(name, abi.BUILD_LBVH)
    L = mpt.lib()
    counts = np.zeros(3, np.int32)
    p = None if prims is None else prims.ctypes.data
    hn, ht = np.zeros(len(nodes), abi.NODE8_DTYPE), np.zeros(len(tris), abi.TRIREC_DTYPE)
    assert L.mpt_bvh_build_host(v.ctypes.data, len(v), idx.ctypes.data, len(idx), p, 0 if prims is None else len(prims),
                                hn.ctypes.data, hn.nbytes, ht.ctypes.data, ht.nbytes, counts.ctypes.data) == 0
    assert counts.tolist() == [len(nodes), len(tris), levels]
    assert hn.tobytes() == nodes.tobytes() and ht.tobytes() == tris.tobytes()


@pytest.mark.parametrize("name", list(INPUTS) + ["chain40"])
def test_ploc_build_host(name):
    v, idx, prims, nodes, tris, levels = built(name, abi.BUILD_PLOC)
    lst = np.arange(len(idx)) if prims is None else prims
    check_layout(nodes, tris, levels, lst, name)
    assert np.array_equal(np.sort(tris["prim"]), np.sort(lst))
    assert 2 * levels + 2 <= 64
    with np.errstate(over="ignore", invalid="ignore"):
        check_refit(nodes, tris, nodes, tris, v, idx, name)
    if name in ("tiny1", "tiny3"):
        b = built(name, abi.BUILD_LBVH)
        assert nodes.tobytes() == b[3].tobytes() and tris.tobytes() == b[4].tobytes()


# ------------------------------------------------------------------------------------
# The definition again, in numpy, per list
# ------------------------------------------------------------------------------------
def area32(lo, hi):
    f32 = np.float32
    d = np.maximum(f32(0), hi - lo)
    return f32(2) * ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0])


def restate_ploc(v, idx, prims=None):
    """(imask, meta, child_base, tri_base) per node in breadth-first order, the records' prims and
    the number of iterations."""
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
    order = np.argsort((code << 32) | np.arange(M, dtype=np.int64), kind="stable")

    # clusters: a subtree is a leaf (its sorted position) or a pair of subtrees
    trees = [int(p) for p in range(M)]
    clo, chi = lo[order].copy(), hi[order].copy()
    iterations = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while len(trees) > 1:
            m = len(trees)
            i = np.arange(m)
            keys = np.full((m, 2 * R + 1), np.iinfo(np.uint64).max, np.uint64)
            for o in range(-R, R + 1):
                j = i + o
                ok = (j >= 0) & (j < m) & (o != 0)
                jj = np.clip(j, 0, m - 1)
                d = area32(np.minimum(clo, clo[jj]), np.maximum(chi, chi[jj])).astype(f32)
                d = np.where(np.isnan(d), f32(np.inf), d) + f32(0)
                k = (d.astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (i ^ jj).astype(np.uint64)
                keys[:, o + R] = np.where(ok, k, keys[:, o + R])
            nn = i + np.argmin(keys, 1) - R
            two = np.sort(keys, 1)[:, :2]
            assert (two[:, 0] != two[:, 1]).all()                 # the key is unique over j
            head = (nn[nn] == i) & (i < nn)
            gone = (nn[nn] == i) & (i > nn)
            assert head.any()
            nt, nlo, nhi = [], [], []
            for a in range(m):
                if gone[a]:
                    continue
                if head[a]:
                    b = int(nn[a])
                    nt.append((trees[a], trees[b]))
                    nlo.append(np.minimum(clo[a], clo[b]))
                    nhi.append(np.maximum(chi[a], chi[b]))
                else:
                    nt.append(trees[a])
                    nlo.append(clo[a])
                    nhi.append(chi[a])
            trees, clo, chi = nt, np.array(nlo, f32), np.array(nhi, f32)
            iterations += 1

    # every subtree as its leaves from left to right; the new order is the root's
    info = {}

    def describe(t):
        """(leaves, lo, hi) of a subtree, memoised by identity."""
        stack = [(t, False)]
        while stack:
            x, done = stack.pop()
            if id(x) in info and not isinstance(x, int):
                continue
            if isinstance(x, int):
                continue
            if not done:
                stack.append((x, True))
                stack.extend((ch, False) for ch in x)
            else:
                parts = [get(ch) for ch in x]
                info[id(x)] = (parts[0][0] + parts[1][0], np.minimum(parts[0][1], parts[1][1]), np.maximum(parts[0][2], parts[1][2]))
        return get(t)

    slo, shi = lo[order], hi[order]

    def get(t):
        return ([t], slo[t], shi[t]) if isinstance(t, int) else info[id(t)]

    root = trees[0]
    describe(root)
    size = lambda t: len(get(t)[0])
    out_nodes, out_prims = [], []
    level, n_alloc = [root], 1
    with np.errstate(over="ignore", invalid="ignore"):
        while level:
            nxt = []
            for nd in level:
                if size(nd) <= 3:
                    ch = [nd]
                else:
                    ch = list(nd)
                    while len(ch) < 8:
                        best, ba = -1, None
                        for k, x in enumerate(ch):
                            if size(x) <= 3:
                                continue
                            a = area32(get(x)[1], get(x)[2])
                            if best < 0 or a > ba:
                                best, ba = k, a
                        if best < 0:
                            break
                        l_, r_ = ch[best]
                        ch[best] = l_
                        ch.append(r_)
                boxes = [(get(x)[1], get(x)[2]) for x in ch]
                nlo, nhi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
                pc = 0.5 * nlo.astype(f64) + 0.5 * nhi.astype(f64)
                vv = [0.5 * b[0].astype(f64) + 0.5 * b[1].astype(f64) - pc for b in boxes]
                in_slot, used = [-1] * 8, [False] * len(ch)
                for _ in ch:
                    best, bi, bs = None, -1, -1
                    for k in range(len(ch)):
                        if used[k]:
                            continue
                        for s in range(8):
                            if in_slot[s] >= 0:
                                continue
                            x = vv[k][0] if s & 1 else -vv[k][0]
                            y = vv[k][1] if s & 2 else -vv[k][1]
                            z = vv[k][2] if s & 4 else -vv[k][2]
                            cost = -((x + y) + z)
                            if bi < 0 or cost < best:
                                best, bi, bs = cost, k, s
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
                        out_prims.extend(P[order[get(x)[0]]].tolist())
                out_nodes.append((imask, meta, child_base, tri_base))
            level = nxt
    return out_nodes, out_prims, iterations


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "tiny4", "tiny9", "tiny25", "tiny257", "copies1000", "cornell",
                                  "cornell_emissive", "tiny9_1e37", "chain40"])
def test_ploc_numpy_restatement(name):
    v, idx, prims, nodes, tris, levels = built(name, abi.BUILD_PLOC)
    ref_nodes, ref_prims, iterations = restate_ploc(v, idx, prims)
    assert len(ref_nodes) == len(nodes), name
    assert tris["prim"].tolist() == ref_prims, f"{name}: record order"
    assert nodes["imask"].tolist() == [n[0] for n in ref_nodes], f"{name}: imask"
    assert nodes["meta"].tolist() == [n[1] for n in ref_nodes], f"{name}: meta"
    assert nodes["child_base"].tolist() == [n[2] for n in ref_nodes], f"{name}: child_base"
    assert nodes["tri_base"].tolist() == [n[3] for n in ref_nodes], f"{name}: tri_base"
    if name == "copies1000":
        assert iterations == 10          # equal boxes pair up as (2 k, 2 k + 1): they halve, not chain
    if name == "chain40":
        assert iterations > 20           # one merge after another


# ------------------------------------------------------------------------------------
# Quality
# ------------------------------------------------------------------------------------
def area_sum(nodes, tris, v, idx):
    """The sum over nodes of the fp32 area of the exact node box, over the root's."""
    _, _, _, _, nlo, nhi = exact_boxes(nodes, tris, v, idx)
    a = area32(nlo, nhi).astype(np.float64)
    return float(a.sum() / a[0])


@pytest.mark.parametrize("name", ["cornell", "city", "city_move"])
def test_ploc_lowers_the_area_sum(name):
    sums = {}
    for mode in (abi.BUILD_LBVH, abi.BUILD_PLOC):
        v, idx, prims, nodes, tris, levels = built(name, mode)
        sums[mode] = area_sum(nodes, tris, v, idx)
    print(f"{name}: area sum LBVH {sums[0]:.3f} PLOC {sums[1]:.3f}")
    assert sums[abi.BUILD_PLOC] < sums[abi.BUILD_LBVH], f"{name}: {sums}"


# ------------------------------------------------------------------------------------
# Errors
# ------------------------------------------------------------------------------------
def test_unknown_mode():
    from test_refit_host import tiny
    v, idx = tiny(9)
    for mode in (2, -1, 255):
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(v, idx, mode=mode)
        assert e.value.code == -1


@pytest.mark.parametrize("mode", [abi.BUILD_LBVH, abi.BUILD_PLOC])
def test_build_host_mode_errors(mode):
    from test_refit_host import tiny
    v, idx = tiny(3)
    L = mpt.lib()
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[4, 1] = bad
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(w, idx, mode=mode)
        assert e.value.code == -1
    with pytest.raises(mpt.MptError) as e:
        mpt.bvh_build_host(v, idx + 7, mode=mode)                # an index past the vertices
    assert e.value.code == -1
    for prims in ([3], [-1], [0, 1, 5]):
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(v, idx, np.array(prims, np.int32), mode=mode)
        assert e.value.code == -1
    counts = np.zeros(3, np.int32)
    f = L.mpt_bvh_build_host_mode
    args = (v.ctypes.data, len(v), idx.ctypes.data, len(idx))
    assert f(None, len(v), idx.ctypes.data, len(idx), None, 0, mode, None, 0, None, 0, counts.ctypes.data) == -1
    assert f(v.ctypes.data, len(v), None, len(idx), None, 0, mode, None, 0, None, 0, counts.ctypes.data) == -1
    one = np.zeros(1, np.int32)
    assert f(*args, one.ctypes.data, 0, mode, None, 0, None, 0, counts.ctypes.data) == -1   # an empty list
    assert f(*args, None, 0, mode, None, 0, None, 0, counts.ctypes.data) == 0               # counts only
    assert counts.tolist() == [1, 3, 1]
    assert f(*args, one.ctypes.data, 1, mode, None, 0, None, 0, counts.ctypes.data) == 0
    assert counts.tolist() == [1, 1, 1]
    small = np.zeros(10, np.uint8)
    assert f(*args, None, 0, mode, small.ctypes.data, 10, small.ctypes.data, 10, None) == -1
