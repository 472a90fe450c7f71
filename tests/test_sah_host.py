"""The binned-SAH build mode on the host (mpt_bvh_build_host_mode, mode 3: the host loop of
csrc/sah.h -- the definition the kernels of mpt_rebuild_bvh_mode share -- between the keys and the
collapse of csrc/lbvh.h), no GPU.

Mode 3 passes the layout and refit checks of tests/test_build_host.py on every input there and on
chain40; tiny1 and tiny3 equal mode 0 byte for byte; modes 0 and 1 through the entry point are what
they were.  An independent numpy restatement of the definition, written per level over all the
level's nodes at once (reduceat / bincount / accumulate over the bins) where the library loops per
node and per member, reproduces topology and record order exactly, also with MPT_SAH_DEPTH=2, where
the tree differs from the default's.  Mode 2 stays refused.

Quality (test_ploc_host.area_sum, lower is better; the reference is the host builder's own tree,
mpt.bvh_refit_host, over the same vertices).  Measured:
                 LBVH    PLOC    mode 3   host builder
    cornell      3.511   1.894   2.034    2.034
    city         8.261   7.116   6.977    6.978
    city_move    6.651   5.332   4.828    4.824
Mode 3 is asserted strictly lower than PLOC on the city and on the city with a part moved.  Cornell
is left out of that assertion because the reference itself fails it there: the host builder's own
binned-SAH tree (2.034, the figure mode 3 reproduces to every printed digit) is above PLOC's 1.894
on those 36 triangles; its sums are still printed.  Mode 3 over the host builder's tree is 1.0000,
0.9999 and 1.0008 on the three inputs; no bound is asserted on that ratio.
"""
import numpy as np
import pytest

import mpt
from mpt import abi

from test_build_host import INPUTS, check_layout
from test_ploc_host import PLOC_INPUTS, area32, area_sum
from test_ploc_host import built as built_mode
from test_refit_host import box_pad, check_refit, tiny

SAH = abi.BUILD_SAH
BINS = 32   # csrc/sah.h SAH_BINS


def test_mode_value():
    assert abi.BUILD_SAH == 3 and abi.BUILD_PLOC == 1 and abi.BUILD_LBVH == 0


@pytest.mark.parametrize("name", list(INPUTS) + ["chain40"])
def test_sah_build_host(name):
    v, idx, prims, nodes, tris, levels = built_mode(name, SAH)
    lst = np.arange(len(idx)) if prims is None else prims
    check_layout(nodes, tris, levels, lst, name)
    assert np.array_equal(np.sort(tris["prim"]), np.sort(lst))
    assert 2 * levels + 2 <= 64
    with np.errstate(over="ignore", invalid="ignore"):
        check_refit(nodes, tris, nodes, tris, v, idx, name)
    if name in ("tiny1", "tiny3"):
        b = built_mode(name, abi.BUILD_LBVH)
        assert nodes.tobytes() == b[3].tobytes() and tris.tobytes() == b[4].tobytes()


@pytest.mark.parametrize("name", ["tiny9", "tiny257", "cornell", "cornell_emissive"])
def test_old_modes_untouched(name):
    """Mode 0 through the entry point is mpt_bvh_build_host; mode 1 differs from mode 3 and passes
    its own restatement in tests/test_ploc_host.py."""
    v, idx, prims, nodes, tris, levels = built_mode(name, abi.BUILD_LBVH)
    L = mpt.lib()
    counts = np.zeros(3, np.int32)
    p = None if prims is None else prims.ctypes.data
    hn, ht = np.zeros(len(nodes), abi.NODE8_DTYPE), np.zeros(len(tris), abi.TRIREC_DTYPE)
    assert L.mpt_bvh_build_host(v.ctypes.data, len(v), idx.ctypes.data, len(idx), p, 0 if prims is None else len(prims),
                                hn.ctypes.data, hn.nbytes, ht.ctypes.data, ht.nbytes, counts.ctypes.data) == 0
    assert counts.tolist() == [len(nodes), len(tris), levels]
    assert hn.tobytes() == nodes.tobytes() and ht.tobytes() == tris.tobytes()
    if name == "cornell":
        assert built_mode(name, abi.BUILD_PLOC)[3].tobytes() != built_mode(name, SAH)[3].tobytes()


# ------------------------------------------------------------------------------------
# The definition again, in numpy, per level
# ------------------------------------------------------------------------------------
def restate_sah(v, idx, prims=None, sah_depth=40):
    """(imask, meta, child_base, tri_base) per node in breadth-first order, the records' prims and
    the number of levels of the binary build."""
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

    # the binary tree, one level of nodes at a time: s, e the ranges of the nodes still to split
    kids = {}
    s, e = (np.array([0]), np.array([M - 1])) if M > 3 else (np.array([], int), np.array([], int))
    level = 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while len(s):
            K = len(s)
            cnt = e - s + 1
            off = np.cumsum(cnt) - cnt
            sid = np.repeat(np.arange(K), cnt)
            k_in = np.arange(cnt.sum()) - off[sid]
            pos = s[sid] + k_in
            mem = order[pos]
            cc, blo, bhi = c[mem], lo[mem], hi[mem]
            cbl, cbh = np.minimum.reduceat(cc, off, axis=0), np.maximum.reduceat(cc, off, axis=0)
            best = np.full(K, np.inf)
            bax, bs = np.full(K, -1), np.zeros(K, int)
            bins = np.zeros((3, len(mem)), int)
            for a in range(3 if level < sah_depth else 0):
                ext = cbh[:, a] - cbl[:, a]
                ok = ext > 0
                t = (cc[:, a] - cbl[sid, a]) / np.where(ok, ext, 1.0)[sid]
                b = np.clip(np.floor(t * BINS), 0, BINS - 1).astype(int)
                bins[a] = b
                key = sid * BINS + b
                bc = np.bincount(key, minlength=K * BINS).reshape(K, BINS)
                bl = np.full((K * BINS, 3), np.inf, f32)
                bh = np.full((K * BINS, 3), -np.inf, f32)
                np.minimum.at(bl, key, blo)
                np.maximum.at(bh, key, bhi)
                bl, bh = bl.reshape(K, BINS, 3), bh.reshape(K, BINS, 3)
                pl, ph, pc = np.minimum.accumulate(bl, 1), np.maximum.accumulate(bh, 1), np.cumsum(bc, 1)
                sl = np.minimum.accumulate(bl[:, ::-1], 1)[:, ::-1]
                sh = np.maximum.accumulate(bh[:, ::-1], 1)[:, ::-1]
                sc = np.cumsum(bc[:, ::-1], 1)[:, ::-1]
                for sp in range(BINS - 1, 0, -1):
                    nl, nr = pc[:, sp - 1], sc[:, sp]
                    cost = area32(pl[:, sp - 1], ph[:, sp - 1]).astype(f64) * nl + area32(sl[:, sp], sh[:, sp]).astype(f64) * nr
                    cost = np.where(np.isnan(cost), np.inf, cost)
                    win = ok & (nl > 0) & (nr > 0) & (cost < best)
                    best, bax, bs = np.where(win, cost, best), np.where(win, a, bax), np.where(win, sp, bs)
            mine = bins[np.maximum(bax, 0)[sid], np.arange(len(mem))]
            left = np.where(bax[sid] >= 0, mine < bs[sid], k_in < (cnt // 2)[sid])
            n_left = np.add.reduceat(left.astype(int), off)
            assert ((n_left >= 1) & (n_left <= cnt - 1)).all()
            order[pos] = mem[np.lexsort((k_in, ~left, sid))]        # stable on both sides
            mid = s + n_left
            for a_, m_, b_ in zip(s.tolist(), mid.tolist(), e.tolist()):
                kids[(a_, b_)] = ((a_, m_ - 1), (m_, b_))
            cs, ce = np.stack([s, mid], 1).ravel(), np.stack([mid - 1, e], 1).ravel()
            keep = ce - cs + 1 > 3
            s, e = cs[keep], ce[keep]
            level += 1

    slo, shi = lo[order], hi[order]

    def box(l, r):
        return slo[l:r + 1].min(0), shi[l:r + 1].max(0)

    size = lambda n: n[1] - n[0] + 1
    out_nodes, out_prims = [], []
    lvl, n_alloc = [(0, M - 1)], 1
    with np.errstate(over="ignore", invalid="ignore"):
        while lvl:
            nxt = []
            for nd in lvl:
                ch = [nd] if size(nd) <= 3 else list(kids[nd])
                while size(nd) > 3 and len(ch) < 8:
                    best, ba = -1, None
                    for i, x in enumerate(ch):
                        if size(x) <= 3:
                            continue
                        a = area32(*box(*x))
                        if best < 0 or a > ba:
                            best, ba = i, a
                    if best < 0:
                        break
                    l_, r_ = kids[ch[best]]
                    ch[best] = l_
                    ch.append(r_)
                boxes = [box(*x) for x in ch]
                nlo, nhi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
                pc_ = 0.5 * nlo.astype(f64) + 0.5 * nhi.astype(f64)
                vv = [0.5 * b[0].astype(f64) + 0.5 * b[1].astype(f64) - pc_ for b in boxes]
                in_slot, used = [-1] * 8, [False] * len(ch)
                for _ in ch:
                    best, bi, bsl = None, -1, -1
                    for i in range(len(ch)):
                        if used[i]:
                            continue
                        for sl_ in range(8):
                            if in_slot[sl_] >= 0:
                                continue
                            x = vv[i][0] if sl_ & 1 else -vv[i][0]
                            y = vv[i][1] if sl_ & 2 else -vv[i][1]
                            z = vv[i][2] if sl_ & 4 else -vv[i][2]
                            cost = -((x + y) + z)
                            if bi < 0 or cost < best:
                                best, bi, bsl = cost, i, sl_
                    used[bi] = True
                    in_slot[bsl] = bi
                imask, meta, rank, off_ = 0, [0] * 8, 0, 0
                child_base, tri_base = n_alloc, len(out_prims)
                for sl_ in range(8):
                    if in_slot[sl_] < 0:
                        continue
                    x = ch[in_slot[sl_]]
                    if size(x) > 3:
                        imask |= 1 << sl_
                        meta[sl_] = rank
                        rank += 1
                        nxt.append(x)
                        n_alloc += 1
                    else:
                        meta[sl_] = (size(x) << 5) | off_
                        off_ += size(x)
                        out_prims.extend(P[order[x[0]:x[1] + 1]].tolist())
                out_nodes.append((imask, meta, child_base, tri_base))
            lvl = nxt
    return out_nodes, out_prims, level


def assert_restated(name, nodes, tris, ref_nodes, ref_prims):
    assert len(ref_nodes) == len(nodes), name
    assert tris["prim"].tolist() == ref_prims, f"{name}: record order"
    assert nodes["imask"].tolist() == [n[0] for n in ref_nodes], f"{name}: imask"
    assert nodes["meta"].tolist() == [n[1] for n in ref_nodes], f"{name}: meta"
    assert nodes["child_base"].tolist() == [n[2] for n in ref_nodes], f"{name}: child_base"
    assert nodes["tri_base"].tolist() == [n[3] for n in ref_nodes], f"{name}: tri_base"


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "tiny4", "tiny9", "tiny25", "tiny257", "copies1000", "cornell",
                                  "cornell_emissive", "tiny9_1e37", "chain40", "city_plane"])
def test_sah_numpy_restatement(name):
    v, idx, prims, nodes, tris, levels = built_mode(name, SAH)
    ref_nodes, ref_prims, binary_levels = restate_sah(v, idx, prims)
    assert_restated(name, nodes, tris, ref_nodes, ref_prims)
    if name == "copies1000":
        assert binary_levels == 9            # equal centres: count splits only, 1000 -> 3 or 4 by halving


def test_depth_hook(monkeypatch):
    """MPT_SAH_DEPTH=2: binned splits on two levels, count splits below."""
    v, idx, prims, nodes, tris, levels = built_mode("cornell", SAH)
    monkeypatch.setenv("MPT_SAH_DEPTH", "2")
    hn, ht, hl = mpt.bvh_build_host(v, idx, mode=SAH)
    monkeypatch.delenv("MPT_SAH_DEPTH")
    ref_nodes, ref_prims, _ = restate_sah(v, idx, None, sah_depth=2)
    assert_restated("cornell at depth 2", hn, ht, ref_nodes, ref_prims)
    assert hn.tobytes() != nodes.tobytes() or ht.tobytes() != tris.tobytes()


# ------------------------------------------------------------------------------------
# Quality
# ------------------------------------------------------------------------------------
_sums = {}


def sums(name):
    if name not in _sums:
        out = {}
        for mode in (abi.BUILD_LBVH, abi.BUILD_PLOC, SAH):
            v, idx, prims, nodes, tris, levels = built_mode(name, mode)
            out[mode] = area_sum(nodes, tris, v, idx)
        hn, ht, _ = mpt.bvh_refit_host(v, idx)
        out["host"] = area_sum(hn, ht, v, idx)
        _sums[name] = out
    return _sums[name]


@pytest.mark.parametrize("name", ["cornell", "city", "city_move"])
def test_sah_lowers_the_area_sum(name):
    """Asserted wherever the host builder's own tree is lower than PLOC's: the city and the city
    with a part moved.  On cornell the reference is not (the module's docstring has the figures),
    so there the sums are printed and only that fact is pinned."""
    s = sums(name)
    print(f"{name}: area sum LBVH {s[0]:.3f} PLOC {s[1]:.3f} SAH {s[SAH]:.3f} host builder {s['host']:.3f}")
    if name == "cornell":
        assert not s["host"] < s[abi.BUILD_PLOC], f"{name}: the reference is below PLOC after all: assert mode 3 here too: {s}"
        return
    assert s["host"] < s[abi.BUILD_PLOC], f"{name}: the reference itself is not below PLOC: {s}"
    assert s[SAH] < s[abi.BUILD_PLOC], f"{name}: {s}"


# ------------------------------------------------------------------------------------
# Errors
# ------------------------------------------------------------------------------------
def test_mode_2_is_still_refused():
    v, idx = tiny(9)
    for mode in (2, 4, -1, 255):
        with pytest.raises(mpt.MptError) as e:
            mpt.bvh_build_host(v, idx, mode=mode)
        assert e.value.code == -1


def test_build_host_mode_errors_sah():
    from test_ploc_host import test_build_host_mode_errors
    test_build_host_mode_errors(SAH)
