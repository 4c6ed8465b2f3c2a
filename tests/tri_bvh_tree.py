"""Node-by-node check of a triangle BVH in the compact layout the walks read
(DESIGN.md §3.10), for the dumps of ``Renderer.tri_bvh()`` and
``Scene.tri_bvh_host()``: plain numpy in float64, independent of the three
builders (rt_scene.cpp build_tri_sah, rt_lbvh.hip, rt_gsah.hip).

``check(dump)`` raises :class:`TreeError` with the invariant, layout, entry
and triangle of the first violation, in this order:

  1  perm is a permutation of 0..n-1 and sorted[k] is byte-equal to isect[perm[k]]
  2  entry 0 is the root and every layout is a proper binary tree in preorder:
     an inner entry i stores o*total + esc with i + 2 < esc <= total, its
     children are i + 1 and end(i + 1), the second child's subtree ends at
     esc(i); a leaf's subtree is itself (end(i) = i + 1)
  3  leaf words: first + count <= n, count <= leaf_max, every leaf-order index
     in exactly one leaf
  4  no fp16 half is NaN; with the near/far slots of octant o undone (the near
     slot of axis a holds hi exactly when bit a of o is set) lo <= hi
  5  a leaf's box holds the vertices v0, fl32(v0 + e1), fl32(v0 + e2) of its
     triangles padded by 0.99 * margin (the slack of tests/native/
     tri_bvh_check.cpp for the fp32 rounding of min - margin)
  6  an inner box holds both child boxes (decoded values, exactly)
  7  the 8 layouts are the same tree: the same multiset of (leaf-order indices
     under the entry, box planes) and, per inner node, the child order of
     layout o ^ 7 is the reverse of layout o's

The set of leaf-order indices under an entry is compared through its size,
its smallest member and a sum of fixed random 64-bit weights: equal sets give
equal keys, and two different sets collide with probability about 2^-64.

``walk(dump, rays)`` is the float64 stackless closest-hit walk of each ray's
octant layout (as tests/native/tri_bvh_check.cpp), ``brute(dump, rays)`` the
id-ordered minimum over every triangle by the same test."""
import numpy as np

f32, f64 = np.float32, np.float64
INNER = np.uint32(0x80000000)


class TreeError(AssertionError):
    def __init__(self, invariant, message, layout=None, entry=None, triangle=None):
        where = ", ".join(f"{k} {v}" for k, v in (("layout", layout), ("entry", entry), ("triangle", triangle))
                          if v is not None)
        super().__init__(f"invariant {invariant}: {message}" + (f" ({where})" if where else ""))
        self.invariant, self.layout, self.entry, self.triangle = invariant, layout, entry, triangle


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def halves(nodes):
    """(8, total, 6) uint16: the six fp16 slots of every entry (near x, y, z, far x, y, z)."""
    w = np.ascontiguousarray(nodes[..., :3], np.uint32)
    return np.stack([w[..., 0] & 0xFFFF, w[..., 0] >> 16, w[..., 1] & 0xFFFF, w[..., 1] >> 16,
                     w[..., 2] & 0xFFFF, w[..., 2] >> 16], -1).astype(np.uint16)


def boxes(nodes):
    """(lo, hi), each (8, total, 3) float64: the slots of octant o undone."""
    h = halves(nodes).view(np.float16).astype(f64)
    neg = ((np.arange(8)[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)[:, None, :]
    return np.where(neg, h[..., 3:], h[..., :3]), np.where(neg, h[..., :3], h[..., 3:])


def tri_vertices(rec):
    """(n, 3, 3) float64: v0, fl32(v0 + e1), fl32(v0 + e2) of 12-float records."""
    r = np.asarray(rec, f32)
    return np.stack([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]], 1).astype(f64)


def structure(dump):
    """Invariant 2 on every layout; returns (inner, end): end[o, i] is one past
    the last entry of i's subtree."""
    nodes = dump["nodes"]
    total = dump["nodes_per_layout"]
    if nodes.shape != (8, total, 4) or total < 1:
        raise TreeError(2, f"node array {nodes.shape} for {total} entries per layout")
    w = nodes[..., 3]
    inner = (w & INNER) != 0
    idx = np.arange(total, dtype=np.int64)
    end = np.empty((8, total), np.int64)
    for o in range(8):
        esc = (w[o] & ~INNER).astype(np.int64) - o * total
        bad = inner[o] & ~((idx + 2 < esc) & (esc <= total))
        if bad.any():
            i = _first(bad)
            raise TreeError(2, f"escape {int(esc[i])} of an inner entry, {total} entries", o, i)
        end[o] = np.where(inner[o], esc, idx + 1)
        if end[o, 0] != total:
            raise TreeError(2, f"the root's subtree ends at {int(end[o, 0])}, not {total}", o, 0)
        ii = idx[inner[o]]
        c2 = end[o, ii + 1]
        bad = c2 >= end[o, ii]
        if bad.any():
            raise TreeError(2, "no room for a second child", o, int(ii[_first(bad)]))
        bad = end[o, c2] != end[o, ii]
        if bad.any():
            raise TreeError(2, "the second child's subtree does not end at the escape", o, int(ii[_first(bad)]))
    return inner, end


def check(dump, expect_nodes=None):
    """All seven invariants; ``expect_nodes``: rt_build_info's tri_bvh_nodes."""
    n, total = dump["n_triangles"], dump["nodes_per_layout"]
    nodes, perm = dump["nodes"], dump["perm"]
    # 1
    if len(perm) != n or len(dump["sorted"]) != n or len(dump["isect"]) != n:
        raise TreeError(1, "array lengths differ from n_triangles")
    seen = np.bincount(perm[perm < n], minlength=n)
    if (perm >= n).any() or (seen != 1).any():
        k = _first((perm >= n) | (seen[np.minimum(perm, n - 1)] != 1))
        raise TreeError(1, f"perm is no permutation: perm[{k}] = {int(perm[k])}", triangle=k)
    same = np.ascontiguousarray(dump["sorted"], f32).view(np.uint32) == \
        np.ascontiguousarray(dump["isect"], f32)[perm].view(np.uint32)
    if not same.all():
        k = _first(~same.all(1))
        raise TreeError(1, f"sorted[{k}] is not isect[perm[{k}]] = isect[{int(perm[k])}]", triangle=k)
    # 2
    if expect_nodes is not None and expect_nodes != total:
        raise TreeError(2, f"{total} entries per layout, the build reports {expect_nodes}")
    inner, end = structure(dump)
    # 3
    w = nodes[..., 3]
    first = (w & 0xFFFFFF).astype(np.int64)
    count = (w >> 24).astype(np.int64) + 1
    owner = np.empty((8, n), np.int64)
    for o in range(8):
        lf = np.flatnonzero(~inner[o])
        bad = first[o, lf] + count[o, lf] > n
        if bad.any():
            raise TreeError(3, f"leaf range past {n} triangles", o, int(lf[_first(bad)]))
        bad = count[o, lf] > dump["leaf_max"]
        if bad.any():
            i = int(lf[_first(bad)])
            raise TreeError(3, f"leaf of {int(count[o, i])} triangles, at most {dump['leaf_max']}", o, i)
        ks = np.repeat(first[o, lf], count[o, lf]) + (np.arange(count[o, lf].sum()) -
                                                      np.repeat(np.cumsum(count[o, lf]) - count[o, lf], count[o, lf]))
        cover = np.bincount(ks, minlength=n)
        if (cover != 1).any():
            k = _first(cover != 1)
            raise TreeError(3, f"leaf-order index {k} lies in {int(cover[k])} leaves", o, triangle=k)
        owner[o, ks] = np.repeat(lf, count[o, lf])
    # 4
    hf = halves(nodes).view(np.float16)
    if np.isnan(hf).any():
        o, i = (int(v) for v in np.argwhere(np.isnan(hf).any(-1))[0])
        raise TreeError(4, "a NaN plane", o, i)
    lo, hi = boxes(nodes)
    if (lo > hi).any():
        o, i = (int(v) for v in np.argwhere((lo > hi).any(-1))[0])
        raise TreeError(4, f"near/far slots out of order: lo {lo[o, i]} hi {hi[o, i]}", o, i)
    # 5
    v = tri_vertices(dump["sorted"])
    pad = 0.99 * f64(dump["margin"])
    vlo, vhi = v.min(1) - pad, v.max(1) + pad
    for o in range(8):
        bad = ((lo[o, owner[o]] > vlo) | (vhi > hi[o, owner[o]])).any(1)
        if bad.any():
            k = _first(bad)
            raise TreeError(5, f"triangle outside its padded leaf box: box {lo[o, owner[o, k]]} .. "
                               f"{hi[o, owner[o, k]]}, padded triangle {vlo[k]} .. {vhi[k]}", o, int(owner[o, k]), k)
    # 6
    for o in range(8):
        ii = np.flatnonzero(inner[o])
        for c in (ii + 1, end[o, ii + 1]):
            bad = ((lo[o, ii] > lo[o, c]) | (hi[o, c] > hi[o, ii])).any(1)
            if bad.any():
                j = _first(bad)
                raise TreeError(6, f"child entry {int(c[j])} reaches outside its parent's box", o, int(ii[j]))
    # 7
    weight = np.random.default_rng(7).integers(0, 2 ** 63, n + 1, dtype=np.uint64)
    weight[0] = 0
    wsum = np.cumsum(weight, dtype=np.uint64)       # wsum[k] = weight of the indices < k (wrapping)
    big = np.int64(n)
    ref = {}
    for o in range(8):
        leaf = ~inner[o]
        contrib = np.where(leaf, wsum[np.minimum(first[o] + count[o], n)] - wsum[np.minimum(first[o], n)], np.uint64(0))
        psum = np.concatenate([[np.uint64(0)], np.cumsum(contrib, dtype=np.uint64)])
        pcnt = np.concatenate([[0], np.cumsum(np.where(leaf, count[o], 0))])
        idx = np.arange(total)
        sethash = psum[end[o]] - psum[idx]
        setcnt = pcnt[end[o]] - pcnt[idx]
        # smallest member: the minimum of `first` over the leaves in [i, end(i)) (one sentinel past the end)
        fmin = np.concatenate([np.where(leaf, first[o], big), [big]])
        setmin = np.minimum.reduceat(fmin, np.stack([idx, end[o]], 1).ravel())[0::2]
        rows = np.concatenate([sethash[:, None].view(np.int64), setcnt[:, None], setmin[:, None],
                               (lo[o] + 0.0).view(np.int64), (hi[o] + 0.0).view(np.int64)], 1)
        order = np.lexsort(rows.T[::-1])
        rows = rows[order]
        ii = np.flatnonzero(inner[o])
        kids = np.stack([sethash[ii], sethash[ii + 1], sethash[end[o, ii + 1]]], 1)
        kids = kids[np.argsort(kids[:, 0], kind="stable")]
        ref[o] = (rows, order, kids)
    for o in range(1, 8):
        a, b = ref[0][0], ref[o][0]
        if a.shape != b.shape or not np.array_equal(a, b):
            j = _first((a != b).any(1)) if a.shape == b.shape else 0
            raise TreeError(7, f"layouts 0 and {o} are not the same tree: entry {int(ref[0][1][j])} of layout 0 "
                               f"has no equal in layout {o}", o, int(ref[o][1][j]))
    for o in range(4):
        a, b = ref[o][2], ref[o ^ 7][2]
        bad = (a[:, 0] != b[:, 0]) | (a[:, 1] != b[:, 2]) | (a[:, 2] != b[:, 1])
        if bad.any():
            raise TreeError(7, f"the child order of layout {o ^ 7} is not the reverse of layout {o}'s at "
                               f"{int(bad.sum())} of {len(a)} inner nodes", o ^ 7)


# ---- float64 walks ---------------------------------------------------------------

def hit_matrix(isect, rays, chunk=256):
    """(rays, triangles) float64: t of the double-precision Moeller-Trumbore
    test (tests/native/tri_bvh_check.cpp) with tmin < t < tmax, else inf."""
    v = tri_vertices(isect)
    e1, e2, v0 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], v[:, 0]
    r = np.asarray(rays, f64)
    out = np.full((len(r), len(v)), np.inf)
    with np.errstate(all="ignore"):
        for b in range(0, len(r), chunk):
            o, d = r[b:b + chunk, None, 0:3], r[b:b + chunk, None, 4:7]
            tmin, tmax = r[b:b + chunk, None, 3], r[b:b + chunk, None, 7]
            p = np.cross(d, e2[None])
            det = np.sum(e1[None] * p, -1)
            s = o - v0[None]
            u = np.sum(s * p, -1) / det
            q = np.cross(s, e1[None])
            vv = np.sum(d * q, -1) / det
            t = np.sum(e2[None] * q, -1) / det
            ok = (np.abs(det) >= 1e-300) & (u >= 0) & (u <= 1) & (vv >= 0) & (u + vv <= 1) & (t > tmin) & (t < tmax)
            out[b:b + chunk] = np.where(ok, t, np.inf)
    return out


def brute(dump, rays, hits=None):
    """(t, id): the smallest t, ties to the lowest id; a miss is (tmax, -1)."""
    hits = hit_matrix(dump["isect"], rays) if hits is None else hits
    ids = np.argmin(hits, 1)
    t = hits[np.arange(len(hits)), ids]
    miss = ~np.isfinite(t)
    return np.where(miss, np.asarray(rays, f64)[:, 7], t), np.where(miss, -1, ids)


def walk(dump, rays, hits=None):
    """(t, id) of the stackless closest-hit walk of each ray's octant layout."""
    hits = hit_matrix(dump["isect"], rays) if hits is None else hits
    total = dump["nodes_per_layout"]
    lo, hi = boxes(dump["nodes"])
    lo, hi = lo.tolist(), hi.tolist()
    word = dump["nodes"][..., 3].tolist()
    perm = dump["perm"].tolist()
    r = np.asarray(rays, f64)
    octs = (np.signbit(r[:, 4]) * 1 + np.signbit(r[:, 5]) * 2 + np.signbit(r[:, 6]) * 4).tolist()
    out_t, out_id = np.empty(len(r)), np.empty(len(r), np.int64)
    for k, ray in enumerate(r.tolist()):
        o, tmin, d, tmax = ray[0:3], ray[3], ray[4:7], ray[7]
        oc = octs[k]
        L, H, Wd, base = lo[oc], hi[oc], word[oc], oc * total
        row = hits[k]
        best, bid = tmax, -1
        i = 0
        while i < total:
            w = Wd[i]
            t0, t1 = tmin, best
            bl, bh = L[i], H[i]
            ok = True
            for a in range(3):
                if d[a] == 0.0:
                    if o[a] < bl[a] or o[a] > bh[a]:
                        ok = False
                        break
                    continue
                ta, tb = (bl[a] - o[a]) / d[a], (bh[a] - o[a]) / d[a]
                if ta > tb:
                    ta, tb = tb, ta
                t0 = ta if ta > t0 else t0
                t1 = tb if tb < t1 else t1
            ok = ok and t0 <= t1 * (1 + 1e-12) + 1e-12
            if not ok:
                i = (w & 0x7FFFFFFF) - base if w & 0x80000000 else i + 1
                continue
            if not w & 0x80000000:
                f = w & 0xFFFFFF
                for j in range(f, f + (w >> 24) + 1):
                    tid = perm[j]
                    t = row[tid]
                    if t <= best and t != np.inf and (t < best or tid < bid or bid < 0):
                        best, bid = t, tid
            i += 1
        out_t[k], out_id[k] = best, bid
    return out_t, out_id
