"""Reference of the path queries (rt_trace_paths) -- TEST
INFRASTRUCTURE ONLY.

The bounce loop of the numpy restatement's ``trace()`` (oracle/pt_oracle_np.py),
built from its ``Scene``, ``halton``, ``_closest``, ``_occluded``, ``_gather``,
``sincos`` and ``normalize``, with three changes:

  * the first segment is the caller's ``(o, d, tmin, tmax)``: its closest hit
    is found once per ray and every sample enters bounce 0 with it (no camera
    ray, Halton dimensions 0 and 1 are not drawn);
  * a seed is masked to its low 20 bits;
  * a ray outside the exactness domain (the four numbers of
    ``Scene.ray_domain()``) is not traced: radiance (0, 0, 0, 0), first hit
    (tmax bit for bit, -1).

``Paths`` traces samples ``[sample_base, sample_base + spp_max)`` of every ray
once, all samples of all rays as one array; ``radiance(spp)`` adds the first
``spp`` of them in ascending order in float32 from +0 and divides by
``float32(spp)``.  All comparisons against it are bit for bit: ``same_words``
compares uint32 views, there is no tolerance anywhere.
"""
from __future__ import annotations

import numpy as np

import pt_oracle_np as onp

f32 = np.float32
V = onp.V


def np_scene(scene):
    """pt_oracle_np.Scene of a gpuraytracer_amd.Scene."""
    return onp.Scene(scene.camera, scene.materials, scene.light, scene.vertices, scene.spheres)


def in_domain(rays, dom):
    """DESIGN.md §3.20 from origin_max, dir_len2_min, dir_len2_max, tmax_max: every
    comparison is false for a NaN, so a NaN in any slot is outside."""
    r = np.asarray(rays, f32)
    d = V(r[:, 4], r[:, 5], r[:, 6])
    with np.errstate(all="ignore"):
        o_ok = ((np.abs(r[:, 0]) <= f32(dom["origin_max"])) & (np.abs(r[:, 1]) <= f32(dom["origin_max"])) &
                (np.abs(r[:, 2]) <= f32(dom["origin_max"])))
        l2 = onp.dot(d, d)
        d_ok = (l2 >= f32(dom["dir_len2_min"])) & (l2 <= f32(dom["dir_len2_max"]))
        t_ok = (r[:, 3] >= f32(0.0)) & (r[:, 3] < r[:, 7]) & (r[:, 7] <= f32(dom["tmax_max"]))
    return o_ok & d_ok & t_ok


def first_hits(sc, rays, dom):
    """(t float32[n], id int32[n], traced bool[n]): the closest hit with the ray's
    own tmin < t < tmax of every in-domain ray; (tmax bits, -1) for a miss and
    for a ray that is not traced."""
    r = np.ascontiguousarray(rays, f32)
    ok = in_domain(r, dom)
    t = r[:, 7].copy()
    ids = np.full(len(r), -1, np.int32)
    if ok.any():
        q = r[ok]
        i, best = onp._closest(sc, V(q[:, 0], q[:, 1], q[:, 2]), V(q[:, 4], q[:, 5], q[:, 6]), q[:, 3].copy(),
                               q[:, 7].copy())
        t[ok] = np.where(i >= 0, best, q[:, 7])
        ids[ok] = i
    return t, ids, ok


def _samples(sc, o, d, ids, th, i, bounces):
    """accumulatedColor of paths that enter bounce 0 with the hit (ids >= 0, th)
    of (o, d): pt_oracle_np.trace() from its bounce loop on."""
    shape = ids.shape
    ids = ids.astype(np.int64)
    acc = V(np.zeros(shape, f32), np.zeros(shape, f32), np.zeros(shape, f32))
    thr = V(np.ones(shape, f32), np.ones(shape, f32), np.ones(shape, f32))
    alive = np.ones(shape, bool)
    tmin, tmax = f32(0.001), f32(1000.0)
    is_light = np.array([p["light"] for p in sc.tris + sc.sph] + [False])
    nT = len(sc.tris)
    for b in range(bounces):
        if b > 0:
            ids, th = onp._closest(sc, o, d, tmin, tmax)
        alive &= ids >= 0
        lit = alive & is_light[ids]
        acc = onp._gather(sc, np.where(lit, ids, -1), "emissive", shape).where(lit, acc)
        alive &= ~lit
        hp = o + d.scale(th)
        N = onp._gather(sc, np.where(alive & (ids < nT), ids, -1), "N", shape)
        right = onp._gather(sc, np.where(alive & (ids < nT), ids, -1), "right", shape)
        fwd = onp._gather(sc, np.where(alive & (ids < nT), ids, -1), "fwd", shape)
        sm = alive & (ids >= nT)
        if sm.any():
            Ns = onp.normalize(hp - onp._gather(sc, np.where(sm, ids, -1), "c", shape))
            rs = onp.normalize(onp.cross(Ns, V(f32(0.0072), f32(1.0), f32(0.0034))))
            fs = onp.cross(rs, Ns)
            N, right, fwd = Ns.where(sm, N), rs.where(sm, right), fs.where(sm, fwd)
        diffuse = onp._gather(sc, np.where(alive, ids, -1), "diffuse", shape)
        p = hp + N.scale(f32(1e-3))
        ux = onp.halton(i, 2 + 5 * b) * f32(2.0) - f32(1.0)
        uy = onp.halton(i, 3 + 5 * b) * f32(2.0) - f32(1.0)
        q = (sc.lc + V(f32(0.25), f32(0.0), f32(0.0)).scale(ux)) + V(f32(0.0), f32(0.0), f32(0.25)).scale(uy)
        L = q - p
        dist = np.sqrt(onp.dot(L, L))
        inv = f32(1.0) / np.maximum(dist, f32(1e-3))
        L = L.scale(inv)
        lc = V(np.broadcast_to(sc.lcol.x, shape), np.broadcast_to(sc.lcol.y, shape),
               np.broadcast_to(sc.lcol.z, shape)).scale(inv * inv)
        lc = lc.scale(onp.saturate(onp.dot(-L, V(f32(0.0), f32(-1.0), f32(0.0)))))
        lc = lc.scale(onp.saturate(onp.dot(N, L)))
        thr = thr.mul(diffuse).where(alive, thr)
        occ = onp._occluded(sc, p, L, f32(0.0), dist - f32(1e-3))
        acc = (acc + lc.mul(thr)).where(alive & ~occ, acc)
        if b + 1 < bounces:
            cu, cv = onp.halton(i, 4 + 5 * b), onp.halton(i, 5 + 5 * b)
            sp, cp = onp.sincos(f32(6.28318548) * cu)
            ct = np.sqrt(cv)
            st = np.sqrt(f32(1.0) - ct * ct)
            nd = (right.scale(st * cp) + N.scale(ct)) + fwd.scale(st * sp)
            d = nd.where(alive, d)
            o = p.where(alive, o)
    return np.stack([acc.x, acc.y, acc.z], -1)


class Paths:
    """Samples [sample_base, sample_base + spp_max) of every ray, traced once."""

    def __init__(self, sc, rays, seeds, spp_max, bounces, dom, sample_base=0):
        r = np.ascontiguousarray(rays, f32)
        n = len(r)
        self.t, self.ids, self.traced = first_hits(sc, r, dom)
        self.samples = np.zeros((n, spp_max, 3), f32)  # a miss and an untraced ray: +0
        k = np.flatnonzero(self.ids >= 0)
        if len(k) and bounces > 0:
            s = (np.asarray(seeds, np.uint32).reshape(-1)[k] & np.uint32(0xFFFFF)).astype(np.uint64)
            ns = np.uint64(sample_base) + np.arange(spp_max, dtype=np.uint64)
            i = (s[:, None] + ns[None, :]).astype(np.uint32).ravel()
            rep = np.repeat(k, spp_max)
            q = r[rep]
            with np.errstate(all="ignore"):
                c = _samples(sc, V(q[:, 0], q[:, 1], q[:, 2]), V(q[:, 4], q[:, 5], q[:, 6]), self.ids[rep],
                             self.t[rep], i, bounces)
            self.samples[k] = c.reshape(len(k), spp_max, 3)

    def radiance(self, spp):
        """(n, 4) float32: (the in-order sum of the first spp samples / float32(spp), 1);
        (0, 0, 0, 0) for a ray that is not traced."""
        lum = np.zeros((len(self.ids), 3), f32)
        for n in range(spp):
            lum = lum + self.samples[:, n]
        out = np.ones((len(self.ids), 4), f32)
        out[:, :3] = lum / f32(spp)
        out[~self.traced] = f32(0.0)
        return out

    def hits(self):
        return self.t, self.ids


def same_words(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return (g.shape == w.shape and g.dtype.itemsize == 4 and w.dtype.itemsize == 4 and
            np.array_equal(g.view(np.uint32), w.view(np.uint32)))


def first_difference(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape:
        return f"shapes differ: got {g.shape}, want {w.shape}"
    bad = g.view(np.uint32) != w.view(np.uint32)
    if bad.ndim > 1:
        bad = bad.reshape(len(bad), -1).any(-1)
    idx = np.flatnonzero(bad)
    if not len(idx):
        return "equal"
    k = int(idx[0])
    return f"{len(idx)} of {len(bad)} rays differ, first at ray {k}: got {g[k]!r}, want {w[k]!r}"
