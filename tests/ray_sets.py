"""Ray sets and their reference answers for the batched ray queries
(tests/test_ray_query.py on the CPU, tests/test_gpu_ray_query.py on the GPU).

A ray is a row of 8 float32: (origin.xyz, tmin, dir.xyz, tmax), the rt_ray of
include/rtpt.h.  The reference is the numpy restatement's id-ordered scan,
``pt_oracle_np._closest`` and ``pt_oracle_np._occluded``, put into the form
``Renderer.trace_rays`` returns:

  closest  (t, id): the hit, or (the ray's tmax bit for bit, -1)
  any      (+0, 1 or 0)

Sets (every scene lies inside [-2.5, 2.5]^3):
  B  4096 incoherent rays from inside the room, tmin 0.001, tmax 1000
  C  4096 segments between two random points, tmin 0, tmax dist - 1e-3
  D  chosen rays: a hit with tmax or tmin exactly at it, rays at the corners
     and edge midpoints of every pair's first triangle (shared edges: id ties),
     rays lying in a face's plane, origins exactly on a face, axis directions
     with +0 and -0 components, origins inside spheres and tangent rays
  E  rays outside the exactness domain mixed into waves of
     in-domain rays, and one block of 64 consecutive ones
  G  rays grazing the box faces of every triangle (tests/test_tri_bvh_tree.py,
     tests/test_gpu_tri_bvh_tree.py)
"""
import functools

import numpy as np

import pt_oracle_np as onp

f32 = np.float32
N = 4096
INTERIOR = (0.1, 0.2, 0.3)  # the fixed origin of the corner and edge rays


def pack(o, d, tmin, tmax):
    o = np.asarray(o, f32).reshape(-1, 3)
    r = np.empty((len(o), 8), f32)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def _unit(v):
    v = np.asarray(v, f32)
    return v / np.sqrt(np.sum(v * v, axis=-1, dtype=f32))[..., None]


@functools.lru_cache(maxsize=None)
def sets_bc():
    """(B, C) by the recipe of the feature's issue (numpy PCG64, seed 2024)."""
    rng = np.random.default_rng(2024)
    o = rng.uniform(-2.4, 2.4, (N, 3)).astype(f32)
    g = rng.standard_normal((N, 3)).astype(f32)
    d = g / np.sqrt(np.sum(g * g, axis=1, dtype=f32))[:, None]
    B = pack(o, d, f32(0.001), f32(1000.0))
    q = rng.uniform(-2.4, 2.4, (N, 3)).astype(f32)
    L = q - o
    dist = np.sqrt(np.sum(L * L, axis=1, dtype=f32))
    C = pack(o, L / dist[:, None], f32(0.0), dist - f32(1e-3))
    return B, C


def np_scene(scene):
    """pt_oracle_np.Scene of a gpuraytracer_amd.Scene."""
    return onp.Scene(scene.camera, scene.materials, scene.light, scene.vertices, scene.spheres)


def _soa(rays):
    r = np.ascontiguousarray(rays, f32)
    return (onp.V(r[:, 0], r[:, 1], r[:, 2]), onp.V(r[:, 4], r[:, 5], r[:, 6]), r[:, 3].copy(), r[:, 7].copy())


def reference(sc, rays, any_hit=False):
    """(t float32[n], id int32[n]) of the id-ordered scan, as trace_rays gives them."""
    o, d, tmin, tmax = _soa(rays)
    with np.errstate(all="ignore"):
        if any_hit:
            occ = onp._occluded(sc, o, d, tmin, tmax)
            return np.zeros(len(rays), f32), occ.astype(np.int32)
        ids, best = onp._closest(sc, o, d, tmin, tmax)
    t = np.where(ids >= 0, best.view(np.uint32), tmax.view(np.uint32)).astype(np.uint32).view(f32)
    return t, ids.astype(np.int32)


def same(got, want):
    """Bit equality of a (t, id) answer: t as uint32 views, id exactly."""
    (gt, gi), (wt, wi) = got, want
    gt, wt = np.ascontiguousarray(gt, f32), np.ascontiguousarray(wt, f32)
    return np.array_equal(gt.view(np.uint32), wt.view(np.uint32)) and np.array_equal(np.asarray(gi), np.asarray(wi))


def first_difference(got, want):
    (gt, gi), (wt, wi) = got, want
    bad = np.flatnonzero((np.ascontiguousarray(gt, f32).view(np.uint32) != np.ascontiguousarray(wt, f32).view(np.uint32))
                         | (np.asarray(gi) != np.asarray(wi)))
    if len(bad) == 0:
        return "equal"
    k = int(bad[0])
    return f"{len(bad)} rays differ; first: ray {k} got (t={gt[k]!r}, id={gi[k]}) want (t={wt[k]!r}, id={wi[k]})"


# ---- set D -------------------------------------------------------------------

def d_tmax_at_hit(B, t, ids):
    """B's hits again with tmax equal to the found t: the strict bound drops the hit."""
    r = B[ids >= 0].copy()
    r[:, 7] = t[ids >= 0]
    return r


def d_tmin_at_hit(B, t, ids):
    r = B[ids >= 0].copy()
    r[:, 3] = t[ids >= 0]
    return r


def _tri_vertices(scene):
    return np.frombuffer(bytes(scene.vertices), f32).reshape(-1, 3, 4)[:, :, :3].copy()


def d_pair_corners(scene, origin=INTERIOR):
    """From ``origin`` at the corners and edge midpoints of every pair's first
    triangle (6 rays a pair): a ray through the shared edge can be accepted by
    both triangles of the pair with one t."""
    v = _tri_vertices(scene)[0::2]
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    targets = np.stack([a, b, c, (a + b) * f32(0.5), (b + c) * f32(0.5), (a + c) * f32(0.5)], 1).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origin, f32), targets.shape)
    return pack(o, _unit(targets - o), f32(0.001), f32(1000.0))


def d_in_plane(scene, tris=(0, 2, 4, 6, 8)):
    """Rays lying in a face's plane: from a point of the face along its edges,
    and from outside the face towards it."""
    v = _tri_vertices(scene)
    rows = []
    for k in tris:
        if k >= len(v):
            continue
        a, e1, e2 = v[k, 0], v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
        p = a + f32(0.3) * e1 + f32(0.2) * e2
        for dirn in (e1, e2, -e1, e1 + e2):
            rows.append(pack(p, _unit(dirn), f32(0.0), f32(1000.0)))
            rows.append(pack(a - f32(0.5) * _unit(dirn), _unit(dirn), f32(0.001), f32(1000.0)))
    return np.concatenate(rows)


def d_on_face(scene, tris=(0, 3, 5, 9, 10, 17, 34)):
    """Origins exactly on a face: along the normal both ways and obliquely,
    with tmin 0 and 0.001."""
    v = _tri_vertices(scene)
    rows = []
    for k in tris:
        if k >= len(v):
            continue
        a, e1, e2 = v[k, 0], v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
        p = a + f32(0.25) * e1 + f32(0.25) * e2
        n = _unit(np.cross(e1, e2).astype(f32))
        for dirn in (n, -n, _unit(n + _unit(e1)), _unit(-n + _unit(e2))):
            for tmin in (0.0, 0.001):
                rows.append(pack(p, dirn, f32(tmin), f32(1000.0)))
    return np.concatenate(rows)


def d_axis_zero_signs():
    """Axis directions whose other two components are +0 or -0."""
    rows = []
    for o in (INTERIOR, (0.0, 0.0, 0.0), (-1.0, 2.0, 0.5)):
        for axis in range(3):
            for s in (1.0, -1.0):
                for z1 in (0.0, -0.0):
                    for z2 in (0.0, -0.0):
                        d = [z1, z2]
                        d.insert(axis, s)
                        rows.append(pack(o, np.array(d, f32), f32(0.001), f32(1000.0)))
    return np.concatenate(rows)


def d_spheres(scene, count=16):
    """Origins inside a sphere (the t2 root) and rays tangent to one, where the
    discriminant's sign is decided by rounding."""
    if scene.n_spheres == 0:
        return np.zeros((0, 8), f32)
    s = np.frombuffer(bytes(scene.spheres), f32).reshape(-1, 20)[:count]
    c, r = s[:, 0:3].copy(), s[:, 16].copy()
    dirs = _unit(np.array([(1, 0, 0), (0, -1, 0), (0.3, 0.5, -0.8), (-0.6, 0.1, 0.7)], f32))
    rows = []
    for dirn in dirs:
        rows.append(pack(c, np.broadcast_to(dirn, c.shape), f32(0.001), f32(1000.0)))             # the centre
        rows.append(pack(c + f32(0.5) * r[:, None] * dirs[0], np.broadcast_to(dirn, c.shape),
                         f32(0.001), f32(1000.0)))                                                    # off centre
    for k in (-2, -1, 0, 1, 2):  # grazing: offset r (1 + k 2^-23) from the axis of a ray along z / x
        off = r * (f32(1.0) + f32(k) * f32(2.0 ** -23))
        ox = c + np.stack([off, np.zeros_like(off), np.full_like(off, -2.0)], 1)
        rows.append(pack(ox, np.broadcast_to(np.array([0, 0, 1], f32), c.shape), f32(0.001), f32(1000.0)))
        oy = c + np.stack([np.full_like(off, 2.0), off, np.zeros_like(off)], 1)
        rows.append(pack(oy, np.broadcast_to(np.array([-1, 0, 0], f32), c.shape), f32(0.001), f32(1000.0)))
    return np.concatenate(rows)


def set_d(scene, B, ref_b, pairs=True, origin=INTERIOR):
    """The whole of set D for a scene; ``ref_b`` is B's closest reference,
    ``origin`` the origin of the corner and edge rays."""
    t, ids = ref_b
    parts = [d_tmax_at_hit(B, t, ids), d_tmin_at_hit(B, t, ids)]
    if pairs:
        parts.append(d_pair_corners(scene, origin))
    parts += [d_in_plane(scene), d_on_face(scene), d_axis_zero_signs(), d_spheres(scene)]
    return np.concatenate(parts)


# ---- set E -------------------------------------------------------------------

def out_of_domain_variants(base, origin_max):
    """One out-of-domain ray per row of ``base`` (in-domain rays), cycling through
    the kinds: far origins, scaled directions, tmax inf / 1e30, a NaN in each of
    the eight slots, a zero direction, tmin < 0, tmin >= tmax."""
    r = np.array(base, f32, copy=True)
    kinds = 21
    for k in range(len(r)):
        q = r[k]
        kind = k % kinds
        if kind == 0:    # origin at 10 * origin_max, aimed back at the old origin
            o = q[0:3].copy()
            q[0:3] = o - q[4:7] * f32(10.0 * origin_max)
        elif kind == 1:  # origin at 1e6
            q[0:3] = q[0:3] - q[4:7] * f32(1e6)
            q[7] = f32(2e6)
        elif kind == 2:
            q[4:7] *= f32(100.0)
        elif kind == 3:
            q[4:7] *= f32(1e-3)
            q[7] = f32(1e6)
        elif kind == 4:
            q[7] = f32(np.inf)
        elif kind == 5:
            q[7] = f32(1e30)
        elif kind <= 13:  # a NaN in each slot
            q[kind - 6] = f32(np.nan)
        elif kind == 14:
            q[4:7] = f32(0.0)
        elif kind == 15:
            q[3] = f32(-1.0)
        elif kind == 16:
            q[3] = q[7] = f32(1.5)
        elif kind == 17:
            q[3], q[7] = f32(10.0), f32(5.0)
        elif kind == 18:  # an infinite origin component
            q[1] = f32(-np.inf)
        elif kind == 19:  # an infinite direction component
            q[5] = f32(np.inf)
        else:            # tmax just past the bound
            q[7] = np.nextafter(f32(1000.0), f32(2000.0))
    return r


def in_domain(rays, dom):
    """The predicate of DESIGN.md §3.20 (rt_raydomain.h), restated."""
    r = np.asarray(rays, f32)
    with np.errstate(all="ignore"):
        o_ok = np.all(np.abs(r[:, 0:3]) <= f32(dom["origin_max"]), axis=1)
        l2 = onp.dot(onp.V(r[:, 4], r[:, 5], r[:, 6]), onp.V(r[:, 4], r[:, 5], r[:, 6]))
        d_ok = (l2 >= f32(dom["dir_len2_min"])) & (l2 <= f32(dom["dir_len2_max"]))
        t_ok = (r[:, 3] >= 0) & (r[:, 3] < r[:, 7]) & (r[:, 7] <= f32(dom["tmax_max"]))
    return o_ok & d_ok & t_ok


def set_e(B, dom):
    """768 rays: B's first 512 with every third ray replaced by an out-of-domain
    variant of itself (waves that hold both kinds), then 64 consecutive
    out-of-domain rays (a wave with none in the domain), then 192 mixed again."""
    r = B[:768].copy()
    out = out_of_domain_variants(B[:768], dom["origin_max"])
    mixed = np.arange(768) % 3 == 0
    mixed[512:576] = True
    r[mixed] = out[mixed]
    return r


# ---- set G -------------------------------------------------------------------

G_INSET = f32(2.0 ** -10)


def set_g(scene, seed=9):
    """(rays, target): rays that graze the faces of the triangles' boxes, six a
    triangle.  For each triangle k and axis a: p = v + 2^-10 (c - v), v the
    triangle's extreme vertex on a (the highest for even k + a, else the
    lowest) and c its centroid; two rays through p whose direction has
    component +0 and -0 on a and a random angle in the other two axes, origin
    p - 0.5 d, tmin 0.001, tmax 1000.  Such a ray runs parallel to the box face
    next to v at 2^-10 of the triangle's size from it: a box that is short by
    an fp16 step there (1e-3 at |x| in [2, 4)) loses the hit.  target[j] is the
    triangle ray j aims at."""
    rng = np.random.default_rng(seed)
    v = _tri_vertices(scene)
    n = len(v)
    c = (v[:, 0] + v[:, 1] + v[:, 2]) / f32(3.0)
    rows, target = [], []
    for a in range(3):
        high = (np.arange(n) + a) % 2 == 0
        pick = np.where(high, np.argmax(v[:, :, a], 1), np.argmin(v[:, :, a], 1))
        ext = v[np.arange(n), pick]
        p = ext + G_INSET * (c - ext)
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        for zero in (0.0, -0.0):
            d = np.empty((n, 3), f32)
            d[:, a] = f32(zero)
            d[:, (a + 1) % 3] = np.cos(th).astype(f32)
            d[:, (a + 2) % 3] = np.sin(th).astype(f32)
            rows.append(pack(p - f32(0.5) * d, d, f32(0.001), f32(1000.0)))
            target.append(np.arange(n))
    return np.concatenate(rows), np.concatenate(target).astype(np.int32)


# ---- rays in the plane of an oblique face ---------------------------------------

def in_plane_random(scene, tris, per_tri=400, seed=5):
    """Random rays lying (to rounding) in the plane of each triangle of
    ``tris``: origin v0 + s e1 + t e2 with (s, t) in [-4, 4]^2 kept inside the
    room, direction a random combination of e1 and e2.  Most pass beside the
    triangle.  For a face whose normal is no world axis, dot(n, d) is then a
    rounding residue and not 0, and so are the barycentric terms: the test of
    DESIGN.md §3.5 can accept such a ray anywhere along it (§3.20, the premise)."""
    rng = np.random.default_rng(seed)
    v = _tri_vertices(scene)
    rows = []
    for k in tris:
        a, e1, e2 = v[k, 0], v[k, 1] - v[k, 0], v[k, 2] - v[k, 0]
        S = rng.uniform(-4, 4, (per_tri, 2)).astype(f32)
        Dc = rng.standard_normal((per_tri, 2)).astype(f32)
        o = a + S[:, :1] * e1 + S[:, 1:] * e2
        d = _unit(Dc[:, :1] * e1 + Dc[:, 1:] * e2)
        keep = np.all(np.abs(o) <= f32(2.5), axis=1)
        rows.append(pack(o[keep], d[keep], f32(0.001), f32(1000.0)))
    return np.concatenate(rows)


RESIDUE = f32(2.0 ** -20)  # |dot(n, d)| <= RESIDUE |n| |d|: the ray lies in the triangle's plane to rounding


def residue_hits(sc, rays):
    """Per ray: does the scan accept a hit on a triangle whose plane holds the
    ray to rounding (|dot(n, d)| <= 2^-20 |n| |d|)?  Such a hit is decided by
    rounding residues and can lie anywhere along the ray."""
    o, d, tmin, tmax = _soa(rays)
    out = np.zeros(len(rays), bool)
    with np.errstate(all="ignore"):
        dl = np.sqrt(onp.dot(d, d))
        for T in sc.tris:
            hit, _ = onp._tri_test(T, o, d, tmin, tmax)
            den = np.abs(onp.dot(T["n"], d))
            out |= hit & (den <= RESIDUE * np.sqrt(onp.dot(T["n"], T["n"])) * dl)
    return out
