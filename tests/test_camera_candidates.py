"""CPU: the per-wave camera-ray candidate mask (gpuraytracer_amd/csrc/rt_beam.hpp,
DESIGN.md §3.16) through the host entry point rt_debug_camera_candidates, which
runs the same source text as the kernel prologue.

Property: for a pixel rectangle, every triangle that the oracle's triangle test
(pto_ray_triangle) accepts at any t > 0.001 for any camera ray of the rectangle
(pto_camera_ray, jitter in [0, 1]) has its byte set.  Only triangles whose byte
is 0 can break it, so only those are tested against every ray.  Rectangles are
the kernel's wave footprints (4x4, 2x2, 8x8 pixels, 16x1 for interleaved rows)
of frames that are no multiple of them, whole tiles at the frame's edge
included.  Two controls show the check can fail and the mask is tight."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import MaterialGPU, Scene, float3
from gpuraytracer_amd._native import lib

W, H = 70, 45
# a handle of its own on the oracle: the prototypes set here stay out of the
# function objects other test modules share through oracle_lib.lib
L = ctypes.CDLL(oracle_lib.lib._name)
_V = ctypes.c_void_p
L.pto_ray_triangle.restype = ctypes.c_int
L.pto_ray_triangle.argtypes = [_V, _V, _V, _V, _V, ctypes.c_float, ctypes.c_float, _V]
L.pto_camera_ray.restype = None
L.pto_camera_ray.argtypes = [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _V]
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
T_MAX = 3.0e38


def candidates(scene, x0, x1, y0, y1):
    out = (ctypes.c_uint8 * scene.n_triangles)()
    assert lib.rt_debug_camera_candidates(ctypes.byref(scene.desc()), x0, x1, y0, y1, out) == 0
    return np.frombuffer(out, np.uint8).copy()


class Tracer:
    """pto_camera_ray + pto_ray_triangle on one scene, pointers prepared once."""

    def __init__(self, scene):
        self.scene = scene
        self.cam = ctypes.addressof(scene.camera)
        self.o = ctypes.addressof(scene.camera.position)
        base = ctypes.addressof(scene.vertices)
        self.v = [base + 16 * i for i in range(3 * scene.n_triangles)]
        self.d = (ctypes.c_float * 3)()
        self.t = ctypes.c_float()

    def accepted(self, x, y, jx, jy, tris):
        """The triangles of `tris` the camera ray (x, y, jx, jy) hits at any t > 0.001."""
        L.pto_camera_ray(self.cam, x, y, jx, jy, self.d)
        v, hit = self.v, []
        for k in tris:
            if L.pto_ray_triangle(self.o, self.d, v[3 * k], v[3 * k + 1], v[3 * k + 2], 0.001, T_MAX,
                                  ctypes.byref(self.t)):
                hit.append(int(k))
        return hit


def tile_rays(xs, ys, rng, n_random=300):
    """Camera rays (x, y, jx, jy) of the pixels xs x ys: the four corners with the
    jitter at the outer end (exactly 1, and the largest float below it), the
    inner ends, the edge midpoints, and seeded random ones."""
    x0, x1, y0, y1 = xs[0], xs[-1], ys[0], ys[-1]
    rays = []
    for hi in (1.0, ONE_BELOW):
        rays += [(x0, y0, 0.0, 0.0), (x1, y0, hi, 0.0), (x0, y1, 0.0, hi), (x1, y1, hi, hi)]
    rays += [(x1, y1, 0.0, 0.0), (x0, y0, 1.0, 1.0)]
    xm, ym = xs[len(xs) // 2], ys[len(ys) // 2]
    rays += [(xm, y0, 0.5, 0.0), (xm, y1, 0.5, 1.0), (x0, ym, 0.0, 0.5), (x1, ym, 1.0, 0.5)]
    jit = rng.random((n_random, 2), dtype=np.float32)
    px = rng.integers(0, len(xs), n_random)
    py = rng.integers(0, len(ys), n_random)
    rays += [(xs[px[i]], ys[py[i]], float(jit[i, 0]), float(jit[i, 1])) for i in range(n_random)]
    return rays


def footprints(rng, per_shape=10):
    """Wave footprints of a W x H frame as (rectangle, pixel columns, pixel rows
    inside the frame): whole frames in 4x4, 2x2 and 8x8 tiles, and the rows
    y = 1 (mod 3) in 4x4 tiles of those rows and in 16x1 rows.  The rectangle is
    the whole tile, also where it overhangs the frame."""
    out = []
    for tw, th, start, step in ((4, 4, 0, 1), (2, 2, 0, 1), (8, 8, 0, 1), (4, 4, 1, 3), (16, 1, 1, 3)):
        rows = (H - 1 - start) // step + 1
        nx, ny = (W + tw - 1) // tw, (rows + th - 1) // th
        picks = {(nx - 1, ny - 1), (0, 0), (nx - 1, 0)}   # the overhanging corner tile first
        while len(picks) < per_shape:
            picks.add((int(rng.integers(0, nx)), int(rng.integers(0, ny))))
        for tx, ty in sorted(picks):
            x0, j0 = tx * tw, ty * th
            rect = (x0, x0 + tw - 1, start + j0 * step, start + (j0 + th - 1) * step)
            xs = [x for x in range(x0, x0 + tw) if x < W]
            ys = [start + j * step for j in range(j0, j0 + th) if j < rows]
            out.append((rect, xs, ys))
    return out


def check_scene(scene, seed, per_shape=10):
    rng = np.random.default_rng(seed)
    tr = Tracer(scene)
    for rect, xs, ys in footprints(rng, per_shape):
        may = candidates(scene, *rect)
        assert may.shape == (scene.n_triangles,) and set(np.unique(may)) <= {0, 1}
        assert (may[0::2] == may[1::2]).all(), "a pair's two triangles share one answer"
        left_out = np.flatnonzero(may == 0)
        for ray in tile_rays(xs, ys, rng):
            hit = tr.accepted(*ray, left_out)
            assert not hit, f"rect {rect}: ray {ray} hits triangles {hit}, left out of {may.tolist()}"


def quad_scene(quads, w=W, h=H, camera=None):
    """Cornell camera and light pair + the given quads (4 corners each) as
    shared-edge triangle pairs."""
    base = Scene.cornell_box(w, h)
    n = 2 * len(quads) + 2
    mats, verts = (MaterialGPU * n)(), (float3 * (3 * n))()
    for q, P in enumerate(quads):
        for t, tri in enumerate(((P[0], P[1], P[2]), (P[0], P[2], P[3]))):
            k = 2 * q + t
            for v in range(3):
                verts[3 * k + v].x, verts[3 * k + v].y, verts[3 * k + v].z = (float(c) for c in tri[v])
            mats[k].diffuse.x = mats[k].diffuse.y = mats[k].diffuse.z = 0.5
            mats[k].diffuse.w = 1.0
    for t in range(2):
        k = 2 * len(quads) + t
        mats[k] = base.materials[34 + t]
        for v in range(3):
            verts[3 * k + v] = base.vertices[3 * (34 + t) + v]
    return Scene(camera or base.camera, mats, verts, base.light)


def box_quads(c, h, R):
    quads = []
    for f in range(6):
        a, s = f // 2, (1.0 if f % 2 else -1.0)
        i, j = (a + 1) % 3, (a + 2) % 3
        quads.append([c + s * h[a] * R[a] + u * h[i] * R[i] + v * h[j] * R[j]
                      for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return quads


def crossing_scene(w=W, h=H):
    """Quads that cross the plane through the camera perpendicular to the view
    axis: one below the camera from in front of it to behind it, one slanted
    through that plane beside it, and one wholly behind it."""
    c = np.array(list(Scene.cornell_box(w, h).camera.position))
    quads = [[c + d for d in np.array([[-1, -0.6, -3], [1, -0.6, -3], [1, -0.6, 2.0], [-1, -0.6, 2.0]])],
             [c + d for d in np.array([[0.7, -1, -2.5], [0.9, 1, -2.5], [0.4, 1, 1.5], [0.2, -1, 1.5]])],
             [c + d for d in np.array([[-1, -1, 1.0], [1, -1, 1.0], [1, 1, 1.0], [-1, 1, 1.0]])],
             [c + d for d in np.array([[-1.5, -1, -4.0], [1.5, -1, -4.0], [1.5, 1, -4.0], [-1.5, 1, -4.0]])]]
    return quad_scene(quads, w, h)


def inside_box_scene(w=W, h=H, seed=5):
    """The camera inside a rotated box (one box cluster), the room's back wall
    and another box outside it."""
    rng = np.random.default_rng(seed)
    c = np.array(list(Scene.cornell_box(w, h).camera.position))
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    quads = box_quads(c + np.array([0.1, -0.05, -0.3]), np.array([0.8, 0.6, 1.2]), R)
    R2, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    quads += box_quads(c + np.array([0.3, 0.2, -3.0]), np.array([0.4, 0.3, 0.5]), R2)
    quads.append([c + d for d in np.array([[-3, -3, -5.0], [3, -3, -5.0], [3, 3, -5.0], [-3, 3, -5.0]])])
    return quad_scene(quads, w, h)


def random_quad_scene(w, h, n_quads, seed, twist=0.0):
    """The generator of the existing cluster tests (tests/test_gpu_parity.py
    random_quad_scene, the same draws): Cornell camera and light + random
    parallelograms; twist > 0 lifts the 4th corner of every other quad off its
    plane (such a pair is in no box cluster)."""
    rng = np.random.default_rng(seed)
    quads = []
    for q in range(n_quads):
        c = rng.uniform(-2.2, 2.2, 3)
        a, b = rng.normal(size=3), rng.normal(size=3)
        a *= rng.uniform(0.05, 1.5) / np.linalg.norm(a)
        b *= rng.uniform(0.05, 1.5) / np.linalg.norm(b)
        P = [c, c + a, c + a + b, c + b]
        if twist and q % 2:
            P[3] = P[3] + twist * np.cross(a, b) / np.linalg.norm(np.cross(a, b))
        quads.append(P)
        rng.uniform(0.1, 0.9, 3), rng.uniform(0.1, 0.9, 3)  # the generator's two colour draws
    return quad_scene(quads, w, h)


def parallelogram_scene(seed, twist=0.0):
    return random_quad_scene(W, H, 14, seed, twist=twist)


def test_cornell_candidates_are_conservative():
    check_scene(Scene.cornell_box(W, H), 1, per_shape=24)


@pytest.mark.parametrize("seed", [0, 1])
def test_rotated_boxes_candidates_are_conservative(seed):
    check_scene(Scene.random_boxes(W, H, 4, seed=seed), 10 + seed)


@pytest.mark.parametrize("seed,twist", [(1, 0.0), (4, 0.2)])
def test_parallelogram_candidates_are_conservative(seed, twist):
    s = parallelogram_scene(seed, twist)
    if twist:
        assert s.describe()["pair_free_mask"] != 0  # pairs in no cluster go through the same test
    check_scene(s, 20 + seed)


def test_quad_across_the_camera_plane_stays_a_candidate():
    s = crossing_scene()
    check_scene(s, 30)
    # the fallback itself: the crossing quads are kept for every rectangle
    for rect in ((0, 3, 0, 3), (32, 35, 20, 23), (64, 71, 40, 47)):
        assert candidates(s, *rect)[0:4].all()


def test_camera_inside_a_box_cluster():
    s = inside_box_scene()
    assert s.describe()["n_box_clusters"] >= 2
    check_scene(s, 40)


# ---- the check can fail, and the mask is tight ---------------------------------

def _tile_ids(ids, tx, ty, reach=0):
    return ids[max(0, 4 * (ty - reach)):4 * (ty + reach + 1), max(0, 4 * (tx - reach)):4 * (tx + reach + 1)]


def test_a_tile_two_tiles_away_hits_a_triangle_the_mask_leaves_out():
    """Negative control: on a box silhouette of the Cornell frame, the mask of
    one 4x4 tile checked with the rays of the tile two tiles beside it must
    show an accepted triangle it leaves out (the property above is not
    vacuous)."""
    s = Scene.cornell_box(W, H)
    ids = oracle_lib.primary_ids(s)
    tr, rng = Tracer(s), np.random.default_rng(7)
    found = 0
    for ty in range(H // 4):
        for tx in range(2, W // 4 - 2):
            here = np.unique(_tile_ids(ids, tx, ty))
            if not ((here >= 10) & (here < 34)).any() or not (here < 10).any():
                continue  # not a box silhouette against a wall
            may = candidates(s, 4 * tx, 4 * tx + 3, 4 * ty, 4 * ty + 3)
            left_out = np.flatnonzero(may == 0)
            for ox in (tx - 2, tx + 2):
                xs, ys = list(range(4 * ox, 4 * ox + 4)), list(range(4 * ty, 4 * ty + 4))
                if any(tr.accepted(*ray, left_out) for ray in tile_rays(xs, ys, rng, 50)):
                    found += 1
                    break
    assert found >= 1, "no silhouette tile whose neighbour two tiles away sees a left-out triangle"


def test_wall_only_tiles_keep_exactly_one_pair():
    """A 4x4 tile whose 3x3-tile neighbourhood shows one room wall at every
    pixel centre keeps that wall's pair and nothing else."""
    s = Scene.cornell_box(W, H)
    ids = oracle_lib.primary_ids(s)
    seen = 0
    for ty in range(1, H // 4 - 1):
        for tx in range(1, W // 4 - 1):
            near = np.unique(_tile_ids(ids, tx, ty, reach=1) // 2)
            if len(near) != 1 or not 0 <= near[0] < 5:
                continue
            may = candidates(s, 4 * tx, 4 * tx + 3, 4 * ty, 4 * ty + 3)
            assert np.flatnonzero(may).tolist() == [2 * near[0], 2 * near[0] + 1], (tx, ty, may.tolist())
            seen += 1
    assert seen >= 3, "the frame has wall-only neighbourhoods"
