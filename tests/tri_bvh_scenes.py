"""Triangle-only scenes for the triangle-BVH builders (tests/test_tri_bvh_tree.py,
tests/test_gpu_tri_bvh_tree.py): the Cornell camera and light, no room, the
materials of test_gpu_parity.triangle_soup (diffuse albedo in [0.1, 0.9],
roughness 0.5, nothing emissive).  Each scene is an input a builder can get
wrong without a render of random small triangles noticing:

  tiny1, tiny2, tiny3   the smallest trees (n == 1 has its own paths)
  soup385               one past the 384-triangle threshold of the BVH layout
  soup1023/1024/1025    counts that straddle a 256-thread block
  grid                  20 x 20 quads in the plane y = -1: shared edges and
                        vertices, zero extent on y, every box of zero thickness
  cell                  600 distinct triangles of size ~1e-4 in a cube of side
                        5e-4 in the middle of one 10-bit Morton cell (one SAH
                        centroid bin of the root), and 8 at the corners of
                        [-2.4, 2.4]^3
  same600               600 copies of one triangle
  far                   400 triangles out to |coordinate| ~7000 (fp16 ulp 4)
                        and 100 near the origin
  past_half             the same out to 7e4, beyond the largest finite fp16
  soup20k               20,000 triangles: 79 workgroups of 256 (structure only)
"""
import ctypes
import functools

import numpy as np

from gpuraytracer_amd import MaterialGPU, Options, Scene, float3

W, H = 40, 24
f32 = np.float32
NAMES = ["tiny1", "tiny2", "tiny3", "soup385", "soup1023", "soup1024", "soup1025", "grid", "cell", "same600",
         "far", "past_half", "soup20k"]
BVH_MIN = 384  # rt_create takes the triangle BVH above this count by itself


def _soup(rng, n, centre=2.3, edge=0.25):
    c = rng.uniform(-centre, centre, size=(n, 1, 3)).astype(f32)
    e = rng.uniform(-edge, edge, size=(n, 2, 3)).astype(f32)
    return np.concatenate([c, c + e], axis=1)


def _grid():
    t = []
    x = (-2.0 + 0.2 * np.arange(21)).astype(f32)
    for i in range(20):
        for j in range(20):
            p = [(x[i + a], f32(-1.0), x[j + b]) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
            t += [(p[0], p[2], p[1]), (p[0], p[3], p[2])]  # normals up, towards the light
    return np.array(t, f32)


def _cell(rng):
    # the middle of Morton cell (576, 500, 430) of a scene spanning [-2.4, 2.4]^3
    mid = -2.4 + 4.8 * (np.array([576, 500, 430]) + 0.5) / 1024
    c = mid + rng.uniform(-2.0e-4, 2.0e-4, size=(600, 1, 3))
    e = rng.uniform(-0.5e-4, 0.5e-4, size=(600, 2, 3))
    small = np.concatenate([c, c + e], axis=1).astype(f32)
    corners = []
    for k in range(8):
        s = np.array([1.0 if (k >> a) & 1 else -1.0 for a in range(3)])
        v = 2.4 * s
        corners.append((v, v - s * (0.2, 0.0, 0.1), v - s * (0.0, 0.2, 0.15)))
    return np.concatenate([small, np.array(corners, f32)])


def _far(rng, scale):
    return np.concatenate([_soup(rng, 400, 6800.0 * scale, 200.0 * scale), _soup(rng, 100)])


def triangles(name):
    """(n, 3, 3) float32 vertices of the scene ``name``."""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("tiny"):
        return _soup(np.random.default_rng(11), 3, 1.0, 0.5)[:int(name[4:])]
    if name.startswith("soup"):
        return _soup(rng, int(name[4:].replace("k", "000")))
    if name == "grid":
        return _grid()
    if name == "cell":
        return _cell(rng)
    if name == "same600":
        return np.tile(np.array([[(0.1, -0.5, 0.2), (0.35, -0.45, 0.25), (0.15, -0.2, 0.1)]], f32), (600, 1, 1))
    if name == "far":
        return _far(rng, 1.0)
    assert name == "past_half", name
    return _far(rng, 10.0)


@functools.lru_cache(maxsize=None)
def build(name, width=W, height=H):
    base = Scene.cornell_box(width, height)
    tri = triangles(name)
    n = len(tri)
    mats = (MaterialGPU * n)()
    verts = (float3 * (3 * n))()
    np.frombuffer(verts, f32).reshape(-1, 4)[:, :3] = tri.reshape(-1, 3)
    mm = np.frombuffer(mats, f32).reshape(-1, 12)
    mm[:, 0:3] = np.random.default_rng(n).uniform(0.1, 0.9, size=(n, 3)).astype(f32)
    mm[:, 3] = 1.0
    mm[:, 5] = 0.5
    assert ctypes.sizeof(mats) == 48 * n
    return Scene(base.camera, mats, verts, base.light)


def options(name, **kw):
    """The options of a context for ``name``: the BVH layout by name where
    rt_create would not take it by itself (n <= 384)."""
    n = len(triangles(name))
    return Options(layout="bvh" if n <= BVH_MIN else "auto", **kw)
