"""Scenes of tests/test_closest_order.py and tests/test_gpu_closest_order.py
(DESIGN.md §3.18): the Cornell scenes, Scene.random_boxes, and three hand-built
ones -- the Cornell room plus boxes placed so that the order of a closest
query's candidates matters."""
import ctypes

import numpy as np


def _rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _box_quads(center, half, R):
    """The six faces of a box as quads of four corners (rows of R: its axes)."""
    c, h = np.asarray(center, float), np.asarray(half, float)
    quads = []
    for f in range(6):
        a, s = f // 2, (1.0 if f % 2 else -1.0)
        i, j = (a + 1) % 3, (a + 2) % 3
        quads.append([c + s * h[a] * R[a] + u * h[i] * R[i] + v * h[j] * R[j]
                      for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return quads


def room_with_quads(width, height, quads, colors):
    """The Cornell room (walls = triangles 0-9), then one shared-edge triangle
    pair per quad, then the light rectangle (as Scene.random_boxes lays out)."""
    from gpuraytracer_amd import Scene
    from gpuraytracer_amd._native import MaterialGPU, float3

    base = Scene.cornell_box(width, height)
    n = 10 + 2 * len(quads) + 2
    mats = (MaterialGPU * n)()
    verts = (float3 * (3 * n))()
    ctypes.memmove(ctypes.addressof(mats), ctypes.addressof(base.materials), 10 * 48)
    ctypes.memmove(ctypes.addressof(verts), ctypes.addressof(base.vertices), 30 * 16)
    vv = np.frombuffer(verts, np.float32).reshape(-1, 4)
    mm = np.frombuffer(mats, np.float32).reshape(-1, 12)
    for q, (P, col) in enumerate(zip(quads, colors)):
        for t, tri in enumerate(((P[0], P[1], P[2]), (P[0], P[2], P[3]))):
            k = 10 + 2 * q + t
            vv[3 * k:3 * k + 3, :3] = np.array(tri, np.float32)
            mm[k, 0:3] = col
            mm[k, 3] = 1.0
            mm[k, 5] = 0.5
    ctypes.memmove(ctypes.addressof(mats) + (n - 2) * 48, ctypes.addressof(base.materials) + 34 * 48, 96)
    ctypes.memmove(ctypes.addressof(verts) + 3 * (n - 2) * 16,
                   ctypes.addressof(base.vertices) + 3 * 34 * 16, 96)
    return Scene(base.camera, mats, verts, base.light)


def protruding_box(width=64, height=48):
    """A box that sticks out through the left wall (x = -2.5): its faces go on
    behind the wall, where a ray's entry-side hit lies beyond the wall's."""
    q = _box_quads((-2.3, -0.4, -0.3), (0.7, 0.6, 0.5), _rot_y(20.0))
    return room_with_quads(width, height, q, [(0.3, 0.6, 0.8)] * 6)


def boxes_in_line(width=64, height=48):
    """Two boxes one behind the other along the view axis: a ray's near set
    holds the entry faces of both."""
    q = _box_quads((0.1, -0.8, 1.2), (0.6, 0.7, 0.4), _rot_y(10.0)) + \
        _box_quads((-0.1, -0.6, -0.9), (0.8, 0.9, 0.5), _rot_y(-15.0))
    return room_with_quads(width, height, q, [(0.8, 0.5, 0.2)] * 6 + [(0.2, 0.7, 0.3)] * 6)


def coplanar_quads(width=64, height=48):
    """A box and, in a cluster of its own, a copy of the box's top face: two
    quads in different clusters with the same t for every ray, so the triangle
    id decides."""
    box = _box_quads((0.3, -1.0, 0.2), (0.8, 0.7, 0.6), _rot_y(25.0))
    return room_with_quads(width, height, box + [box[3]], [(0.7, 0.7, 0.2)] * 6 + [(0.9, 0.1, 0.1)])


def scenes(width=64, height=48):
    """name -> builder of every scene of the two tests."""
    from gpuraytracer_amd import Scene

    s = {"cornell": lambda: Scene.cornell_box(width, height),
         "cornell_mis": lambda: Scene.cornell_box_mis(width, height),
         "protruding": lambda: protruding_box(width, height),
         "in_line": lambda: boxes_in_line(width, height),
         "coplanar": lambda: coplanar_quads(width, height)}
    for n in range(1, 7):
        for seed in ((1, 2) if n in (1, 6) else (n,)):
            s[f"boxes{n}_s{seed}"] = (lambda n=n, seed=seed: Scene.random_boxes(width, height, n, seed=seed))
    return s


# Scene.random_boxes with 5 and 6 boxes has 36 and 42 triangle pairs: more than
# the 31 a pair mask holds, so the scene compiler builds no clusters and such a
# scene runs on the pair kernel (rt_scene.cpp build_clusters).
NO_CLUSTERS = {"boxes5_s5", "boxes6_s1", "boxes6_s2"}


def write_scene_file(scene, path):
    """The scene file of tests/native/closest_order_host.hpp."""
    with open(path, "wb") as f:
        f.write(bytes(scene.camera))
        f.write(bytes(scene.light))
        f.write(np.uint32(scene.n_triangles).tobytes())
        f.write(bytes(scene.materials))
        f.write(bytes(scene.vertices))
