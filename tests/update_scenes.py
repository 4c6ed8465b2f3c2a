"""Updated scenes for rt_update_scene (tests/test_update_scene.py,
tests/test_gpu_update_scene.py): each is derived from a scene of
tests/tri_bvh_scenes.py -- the same triangle count, materials, light and
resolution -- so that a tree built for the one can be refitted onto the other:

  same      unchanged
  shift     translated by (0.3, -0.2, 0.1)
  grow      scaled 1.7 about the origin: the extent and so the margin grow
  shrink    scaled 0.5
  shuffle   triangle k takes the vertices of triangle pi(k), a fixed random
            permutation: the kept topology means nothing, every box is huge
  collapse  all vertices in one point: zero-area triangles, zero-size boxes
  to_far    four fifths of the triangles out to |coordinate| ~7e4 (the
            coordinates of tri_bvh_scenes ``past_half``): planes past the
            largest finite fp16 appear through the refit as +-inf

Every kind but ``same`` also moves the camera (another position and look-at,
the same resolution); ``same`` is the scene of tri_bvh_scenes itself."""
import ctypes
import functools

import numpy as np

import tri_bvh_scenes as ts
from gpuraytracer_amd import CameraGPU, MaterialGPU, Scene, float3

f32 = np.float32
KINDS = ["same", "shift", "grow", "shrink", "shuffle", "collapse", "to_far"]
MOVED = [k for k in KINDS if k != "same"]


def moved_camera(camera, eye=(0.6, 0.4, 6.5), look_at=(-0.3, -0.2, 0.0)):
    """A copy of ``camera`` at ``eye`` looking at ``look_at``: the resolution, fov and up stay."""
    cam = CameraGPU()
    ctypes.memmove(ctypes.addressof(cam), ctypes.addressof(camera), ctypes.sizeof(CameraGPU))
    e, t = np.array(eye, f32), np.array(look_at, f32)
    d = t - e
    cam.position.x, cam.position.y, cam.position.z = (float(v) for v in e)
    cam.direction.x, cam.direction.y, cam.direction.z = (float(v) for v in d)
    return cam


def vertices(name, kind):
    """(n, 3, 3) float32: the triangles of ``tri_bvh_scenes.triangles(name)`` after ``kind``."""
    tri = ts.triangles(name).copy()
    n = len(tri)
    rng = np.random.default_rng(1000 + sum(kind.encode()) + n)
    if kind == "same":
        return tri
    if kind == "shift":
        return (tri + np.array([0.3, -0.2, 0.1], f32)).astype(f32)
    if kind == "grow":
        return (tri * f32(1.7)).astype(f32)
    if kind == "shrink":
        return (tri * f32(0.5)).astype(f32)
    if kind == "shuffle":
        return tri[rng.permutation(n)]
    if kind == "collapse":
        return np.broadcast_to(np.array([0.25, -0.5, 0.125], f32), tri.shape).copy()
    assert kind == "to_far", kind
    m = (4 * n) // 5
    tri[:m] = ts._soup(rng, m, 6800.0 * 10.0, 200.0 * 10.0)
    return tri


def with_vertices(scene, tri, camera=None):
    """``scene`` with the (n, 3, 3) vertices ``tri`` (and ``camera``): materials and light shared."""
    n = scene.n_triangles
    assert tri.shape == (n, 3, 3)
    verts = (float3 * (3 * n))()
    np.frombuffer(verts, f32).reshape(-1, 4)[:, :3] = np.asarray(tri, f32).reshape(-1, 3)
    return Scene(scene.camera if camera is None else camera, scene.materials, verts, scene.light, scene.spheres)


@functools.lru_cache(maxsize=None)
def build(name, kind):
    """The scene ``name`` of tri_bvh_scenes after ``kind``."""
    base = ts.build(name)
    if kind == "same":
        return base
    return with_vertices(base, vertices(name, kind), moved_camera(base.camera))


def recolored(scene, triangles, rgb):
    """A copy of ``scene``'s materials with the diffuse colour of ``triangles`` set to ``rgb``."""
    n = scene.n_triangles
    mats = (MaterialGPU * n)()
    ctypes.memmove(ctypes.addressof(mats), ctypes.addressof(scene.materials), 48 * n)
    mm = np.frombuffer(mats, f32).reshape(-1, 12)
    mm[list(triangles), 0:3] = np.array(rgb, f32)
    return mats
