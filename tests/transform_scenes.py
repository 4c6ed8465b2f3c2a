"""Similarity transforms of whole scenes for tests/test_transforms.py and
tests/test_gpu_transforms.py: the geometry, the camera and the
light moved together.  Every box-cluster scene of the suite is the Cornell room
world-aligned about the origin, about 5 units across, and the headline path is
full of constants that mean something only there: the reference's tmin = 1e-3,
tmax = 1000 and N * 1e-3 lift, the extent floor 2.5 of the culling margin, the
tolerances of build_clusters relative to max(1, extent), the own-light flag
withheld above extent 256, the exact c == +-1 test for world axes.

``transformed(scene, s, R, t)`` maps every point p to R (s p) + t in float64
and rounds each value to fp32 once; equal input vertices give equal output
bits, so the shared-vertex pairs of the scene compiler (which compares bits)
survive.  An image under a transform is NOT the image of the control: the
reference's constants do not move with the scene.  Each transformed scene is
compared with the oracle on the same transformed scene.

TRANSFORMS (s, R, t):

  id         the control; ``apply`` returns the scene itself
  half       s = 1/2: an exact scale, every mantissa kept; extent 1.25 is under the floor 2.5
  x1_16      s = 1.16: near 1 and no power of two, every vertex rounds anew
  tiny       s = 2^-10: the room is 5e-3 across, tmin and the 1e-3 lift are as large as it
  x37        s = 37: extent 92, camera at 333; the whole room still inside tmax
  x100       s = 100: the camera at 900 and the back wall at 1150, beyond tmax = 1000
  x103       s = 103: extent 257.5 > 256, the own-light flag is withheld by extent
  offset     t = (40, -25, 60): vertices round at 2^-18 .. 2^-19, a box splits into partial clusters
  offset900  t = (900, 0, 0): x rounds at 2^-14; many single-face clusters, no own-light
  perm       (x, y, z) -> (x, -z, y) exactly: world axes kept, the light's quad leaves the
             xz plane its samples are drawn in (the flip branch of the exact-axis test)
  roty30     30 degrees about y: the room is turned about one world axis, no container
  rot123     40 degrees about (1, 2, 3): nothing is world-aligned
  rot_tiny   1e-4 rad about z: just off the exact-axis tests
  x100rot    s = 100, rot123, t = (30, 10, -20): all three at once

``x150`` is left out.  At s = 150 the camera sits 975 from the room's open
side and every surface lies beyond tmax: the frame is the all-miss frame
(lit share 0.00), which ``away`` of tests/pose_scenes.py already pins on every
kernel, and nothing of the scene is exercised.
"""
import functools
import math

import numpy as np

from gpuraytracer_amd import CameraGPU, Scene, SquareLightGPU

f32 = np.float32
W, H = 64, 48                       # the GPU tests' frame


def _axis_angle(axis, rad):
    """The rotation by ``rad`` about ``axis`` (Rodrigues), float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(rad) * K + (1.0 - math.cos(rad)) * (K @ K)


I3 = np.eye(3)
PERM = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # (x, y, z) -> (x, -z, y)
ROT123 = _axis_angle((1, 2, 3), math.radians(40.0))

TRANSFORMS = {
    "id": None,
    "half": dict(s=0.5),
    "x1_16": dict(s=1.16),
    "tiny": dict(s=2.0 ** -10),
    "x37": dict(s=37.0),
    "x100": dict(s=100.0),
    "x103": dict(s=103.0),
    "offset": dict(t=(40.0, -25.0, 60.0)),
    "offset900": dict(t=(900.0, 0.0, 0.0)),
    "perm": dict(R=PERM),
    "roty30": dict(R=_axis_angle((0, 1, 0), math.radians(30.0))),
    "rot123": dict(R=ROT123),
    "rot_tiny": dict(R=_axis_angle((0, 0, 1), 1e-4)),
    "x100rot": dict(s=100.0, R=ROT123, t=(30.0, 10.0, -20.0)),
}
SCALES = ["half", "x1_16", "tiny", "x37", "x100", "x103"]
OFFSETS = ["offset", "offset900"]
ROTATIONS = ["perm", "roty30", "rot123", "rot_tiny"]
MOVED = [k for k in TRANSFORMS if k != "id"]
# the transforms at which the reference's own clamps, the extent rule, the
# coarse rounding and the axis tests bite hardest: what the entry points other
# than rt_render run at
KEY = ["tiny", "x100", "x103", "offset900", "perm", "rot123"]
# the four at which the MIS oracle, the lane forms and the interleaved rows run
CORE = ["tiny", "x100", "offset900", "rot123"]


def _map(p, s, R, t, translate=True):
    """R (s p) + t of the rows of ``p`` (n, 3), float64, elementwise products
    and sums in a fixed order: equal rows give equal bits."""
    p = np.asarray(p, np.float64) * (s if translate else 1.0)
    out = np.empty_like(p)
    for i in range(3):
        out[:, i] = (R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]
        if translate:
            out[:, i] += t[i]
    return out


def _set3(field, v):
    field.x, field.y, field.z = (float(f32(c)) for c in v)


def _get3(field):
    return np.array([[field.x, field.y, field.z]], np.float64)


def transformed(scene, s=1.0, R=None, t=(0.0, 0.0, 0.0)):
    """A new Scene: every vertex, sphere centre, the camera position and the
    light centre at R (s p) + t, sphere radii s r, the camera's direction and
    up rotated by R; computed in float64, each value rounded to fp32 once.
    Materials are shared; resolution, fov and the light's width / depth stay."""
    R = I3 if R is None else np.asarray(R, np.float64)
    s, t = float(s), np.asarray(t, np.float64)
    verts = type(scene.vertices).from_buffer_copy(scene.vertices)
    vv = np.frombuffer(verts, f32).reshape(-1, 4)
    vv[:, :3] = _map(vv[:, :3], s, R, t).astype(f32)
    spheres = None
    if scene.spheres is not None:
        spheres = type(scene.spheres).from_buffer_copy(scene.spheres)
        ss = np.frombuffer(spheres, f32).reshape(-1, 20)
        ss[:, 0:3] = _map(ss[:, 0:3], s, R, t).astype(f32)
        ss[:, 16] = (ss[:, 16].astype(np.float64) * s).astype(f32)
    cam = CameraGPU.from_buffer_copy(scene.camera)
    _set3(cam.position, _map(_get3(cam.position), s, R, t)[0])
    _set3(cam.direction, _map(_get3(cam.direction), s, R, t, translate=False)[0])
    _set3(cam.up, _map(_get3(cam.up), s, R, t, translate=False)[0])
    light = SquareLightGPU.from_buffer_copy(scene.light)
    _set3(light.center, _map(_get3(light.center), s, R, t)[0])
    return Scene(cam, scene.materials, verts, light, spheres)


def apply(scene, name):
    """``scene`` under the transform of that name (``id``: the scene itself)."""
    kw = TRANSFORMS[name]
    return scene if kw is None else transformed(scene, **kw)


def extent(scene):
    """max |coordinate| over the vertices, the sphere bounds and nothing else."""
    e = float(np.abs(np.frombuffer(scene.vertices, f32).reshape(-1, 4)[:, :3]).max())
    if scene.spheres is not None:
        ss = np.frombuffer(scene.spheres, f32).reshape(-1, 20)
        e = max(e, float((np.abs(ss[:, 0:3]) + np.abs(ss[:, 16:17])).max()))
    return e


def point(name, p):
    """One point under the transform of that name, rounded to fp32."""
    kw = TRANSFORMS[name] or {}
    R = I3 if kw.get("R") is None else np.asarray(kw["R"], np.float64)
    return tuple(float(c) for c in _map(np.asarray([p], np.float64), float(kw.get("s", 1.0)), R,
                                        np.asarray(kw.get("t", (0.0, 0.0, 0.0)), np.float64))[0].astype(f32))


@functools.lru_cache(maxsize=None)
def rays_bc(name):
    """Sets B and C of tests/ray_sets.py with the scene: the same draws (numpy
    PCG64, seed 2024), the origins and end points mapped by the transform and
    rounded to fp32, B's directions rotated and normalised in fp32, C's formed
    from the mapped points; tmin, tmax = 1000 and the 1e-3 cut of C's segments
    are the reference's own and stay.  So the origin bounds follow the scene's
    extent and the sets stay inside the exactness domain."""
    import ray_sets
    if TRANSFORMS[name] is None:
        return ray_sets.sets_bc()
    kw = TRANSFORMS[name]
    R = I3 if kw.get("R") is None else np.asarray(kw["R"], np.float64)
    s, t = float(kw.get("s", 1.0)), np.asarray(kw.get("t", (0.0, 0.0, 0.0)), np.float64)
    rng = np.random.default_rng(2024)
    o = _map(rng.uniform(-2.4, 2.4, (ray_sets.N, 3)).astype(f32), s, R, t).astype(f32)
    g = _map(rng.standard_normal((ray_sets.N, 3)).astype(f32), s, R, t, translate=False).astype(f32)
    d = g / np.sqrt(np.sum(g * g, axis=1, dtype=f32))[:, None]
    B = ray_sets.pack(o, d, f32(0.001), f32(1000.0))
    q = _map(rng.uniform(-2.4, 2.4, (ray_sets.N, 3)).astype(f32), s, R, t).astype(f32)
    L = q - o
    dist = np.sqrt(np.sum(L * L, axis=1, dtype=f32))
    C = ray_sets.pack(o, L / dist[:, None], f32(0.0), dist - f32(1e-3))
    return B, C
