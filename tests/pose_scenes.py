"""Camera poses and light positions for tests/test_poses.py and
tests/test_gpu_poses.py: views that the conservative shortcuts
of the render kernels -- beam masks, light shafts, the wave-mask table, dead
waves, the own-light skip, the octant layouts of the BVH walks, the
camera-scaled margin -- never meet at the Cornell camera (0, 0, 9) -> -z with
the light at the ceiling centre.

POSES (``eye -> look_at`` gives direction = look_at - eye, not normalised):

  cornell          unchanged (control)
  behind_left      eye (-7, 1.5, -8) -> (0, 0, 0): behind the back wall
  rolled           up (3, 4, 0), not a unit vector
  diag_roll        eye (5, 4, 7) -> (0, -0.5, -0.5), up (0.3, 1, -0.2)
  narrow_far       eye (0, 0, 900), fov 0.5 degrees
  wall_plane       eye (-2.5, 0, 4) -> (1, -1, -1): the apex in the left wall's plane
  up_from_floor    eye (0.3, -2.2, 0.4) -> (0.1, 2.5, -0.2), up (0, 0, -1)
  straight_down    eye (0.2, 2.2, 0.1), direction exactly (0, -1, 0), up (0, 0, -1)
  wide             eye (0, 0, 2), fov 170 degrees
  inside_tall_box  eye = mean of the vertices of triangles 22-33 -> (0.5, 0.3, 3)
  away             direction (0, 0, +1): sees nothing
  oct0 .. oct7     eye (+-6, +-5, +-7) -> (0, 0, 0), up (0.2, 1, 0.1): octK's
                   centre ray lies in BVH octant K (bit a set: component a < 0)
  aspect3          diag_roll on a 72 x 24 frame (FRAME): integer aspectRatio 3

INSIDE poses have the eye inside the room (or inside a box in it): every pair
has a corner behind the camera plane or the shafts decide nothing.  OUTSIDE
poses look at the room from outside.  ``away`` is neither.

LIGHTS move SquareLightGPU.center only; the emissive quad stays in the ceiling:

  ceiling        unchanged (0, 2.49, 0) (control)
  low            (0.8, -1.0, 0.5): shadow segments go down from everything above
                 it, the own-light flag is withheld
  outside        (6, 1, 3): outside the room
  ceiling_plane  (1.7, 2.5, -1.7): coplanar with the ceiling wall, not with the
                 emissive quad.  Checked on the CPU: its oracle frame on the
                 Cornell scene (70 x 45, 2 spp, 3 bounces) is NaN-free with
                 0.80 of the pixels lit (tests/test_poses.py asserts >= 0.10);
                 the position stayed as first chosen.
"""
import math

import numpy as np

from gpuraytracer_amd import CameraGPU, Scene, SquareLightGPU

f32 = np.float32
W, H = 64, 48                       # the GPU tests' frame (aspect 1)
FRAME = {"aspect3": (72, 24)}       # poses with a frame of their own


def _set3(field, v):
    field.x, field.y, field.z = (float(f32(c)) for c in v)


def posed(scene, eye=None, look_at=None, direction=None, up=None, fov=None):
    """``scene`` seen from another camera: materials, vertices, light and
    spheres shared, the CameraGPU a copy (the resolution stays)."""
    assert look_at is None or direction is None
    cam = CameraGPU.from_buffer_copy(scene.camera)
    if eye is not None:
        _set3(cam.position, eye)
    if look_at is not None:
        e = np.array([cam.position.x, cam.position.y, cam.position.z], f32)
        _set3(cam.direction, np.array(look_at, f32) - e)
    if direction is not None:
        _set3(cam.direction, direction)
    if up is not None:
        _set3(cam.up, up)
    if fov is not None:
        cam.horizontalFov = float(f32(fov))
    return Scene(cam, scene.materials, scene.vertices, scene.light, scene.spheres)


def lit(scene, center):
    """``scene`` with the light's centre at ``center``: everything else shared."""
    light = SquareLightGPU.from_buffer_copy(scene.light)
    _set3(light.center, center)
    return Scene(scene.camera, scene.materials, scene.vertices, light, scene.spheres)


def _tall_box_centre():
    s = Scene.cornell_box(W, H)
    v = np.frombuffer(s.vertices, f32).reshape(-1, 4)[3 * 22:3 * 34, :3]
    return tuple(float(c) for c in v.astype(np.float64).mean(axis=0).astype(f32))


POSES = {
    "cornell": {},
    "behind_left": dict(eye=(-7, 1.5, -8), look_at=(0, 0, 0)),
    "rolled": dict(up=(3, 4, 0)),
    "diag_roll": dict(eye=(5, 4, 7), look_at=(0, -0.5, -0.5), up=(0.3, 1, -0.2)),
    "narrow_far": dict(eye=(0, 0, 900), fov=math.radians(0.5)),
    "wall_plane": dict(eye=(-2.5, 0, 4), look_at=(1, -1, -1)),
    "up_from_floor": dict(eye=(0.3, -2.2, 0.4), look_at=(0.1, 2.5, -0.2), up=(0, 0, -1)),
    "straight_down": dict(eye=(0.2, 2.2, 0.1), direction=(0, -1, 0), up=(0, 0, -1)),
    "wide": dict(eye=(0, 0, 2), fov=math.radians(170)),
    "inside_tall_box": dict(eye=_tall_box_centre(), look_at=(0.5, 0.3, 3)),
    "away": dict(direction=(0, 0, 1)),
}
# octK: the centre ray points from the eye to the origin, so component a of it is
# negative where the eye's is positive
OCTANTS = {f"oct{k}": dict(eye=(6 if k & 1 else -6, 5 if k & 2 else -5, 7 if k & 4 else -7),
                           look_at=(0, 0, 0), up=(0.2, 1, 0.1)) for k in range(8)}
POSES.update(OCTANTS)
POSES["aspect3"] = POSES["diag_roll"]

OUTSIDE = ["cornell", "behind_left", "rolled", "diag_roll", "narrow_far", "wall_plane"] + list(OCTANTS)
INSIDE = ["up_from_floor", "straight_down", "wide", "inside_tall_box"]
MAIN = [p for p in POSES if p not in OCTANTS and p != "aspect3"]   # the poses of the 64 x 48 table

LIGHTS = {
    "ceiling": (0.0, 2.49, 0.0),
    "low": (0.8, -1.0, 0.5),
    "outside": (6.0, 1.0, 3.0),
    "ceiling_plane": (1.7, 2.5, -1.7),
}
MOVED_LIGHTS = [k for k in LIGHTS if k != "ceiling"]


def frame_of(pose):
    return FRAME.get(pose, (W, H))


def view(scene, pose="cornell", light="ceiling"):
    """``scene`` at the pose and light of those names (the scene's own where unchanged)."""
    s = posed(scene, **POSES[pose]) if POSES[pose] else scene
    return s if light == "ceiling" else lit(s, LIGHTS[light])
