"""Scenes of tests/test_lean_filter.py and tests/test_gpu_lean_filter.py
(DESIGN.md §3.19): Cornell, Scene.random_boxes with 1 to 4 boxes, and hand-built
rooms that hold each cluster kind of the lean filter and each case in which the
scene compiler must withhold a kind."""
import ctypes

import numpy as np

from closest_order_scenes import _box_quads, _rot_y, room_with_quads

# cluster flag bits (gpuraytracer_amd/csrc/rt_cluorder.hpp)
CONTAINER, SINGLE, TURNED, INSIDE, OWN_LIGHT = 8, 16, 32, 64, 128


def _rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def one_box(R, width=64, height=48, center=(0.3, -0.9, 0.2), half=(0.7, 0.6, 0.5)):
    """The room and one box with axes R (rows)."""
    return room_with_quads(width, height, _box_quads(center, half, R), [(0.7, 0.6, 0.3)] * 6)


def _copy_camera(cam):
    return type(cam).from_buffer_copy(bytes(cam))


def outside(width=64, height=48):
    """The camera moved back and up, out of the room, and a box in front of the
    room's open side: rays that start on that box start outside the container."""
    s = room_with_quads(width, height, _box_quads((0.2, -0.8, 4.0), (0.5, 0.6, 0.4), _rot_y(30.0)),
                        [(0.4, 0.7, 0.5)] * 6)
    cam = _copy_camera(s.camera)
    cam.position.z += 3.0
    cam.position.y += 0.5
    s.camera = cam
    return s


def second_emitter(width=64, height=48, drop=5e-4):
    """An emissive quad `drop` below the plane the light samples are drawn
    from, wider than the light, in a cluster of its own (a turned box follows it
    in the pair list, so neither the room nor the light can take it in)."""
    base = room_with_quads(width, height, [], [])
    ly, lx, lz = base.light.center.y, base.light.center.x, base.light.center.z
    y = float(np.float32(ly) - np.float32(drop))
    quad = [np.array(p) for p in ((lx - 0.6, y, lz - 0.6), (lx + 0.6, y, lz - 0.6),
                                   (lx + 0.6, y, lz + 0.6), (lx - 0.6, y, lz + 0.6))]
    s = room_with_quads(width, height, [quad] + _box_quads((0.2, -1.0, 0.1), (0.6, 0.7, 0.5), _rot_y(20.0)),
                        [(0.5, 0.5, 0.5)] * 7)
    n = s.n_triangles
    # the quad's two triangles (ids 10, 11) get the light's material
    ctypes.memmove(ctypes.addressof(s.materials) + 10 * 48, ctypes.addressof(s.materials) + (n - 2) * 48, 96)
    return s


def light_at_minus_zero(width=64, height=48):
    """The light, and its centre, at y = -0.0 (the kernel then takes the
    literal sample expression, not the light_plain one)."""
    s = one_box(_rot_y(20.0), width, height, center=(0.2, -1.5, 0.1), half=(0.6, 0.5, 0.5))
    n = s.n_triangles
    vv = np.frombuffer(s.vertices, np.float32).reshape(-1, 4)
    vv[3 * (n - 2):3 * n, 1] = -0.0
    light = type(s.light).from_buffer_copy(bytes(s.light))
    light.center.y = -0.0
    s.light = light
    return s


def scenes(width=64, height=48):
    """name -> builder of every scene of the two tests."""
    from gpuraytracer_amd import Scene

    s = {"cornell": lambda: Scene.cornell_box(width, height),
         "turned_0deg": lambda: one_box(_rot_y(0.0), width, height),
         "turned_90deg": lambda: one_box(_rot_y(90.0), width, height),
         "turned_y_minus": lambda: one_box(_rot_y(-33.0), width, height),
         "turned_x": lambda: one_box(_rot_x(25.0), width, height),
         "turned_z": lambda: one_box(_rot_z(-40.0), width, height),
         "tilted": lambda: one_box(_rot_x(15.0) @ _rot_y(25.0), width, height),
         "outside": lambda: outside(width, height),
         "second_emitter": lambda: second_emitter(width, height),
         "light_minus_zero": lambda: light_at_minus_zero(width, height)}
    for n in range(1, 5):
        s[f"boxes{n}"] = (lambda n=n: Scene.random_boxes(width, height, n, seed=n))
    return s


def kinds(scene):
    """The cluster flag words of a scene as a sorted list of their kind bits."""
    return sorted(f & (CONTAINER | SINGLE | TURNED | INSIDE | OWN_LIGHT) for f in scene.cluster_kinds())
