"""Scenes of tests/test_light_mask.py and tests/test_gpu_light_mask.py
(DESIGN.md §3.21): quads whose two triangles differ in the light flag or in
colour, next to the scenes of tests/lean_filter_scenes.py."""
import ctypes

import numpy as np

from closest_order_scenes import _box_quads, _rot_y, room_with_quads


def _quad_and_box(width, height, colors):
    """The room, one horizontal quad (triangles 10, 11) in mid-air, a turned
    box after it (triangles 12-23) and the light."""
    quad = [np.array(p) for p in ((-1.4, 0.3, -0.8), (-0.2, 0.3, -0.8), (-0.2, 0.3, 0.4), (-1.4, 0.3, 0.4))]
    return room_with_quads(width, height, [quad] + _box_quads((0.6, -1.2, 0.1), (0.6, 0.7, 0.5), _rot_y(20.0)),
                           colors)


def half_light_quad(width=64, height=48):
    """A quad whose triangle A (id 10) carries the light's material and whose
    triangle B (id 11) a diffuse one: one pair, two light bits."""
    s = _quad_and_box(width, height, [(0.5, 0.5, 0.5)] * 7)
    n = s.n_triangles
    ctypes.memmove(ctypes.addressof(s.materials) + 10 * 48, ctypes.addressof(s.materials) + (n - 2) * 48, 48)
    return s


def two_colour_quad(width=64, height=48):
    """A quad whose two triangles have different diffuse colours."""
    s = _quad_and_box(width, height, [(0.5, 0.5, 0.5)] * 7)
    mm = np.frombuffer(s.materials, np.float32).reshape(-1, 12)
    mm[10, 0:3] = (0.8, 0.3, 0.2)
    mm[11, 0:3] = (0.2, 0.4, 0.8)
    return s


def emissive_ids(scene):
    """Triangle ids whose material emits (raytrace.metal:57: length(emissive) > 0)."""
    mm = np.frombuffer(scene.materials, np.float32).reshape(-1, 12)
    return [k for k in range(scene.n_triangles) if np.any(mm[k, 8:11] != 0.0)]
