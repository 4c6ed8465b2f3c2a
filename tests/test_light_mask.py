"""CPU: the light mask the box-cluster kernel tests instead of loading a hit
triangle's light flag, through the host entry point
rt_debug_light_mask, which reports what rt_render hands the kernel
(rt_scene.cpp light_mask) and the 64-B shading records it is made from: the
mask is the set of emissive triangles computed here from the scene's
materials, equals the records' flag words, and the records' colour and
emissive words are bit copies of the materials."""
import ctypes

import numpy as np
import pytest

import gpuraytracer_amd as g
from gpuraytracer_amd import Scene
from lean_filter_scenes import second_emitter
from light_mask_scenes import emissive_ids, half_light_quad, two_colour_quad

SCENES = {"cornell": lambda: Scene.cornell_box(64, 48),
          "second_emitter": lambda: second_emitter(64, 48),
          "half_light_quad": lambda: half_light_quad(64, 48),
          "two_colour_quad": lambda: two_colour_quad(64, 48)}
for _n in range(1, 5):
    SCENES[f"boxes{_n}"] = (lambda n=_n: Scene.random_boxes(64, 48, n, seed=n))

# name -> the emissive triangle ids
EXPECT = {"cornell": [34, 35], "second_emitter": [10, 11, 24, 25], "half_light_quad": [10, 24, 25],
          "two_colour_quad": [24, 25], "boxes1": [22, 23], "boxes2": [34, 35], "boxes3": [46, 47],
          "boxes4": [58, 59]}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_mask_is_the_set_of_emissive_triangles(name):
    s = SCENES[name]()
    mask, records = s.light_mask()
    lights = emissive_ids(s)
    assert lights == EXPECT[name]
    assert mask == sum(1 << k for k in lights), (name, hex(mask), lights)
    rec = records.view(np.uint32)
    assert rec.shape == (s.n_triangles, 16)
    assert [k for k in range(s.n_triangles) if records[k, 3] != 0.0] == lights
    mm = np.frombuffer(s.materials, np.float32).reshape(-1, 12).view(np.uint32)
    assert np.array_equal(rec[:, [7, 11, 15]], mm[:, 0:3]), "record colour words: the material's diffuse"
    assert np.array_equal(rec[:, 12:15], mm[:, 8:11]), "record emissive words: the material's"


def test_mask_bits_above_31():
    s = Scene.random_boxes(64, 48, 4, seed=4)  # 60 triangles, the light's are 58 and 59
    assert s.light_mask()[0] == (1 << 58) | (1 << 59)


def test_more_than_64_triangles_have_no_mask():
    assert Scene.random_triangles(16, 8, 1000).light_mask()[0] == 0


def test_bad_arguments_are_status_codes():
    m = ctypes.c_uint64()
    d = Scene.cornell_box(16, 8).desc()
    assert g.lib.rt_debug_light_mask(None, ctypes.byref(m), None, 0) == 1
    assert g.lib.rt_debug_light_mask(ctypes.byref(d), None, None, 0) == 1
    assert g.lib.rt_debug_light_mask(ctypes.byref(d), ctypes.byref(m), None, 1) == 1
    assert g.lib.rt_debug_light_mask(ctypes.byref(d), ctypes.byref(m), None, 0) == 0
    assert m.value == 3 << 34
