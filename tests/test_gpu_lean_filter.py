"""GPU: the box-cluster kernel with the lean filter paths (rt_cluorder.hpp
kCluTurned / kCluInside / kCluOwnLight) against the C oracle,
bit for bit on uint32 views: every scene of tests/test_lean_filter.py at 64x48
x 8 spp x 3 bounces -- Cornell, Scene.random_boxes with 1 to 4 boxes, boxes
turned about each world axis, a tilted one, the camera and a box outside the
room (the exit-only path falls back), a second emitter off the sampling plane
and a light at y = -0.0 (the own-light kind withheld) -- Cornell also at 4 and 16
samples (the launcher's other lanes-per-pixel choices) and as a row-interleaved
share.  Every case asserts through rt_last_launch that the box-cluster kernel
ran.  The library has no run-time switch for the kinds, so the oracle is the
one reference; with RTPT_LIB naming an RT_CLU_LEAN=0 build the same tests run
the one filter."""
import pytest

import oracle_lib
from gpuraytracer_amd import RenderParams, Renderer, Scene, seed_splitmix
from lean_filter_scenes import CONTAINER, INSIDE, OWN_LIGHT, SINGLE, TURNED, kinds, scenes
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits

pytestmark = pytest.mark.gpu

SCENES = scenes(64, 48)


def render(s, sd, params):
    with Renderer(s, seeds=sd) as r:
        out = r.render(params)
        info = r.last_launch()
    assert CLUSTER_KERNEL % params.bounces in info["kernel"], info
    return out, info


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_bit_exact(name):
    s = SCENES[name]()
    sd = seed_splitmix(64, 48, key=41)
    out, _ = render(s, sd, RenderParams(spp=8, bounces=3))
    same_bits(out, oracle_lib.render(s, sd, 8, 3), name)


def test_cornell_kinds_and_lanes_per_pixel():
    s = Scene.cornell_box(64, 48)
    assert kinds(s) == sorted([CONTAINER | INSIDE, TURNED, TURNED, SINGLE | OWN_LIGHT])
    sd = seed_splitmix(64, 48, key=42)
    lanes = set()
    for spp in (4, 16):
        out, info = render(s, sd, RenderParams(spp=spp, bounces=3))
        lanes.add(info["lanes_per_pixel"])
        same_bits(out, oracle_lib.render(s, sd, spp, 3), f"spp {spp}")
    assert lanes == {4, 16}, lanes


def test_cornell_every_eighth_row():
    s = Scene.cornell_box(64, 48)
    sd = seed_splitmix(64, 48, key=43)
    out, _ = render(s, sd, RenderParams(spp=8, bounces=3, row_start=5, row_step=8))
    same_bits(out, oracle_lib.render(s, sd, 8, 3, row_start=5, row_step=8), "rows 5 (mod 8)")
