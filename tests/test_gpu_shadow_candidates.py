"""GPU: the box-cluster kernel with the per-wave occluder mask of the bounce-0
shadow query (rt_shaft.hpp) against the oracle, bit for bit on
uint32 views, on the scenes of tests/test_shadow_candidates.py at 70x45: every
wave footprint (8x8, 4x4, 2x2 pixels, one row for interleaved rows), 1, 3 and
4 bounces, and a progressive render.  The default build has the mask on
(RT_SHD_CAND=1); with RTPT_LIB naming an RT_SHD_CAND=0 build the same tests run
the generic query."""
import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from test_camera_candidates import H, W, crossing_scene, inside_box_scene, parallelogram_scene
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits
from test_camera_candidates import candidates
from test_shadow_candidates import light_plane_cut_scene, low_quad_scene, shadow_candidates

pytestmark = pytest.mark.gpu

SCENES = {
    "cornell": lambda: Scene.cornell_box(W, H),
    "boxes": lambda: Scene.random_boxes(W, H, 4, seed=1),
    "quads": lambda: parallelogram_scene(1),
    "twisted": lambda: parallelogram_scene(4, 0.2),
    "crossing": crossing_scene,
    "inside_box": inside_box_scene,
    "low_quad": low_quad_scene,
    "light_plane_cut": light_plane_cut_scene,
}


@pytest.fixture(scope="module")
def cornell():
    s = SCENES["cornell"]()
    sd = seed_splitmix(W, H, key=78)
    return s, sd, oracle_lib.render(s, sd, 8, 3)


def render(s, sd, params, lanes=None):
    with Renderer(s, seeds=sd, options=Options(lanes=lanes) if lanes else None) as r:
        out = r.render(params)
        info = r.last_launch()
    assert CLUSTER_KERNEL % params.bounces in info["kernel"], info
    return out, info


@pytest.mark.parametrize("name", [n for n in SCENES if n != "cornell"])
def test_scenes_bit_exact(name):
    s = SCENES[name]()
    sd = seed_splitmix(W, H, key=11)
    out, _ = render(s, sd, RenderParams(spp=8, bounces=3))
    same_bits(out, oracle_lib.render(s, sd, 8, 3), name)


@pytest.mark.parametrize("lanes,spp,ran", [(1, 8, 1), (4, 8, 4), (16, 8, 1), (16, 16, 16)])
def test_cornell_every_lanes_per_pixel(cornell, lanes, spp, ran):
    s, sd, ref8 = cornell
    out, info = render(s, sd, RenderParams(spp=spp, bounces=3), lanes)
    assert info["lanes_per_pixel"] == ran, info
    same_bits(out, ref8 if spp == 8 else oracle_lib.render(s, sd, spp, 3), f"lanes {lanes} spp {spp}")


def test_cornell_interleaved_rows(cornell):
    s, sd, ref8 = cornell
    out, _ = render(s, sd, RenderParams(spp=8, bounces=3, row_start=1, row_step=3))
    same_bits(out, ref8[1::3], "rows 1 (mod 3)")


@pytest.mark.parametrize("bounces", [1, 4])
def test_cornell_other_bounce_counts(cornell, bounces):
    s, sd, _ = cornell
    out, _ = render(s, sd, RenderParams(spp=8, bounces=bounces))
    same_bits(out, oracle_lib.render(s, sd, 8, bounces), f"bounces {bounces}")


def test_progressive_two_batches_equal_one_launch(cornell):
    import torch
    s, sd, ref8 = cornell
    with Renderer(s, seeds=sd) as r:
        one = r.render(RenderParams(spp=8, bounces=3))
        assert CLUSTER_KERNEL % 3 in r.last_launch()["kernel"]
        d = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        r.render_progressive(RenderParams(spp=8, bounces=3), 4, out=d)
        torch.cuda.synchronize()
        assert CLUSTER_KERNEL % 3 in r.last_launch()["kernel"]
    same_bits(d.cpu().numpy(), one, "2 x 4 spp vs one launch of 8")
    same_bits(one, ref8, "one launch of 8 vs oracle")


def test_cornell_280x180_takes_both_mask_paths():
    """At 70x45 most waves see more than one pair and stay undecided.  On this
    frame the masks themselves (the same header on the host) show that 4x4
    waves take both new paths -- one camera pair with an empty occluder mask
    (no query) and one camera pair with a non-empty mask (the restricted
    query) -- and the render at 4 lanes per pixel (4x4-pixel waves) is bit-exact."""
    w, h = 280, 180
    s = Scene.cornell_box(w, h)
    empty = restricted = 0
    for y0 in range(0, h, 4):
        for x0 in range(0, w, 4):
            if candidates(s, x0, x0 + 3, y0, y0 + 3)[0::2].sum() != 1:
                continue  # the kernel decides one-pair waves only
            may, avail = shadow_candidates(s, x0, x0 + 3, y0, y0 + 3)
            if avail:
                empty += not may.any()
                restricted += bool(may.any() and not may.all())
    assert empty >= 100 and restricted >= 100, (empty, restricted)
    sd = seed_splitmix(w, h, key=12)
    out, info = render(s, sd, RenderParams(spp=8, bounces=3), lanes=4)
    assert info["lanes_per_pixel"] == 4, info
    same_bits(out, oracle_lib.render(s, sd, 8, 3), "280x180")
