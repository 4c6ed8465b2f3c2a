"""GPU: the box-cluster kernel shading with the light flag from the launch's
light mask and the light's own cluster passed over in shade()'s shadow
queries against the C oracle, bit for bit on
uint32 views, no pixel excluded.  Scenes of 64x48 or smaller at up to 16 spp:
a pair with one light and one diffuse triangle, a pair of two colours, a
second emitter that is not the sampled light, light-mask bits above 31 (ids
up to 61), 1-3 bounces, every lanes-per-pixel form, interleaved rows and
progressive batches.  Every case asserts through rt_last_launch that the
box-cluster kernel ran and that its dynamic LDS is what it was: 112 B per pair
and per cluster and the 4,679 floats of the Halton tables."""
import pytest

import oracle_lib
from gpuraytracer_amd import RenderParams, Renderer, Scene, seed_splitmix
from lean_filter_scenes import second_emitter
from light_mask_scenes import half_light_quad, two_colour_quad
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits

pytestmark = pytest.mark.gpu

W, H = 64, 48


def render(s, sd, params):
    d = s.describe()
    with Renderer(s, seeds=sd) as r:
        out = r.render(params)
        info = r.last_launch()
    assert CLUSTER_KERNEL % params.bounces in info["kernel"], info
    assert info["lds_bytes"] == 112 * d["n_triangle_pairs"] + 112 * d["n_box_clusters"] + 4 * 4679, info
    return out, info


def check(s, name, spp, lanes, bounces=3, key=51, **rows):
    sd = seed_splitmix(s.width, s.height, key=key)
    out, info = render(s, sd, RenderParams(spp=spp, bounces=bounces, **rows))
    assert info["lanes_per_pixel"] == lanes, info
    same_bits(out, oracle_lib.render(s, sd, spp, bounces, **rows), f"{name} spp {spp}")
    return info


@pytest.mark.parametrize("spp,lanes", [(8, 4), (16, 16)])
def test_quad_with_one_light_triangle(spp, lanes):
    check(half_light_quad(W, H), "half_light_quad", spp, lanes)


@pytest.mark.parametrize("spp,lanes", [(8, 4), (16, 16)])
def test_quad_of_two_colours(spp, lanes):
    check(two_colour_quad(W, H), "two_colour_quad", spp, lanes)


def test_second_emitter():
    """Two emitters, one of them not the sampled light (triangles 10, 11 of 26)."""
    check(second_emitter(W, H), "second_emitter", 8, 4)


@pytest.mark.parametrize("boxes,pairs", [(2, 18), (3, 24), (4, 30)])
def test_random_boxes(boxes, pairs):
    """Ids up to 59: the light's mask bits are 34-35, 46-47 and 58-59."""
    s = Scene.random_boxes(W, H, boxes, seed=boxes)
    assert s.describe()["n_triangle_pairs"] == pairs
    assert s.light_mask()[0] == 3 << (2 * pairs - 2)
    check(s, f"boxes{boxes}", 8, 4)
    check(s, f"boxes{boxes}", 16, 16, key=52)


def test_31_pairs_of_random_quads():
    """The largest scene that still gets clusters: ids up to 61."""
    from test_gpu_parity import random_quad_scene
    s = random_quad_scene(48, 32, 30, 2)
    assert s.light_mask()[0] == 3 << 60
    check(s, "quads30", 8, 4)
    check(s, "quads30", 16, 16, key=52)


def test_cornell_without_halton_tables():
    info = check(Scene.cornell_box(W, H), "cornell", 2, 1)
    assert info["halton_tables"] == 0


def test_cornell_both_lanes_per_pixel():
    s = Scene.cornell_box(W, H)
    lanes = {check(s, "cornell", spp, spp)["lanes_per_pixel"] for spp in (4, 16)}
    assert lanes == {4, 16}


@pytest.mark.parametrize("bounces", [1, 2])
def test_cornell_fewer_bounces(bounces):
    check(Scene.cornell_box(W, H), "cornell", 8, 4, bounces=bounces)


def test_cornell_every_eighth_row():
    check(Scene.cornell_box(W, H), "cornell", 8, 4, row_start=5, row_step=8)


def test_cornell_progressive_two_batches():
    import torch
    s = Scene.cornell_box(W, H)
    sd = seed_splitmix(W, H, key=53)
    with Renderer(s, seeds=sd) as r:
        one = r.render(RenderParams(spp=8, bounces=3))
        d = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        r.render_progressive(RenderParams(spp=8, bounces=3), 4, out=d)
        torch.cuda.synchronize()
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"] and info["lds_bytes"] == 112 * 18 + 112 * 4 + 4 * 4679, info
    same_bits(d.cpu().numpy(), one, "2 x 4 spp vs one launch of 8")
    same_bits(one, oracle_lib.render(s, sd, 8, 3), "one launch of 8 vs oracle")
