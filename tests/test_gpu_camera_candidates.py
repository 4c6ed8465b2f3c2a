"""GPU: the box-cluster kernel with the per-wave camera-ray candidate mask
(rt_beam.hpp) against the oracle, bit for bit on uint32 views:
every wave footprint (8x8, 4x4, 2x2 pixels, 16x1 for interleaved rows) on
frames that are no multiple of it, scenes whose pairs lie in rotated boxes, flat
clusters and no cluster, the two odd-camera scenes of the CPU tests, and a
progressive render.  The CPU side is tests/test_camera_candidates.py.
The default build has the mask on (RT_CAM_CAND=1); with RTPT_LIB naming an
RT_CAM_CAND=0 build the same tests run the generic query."""
import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from test_camera_candidates import crossing_scene, inside_box_scene, random_quad_scene

pytestmark = pytest.mark.gpu
CLUSTER_KERNEL = "path_trace_kernel<%d, 6,"  # rt_kernel.hpp kLayPairClu


def same_bits(gpu, ref, what):
    gpu, ref = np.asarray(gpu, np.float32), np.asarray(ref, np.float32)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    diff = gpu.view(np.uint32) != ref.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[:6].tolist()}"


@pytest.fixture(scope="module")
def cornell():
    s = Scene.cornell_box(70, 45)
    sd = seed_splitmix(70, 45, key=77)
    return s, sd, oracle_lib.render(s, sd, 8, 3)


@pytest.mark.parametrize("lanes,spp,ran", [(1, 8, 1), (4, 8, 4), (16, 8, 1), (16, 16, 16)])
def test_cornell_every_lanes_per_pixel(cornell, lanes, spp, ran):
    """8 spp at 1, 4 and 16 requested lanes (16 lanes need 16 samples: at 8 spp
    the launcher takes 1), and 16 spp where 16 lanes run 2x2-pixel waves."""
    s, sd, ref8 = cornell
    with Renderer(s, seeds=sd, options=Options(lanes=lanes)) as r:
        out = r.render(RenderParams(spp=spp, bounces=3))
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"] and info["lanes_per_pixel"] == ran, info
    same_bits(out, ref8 if spp == 8 else oracle_lib.render(s, sd, spp, 3), f"lanes {lanes} spp {spp}")


def test_cornell_interleaved_rows(cornell):
    s, sd, ref8 = cornell
    with Renderer(s, seeds=sd) as r:
        out = r.render(RenderParams(spp=8, bounces=3, row_start=1, row_step=3))
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"], info
    same_bits(out, ref8[1::3], "rows 1 (mod 3)")


@pytest.mark.parametrize("kind", ["boxes", "quads", "twisted"])
@pytest.mark.parametrize("bounces", [1, 3])
def test_boxes_and_parallelograms(kind, bounces):
    s = {"boxes": lambda: Scene.random_boxes(48, 32, 4, seed=1),
         "quads": lambda: random_quad_scene(48, 32, 14, 2),
         "twisted": lambda: random_quad_scene(48, 32, 14, 4, twist=0.2)}[kind]()
    if kind == "twisted":
        assert s.describe()["pair_free_mask"] != 0
    sd = seed_splitmix(48, 32, key=5)
    with Renderer(s, seeds=sd) as r:
        out = r.render(RenderParams(spp=4, bounces=bounces))
        info = r.last_launch()
    assert CLUSTER_KERNEL % bounces in info["kernel"], info
    same_bits(out, oracle_lib.render(s, sd, 4, bounces), f"{kind} bounces {bounces}")


@pytest.mark.parametrize("make", [crossing_scene, inside_box_scene])
def test_odd_cameras(make):
    s = make(32, 32)
    sd = seed_splitmix(32, 32, key=9)
    with Renderer(s, seeds=sd) as r:
        out = r.render(RenderParams(spp=4, bounces=3))
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"], info
    same_bits(out, oracle_lib.render(s, sd, 4, 3), make.__name__)


def test_progressive_two_batches_equal_one_launch(cornell):
    import torch
    s, sd, ref8 = cornell
    with Renderer(s, seeds=sd) as r:
        one = r.render(RenderParams(spp=8, bounces=3))
        d = torch.empty((45, 70, 4), dtype=torch.float32, device="cuda")
        r.render_progressive(RenderParams(spp=8, bounces=3), 4, out=d)
        torch.cuda.synchronize()
    same_bits(d.cpu().numpy(), one, "2 x 4 spp vs one launch of 8")
    same_bits(one, ref8, "one launch of 8 vs oracle")
