"""GPU: the box-cluster kernel with the ordered and culled closest queries of
bounce >= 1 (rt_cluorder.hpp) against the C oracle, bit for bit
on uint32 views: Cornell at 64x48 and at 37x29 (partial tiles) with 4, 8 and 16
samples and 1 to 4 bounces, a row-interleaved launch (every 8th row), and the
scenes of tests/test_closest_order.py at 64x48 x 8 spp.  Every case asserts
through rt_last_launch that the box-cluster kernel ran -- except the
Scene.random_boxes scenes of 5 and 6 boxes, which hold more pairs than a pair
mask has bits: the scene compiler builds no clusters for them, the pair kernel
runs (asserted too), and they are kept as bit-exact cases of that kernel.  The
default build has the order on (RT_CLU_ORDER=1); with RTPT_LIB naming an
RT_CLU_ORDER=0 build the same tests run the single-mask query."""
import pytest

import oracle_lib
from closest_order_scenes import NO_CLUSTERS, scenes
from gpuraytracer_amd import RenderParams, Renderer, Scene, seed_splitmix
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits

pytestmark = pytest.mark.gpu

SCENES = scenes(64, 48)


def render(s, sd, params, clusters=True):
    with Renderer(s, seeds=sd) as r:
        out = r.render(params)
        info = r.last_launch()
    assert (CLUSTER_KERNEL % params.bounces in info["kernel"]) == clusters, info
    return out


@pytest.mark.parametrize("bounces", [1, 2, 3, 4])
@pytest.mark.parametrize("spp", [4, 8, 16])
@pytest.mark.parametrize("w,h", [(64, 48), (37, 29)])
def test_cornell_bit_exact(w, h, spp, bounces):
    s = Scene.cornell_box(w, h)
    sd = seed_splitmix(w, h, key=31)
    out = render(s, sd, RenderParams(spp=spp, bounces=bounces))
    same_bits(out, oracle_lib.render(s, sd, spp, bounces), f"{w}x{h} spp {spp} bounces {bounces}")


def test_cornell_every_eighth_row():
    s = Scene.cornell_box(64, 48)
    sd = seed_splitmix(64, 48, key=32)
    out = render(s, sd, RenderParams(spp=8, bounces=3, row_start=3, row_step=8))
    same_bits(out, oracle_lib.render(s, sd, 8, 3, row_start=3, row_step=8), "rows 3 (mod 8)")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_bit_exact(name):
    s = SCENES[name]()
    sd = seed_splitmix(64, 48, key=33)
    out = render(s, sd, RenderParams(spp=8, bounces=3), clusters=name not in NO_CLUSTERS)
    same_bits(out, oracle_lib.render(s, sd, 8, 3), name)
