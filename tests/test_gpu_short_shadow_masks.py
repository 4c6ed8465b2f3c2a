"""GPU: bounce-0 occluder masks of a few pairs are tested directly, pair by pair,
without the cluster filter (RT_SHD_SHORT); larger masks keep
the filter.  The frames are chosen on the CPU, through the header's own mask
(rt_debug_camera_candidates / rt_debug_shadow_candidates on the 4x4-pixel
footprints of a launch at 4 lanes per pixel): between them the waves that the
kernel decides (one camera pair) hold masks of 0, 1, ..., K_MAX + 1 pairs, for
the largest K the switch is chosen from, so both sides of every threshold run.
A missing size fails the test.  Every frame is compared with the oracle bit
for bit, at 1 and 3 bounces; black materials and surfaces the light lies behind
keep the `lit` skip in front of the query pinned (an unlit lane runs no query)."""
import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from test_camera_candidates import candidates
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits
from test_shadow_candidates import shadow_candidates

pytestmark = pytest.mark.gpu
K_MAX = 3  # RT_SHD_SHORT is chosen from 1, 2, 3
FRAMES = {
    "cornell": (96, 64, lambda: Scene.cornell_box(96, 64)),
    "boxes": (96, 64, lambda: Scene.random_boxes(96, 64, 4, seed=1)),
}


def mask_sizes(scene, w, h):
    """Sizes (pairs) of the occluder masks of the 4x4 waves the kernel decides."""
    sizes = set()
    for y0 in range(0, h, 4):
        for x0 in range(0, w, 4):
            if candidates(scene, x0, x0 + 3, y0, y0 + 3)[0::2].sum() != 1:
                continue  # more camera pairs, or none: nothing is decided
            may, avail = shadow_candidates(scene, x0, x0 + 3, y0, y0 + 3)
            if avail:
                sizes.add(int(may[0::2].sum()))
    return sizes


def render(s, sd, spp, bounces):
    with Renderer(s, seeds=sd, options=Options(lanes=4)) as r:
        out = r.render(RenderParams(spp=spp, bounces=bounces))
        info = r.last_launch()
    assert CLUSTER_KERNEL % bounces in info["kernel"] and info["lanes_per_pixel"] == 4, info
    return out


def test_frames_hold_every_mask_size_round_the_threshold():
    seen = set()
    for w, h, make in FRAMES.values():
        seen |= mask_sizes(make(), w, h)
    assert set(range(K_MAX + 2)) <= seen, sorted(seen)


@pytest.mark.parametrize("bounces", [1, 3])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_bit_exact(name, bounces):
    w, h, make = FRAMES[name]
    s, sd = make(), seed_splitmix(w, h, key=31)
    same_bits(render(s, sd, 16, bounces), oracle_lib.render(s, sd, 16, bounces), f"{name} bounces {bounces}")


def test_black_materials_and_light_behind_surfaces_bit_exact():
    """A black wall and black boxes (zero throughput: no later lane is lit), the
    ceiling and the tall box's far faces (the light behind the surface): those
    lanes run no shadow query, next to lanes of the same wave that run the
    short-mask test."""
    w, h, make = FRAMES["cornell"]
    s = make()
    assert {1, 2} <= mask_sizes(s, w, h)
    mats = s.materials
    for k in list(range(0, 2)) + list(range(10, 34)):  # a wall and both boxes
        mats[k].diffuse.x = mats[k].diffuse.y = mats[k].diffuse.z = 0.0
    scene = Scene(s.camera, mats, s.vertices, s.light, None)
    sd = seed_splitmix(w, h, key=32)
    out = render(scene, sd, 16, 3)
    same_bits(out, oracle_lib.render(scene, sd, 16, 3), "black materials")
    assert np.isfinite(out).all()
