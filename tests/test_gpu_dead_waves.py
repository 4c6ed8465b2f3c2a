"""GPU: waves of the box-cluster kernel whose camera mask is empty skip the
sample loop and add +0 to their pixels' sums once.  Cornell at
512x32 has such waves next to waves that see the room, at every wave footprint;
that is asserted on the CPU first, through rt_debug_camera_candidates on the
footprints of each launch.  Every launch is compared with the oracle bit for
bit on uint32 views, alpha included: 1, 4 and 16 lanes per pixel, the
interleaved rows of an N = 8 share, the fp16 and tonemapped stores, and a
progressive render in batches (the sums and sample counts the dead waves write
are what the next batch and the last division read)."""
import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from test_camera_candidates import candidates
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits

pytestmark = pytest.mark.gpu
W, H = 512, 32


def wave_masks(scene, tw, th, start=0, step=1):
    """(waves with an empty camera mask, waves with a pair) for tw x th-pixel
    waves over the rows start + j * step: the kernel prologue's rectangles."""
    rows = (H - 1 - start) // step + 1
    empty = seen = 0
    for j0 in range(0, rows, th):
        for x0 in range(0, W, tw):
            may = candidates(scene, x0, x0 + tw - 1, start + j0 * step, start + (j0 + th - 1) * step)
            empty += not may.any()
            seen += bool(may.any())
    return empty, seen


@pytest.fixture(scope="module")
def cornell():
    s = Scene.cornell_box(W, H)
    sd = seed_splitmix(W, H, key=26)
    return s, sd, {}


def reference(cornell, spp):
    s, sd, refs = cornell
    if spp not in refs:
        refs[spp] = oracle_lib.render(s, sd, spp, 3)
    return refs[spp]


def render(cornell, params, lanes, ran):
    s, sd, _ = cornell
    with Renderer(s, seeds=sd, options=Options(lanes=lanes)) as r:
        out = r.render(params)
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"] and info["lanes_per_pixel"] == ran, info
    return out


# lanes per pixel, spp, wave footprint of a whole frame
@pytest.mark.parametrize("lanes,spp,tile", [(1, 2, (8, 8)), (4, 32, (4, 4)), (16, 16, (2, 2))])
def test_whole_frame(cornell, lanes, spp, tile):
    empty, seen = wave_masks(cornell[0], *tile)
    assert empty >= 1 and seen >= 1, (empty, seen)
    out = render(cornell, RenderParams(spp=spp, bounces=3), lanes, lanes)
    same_bits(out, reference(cornell, spp), f"lanes {lanes} spp {spp}")


@pytest.mark.parametrize("lanes,tile", [(16, (4, 1)), (4, (16, 1))])
def test_interleaved_rows_of_a_share_of_8(cornell, lanes, tile):
    """Rank 3's rows of an N = 8 share: one-row waves of 64 / lanes pixels."""
    empty, seen = wave_masks(cornell[0], *tile, start=3, step=8)
    assert empty >= 1 and seen >= 1, (empty, seen)
    out = render(cornell, RenderParams(spp=16, bounces=3, row_start=3, row_step=8), lanes, lanes)
    same_bits(out, reference(cornell, 16)[3::8], f"rows 3 (mod 8), lanes {lanes}")


def test_fp16_and_tonemapped_stores(cornell):
    ref = reference(cornell, 32)
    h16 = render(cornell, RenderParams(spp=32, bounces=3, fp16=True), 4, 4)
    u8 = render(cornell, RenderParams(spp=32, bounces=3, rgba8=True), 4, 4)
    assert np.array_equal(h16, ref.astype(np.float16).view(np.uint16))
    assert np.array_equal(u8, oracle_lib.tonemap(ref))


@pytest.mark.parametrize("lanes", [1, 4])
def test_progressive_batches_equal_one_launch(cornell, lanes):
    """32 spp as 3 launches of 12, 12 and 8 samples into the running sums: a dead
    wave's sum and sample count are read back by the next batch and divided by
    the last, so the frame equals the single launch (and the oracle)."""
    import torch
    s, sd, _ = cornell
    with Renderer(s, seeds=sd, options=Options(lanes=lanes)) as r:
        one = r.render(RenderParams(spp=32, bounces=3))
        d = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        r.render_progressive(RenderParams(spp=32, bounces=3), 12, out=d)
        torch.cuda.synchronize()
        assert CLUSTER_KERNEL % 3 in r.last_launch()["kernel"]
    same_bits(d.cpu().numpy(), one, "12 + 12 + 8 spp vs one launch of 32")
    same_bits(one, reference(cornell, 32), "one launch of 32 vs oracle")
