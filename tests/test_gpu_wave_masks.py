"""GPU: the per-wave mask table of the box-cluster render kernel (wave_masks_kernel,
DESIGN.md §3.29), read back with rt_debug_wave_masks, against the host twins of
the same header text on every wave's own rectangle: rt_debug_camera_candidates
for the camera mask, rt_debug_shadow_candidates -- which forms the union over
every source pair of the camera mask -- for the occluder mask and whether it is
decided.  Equality, bit for bit: the headers use + - * /, sqrtf and fma-dots
only, correctly rounded on both sides under -ffp-contract=off."""
import numpy as np
import pytest

from gpuraytracer_amd import Options, RenderParams, Renderer, Scene
from test_camera_candidates import candidates
from test_shadow_candidates import shadow_candidates

pytestmark = pytest.mark.gpu


def bits(may):
    """One byte per triangle (a pair's two triangles agree) -> one bit per pair."""
    assert (may[0::2] == may[1::2]).all()
    return sum(1 << k for k in np.flatnonzero(may[0::2]))


def check_table(scene, params, lanes, shape):
    """The table of the launch (params, lanes) equals the host's on every wave that
    holds a pixel; returns [(cam pairs, decided, occluder pairs)] of those waves."""
    with Renderer(scene, options=Options(lanes=lanes)) as r:
        rec, fills = r.wave_masks(params, lanes)
    assert fills == 1 and rec.size, (fills, rec.shape)
    return check_records(scene, params, rec, shape)


def check_records(scene, params, rec, shape):
    """``rec``, the table some context of ``scene`` gave for ``params``, equals the
    host's on every wave that holds a pixel (as check_table returns)."""
    assert rec.size, rec.shape
    q0 = rec[0, 0]
    assert (q0["x1"] - q0["x0"] + 1, (q0["y1"] - q0["y0"]) // params.row_step + 1) == shape, q0
    last_row = params.row_start + (params.rows(scene.height) - 1) * params.row_step
    seen, bad = [], []
    for q in rec.reshape(-1):
        if q["x0"] >= scene.width or q["y0"] > last_row:
            continue  # a wave past the frame's edge: no lane of it runs
        rect = (int(q["x0"]), int(q["x1"]), int(q["y0"]), int(q["y1"]))
        cam = bits(candidates(scene, *rect))
        may, avail = shadow_candidates(scene, *rect)
        occ = bits(may) if avail else None
        got = (int(q["cam_mask"]), int(q["shd_available"]), int(q["shd_mask"]) if avail else None)
        if got != (cam, avail, occ):
            bad.append((rect, "device cam %#x avail %d occ %s" % got, "host cam %#x avail %d occ %s" % (cam, avail, occ)))
        seen.append((bin(cam).count("1"), avail, None if occ is None else bin(occ).count("1")))
    assert not bad, f"{len(bad)} waves differ, first: {bad[:4]}"
    return seen


CORNELL = [
    ("L4", 96, 72, 4, RenderParams(spp=8), (4, 4)),
    ("L16", 96, 72, 16, RenderParams(spp=16), (2, 2)),
    ("L1", 96, 72, 1, RenderParams(spp=8), (8, 8)),
    ("rows L4", 96, 72, 4, RenderParams(spp=8, row_start=1, row_step=3), (16, 1)),
    ("rows L16", 96, 72, 16, RenderParams(spp=16, row_start=1, row_step=3), (4, 1)),
    ("edges L4", 70, 45, 4, RenderParams(spp=8), (4, 4)),
    ("edges L16", 70, 45, 16, RenderParams(spp=16), (2, 2)),
    ("edges L1", 70, 45, 1, RenderParams(spp=8), (8, 8)),
]


@pytest.mark.parametrize("name,w,h,lanes,params,shape", CORNELL, ids=[c[0] for c in CORNELL])
def test_cornell_tables_equal_the_host(name, w, h, lanes, params, shape):
    seen = check_table(Scene.cornell_box(w, h), params, lanes, shape)
    assert any(cam == 1 for cam, _, _ in seen) and any(cam >= 2 for cam, _, _ in seen), "both kinds of waves"


def test_cornell_280x180_holds_both_mask_paths_and_multi_pair_masks():
    """280x180 at 4 lanes: one-pair waves with an empty mask (no query) and with a
    non-empty, non-full one (the restricted query), and waves with several
    camera pairs whose union is decided and leaves pairs out, some of them
    every pair -- the masks the table adds."""
    s = Scene.cornell_box(280, 180)
    seen = check_table(s, RenderParams(spp=8), 4, (4, 4))
    n_pairs = s.n_triangles // 2
    one = [occ for cam, avail, occ in seen if cam == 1 and avail]
    assert sum(occ == 0 for occ in one) >= 100 and sum(0 < occ < n_pairs for occ in one) >= 100
    multi = [occ for cam, avail, occ in seen if cam >= 2 and avail]
    assert sum(0 < occ < n_pairs for occ in multi) >= 100, "no multi-pair wave with a decided, non-full occluder mask"
    assert any(occ == 0 for occ in multi), "no multi-pair wave with an empty occluder mask"


def test_undecided_waves_are_reported():
    """Cornell 96x72 at 4 lanes holds waves with a grazing source plane: nothing is
    decided there, on the device as on the host (check_table compares them)."""
    seen = check_table(Scene.cornell_box(96, 72), RenderParams(spp=8), 4, (4, 4))
    assert any(not avail for _, avail, _ in seen)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("lanes,spp", [(4, 8), (16, 16)])
def test_rotated_boxes_tables_equal_the_host(seed, lanes, spp):
    s = Scene.random_boxes(70, 45, 4, seed=seed)
    assert s.describe()["kernel_layout"] == 6
    check_table(s, RenderParams(spp=spp), lanes, (4, 4) if lanes == 4 else (2, 2))


def test_no_table_for_another_layout():
    """A sphere scene takes another kernel: no table, nothing filled."""
    with Renderer(Scene.random_spheres(32, 32, 8, seed=1)) as r:
        rec, fills = r.wave_masks(RenderParams(spp=8))
    assert rec.size == 0 and fills == 0
