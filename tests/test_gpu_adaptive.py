"""GPU: adaptive sampling.  rt_render_counts against the
oracle's per-pixel in-order sums (tests/adaptive_ref.py SampleFrames) on every
lockstep layout, bit for bit on uint32 views -- image, totals and, through the
calls that continue it, the kept sum; the device planner against the host
function; and render_adaptive against its four calls made by hand."""
import numpy as np
import pytest

import adaptive_ref as ar
import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, RtError, Scene, plan_samples_host, seed_splitmix
from test_adaptive import images

pytestmark = pytest.mark.gpu
W, H, CAP = 37, 21, 48
VALUES = np.array([0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 60], np.uint32)  # 60: above the cap
RT_ERR_STATE = 5


def count_map(w=W, h=H, seed=0):
    """Counts from VALUES: the four pixels of every aligned 2 x 2 block differ
    (consecutive entries of VALUES), except that the 16 x 16 block at the
    origin is all zero, the 2 x 2 block at (20, 16) is all zero inside a busy
    tile, and the 2 x 2 block at (24, 18) has one non-zero pixel.  The last
    column and the last row (partial tiles) hold non-zero counts."""
    y, x = np.mgrid[0:h, 0:w]
    idx = (2 * (y % 2) + (x % 2) + 4 * ((y // 2) * 7 + (x // 2) * 3 + seed)) % len(VALUES)
    m = VALUES[idx].copy()
    edge = np.zeros((h, w), bool)
    edge[h - 1, :] = edge[:, w - 1] = True
    m[edge & (m == 0)] = 2  # not in VALUES: differs from every neighbour
    m[0:16, 0:16] = 0
    m[16:18, 20:22] = 0
    m[18:20, 24:26] = 0
    m[19, 24] = 5
    return m


def test_count_map_properties():
    m = count_map()
    assert set(np.unique(m)) <= set(VALUES) | {2} and (m == 60).any()
    assert (m[0:16, 0:16] == 0).all() and (m[16:18, 20:22] == 0).all() and (m[16:20, 16:32] != 0).any()
    assert np.count_nonzero(m[18:20, 24:26]) == 1
    assert (m[H - 1, :] != 0).all() and (m[:, W - 1] != 0).all()
    for y0 in range(0, H, 2):
        for x0 in range(0, W, 2):
            if (y0 < 16 and x0 < 16) or (y0, x0) in ((16, 20), (18, 24)):
                continue
            blk = m[y0:y0 + 2, x0:x0 + 2].ravel()
            assert len(set(blk)) == blk.size, (y0, x0, blk)


def scene_of(name):
    if name == "cornell":
        return Scene.cornell_box(W, H)
    if name == "spheres":
        return Scene.random_spheres(W, H, 50, seed=19)
    return Scene.random_triangles(W, H, 500)


_FRAMES = {}


def frames_of(name, bounces):
    """The scene, its seeds and the oracle's single-sample frames, made once."""
    key = (name, bounces)
    if key not in _FRAMES:
        s, sd = scene_of(name), seed_splitmix(W, H, key=20 + bounces)
        _FRAMES[key] = (s, sd, ar.SampleFrames(s, sd, bounces))
    return _FRAMES[key]


def check(got, want, what):
    assert ar.same_words(got, want), f"{what}: {ar.first_difference(got, want)}"


# context -> (scene, options, kernel layout in rt_last_launch or None, spheres)
CONTEXTS = {
    "cornell": ("cornell", {}, 6, False),
    "cornell-pairs": ("cornell", dict(layout="pairs"), 1, False),
    "cornell-single": ("cornell", dict(layout="single"), 0, False),
    "cornell-global": ("cornell", dict(layout="global"), 2, False),
    "cornell-pairsmem": ("cornell", dict(layout="pairsmem"), 4, False),
    "cornell-sorted-layout": ("cornell", dict(layout="sorted"), 1, False),
    "spheres": ("spheres", {}, 7, True),
    "spheres-leaf129": ("spheres", dict(sphere_leaf_max=129), None, True),
    "spheres-free": ("spheres", dict(walk="free"), 7, True),
    "spheres-sorted": ("spheres", dict(walk="sorted"), 7, True),
    "triangles": ("triangles", {}, 5, False),
    "triangles-free": ("triangles", dict(walk="free"), 5, False),
    "triangles-sorted": ("triangles", dict(walk="sorted"), 5, False),
}


@pytest.mark.parametrize("bounces", [0, 1, 3])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_count_map_parity(ctx, bounces):
    name, opt, layout, sph = CONTEXTS[ctx]
    s, sd, frames = frames_of(name, bounces)
    counts = count_map()
    want = np.minimum(counts, CAP)
    zeros, ones = np.zeros_like(counts), np.ones_like(counts)
    with Renderer(s, seeds=sd, options=Options(lanes=4, **opt)) as r:  # lanes_per_pixel is ignored
        img, tot = r.render_counts(RenderParams(spp=CAP, bounces=bounces, keep_sum=True), counts, totals=True)
        info = r.last_launch()
        # the kept sum: its counts and sum / count come back from a call that adds nothing,
        # and one more sample per pixel continues every pixel's own sequence
        img0, tot0 = r.render_counts(RenderParams(spp=CAP, bounces=bounces, accumulate=True), zeros, totals=True)
        img1, tot1 = r.render_counts(RenderParams(spp=1, bounces=bounces, accumulate=True), ones, totals=True)
    assert "rt::path_counts_kernel<" in info["kernel"] and info["lanes_per_pixel"] == 16, info
    if layout is not None:
        flag = "true" if sph else "false"
        assert info["kernel"] == f"rt::path_counts_kernel<{bounces}, {layout}, {flag}, true, 16>", info
    check(tot, want, "totals")
    check(img, frames.image(want), "image")
    check(tot0, want, "kept counts")
    check(img0, img, "kept sum / count")
    check(tot1, want + 1, "totals after one more")
    check(img1, frames.image(want + 1), "image after one more")


def test_full_range_seeds_take_the_general_halton_form():
    s = scene_of("cornell")
    sd = np.random.default_rng(5).integers(0, 1 << 32, size=(H, W), dtype=np.uint64).astype(np.uint32)
    sd[0, 0] = 0xFFFFFFFF
    frames = ar.SampleFrames(s, sd, 3)
    counts = count_map(seed=2)
    want = np.minimum(counts, CAP)
    with Renderer(s, seeds=sd) as r:
        img, tot = r.render_counts(RenderParams(spp=CAP, bounces=3), counts, totals=True)
        info = r.last_launch()
    assert info["kernel"] == "rt::path_counts_kernel<3, 6, false, false, 1>" and info["lanes_per_pixel"] == 1, info
    check(tot, want, "totals")
    check(img, frames.image(want), "image")


@pytest.mark.parametrize("c", [1, 16, 17])
def test_uniform_counts_equal_rt_render(c):
    s, sd, _ = frames_of("cornell", 3)
    counts = np.full((H, W), c, np.uint32)
    with Renderer(s, seeds=sd) as r:
        for fmt in ({}, dict(fp16=True), dict(rgba8=True)):
            want = r.render(RenderParams(spp=c, bounces=3, sample_base=7, **fmt))
            got, tot = r.render_counts(RenderParams(spp=CAP, bounces=3, sample_base=7, **fmt), counts, totals=True)
            assert got.dtype == want.dtype and np.array_equal(got, want), (c, fmt)
            assert (tot == c).all()


@pytest.mark.parametrize("rows", [dict(), dict(row_start=1, row_step=3)])
def test_accumulation_chain(rows):
    s, sd, _ = frames_of("cornell", 3)
    frames = ar.SampleFrames(s, sd, 3, sample_base=11, **rows)
    n = RenderParams(**rows).rows(H)
    a = count_map(seed=1)[:n]
    b = count_map(seed=4)[:n].copy()
    b[:, 16:32] = 0  # a whole tile without a sample in the second call
    part = dict(bounces=3, sample_base=11, **rows)
    with Renderer(s, seeds=sd) as r:
        r.render(RenderParams(spp=5, keep_sum=True, **part))
        _, ta = r.render_counts(RenderParams(spp=CAP, accumulate=True, keep_sum=True, **part), a, totals=True)
        img, tb = r.render_counts(RenderParams(spp=CAP, accumulate=True, keep_sum=True, **part), b, totals=True)
        want = 5 + np.minimum(a, CAP) + np.minimum(b, CAP)
        check(ta, 5 + np.minimum(a, CAP), "totals after the first map")
        check(tb, want, "totals")
        check(img, frames.image(want), "image")
        # the sum now holds per-pixel counts: a uniform render cannot continue it
        for base in (11, 11 + 5 + 2 * CAP):
            with pytest.raises(RtError) as e:
                r.render(RenderParams(spp=1, bounces=3, sample_base=base, accumulate=True, **rows))
            assert e.value.status == RT_ERR_STATE and len(str(e.value)) > len("RT_ERR_STATE: ")
        # nor a counts render whose sequence starts elsewhere
        with pytest.raises(RtError) as e:
            r.render_counts(RenderParams(spp=1, bounces=3, sample_base=12, accumulate=True, **rows), a)
        assert e.value.status == RT_ERR_STATE and len(str(e.value)) > len("RT_ERR_STATE: ")
        # both left the sum as it was
        img2, t2 = r.render_counts(RenderParams(spp=1, accumulate=True, **part), np.zeros_like(a), totals=True)
        check(t2, want, "totals after the refused calls")
        check(img2, img, "image after the refused calls")
        # a new uniform sum clears the state
        r.render(RenderParams(spp=2, keep_sum=True, **part))
        r.render(RenderParams(spp=1, bounces=3, sample_base=13, accumulate=True, **rows))


def test_dead_wave_scene():
    """Cornell 512 x 32 of tests/test_gpu_dead_waves.py: 2 x 2-pixel waves with an
    empty camera mask next to waves that see the room."""
    import test_gpu_dead_waves as dw
    s = Scene.cornell_box(dw.W, dw.H)
    sd = seed_splitmix(dw.W, dw.H, key=26)
    empty, seen = dw.wave_masks(s, 2, 2)
    assert empty >= 1 and seen >= 1, (empty, seen)
    frames = ar.SampleFrames(s, sd, 3)
    counts = np.array([0, 1, 2, 3, 5, 9], np.uint32)[np.random.default_rng(3).integers(0, 6, size=(dw.H, dw.W))]
    want = np.minimum(counts, 6)
    with Renderer(s, seeds=sd) as r:
        r.render(RenderParams(spp=1, bounces=3, keep_sum=True))
        img, tot = r.render_counts(RenderParams(spp=6, bounces=3, accumulate=True), counts, totals=True)
        assert r.last_launch()["kernel"] == "rt::path_counts_kernel<3, 6, false, true, 16>"
        img2, tot2 = r.render_counts(RenderParams(spp=6, bounces=3), counts, totals=True)
    check(tot, want + 1, "totals")
    check(img, frames.image(want + 1), "image")
    check(tot2, want, "totals of a new sum")
    check(img2, frames.image(want), "image of a new sum")


def test_empty_map():
    s, sd, _ = frames_of("cornell", 3)
    zeros = np.zeros((H, W), np.uint32)
    with Renderer(s, seeds=sd) as r:
        img, tot = r.render_counts(RenderParams(spp=CAP, bounces=3, keep_sum=True), zeros, totals=True)
        u8 = r.render_counts(RenderParams(spp=CAP, bounces=3, rgba8=True), zeros)
        h16 = r.render_counts(RenderParams(spp=0, bounces=3, fp16=True), count_map())  # a cap of 0
        one = count_map()
        one[one > 0] = 1
        img1, tot1 = r.render_counts(RenderParams(spp=CAP, bounces=3, accumulate=True), one, totals=True)
    want = np.zeros((H, W, 4), np.float32)
    want[..., 3] = 1.0
    check(img, want, "all-zero map")
    assert (tot == 0).all() and (u8 == np.array([0, 0, 0, 255], np.uint8)).all()
    assert (h16 == np.array([0, 0, 0, 0x3C00], np.uint16)).all()
    zero_px = one == 0
    check(img1[zero_px], want[zero_px], "zero-total pixels")
    check(tot1, one, "totals")


def test_async_variants_on_a_torch_stream():
    import torch
    s, sd, frames = frames_of("cornell", 3)
    counts = count_map(seed=3)
    want = np.minimum(counts, CAP)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with Renderer(s, seeds=sd) as r:
        with torch.cuda.stream(stream):
            dc = torch.from_numpy(counts.astype(np.int32)).to(dev, non_blocking=False)
            out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
            tot = torch.empty((H, W), dtype=torch.int32, device=dev)
        stream.synchronize()
        r.render_counts(RenderParams(spp=CAP, bounces=3), dc, out=out, totals=tot, stream=stream)
        info = r.last_launch()
        f, a = images(H, W, 11, special=True)
        df, da = torch.from_numpy(f).to(dev), torch.from_numpy(a).to(dev)
        torch.cuda.synchronize(dev)
        pc, ps = r.plan_samples(df, da, budget=5000, radius=2, relative=True, return_stats=True, stream=stream)
        stream.synchronize()
    assert info["kernel"] == "rt::path_counts_kernel<3, 6, false, true, 16>", info
    check(tot.cpu().numpy(), want, "totals")
    check(out.cpu().numpy(), frames.image(want), "image")
    hc, hs = plan_samples_host(f, a, budget=5000, radius=2, relative=True, return_stats=True)
    check(pc.cpu().numpy(), hc, "device plan on a stream")
    assert ps == hs, (ps, hs)


@pytest.mark.parametrize("shape", [(21, 37), (16, 16)])
def test_device_planner_equals_host_planner(shape):
    import torch
    rows, w = shape
    s = Scene.cornell_box(w, rows)
    with Renderer(s) as r:
        for special in (False, True):
            f, a = images(rows, w, 2 + special, special)
            df, da = torch.from_numpy(f).cuda(), torch.from_numpy(a).cuda()
            for radius in (0, 1, 2):
                for relative in (False, True):
                    kw = dict(budget=8 * rows * w, radius=radius, relative=relative, count_min=1, count_max=40)
                    hc, hs = plan_samples_host(f, a, return_stats=True, **kw)
                    gc, gs = r.plan_samples(f, a, return_stats=True, **kw)
                    what = f"{shape} radius {radius} relative {relative} special {special}"
                    check(gc, hc, what + " (host buffers)")
                    assert gs == hs, (what, gs, hs)
                    dc, ds = r.plan_samples(df, da, return_stats=True, **kw)
                    check(dc.cpu().numpy(), hc, what + " (device buffers)")
                    assert ds == hs, (what, ds, hs)
        assert r.last_launch()["kernel"] == "rt::plan_counts_kernel"
        # fewer rows than the camera's: a tile of its own
        f, a = images(rows - 3, w, 9)
        check(r.plan_samples(f, a, budget=999), plan_samples_host(f, a, budget=999), "a shorter tile")
        with pytest.raises(RtError) as e:
            r.plan_samples(*images(rows + 1, w, 9), budget=1)
        assert e.value.status == 1


@pytest.mark.parametrize("device", [False, True])
def test_render_adaptive_equals_its_four_calls(device):
    w, h = 64, 48
    s = Scene.cornell_box(w, h)
    sd = seed_splitmix(w, h, key=31)
    frames = ar.SampleFrames(s, sd, 3, sample_base=3)
    p = RenderParams(spp=24, bounces=3, sample_base=3)
    with Renderer(s, seeds=sd) as r:
        img, tot, stats = r.render_adaptive(p, pilot_spp=4, mean_spp=8, return_totals=True, return_stats=True,
                                            device=device)
        if device:
            img, tot = img.cpu().numpy(), tot.cpu().numpy()
        first = r.render(RenderParams(spp=2, bounces=3, sample_base=3, keep_sum=True))
        both = r.render(RenderParams(spp=2, bounces=3, sample_base=5, accumulate=True, keep_sum=True))
        counts, st = r.plan_samples(first, both, budget=4 * w * h, count_max=20, return_stats=True)
        img2, tot2 = r.render_counts(RenderParams(spp=20, bounces=3, sample_base=3, accumulate=True, keep_sum=True),
                                     counts, totals=True)
    check(tot, tot2, "totals")
    check(img, img2, "image")
    assert stats == st and st["samples"] <= 4 * w * h
    check(tot, counts + 4, "totals = pilot + plan")
    assert tot.max() <= 24 and tot.min() >= 4
    check(img, frames.image(tot), "image against the reference of its totals")
