"""GPU: every entry point at the camera poses and light positions of
tests/pose_scenes.py, bit for bit against the CPU references
that tests/test_poses.py pins at the same views.  The rest of the suite
renders from the Cornell camera with the light at the ceiling centre; the
conservative shortcuts of the kernels -- beam and shaft masks, the wave-mask
table, dead waves, the own-light skip, the octant layouts of the BVH walks, the
camera-scaled margin and exactness domain -- are geometry relative to both.

One 64 x 48 frame (72 x 24 for ``aspect3``), one seed texture, 8 spp and 3
bounces (16 spp where 16 lanes per pixel run).  An oracle frame is computed
once per (scene, pose, light, spp) and shared.  Every case names the kernel it
ran through last_launch(), so that a pose cannot change the layout unseen; the
MIS launcher reports none, its cases assert the layout the context describes."""
import functools

import numpy as np
import pytest

import adaptive_ref as adr
import aov_ref
import oracle_lib
import pose_scenes as ps
import ray_sets as rs
from gpuraytracer_amd import MisParams, Options, RenderParams, Renderer, Scene, seed_splitmix
from test_gpu_camera_candidates import same_bits
from test_gpu_wave_masks import check_table

pytestmark = pytest.mark.gpu
SPP, BOUNCES, KEY = 8, 3, 0x905E

SCENES = {
    "cornell": lambda w, h: Scene.cornell_box(w, h),
    "boxes0": lambda w, h: Scene.random_boxes(w, h, 4, seed=0),
    "boxes1": lambda w, h: Scene.random_boxes(w, h, 4, seed=1),
    "spheres": lambda w, h: Scene.random_spheres(w, h, 200),
    "triangles": lambda w, h: Scene.random_triangles(w, h, 600),
    "mis": lambda w, h: Scene.cornell_box_mis(w, h),
}
# context -> (scene, options, kernel function, its GEO template argument, spheres)
CONTEXTS = {
    "cornell": ("cornell", {}, "path_trace_kernel", 6, False),
    "cornell-pairs": ("cornell", dict(layout="pairs"), "path_trace_kernel", 1, False),
    "boxes0": ("boxes0", {}, "path_trace_kernel", 6, False),
    "boxes1": ("boxes1", {}, "path_trace_kernel", 6, False),
    "spheres": ("spheres", {}, "path_trace_kernel", 7, True),
    "spheres-free": ("spheres", dict(walk="free"), "path_free_kernel", 7, True),
    "spheres-sorted": ("spheres", dict(walk="sorted"), "path_trace_sorted_kernel", 7, True),
    "triangles": ("triangles", {}, "path_trace_kernel", 5, False),
    "triangles-free": ("triangles", dict(walk="free"), "path_free_kernel", 5, False),
    "triangles-sorted": ("triangles", dict(walk="sorted"), "path_trace_sorted_kernel", 5, False),
}
OCT_CONTEXTS = ["cornell"] + [c for c in CONTEXTS if c.startswith(("spheres", "triangles"))]
CHAIN = [p for p in ps.POSES if p not in ps.FRAME]   # the poses of one resolution: what an update can walk


@functools.lru_cache(maxsize=None)
def seeds_of(w, h):
    sd = seed_splitmix(w, h, key=KEY)
    sd.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def view(scene, pose="cornell", light="ceiling"):
    """(scene at the pose and light, its seeds)."""
    w, h = ps.frame_of(pose)
    return ps.view(SCENES[scene](w, h), pose, light), seeds_of(w, h)


@functools.lru_cache(maxsize=None)
def oracle(scene, pose="cornell", light="ceiling", spp=SPP):
    s, sd = view(scene, pose, light)
    ref = oracle_lib.render(s, sd, spp, BOUNCES)
    ref.setflags(write=False)
    return ref


def kernel_prefix(ctx, fn=None, bounces=BOUNCES):
    _, _, kernel, geo, sph = CONTEXTS[ctx]
    return f"rt::{fn or kernel}<{bounces}, {geo}, {'true' if sph else 'false'}, "


def renderer(ctx, pose="cornell", light="ceiling", **more):
    name, opt = CONTEXTS[ctx][:2]
    s, sd = view(name, pose, light)
    return Renderer(s, seeds=sd, options=Options(**opt, **more))


def render_case(ctx, pose, light="ceiling"):
    with renderer(ctx, pose, light) as r:
        out = r.render(RenderParams(spp=SPP, bounces=BOUNCES))
        info = r.last_launch()
    assert info["kernel"].startswith(kernel_prefix(ctx)), (ctx, pose, light, info)
    same_bits(out, oracle(CONTEXTS[ctx][0], pose, light), f"{ctx} at {pose}, light {light}")


# ---- poses and lights ---------------------------------------------------------------

@pytest.mark.parametrize("pose", ps.MAIN)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_pose_parity(ctx, pose):
    render_case(ctx, pose)


@pytest.mark.parametrize("pose", list(ps.OCTANTS))
@pytest.mark.parametrize("ctx", OCT_CONTEXTS)
def test_octant_view_parity(ctx, pose):
    """A view whose centre ray lies in each of the eight BVH octants: the packet
    walks follow the layout of a wave's first lane, the sorted scheduler sorts
    by octant, the sphere walk has one layout per octant."""
    render_case(ctx, pose)


@pytest.mark.parametrize("ctx", ["cornell", "triangles"])
def test_aspect_ratio_3_parity(ctx):
    s, _ = view(CONTEXTS[ctx][0], "aspect3")
    assert (s.width, s.height) == (72, 24)
    render_case(ctx, "aspect3")


@pytest.mark.parametrize("pose,light", [("cornell", l) for l in ps.MOVED_LIGHTS] + [("diag_roll", "low")])
@pytest.mark.parametrize("ctx", ["cornell", "cornell-pairs", "boxes0", "spheres", "triangles"])
def test_light_parity(ctx, pose, light):
    """The light off the emissive quad: below most of the scene (shadow segments
    go down), outside the room, and in the plane of the ceiling wall."""
    render_case(ctx, pose, light)


# ---- the cluster kernel's forms -------------------------------------------------------

@pytest.mark.parametrize("pose", ["rolled", "diag_roll", "straight_down"])
@pytest.mark.parametrize("lanes,spp", [(1, 8), (4, 8), (16, 16)])
def test_cluster_kernel_lanes(pose, lanes, spp):
    with renderer("cornell", pose, lanes=lanes) as r:
        out = r.render(RenderParams(spp=spp, bounces=BOUNCES))
        info = r.last_launch()
    assert info["kernel"] == kernel_prefix("cornell") + f"true, {lanes}>" and info["lanes_per_pixel"] == lanes, info
    same_bits(out, oracle("cornell", pose, spp=spp), f"{pose}, {lanes} lanes")


@pytest.mark.parametrize("pose", ["rolled", "diag_roll", "straight_down"])
@pytest.mark.parametrize("lanes,spp", [(4, 8), (16, 16)])
def test_cluster_kernel_interleaved_rows(pose, lanes, spp):
    with renderer("cornell", pose, lanes=lanes) as r:
        out = r.render(RenderParams(spp=spp, bounces=BOUNCES, row_start=1, row_step=3))
        info = r.last_launch()
    assert info["kernel"] == kernel_prefix("cornell") + f"true, {lanes}>", info
    same_bits(out, oracle("cornell", pose, spp=spp)[1::3], f"{pose}, rows 1 (mod 3), {lanes} lanes")


# ---- the mask table ---------------------------------------------------------------------

DEAD_WAVE_POSES = ("narrow_far", "behind_left")
TABLE_CASES = [(p, "ceiling") for p in ps.POSES] + [("cornell", l) for l in ps.MOVED_LIGHTS] + [("diag_roll", "low")]


@pytest.mark.parametrize("pose,light", TABLE_CASES, ids=[p if l == "ceiling" else f"{p}-light-{l}" for p, l in TABLE_CASES])
@pytest.mark.parametrize("lanes,spp,shape", [(4, 8, (4, 4)), (16, 16, (2, 2))])
@pytest.mark.parametrize("scene", ["cornell", "boxes0"])
def test_wave_mask_table_equals_the_host(scene, lanes, spp, shape, pose, light):
    """The device table equals the host twins on every wave (check_table), at a
    generic camera basis: sqrtf and the fma-dots meet operands the Cornell
    camera's exact zeros never give them; ``aspect3`` adds another halfH.  The
    table belongs to the box-cluster kernel, layout 6 (check_table launches
    nothing but wave_masks_kernel; the renders that read these tables name
    their kernel in the parity tests above).  Outside poses: some wave has one
    camera pair and a decided occluder mask.  ``narrow_far`` and ``behind_left``
    frame more than the room: some waves have an empty camera mask, the dead
    waves whose frames test_pose_parity compares with the oracle.  Inside poses
    and ``away``: no wave decides its occluder mask; at ``away`` every wave
    keeps every pair (the behind-the-camera fallback: no wave is dead)."""
    s, _ = view(scene, pose, light)
    assert s.describe()["kernel_layout"] == 6
    seen = check_table(s, RenderParams(spp=spp, bounces=BOUNCES), lanes, shape)
    if pose in ps.OUTSIDE or pose in ps.FRAME:
        assert any(cam == 1 and avail for cam, avail, _ in seen), "no one-pair wave with a decided mask"
    else:
        assert not any(avail for _, avail, _ in seen)
    if pose in DEAD_WAVE_POSES:
        assert any(cam == 0 for cam, _, _ in seen), "no wave with an empty camera mask"
    if pose == "away":
        assert all(cam == s.n_triangles // 2 for cam, _, _ in seen)


# ---- the update chain ---------------------------------------------------------------------

@pytest.mark.parametrize("ctx", ["cornell", "triangles"])
def test_update_chain_through_every_pose_and_light(ctx):
    """One context walked through all poses, then all lights, with update_scene:
    every frame equals the oracle frame of that view.  On the cluster kernel the
    table is refilled once per update (its key holds the camera and the light
    centre), and not by a second render of the same view."""
    name = CONTEXTS[ctx][0]
    p = RenderParams(spp=SPP, bounces=BOUNCES)
    steps = [(q, "ceiling") for q in CHAIN if q != "cornell"] + [("cornell", l) for l in ps.MOVED_LIGHTS] + \
            [("diag_roll", "low"), ("cornell", "ceiling")]
    with renderer(ctx) as r:
        same_bits(r.render(p), oracle(name), f"{ctx} before any update")
        assert r.last_launch()["kernel"].startswith(kernel_prefix(ctx))
        for k, (pose, light) in enumerate(steps):
            r.update_scene(view(name, pose, light)[0])
            same_bits(r.render(p), oracle(name, pose, light), f"{ctx} update {k}: {pose}, light {light}")
            assert r.last_launch()["kernel"].startswith(kernel_prefix(ctx)), (pose, light, r.last_launch())
            if ctx == "cornell":
                same_bits(r.render(p), oracle(name, pose, light), f"{ctx} update {k} again")
                assert r.wave_masks(p)[1] == 2 + k, f"update {k} ({pose}, light {light}): one refill"
        assert r.update_info()["updates"] == len(steps)


# ---- feature buffers ----------------------------------------------------------------------

AOV_SPP = 3


@pytest.mark.parametrize("pose", ["rolled", "diag_roll", "straight_down", "narrow_far", "inside_tall_box"])
@pytest.mark.parametrize("ctx", ["cornell", "spheres", "triangles"])
def test_aov_parity(ctx, pose):
    name, _, _, geo, sph = CONTEXTS[ctx]
    s, sd = view(name, pose)
    want = aov_ref.buffers(aov_ref.np_scene(s), sd, AOV_SPP)
    with renderer(ctx, pose) as r:
        got = r.render_aov(spp=AOV_SPP)
        info = r.last_launch()
    assert info["kernel"] == f"rt::aov_kernel<{geo}, {'true' if sph else 'false'}, true>", info
    for k in ("albedo", "normal_depth", "first_hit"):
        assert aov_ref.same(got[k], want[k]), f"{ctx} at {pose}, {k}: " + aov_ref.first_difference(got[k], want[k])
    if pose != "inside_tall_box":
        assert len(np.unique(want["first_hit"]["id"])) >= 3


# ---- per-pixel sample counts ----------------------------------------------------------------

def count_map():
    """0, 1, 5, 16 and 17 mixed so that neighbours differ, row 7 empty, the last column and row non-zero."""
    y, x = np.mgrid[0:ps.H, 0:ps.W]
    m = np.array([0, 1, 5, 16, 17], np.uint32)[(3 * x + 2 * y + (x // 4) * (y // 4)) % 5]
    m[ps.H - 1, :] = np.where(m[ps.H - 1, :] == 0, 5, m[ps.H - 1, :])
    m[:, ps.W - 1] = np.where(m[:, ps.W - 1] == 0, 1, m[:, ps.W - 1])
    m[7, :] = 0
    return m


@pytest.mark.parametrize("pose", ["diag_roll", "straight_down", "behind_left"])
@pytest.mark.parametrize("ctx", ["cornell", "triangles"])
def test_counts_render_parity(ctx, pose):
    name, _, _, geo, _ = CONTEXTS[ctx]
    s, sd = view(name, pose)
    counts = count_map()
    assert set(np.unique(counts)) == {0, 1, 5, 16, 17} and not counts[7].any() and counts[ps.H - 1].all()
    frames = adr.SampleFrames(s, sd, BOUNCES)
    with renderer(ctx, pose) as r:
        img, tot = r.render_counts(RenderParams(spp=17, bounces=BOUNCES), counts, totals=True)
        info = r.last_launch()
    assert info["kernel"] == f"rt::path_counts_kernel<{BOUNCES}, {geo}, false, true, 16>", info
    assert adr.same_words(tot, counts), adr.first_difference(tot, counts)
    want = frames.image(counts)
    assert adr.same_words(img, want), f"{ctx} at {pose}: " + adr.first_difference(img, want)


# ---- the MIS integrator -----------------------------------------------------------------------

@pytest.mark.parametrize("pose,light", [("rolled", "ceiling"), ("diag_roll", "ceiling"), ("straight_down", "ceiling"),
                                        ("behind_left", "ceiling"), ("cornell", "low")])
@pytest.mark.parametrize("layout,expect", [("auto", 6), ("single", 0)])
def test_mis_parity(layout, expect, pose, light):
    s, _ = view("mis", pose, light)
    ref, ref8 = oracle_lib.render_mis(s, 2, 9)
    assert np.isfinite(ref).all() and ref[..., :3].any()
    assert s.describe(Options(layout=layout))["kernel_layout"] == expect  # rt_last_launch does not cover rt_render_mis
    with Renderer(s, options=Options(layout=layout)) as r:
        out, out8 = r.render_mis(MisParams(camera_rays=2, mis_samples=9))
    same_bits(out, ref, f"MIS sum at {pose}, light {light}, layout {layout}")
    assert np.array_equal(out8, ref8)


# ---- ray queries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,geo", [("auto", 7), ("pairs", 1)])
def test_far_camera_rays_hit_the_spheres_the_scan_hits(layout, geo):
    """The narrowest case of what ``narrow_far`` found: from (0, 0, 900) the
    sphere test's rounding lets the id-ordered scan accept rays up to 0.24
    beside a sphere of radius 0.1 (tests/test_poses.py), and boxes padded by
    the culling margin alone culled them.  The camera rays of sample 0 as ray
    queries, through the leaf-box walk of the sphere kernel and the 32-byte
    nodes of the pair layout, closest and any hit, against the numpy scan."""
    s, sd = view("spheres", "narrow_far")
    sc = rs.np_scene(s)
    yy, xx = np.meshgrid(np.arange(ps.H), np.arange(ps.W), indexing="ij")
    i = sd.ravel().astype(np.uint32)
    o, d = aov_ref.camera_rays(sc, xx.ravel(), yy.ravel(), aov_ref.onp.halton(i, 0), aov_ref.onp.halton(i, 1))
    rays = rs.pack(np.stack([np.broadcast_to(c, i.shape) for c in (o.x, o.y, o.z)], -1), np.stack([d.x, d.y, d.z], -1),
                   np.float32(0.001), np.float32(1000.0))
    want_t, want_id = rs.reference(sc, rays, False)
    assert np.count_nonzero(want_id >= s.n_triangles) >= 100, "the view shows spheres"
    with Renderer(s, options=Options(layout=layout)) as r:
        for any_hit in (False, True):
            got = r.trace_rays(rays, any_hit=any_hit)
            kernel = r.last_launch()["kernel"]
            assert kernel == f"rt::ray_query_kernel<{geo}, true, {'true' if any_hit else 'false'}>", kernel
            want = rs.reference(sc, rays, any_hit)
            assert rs.same(got, want), f"{layout} any={any_hit}: " + rs.first_difference(got, want)


@pytest.mark.parametrize("ctx", ["cornell", "triangles"])
def test_ray_queries_with_the_camera_at_900(ctx):
    """compile_scene scales the culling margin and the exactness domain with
    max|camera.position|: 900 at ``narrow_far``, 9 in every other test.  Sets B
    and C of tests/ray_sets.py, closest and any hit, against the numpy scan."""
    name, _, _, geo, _ = CONTEXTS[ctx]
    s, _ = view(name, "narrow_far")
    assert s.ray_domain()["origin_max"] != view(name)[0].ray_domain()["origin_max"]
    sc = rs.np_scene(s)
    with renderer(ctx, "narrow_far") as r:
        for which, rays in zip("BC", rs.sets_bc()):
            for any_hit in (False, True):
                got = r.trace_rays(rays, any_hit=any_hit)
                kernel = r.last_launch()["kernel"]
                assert kernel == f"rt::ray_query_kernel<{geo}, false, {'true' if any_hit else 'false'}>", kernel
                want = rs.reference(sc, rays, any_hit)
                assert rs.same(got, want), f"{ctx} set {which} any={any_hit}: " + rs.first_difference(got, want)
