"""GPU: every entry point on scenes scaled, moved and turned as a whole
(tests/transform_scenes.py), bit for bit against the CPU
references that tests/test_transforms.py pins at the same transforms.  The
rest of the suite renders the Cornell room world-aligned about the origin, 5
units across; the constants of the headline path -- tmin, tmax and the 1e-3
lifts of the reference, the culling margin's extent floor, the tolerances of the
cluster compiler, the own-light rule, the exact world-axis tests, the light
shafts' 1e-3 terms -- mean something only at that scale and orientation.

One 64 x 48 frame, one seed texture, 8 spp and 3 bounces (16 spp where 16
lanes per pixel run).  An oracle frame is computed once per (scene, transform,
spp) and shared.  Every case names the kernel it ran through last_launch(), so
that a transform cannot change the layout unseen; the MIS launcher reports
none, its cases assert the layout the context describes."""
import functools

import numpy as np
import pytest

import adaptive_ref as adr
import aov_ref
import oracle_lib
import path_ray_sets as prs
import paths_ref as pr
import ray_sets as rs
import transform_scenes as ts
from gpuraytracer_amd import MisParams, Options, RenderParams, Renderer
from test_gpu_camera_candidates import same_bits
from test_gpu_poses import BOUNCES, CONTEXTS, SCENES, SPP, count_map, kernel_prefix, seeds_of
from test_gpu_wave_masks import check_records, check_table
from test_transforms import KINDS, NAMES, ray_case

pytestmark = pytest.mark.gpu
OWN_LIGHT = 128


@functools.lru_cache(maxsize=None)
def scene_at(scene, tr="id"):
    return ts.apply(SCENES[scene](ts.W, ts.H), tr)


@functools.lru_cache(maxsize=None)
def oracle(scene, tr="id", spp=SPP):
    ref = oracle_lib.render(scene_at(scene, tr), seeds_of(ts.W, ts.H), spp, BOUNCES)
    ref.setflags(write=False)
    return ref


def renderer(ctx, tr="id", **more):
    name, opt = CONTEXTS[ctx][:2]
    return Renderer(scene_at(name, tr), seeds=seeds_of(ts.W, ts.H), options=Options(**opt, **more))


# ---- rt_render ----------------------------------------------------------------------

@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_render_parity(ctx, tr):
    """Every context at every transform.  For ``spheres`` the room moves with
    the spheres, and the quadratic sphere padding (rt_scene.cpp sphere_margin)
    has to hold at ``x100`` and ``offset900`` with the spheres, not the camera
    alone, far from the origin."""
    with renderer(ctx, tr) as r:
        out = r.render(RenderParams(spp=SPP, bounces=BOUNCES))
        info = r.last_launch()
    assert info["kernel"].startswith(kernel_prefix(ctx)), (ctx, tr, info)
    same_bits(out, oracle(CONTEXTS[ctx][0], tr), f"{ctx} at {tr}")


@pytest.mark.parametrize("tr", ts.CORE)
@pytest.mark.parametrize("lanes,spp", [(1, 8), (4, 8), (16, 16)])
def test_cluster_kernel_lanes(tr, lanes, spp):
    with renderer("cornell", tr, lanes=lanes) as r:
        out = r.render(RenderParams(spp=spp, bounces=BOUNCES))
        info = r.last_launch()
    assert info["kernel"] == kernel_prefix("cornell") + f"true, {lanes}>" and info["lanes_per_pixel"] == lanes, info
    same_bits(out, oracle("cornell", tr, spp), f"{tr}, {lanes} lanes")


@pytest.mark.parametrize("tr", ts.CORE)
@pytest.mark.parametrize("lanes,spp", [(4, 8), (16, 16)])
def test_cluster_kernel_interleaved_rows(tr, lanes, spp):
    with renderer("cornell", tr, lanes=lanes) as r:
        out = r.render(RenderParams(spp=spp, bounces=BOUNCES, row_start=1, row_step=3))
        info = r.last_launch()
    assert info["kernel"] == kernel_prefix("cornell") + f"true, {lanes}>", info
    same_bits(out, oracle("cornell", tr, spp)[1::3], f"{tr}, rows 1 (mod 3), {lanes} lanes")


# ---- the mask table -------------------------------------------------------------------

@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("lanes,spp,shape", [(4, 8, (4, 4)), (16, 16, (2, 2))])
@pytest.mark.parametrize("scene", ["cornell", "boxes0"])
def test_wave_mask_table_equals_the_host(scene, lanes, spp, shape, tr):
    """The device table equals the host twins on every wave (check_table).  The
    camera looks at the room from outside at every transform: some wave has
    one camera pair and a decided occluder mask."""
    s = scene_at(scene, tr)
    assert s.describe()["kernel_layout"] == 6
    seen = check_table(s, RenderParams(spp=spp, bounces=BOUNCES), lanes, shape)
    assert any(cam == 1 and avail for cam, avail, _ in seen), "no one-pair wave with a decided mask"


# ---- the update chain -------------------------------------------------------------------

def test_update_chain_through_every_transform_on_the_cluster_kernel():
    """One context walked through every transform in table order and back with
    update_scene: after each step the frame equals the oracle's and the
    wave-mask table the host twins', as a fresh context's do
    (test_render_parity, test_wave_mask_table_equals_the_host).  The cluster
    count goes 4 -> 5 -> 7 and back, the own-light flag comes and goes."""
    p = RenderParams(spp=SPP, bounces=BOUNCES)
    kernel = kernel_prefix("cornell") + "true, 4>"
    steps = ts.MOVED + ["id"]
    counts, own = [], []
    with renderer("cornell", lanes=4) as r:
        same_bits(r.render(p), oracle("cornell"), "cornell before any update")
        assert r.last_launch()["kernel"] == kernel
        for k, tr in enumerate(steps):
            s = scene_at("cornell", tr)
            r.update_scene(s)
            same_bits(r.render(p), oracle("cornell", tr), f"update {k}: {tr}")
            assert r.last_launch()["kernel"] == kernel, (tr, r.last_launch())
            rec, fills = r.wave_masks(p)
            assert fills == 2 + k, f"update {k} ({tr}): one refill"
            check_records(s, p, rec, (4, 4))
            counts.append(len(KINDS["cornell"][tr]))
            own.append(any(f & OWN_LIGHT for f in KINDS["cornell"][tr]))
        assert r.update_info()["updates"] == len(steps)
    assert {4, 5, 7} <= set(counts) and True in own and False in own and own[-1]


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
def test_update_chain_through_every_transform_on_the_triangle_bvh(rebuild):
    p = RenderParams(spp=SPP, bounces=BOUNCES)
    steps = ts.MOVED + ["id"]
    with renderer("triangles") as r:
        same_bits(r.render(p), oracle("triangles"), "triangles before any update")
        for k, tr in enumerate(steps):
            r.update_scene(scene_at("triangles", tr), rebuild=rebuild)
            assert r.update_info()["tri_bvh"] == (2 if rebuild else 1)
            same_bits(r.render(p), oracle("triangles", tr), f"update {k}: {tr}, rebuild={rebuild}")
            assert r.last_launch()["kernel"].startswith(kernel_prefix("triangles")), (tr, r.last_launch())
        assert r.update_info()["updates"] == len(steps)


# ---- feature buffers -----------------------------------------------------------------------

AOV_SPP = 3


@pytest.mark.parametrize("tr", ts.KEY)
@pytest.mark.parametrize("ctx", ["cornell", "spheres", "triangles"])
def test_aov_parity(ctx, tr):
    name, _, _, geo, sph = CONTEXTS[ctx]
    s, sd = scene_at(name, tr), seeds_of(ts.W, ts.H)
    sc = aov_ref.np_scene(s)
    want = aov_ref.buffers(sc, sd, AOV_SPP)
    centre = aov_ref.buffers(sc, None, 1, center=True)
    with renderer(ctx, tr) as r:
        got = r.render_aov(spp=AOV_SPP)
        info = r.last_launch()
        got_centre = r.render_aov(center=True)
    assert info["kernel"] == f"rt::aov_kernel<{geo}, {'true' if sph else 'false'}, true>", info
    for k in ("albedo", "normal_depth", "first_hit"):
        assert aov_ref.same(got[k], want[k]), f"{ctx} at {tr}, {k}: " + aov_ref.first_difference(got[k], want[k])
        assert aov_ref.same(got_centre[k], centre[k]), \
            f"{ctx} at {tr}, centre {k}: " + aov_ref.first_difference(got_centre[k], centre[k])
    assert len(np.unique(want["first_hit"]["id"])) >= 3
    if not sph:
        assert np.array_equal(got_centre["first_hit"]["id"], oracle_lib.primary_ids(s))


# ---- ray queries ------------------------------------------------------------------------------

RAY_CONTEXTS = {"cornell": 6, "spheres": 7, "tri400": 5}


@pytest.mark.parametrize("tr", ts.KEY)
@pytest.mark.parametrize("name", list(RAY_CONTEXTS))
def test_ray_queries(name, tr):
    """Sets B, C, D and E of the transformed scene (tests/test_transforms.py
    ray_case: at least half of each inside the exactness domain), closest and
    any hit, on the accelerated path and, for B, through RT_RAYS_EXACT, against
    the numpy scan."""
    s, sc, _, sets = ray_case(name, tr)
    geo, sph = RAY_CONTEXTS[name], "true" if s.n_spheres else "false"
    with Renderer(s) as r:
        for which, rays in sets.items():
            for any_hit in (False, True):
                want = rs.reference(sc, rays, any_hit)
                for exact in ((False, True) if which == "B" else (False,)):
                    got = r.trace_rays(rays, any_hit=any_hit, exact=exact)
                    kernel = r.last_launch()["kernel"]
                    assert kernel == f"rt::ray_query_kernel<{geo}, {sph}, {'true' if any_hit else 'false'}>", kernel
                    assert rs.same(got, want), \
                        f"{name} at {tr}, set {which} any={any_hit} exact={exact}: " + rs.first_difference(got, want)


# ---- path queries --------------------------------------------------------------------------------

@pytest.mark.parametrize("tr", ts.KEY)
@pytest.mark.parametrize("ctx", ["cornell", "spheres", "triangles"])
def test_path_queries_equal_the_renders_samples(ctx, tr):
    """The camera rays of sample 0 as path queries, at one and at sixteen lanes
    per ray: the oracle's single-sample frame."""
    name, _, _, geo, sph = CONTEXTS[ctx]
    s, sd = scene_at(name, tr), seeds_of(ts.W, ts.H)
    rays, seeds = prs.camera_rays(pr.np_scene(s), sd, 0)
    assert pr.in_domain(rays, s.ray_domain()).all()
    want = np.ones((ts.W * ts.H, 4), np.float32)
    want[:, :3] = oracle_lib.render(s, sd, 1, BOUNCES)[..., :3].reshape(-1, 3)
    with renderer(ctx, tr) as r:
        for lanes in (1, 16):
            got = r.trace_paths(rays, spp=1, bounces=BOUNCES, seeds=seeds, lanes=lanes)
            info = r.last_launch()
            assert info["kernel"] == f"rt::path_query_kernel<{BOUNCES}, {geo}, {'true' if sph else 'false'}, true, {lanes}>", info
            assert pr.same_words(got, want), f"{ctx} at {tr}, {lanes} lanes: " + pr.first_difference(got, want)


# ---- per-pixel sample counts -------------------------------------------------------------------------

@pytest.mark.parametrize("tr", ts.KEY)
@pytest.mark.parametrize("ctx", ["cornell", "triangles"])
def test_counts_render_parity(ctx, tr):
    name, _, _, geo, _ = CONTEXTS[ctx]
    s, sd = scene_at(name, tr), seeds_of(ts.W, ts.H)
    counts = count_map()
    frames = adr.SampleFrames(s, sd, BOUNCES)
    with renderer(ctx, tr) as r:
        img, tot = r.render_counts(RenderParams(spp=17, bounces=BOUNCES), counts, totals=True)
        info = r.last_launch()
    assert info["kernel"] == f"rt::path_counts_kernel<{BOUNCES}, {geo}, false, true, 16>", info
    assert adr.same_words(tot, counts), adr.first_difference(tot, counts)
    want = frames.image(counts)
    assert adr.same_words(img, want), f"{ctx} at {tr}: " + adr.first_difference(img, want)


# ---- the MIS integrator ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tr", ts.KEY)
@pytest.mark.parametrize("layout,expect", [("auto", 6), ("single", 0)])
def test_mis_parity(layout, expect, tr):
    s = scene_at("mis", tr)
    ref, ref8 = oracle_lib.render_mis(s, 2, 9)
    assert np.isfinite(ref).all() and ref[..., :3].any()
    assert s.describe(Options(layout=layout))["kernel_layout"] == expect  # rt_last_launch does not cover rt_render_mis
    with Renderer(s, options=Options(layout=layout)) as r:
        out, out8 = r.render_mis(MisParams(camera_rays=2, mis_samples=9))
    same_bits(out, ref, f"MIS sum at {tr}, layout {layout}")
    assert np.array_equal(out8, ref8)
