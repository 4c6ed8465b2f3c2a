"""GPU: the device buffers a context owns (rt_api.cpp DevBuf) over their whole
life -- staging that grows and is reused when smaller, the output staging
shared between pixel formats and the MIS integrator, the running sum's
reallocation, the tree and its refit table through refit / rebuild / refit,
and teardown with every buffer live.  Every comparison is bit for bit, against
a context newly created for that one call or against the CPU oracle.

The Cornell box at 32 x 24 unless a test says otherwise."""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_sets as rs
import tri_bvh_scenes as ts
import update_scenes as us
from gpuraytracer_amd import (MisParams, Options, RenderParams, Renderer, RtError, Scene, comm_unique_id, lib,
                              seed_splitmix)
from test_gpu_denoise import synth
from test_gpu_parity import assert_parity
from test_gpu_update_scene import assert_same_dump

pytestmark = pytest.mark.gpu
W, H = 32, 24
OK, STATE = 0, 5


@functools.lru_cache(maxsize=None)
def cornell():
    return Scene.cornell_box(W, H)


@functools.lru_cache(maxsize=None)
def seeds():
    s = seed_splitmix(W, H)
    s.setflags(write=False)
    return s


def fresh(call, **kw):
    """``call(r)`` on a context created for it alone."""
    with Renderer(cornell(), seeds=seeds(), **kw) as r:
        return call(r)


def same_bytes(got, want, what):
    """Arrays, or tuples / dicts of arrays, equal byte for byte."""
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        got, want = tuple(got[k] for k in want), tuple(want.values())
    if not isinstance(want, tuple):
        got, want = (got,), (want,)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what} [{k}]"


def check_sequence(steps, **kw):
    """Every step on ONE context, in order; then each against a fresh context."""
    with Renderer(cornell(), seeds=seeds(), **kw) as r:
        got = [call(r) for _, call in steps]
    for (what, call), g in zip(steps, got):
        same_bytes(g, fresh(call, **kw), what)


# ---- a: ray staging grows, then is reused when smaller -----------------------------

def test_ray_staging_grows_and_is_reused():
    rays = np.concatenate(rs.sets_bc())  # 8192 rays; 4097 = two 2048-ray chunks and one ray
    check_sequence([(f"{n} rays", lambda r, n=n: r.trace_rays(rays[:n])) for n in (64, 4097, 1, 2048)])


# ---- b: the output staging shared by the pixel formats and the MIS integrator ------

def test_output_staging_shared_between_formats_and_mis():
    p = dict(spp=2, bounces=2)
    check_sequence([
        ("one row fp32", lambda r: r.render(RenderParams(row_count=1, **p))),
        ("frame rgba8", lambda r: r.render(RenderParams(rgba8=True, **p))),
        ("two rows fp16", lambda r: r.render(RenderParams(row_count=2, fp16=True, **p))),
        ("mis, both outputs", lambda r: r.render_mis(MisParams(camera_rays=2, mis_samples=6))),
        ("frame fp32", lambda r: r.render(RenderParams(**p))),
    ])


# ---- c: the running sum's reallocation and validity ---------------------------------

def test_sum_reallocation_drops_the_old_partition():
    two = dict(spp=1, bounces=2, row_count=2)
    with Renderer(cornell(), seeds=seeds()) as r:
        r.render(RenderParams(keep_sum=True, **two))
        out = r.render(RenderParams(sample_base=1, accumulate=True, **two))  # the sum is there
        r.render(RenderParams(spp=1, bounces=2, keep_sum=True))               # the whole frame: a larger sum
        with pytest.raises(RtError) as e:
            r.render(RenderParams(sample_base=1, accumulate=True, **two))
        assert e.value.status == STATE
    same_bytes(out, fresh(lambda f: f.render(RenderParams(spp=2, bounces=2, row_count=2))), "2 rows, 1 + 1 samples")


# ---- d: feature-buffer and denoiser staging ------------------------------------------

def test_aov_and_denoise_staging():
    import torch
    bufs = synth(3, W, H)

    def on_device(r):
        t = {k: torch.from_numpy(v).to(f"cuda:{r.device}") for k, v in bufs.items()}
        return r.denoise(**t).cpu().numpy()

    check_sequence([
        ("albedo only", lambda r: r.render_aov(spp=2, normal_depth=False, first_hit=False)),
        ("all three", lambda r: r.render_aov(spp=2)),
        ("first_hit only", lambda r: r.render_aov(spp=2, albedo=False, normal_depth=False)),
        ("denoise host", lambda r: r.denoise(**bufs)),
        ("denoise device", on_device),
        ("denoise host again", lambda r: r.denoise(**bufs)),
    ])


# ---- e: the tree and its refit table through refit, rebuild, refit -------------------

def test_tree_lifetime_refit_rebuild_refit():
    name = "tiny1"  # the smallest scene of tests/update_scenes.py
    opt = ts.options(name)
    assert opt.layout == "bvh"
    with Renderer(ts.build(name), options=opt) as r:
        r.update_scene(us.build(name, "shift"))
        assert r.update_info()["tri_bvh"] == 1
        r.update_scene(us.build(name, "grow"), rebuild=True)
        assert r.update_info()["tri_bvh"] == 2
        with Renderer(us.build(name, "grow"), options=opt) as f:
            assert_same_dump(r.tri_bvh(), f.tri_bvh(), "after the rebuild")
        before = r.tri_bvh()
        r.update_scene(us.build(name, "grow"))  # a refit of the rebuilt tree onto the same triangles
        assert r.update_info()["tri_bvh"] == 1
        assert_same_dump(r.tri_bvh(), before, "refit onto the same triangles")
    with Renderer(cornell(), seeds=seeds()) as r:  # an LDS layout: no tree before, none after
        assert r.build_info()["tri_bvh_nodes"] == 0
        r.update_scene(Scene.cornell_box(W, H))
        info = r.build_info()
        assert r.update_info()["tri_bvh"] == 0 and info["tri_bvh_build"] == 0 and info["tri_bvh_nodes"] == 0, info


# ---- f: teardown with every buffer live ----------------------------------------------

def test_create_and_destroy_with_every_buffer_live():
    """Eight contexts in a row, each destroyed after every entry point has run
    once (a failing status raises RtError); then a ninth renders the oracle's image."""
    bufs = synth(5, W, H)
    rays = rs.sets_bc()[0][:64]
    opt = Options(layout="bvh")  # a tree, so that the update is a refit with its table
    for k in range(8):
        r = Renderer(cornell(), seeds=seeds(), options=opt)
        r.render(RenderParams(spp=1, bounces=2, keep_sum=True))
        r.render_mis(MisParams(camera_rays=3, mis_samples=6))  # 3 rays: a split launch with its records
        r.trace_rays(rays)
        r.render_aov(spp=1)
        r.denoise(**bufs)
        r.update_scene(cornell())
        assert r.update_info()["tri_bvh"] == 1
        r.comm_init(0, 1, comm_unique_id())
        r.render_gather(RenderParams(spp=1, bounces=2))
        ctx, r._ctx = r._ctx, None
        assert lib.rt_destroy(ctx) == OK, k
    out = fresh(lambda f: f.render(RenderParams(spp=2, bounces=2)))
    assert_parity(out, oracle_lib.render(cornell(), seeds(), 2, 2), "the ninth context")


# ---- g: one rule for the triangle BVH -------------------------------------------------

# rt_create builds a tree above 384 triangles, when the records fit neither LDS
# layout, or when the layout is forced.  No scene of under 384 triangles fits
# neither LDS layout (its single-triangle records are 48 B x 383 = 18 KB of the
# 64 KB), so the rule's other branches stand in for that case: the BVH layout
# forced below the threshold, and an LDS layout forced above it.
@pytest.mark.parametrize("name,layout,tree", [("soup384", "auto", False), ("soup385", "auto", True),
                                              ("soup100", "bvh", True), ("soup385", "single", False)])
def test_describe_and_create_agree_on_the_tree(name, layout, tree):
    scene, opt = ts.build(name), Options(layout=layout)
    described = scene.describe(opt)["n_triangle_bvh_nodes"] != 0
    with Renderer(scene, options=opt) as r:
        built = r.build_info()["tri_bvh_nodes"] != 0
    assert described == built == tree, (name, layout, described, built)
