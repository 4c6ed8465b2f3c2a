"""The shapes at which the kernels' shared copy loop (rt_trace.hpp
stage_records) can go wrong and which no other scene pins, through every
kernel that calls it:

  (a) the smallest pair scene, one quad + the light pair: 2 pairs = 14 float4,
      fewer than one wave of copy lanes (and 2 flat box clusters = 14 more);
  (b) 36 quads + the light pair: 37 pairs = 259 float4, three past one pass of
      a 256-thread workgroup, four passes and a tail of the one-wave kernels,
      no multiple of 64.  (Box clusters exist up to 31 pairs, rt_scene.cpp, so
      the lockstep kernel of (b) is the plain pair kernel.)

Renders at 16x16, 2 spp, 3 bounces are compared bit for bit with the C oracle,
the MIS kernel with its numpy restatement, 65 rays (one wave and one ray) with
the id-ordered scan of tests/ray_sets.py.  Each case also states the kernel it
ran and that the launch requested exactly the layout's staged bytes.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_sets as rs
from gpuraytracer_amd import MisParams, Options, RenderParams, Renderer, Scene, seed_splitmix
from test_gpu_mis import assert_same
from test_gpu_parity import assert_parity, random_quad_scene

W = H = 16
SPP, BOUNCES = 2, 3
PAIR, CLU, HALTON, SORT = 112, 112, 4 * 4679, 16 * 1097  # bytes: pair record, box cluster, Halton tables, sort buffers
QUADS = {"a": (1, 2), "b": (36, 12)}  # scene -> (quads, seed of random_quad_scene)


@functools.lru_cache(maxsize=None)
def scene_of(name, spheres=False):
    n_quads, seed = QUADS[name]
    s = random_quad_scene(W, H, n_quads, seed)
    assert s.describe()["n_triangle_pairs"] == n_quads + 1
    if spheres:
        s = Scene(s.camera, s.materials, s.vertices, s.light, Scene.random_spheres(W, H, 5, seed=7).spheres)
    return s


@functools.lru_cache(maxsize=None)
def seeds_of(name):
    return seed_splitmix(W, H, key=QUADS[name][1])


@functools.lru_cache(maxsize=None)
def oracle_of(name, spheres=False):
    ref = oracle_lib.render(scene_of(name, spheres), seeds_of(name), SPP, BOUNCES)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("spheres", [False, True])
def test_oracle_renders_the_scenes_without_nan(name, spheres):
    """CPU: every pixel of every reference is a number and some are lit, so no
    case below needs excluding."""
    ref = oracle_of(name, spheres)
    assert not np.isnan(ref).any()
    assert (ref[..., :3] > 0).any()


# (scene, spheres, options, kernel prefix, dynamic LDS of nP pairs and nC clusters)
CASES = {
    "a-clustered": ("a", False, {}, "rt::path_trace_kernel<3, 6, false,", lambda nP, nC: PAIR * nP + CLU * nC + HALTON),
    "a-pairs": ("a", False, {"layout": "pairs"}, "rt::path_trace_kernel<3, 1, false,", lambda nP, nC: PAIR * nP),
    "a-sorted": ("a", False, {"layout": "sorted"}, "rt::path_trace_sorted_kernel<3, 1, false,", lambda nP, nC: SORT + PAIR * nP),
    "a-sphere": ("a", True, {}, "rt::path_trace_kernel<3, 7, true,", lambda nP, nC: PAIR * nP),
    "a-sphere-free": ("a", True, {"walk": "free"}, "rt::path_free_kernel<3, 7, true,", lambda nP, nC: PAIR * nP),
    "a-sphere-sorted": ("a", True, {"walk": "sorted"}, "rt::path_trace_sorted_kernel<3, 7, true,", lambda nP, nC: SORT + PAIR * nP),
    "b-lockstep": ("b", False, {}, "rt::path_trace_kernel<3, 1, false,", lambda nP, nC: PAIR * nP),
    "b-pairs": ("b", False, {"layout": "pairs"}, "rt::path_trace_kernel<3, 1, false,", lambda nP, nC: PAIR * nP),
    "b-sorted": ("b", False, {"layout": "sorted"}, "rt::path_trace_sorted_kernel<3, 1, false,", lambda nP, nC: SORT + PAIR * nP),
    "b-sphere": ("b", True, {}, "rt::path_trace_kernel<3, 7, true,", lambda nP, nC: PAIR * nP),
    "b-sphere-free": ("b", True, {"walk": "free"}, "rt::path_free_kernel<3, 7, true,", lambda nP, nC: PAIR * nP),
    "b-sphere-sorted": ("b", True, {"walk": "sorted"}, "rt::path_trace_sorted_kernel<3, 7, true,", lambda nP, nC: SORT + PAIR * nP),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_render_bit_exact_vs_oracle(case):
    name, spheres, opt, kernel, lds = CASES[case]
    s = scene_of(name, spheres)
    info = s.describe()
    assert (info["n_box_clusters"] > 0) == (name == "a"), info
    with Renderer(s, seeds=seeds_of(name), options=Options(**opt)) as r:
        out = r.render(RenderParams(spp=SPP, bounces=BOUNCES))
        L = r.last_launch()
    assert L["kernel"].startswith(kernel), L
    assert L["lds_bytes"] == lds(info["n_triangle_pairs"], info["n_box_clusters"]), L
    assert_parity(out, oracle_of(name, spheres), case)


@pytest.mark.gpu
def test_mis_kernel_37_pairs_vs_numpy_restatement():
    import pt_oracle_mis_np as M
    s = scene_of("b")
    with np.errstate(all="ignore"):  # the restatement evaluates both sides of its selects
        ref, ref8 = M.render_mis(M.Scene(s.camera, s.materials, s.light, s.vertices), 2, 6)
    assert not np.isnan(ref).any() and (ref[..., :3] > 0).any()
    with Renderer(s) as r:
        out, out8 = r.render_mis(MisParams(camera_rays=2, mis_samples=6))
    assert_same(out, ref, "sum")
    assert_same(out8, ref8, "rgba8")


@pytest.mark.gpu
@pytest.mark.parametrize("any_hit", [False, True])
def test_65_rays_37_pairs_vs_scan(any_hit):
    s = scene_of("b")
    rays = rs.sets_bc()[0][:65]
    want = rs.reference(rs.np_scene(s), rays, any_hit)
    with Renderer(s) as r:
        got = r.trace_rays(rays, any_hit=any_hit)
        L = r.last_launch()
    assert L["kernel"] == f"rt::ray_query_kernel<1, false, {'true' if any_hit else 'false'}>", L
    assert L["lds_bytes"] == PAIR * 37 and L["grid_x"] == 1, L
    assert rs.same(got, want), rs.first_difference(got, want)
