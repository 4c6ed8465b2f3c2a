"""CPU: the path queries' reference (tests/paths_ref.py) against
the C oracle, the properties of the chosen ray set that the GPU tests trace
(tests/path_ray_sets.py), and the layout of rt_path_params."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib
import path_ray_sets as prs
import paths_ref as pr
import ray_sets
from gpuraytracer_amd import Scene, lib, seed_splitmix
from gpuraytracer_amd._native import PathParamsC

W, H = 16, 12


@functools.lru_cache(maxsize=None)
def scene_of(name, w=W, h=H):
    if name == "cornell":
        return Scene.cornell_box(w, h)
    if name == "spheres":
        return Scene.random_spheres(w, h, 60, seed=19)
    return Scene.random_triangles(w, h, 200)


def check(got, want, what):
    assert pr.same_words(got, want), f"{what}: {pr.first_difference(got, want)}"


@pytest.mark.parametrize("bounces", [0, 1, 3])
@pytest.mark.parametrize("name", ["cornell", "spheres", "triangles"])
def test_reference_reproduces_the_oracle_on_camera_rays(name, bounces):
    """The camera ray of pixel p, sample n, with the pixel's seed, spp = 1 and
    sample_base = n is the oracle's sample n of that pixel, bit for bit."""
    s = scene_of(name)
    sc, dom = pr.np_scene(s), s.ray_domain()
    sd = seed_splitmix(W, H, key=40 + bounces)
    for n in (0, 3):
        rays, seeds = prs.camera_rays(sc, sd, n)
        assert pr.in_domain(rays, dom).all()
        paths = pr.Paths(sc, rays, seeds, 1, bounces, dom, sample_base=n)
        want = oracle_lib.render(s, sd, 1, bounces, sample_base=n).reshape(-1, 4)
        check(paths.radiance(1), want, f"{name}, {bounces} bounces, sample {n}")
        if bounces == 3:
            assert np.any(want[:, :3] != 0)


def test_seeds_are_masked_to_20_bits():
    s = scene_of("cornell")
    sc, dom = pr.np_scene(s), s.ray_domain()
    sd = seed_splitmix(W, H, key=7)
    rays, seeds = prs.camera_rays(sc, sd, 0)
    high = seeds | (np.arange(len(seeds), dtype=np.uint32) << np.uint32(20))
    assert np.any(high != seeds)
    check(pr.Paths(sc, rays, high, 2, 3, dom).radiance(2), pr.Paths(sc, rays, seeds, 2, 3, dom).radiance(2), "masked")


@pytest.mark.parametrize("name", ["cornell", "spheres", "triangles"])
def test_first_hits_are_the_ray_query_reference(name):
    s = scene_of(name)
    sc, dom = pr.np_scene(s), s.ray_domain()
    rays, out = prs.ray_set(s, sc, dom)
    t, ids, traced = pr.first_hits(sc, rays, dom)
    assert np.array_equal(traced, ~out)
    wt, wi = ray_sets.reference(sc, rays[~out])
    assert ray_sets.same((t[~out], ids[~out]), (wt, wi)), ray_sets.first_difference((t[~out], ids[~out]), (wt, wi))
    check(t[out], rays[out, 7], "tmax of the untraced rays")
    assert (ids[out] == -1).all()


def test_chosen_ray_set_properties():
    s = scene_of("cornell")
    sc, dom = pr.np_scene(s), s.ray_domain()
    rays, out = prs.ray_set(s, sc, dom)
    assert rays.shape == (prs.N_RAYS, 8) and prs.N_RAYS % 64 and prs.N_RAYS % 16 and prs.N_RAYS % 4
    inside = pr.in_domain(rays, dom)
    assert np.array_equal(inside, ~out) and np.array_equal(inside, ray_sets.in_domain(rays, dom))
    assert 2 * np.count_nonzero(inside) > prs.N_RAYS
    # every kind of out_of_domain_variants is there (21 kinds, cycled)
    assert np.count_nonzero(out) >= 2 * 21
    # one wave holds traced and untraced rays, a 16-lane row's neighbours differ, one wave holds none
    w = out[prs.OUT_MIXED[0] // 64 * 64 + 64:][:64]
    assert w.any() and not w.all() and np.any(w[:-1] != w[1:])
    assert prs.OUT_BLOCK[0] % 64 == 0 and out[prs.OUT_BLOCK[0]:prs.OUT_BLOCK[0] + 64].all()
    t, ids, _ = pr.first_hits(sc, rays, dom)
    hit = ids[inside]
    assert (hit == -1).any(), "no miss"
    lights = [k for k, T in enumerate(sc.tris) if T["light"]]
    assert lights and all((hit == k).any() for k in lights), "no direct light hit"
    assert set(range(36)) <= set(hit.tolist()), sorted(set(range(36)) - set(hit.tolist()))
    # tmax / tmin at a known hit changed the answer of those rays
    B = ray_sets.sets_bc()[0]
    bt, bi = ray_sets.reference(sc, B[:384])
    assert not ray_sets.same((t[584:648], ids[584:648]), (bt[bi >= 0][:64], bi[bi >= 0][:64]))
    # a condition on the inputs: no first segment is decided by rounding residues
    assert not ray_sets.residue_hits(sc, rays[inside]).any()
    for name in ("spheres", "triangles"):
        s2 = scene_of(name)
        sc2, dom2 = pr.np_scene(s2), s2.ray_domain()
        r2, o2 = prs.ray_set(s2, sc2, dom2)
        assert np.array_equal(pr.in_domain(r2, dom2), ~o2)
        assert not ray_sets.residue_hits(sc2, r2[~o2]).any(), name


def test_untraced_rays_and_misses_differ_in_alpha():
    s = scene_of("cornell")
    sc, dom = pr.np_scene(s), s.ray_domain()
    rays, out = prs.ray_set(s, sc, dom)
    paths = pr.Paths(sc, rays, seed_splitmix(prs.N_RAYS, 1, key=3), 2, 3, dom)
    rad = paths.radiance(2)
    assert (rad[out] == 0).all() and (rad[~out, 3] == 1).all()
    miss = ~out & (paths.ids < 0)
    assert miss.any() and (rad[miss, :3] == 0).all()
    assert np.any(rad[~out, :3] != 0)


def test_path_params_layout_and_default():
    assert ctypes.sizeof(PathParamsC) == 32
    offs = {n: getattr(PathParamsC, n).offset for n, _ in PathParamsC._fields_}
    assert offs == dict(spp=0, bounces=4, sample_base=8, lanes_per_ray=12, seed_key=16, flags=24, reserved=28)
    p = PathParamsC()
    ctypes.memset(ctypes.byref(p), 0xFF, 32)
    lib.rt_path_params_default(ctypes.byref(p))
    assert (p.spp, p.bounces, p.sample_base, p.lanes_per_ray, p.seed_key, p.flags, p.reserved) == (1, 3, 0, 0, 0, 0, 0)
    lib.rt_path_params_default(None)  # a null pointer is ignored


def test_null_context_is_an_argument_error():
    p = PathParamsC()
    assert lib.rt_trace_paths(None, ctypes.byref(p), None, None, 0, None, None) == 1
    assert lib.rt_trace_paths_async(None, ctypes.byref(p), None, None, 0, None, None, None) == 1
    assert b"null" in lib.rt_last_error(None)
