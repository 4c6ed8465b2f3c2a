"""GPU: path queries (rt_trace_paths) on every lockstep layout
at one and at sixteen lanes per ray, bit for bit on uint32 views: the camera
rays of a frame against the C oracle's single-sample frames, the chosen ray set
(tests/path_ray_sets.py) against tests/paths_ref.py and Renderer.trace_rays,
the seed rules, the invariants of a ray's result, and the argument checks."""
import ctypes
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import path_ray_sets as prs
import paths_ref as pr
import ray_sets
from gpuraytracer_amd import Options, Renderer, RtError, Scene, lib, seed_splitmix
from gpuraytracer_amd._native import PathParamsC
from test_gpu_adaptive import CONTEXTS, H, W, scene_of

pytestmark = pytest.mark.gpu
SPPS = (1, 5, 16, 17, 33)
LANES = (1, 16)
RT_ERR_INVALID_ARG = 1


def check(got, want, what):
    assert pr.same_words(got, want), f"{what}: {pr.first_difference(got, want)}"


@functools.lru_cache(maxsize=None)
def np_scene(name):
    s = scene_of(name)
    return s, pr.np_scene(s), s.ray_domain()


@functools.lru_cache(maxsize=None)
def frames_of(name, bounces):
    """The oracle's single-sample frames of a scene from sample 0 on, and the seeds."""
    sd = seed_splitmix(W, H, key=50 + bounces)
    return sd, ar.SampleFrames(scene_of(name), sd, bounces)


@functools.lru_cache(maxsize=None)
def set_of(name):
    """The chosen ray set of a scene, its seeds and its reference: 33 samples a ray, traced once."""
    s, sc, dom = np_scene(name)
    rays, out = prs.ray_set(s, sc, dom)
    seeds = seed_splitmix(prs.N_RAYS, 1, key=61).reshape(-1)
    return rays, out, seeds, pr.Paths(sc, rays, seeds, max(SPPS), 3, dom)


def kernel_name(ctx, bounces, lanes):
    _, _, layout, sph = CONTEXTS[ctx]
    return None if layout is None else f"rt::path_query_kernel<{bounces}, {layout}, {'true' if sph else 'false'}, true, {lanes}>"


def renderer(ctx):
    name, opt, _, _ = CONTEXTS[ctx]
    return Renderer(scene_of(name), options=Options(lanes=4, **opt))  # no seeds; lanes_per_pixel is ignored


@pytest.mark.parametrize("bounces", [0, 1, 3])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_camera_rays_equal_the_oracles_samples(ctx, bounces):
    name = CONTEXTS[ctx][0]
    _, sc, _ = np_scene(name)
    sd, frames = frames_of(name, bounces)
    with renderer(ctx) as r:
        for base in (0, 5):
            rays, seeds = prs.camera_rays(sc, sd, base)
            want = np.ones((W * H, 4), np.float32)
            want[:, :3] = frames.frame(base).reshape(-1, 3)
            for lanes in LANES:
                got = r.trace_paths(rays, spp=1, bounces=bounces, sample_base=base, seeds=seeds, lanes=lanes)
                info = r.last_launch()
                assert "rt::path_query_kernel<" in info["kernel"] and info["lanes_per_pixel"] == lanes, info
                if kernel_name(ctx, bounces, lanes):
                    assert info["kernel"] == kernel_name(ctx, bounces, lanes), info
                check(got, want, f"sample {base}, {lanes} lanes")


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_ray_set_equals_the_reference(ctx, lanes):
    rays, out, seeds, paths = set_of(CONTEXTS[ctx][0])
    wt, wi = paths.hits()
    with renderer(ctx) as r:
        for spp in SPPS:
            rad, (t, ids) = r.trace_paths(rays, spp=spp, bounces=3, seeds=seeds, lanes=lanes, first_hits=True)
            assert r.last_launch()["lanes_per_pixel"] == lanes
            check(rad, paths.radiance(spp), f"radiance at {spp} spp")
            check(t, wt, f"first-hit t at {spp} spp")
            assert np.array_equal(ids, wi), f"first-hit id at {spp} spp"
        qt, qi = r.trace_rays(rays[~out])
    assert ray_sets.same((t[~out], ids[~out]), (qt, qi)), ray_sets.first_difference((t[~out], ids[~out]), (qt, qi))
    assert (rad[out] == 0).all() and (rad[~out, 3] == 1).all()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ctx", ["cornell", "spheres", "triangles"])
def test_seed_rules(ctx, lanes):
    rays, _, seeds, paths = set_of(CONTEXTS[ctx][0])
    key = 0x1234567
    high = seeds | (np.arange(len(seeds), dtype=np.uint32) << np.uint32(20)) | np.uint32(0x80000000)
    with renderer(ctx) as r:
        none = r.trace_paths(rays, spp=5, seed_key=key, lanes=lanes)
        explicit = r.trace_paths(rays, spp=5, seeds=seed_splitmix(len(rays), 1, key=key), lanes=lanes)
        masked = r.trace_paths(rays, spp=5, seeds=high, lanes=lanes)
    check(none, explicit, "seeds=None against seed_splitmix")
    check(masked, paths.radiance(5), "seeds with high bits")
    assert not pr.same_words(none, masked)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ctx", ["cornell", "cornell-pairs", "spheres", "triangles"])
def test_a_rays_result_does_not_depend_on_its_batch(ctx, lanes):
    rays, _, seeds, paths = set_of(CONTEXTS[ctx][0])
    want, (wt, wi) = paths.radiance(17), paths.hits()
    perm = np.random.default_rng(8).permutation(len(rays))[:333]
    with renderer(ctx) as r:
        rad, (t, ids) = r.trace_paths(rays[perm], spp=17, seeds=seeds[perm], lanes=lanes, first_hits=True)
        check(rad, want[perm], "a permuted sub-batch")
        check(t, wt[perm], "its first-hit t")
        assert np.array_equal(ids, wi[perm])
        for k in (0, 449, 600, 713, 1002):  # a hit, a light ray, a dropped hit, a mixed-wave ray, the last
            one = r.trace_paths(rays[k:k + 1], spp=17, seeds=seeds[k:k + 1], lanes=lanes)
            assert r.last_launch()["grid_x"] == 1
            check(one, want[k:k + 1], f"ray {k} alone")


@pytest.mark.parametrize("lanes", LANES)
def test_many_rays_take_several_passes_per_workgroup(lanes):
    """Past 2048 workgroups a workgroup loops over several passes of rays: 600
    copies of the ray set give every copy the words of the set traced alone."""
    rays, _, seeds, paths = set_of("cornell")
    copies = 600
    with renderer("cornell") as r:
        got = r.trace_paths(np.tile(rays, (copies, 1)), spp=1, seeds=np.tile(seeds, copies), lanes=lanes)
        info = r.last_launch()
    per_pass = info["block_threads"] // lanes
    assert info["grid_x"] * per_pass < copies * len(rays), info
    want = paths.radiance(1)
    got = got.reshape(copies, len(rays), 4)
    bad = [c for c in range(copies) if not pr.same_words(got[c], want)]
    assert not bad, f"copies {bad[:5]}: {pr.first_difference(got[bad[0]], want)}"


def test_device_pointers_and_a_stream_equal_the_host_form():
    import torch
    rays, _, seeds, paths = set_of("cornell")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with renderer("cornell") as r:
        d_rays = torch.from_numpy(rays).to(dev)
        d_seeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        rad = torch.empty((len(rays), 4), dtype=torch.float32, device=dev)
        hits = torch.empty((len(rays), 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        r.trace_paths(d_rays, spp=33, seeds=d_seeds, first_hits=True, out=(rad, hits), stream=stream)
        info = r.last_launch()
        stream.synchronize()
        now = r.trace_paths(d_rays, spp=16, seeds=d_seeds)  # torch's current stream, waited for
        assert r.last_kernel_ms() > 0
    assert info["kernel"] == "rt::path_query_kernel<3, 6, false, true, 16>", info  # the automatic choice at 33 spp
    check(rad.cpu().numpy(), paths.radiance(33), "radiance on a stream")
    wt, wi = paths.hits()
    check(hits[:, 0].cpu().numpy().view(np.float32), wt, "first-hit t on a stream")
    assert np.array_equal(hits[:, 1].cpu().numpy(), wi)
    check(now.cpu().numpy(), paths.radiance(16), "radiance on the current stream")


def test_automatic_lanes_and_the_general_halton_form():
    rays, _, seeds, paths = set_of("cornell")
    with renderer("cornell") as r:
        # the automatic rule: 16 lanes from 4 spp on up to 4096 rays, from 8 on up to 65536, from 16 on
        # beyond.  The repeated rays are copies: only the launch is looked at
        for n, spp, lanes in [(len(rays), 3, 1), (len(rays), 4, 16), (4096, 4, 16), (4097, 4, 1), (4097, 7, 1),
                              (4097, 8, 16), (65536, 8, 16), (65537, 8, 1), (65537, 15, 1), (65537, 16, 16)]:
            k = np.arange(n) % len(rays)
            r.trace_paths(rays[k], spp=spp, seeds=seeds[k])
            info = r.last_launch()
            assert info["kernel"] == f"rt::path_query_kernel<3, 6, false, true, {lanes}>", (n, spp, info)
            tables = int((spp + lanes - 1) // lanes >= 8)  # halton_tables_on: 8 rounds per lane
            assert info["halton_tables"] == tables and info["lds_bytes"] == (18 + 4) * 112 + tables * 4 * 4679, info
        # the Halton tables from 8 rounds per lane on, and their LDS only then
        r.trace_paths(rays, spp=128, seeds=seeds)
        info = r.last_launch()
        assert info["halton_tables"] == 1 and info["lds_bytes"] == (18 + 4) * 112 + 4 * 4679, info
        r.trace_paths(rays, spp=8, seeds=seeds, lanes=1)
        assert r.last_launch()["halton_tables"] == 1
        # 0xFFFFF + sample_base + spp - 1 reaches 3^13: the general digit loop, one lane per ray
        base = 3 ** 13 - 0xFFFFF
        lo = r.trace_paths(rays, spp=1, sample_base=base - 1, seeds=seeds, lanes=16)
        assert r.last_launch()["kernel"] == "rt::path_query_kernel<3, 6, false, true, 16>"
        hi = r.trace_paths(rays, spp=2, sample_base=base - 1, seeds=seeds, lanes=16)
        info = r.last_launch()
        assert info["kernel"] == "rt::path_query_kernel<3, 6, false, false, 1>" and info["small_index"] == 0, info
        far = r.trace_paths(rays[:64], spp=1, sample_base=2 ** 32 - 2 ** 20 - 1, seeds=seeds[:64])
    _, sc, dom = np_scene("cornell")
    check(lo, pr.Paths(sc, rays, seeds, 1, 3, dom, sample_base=base - 1).radiance(1), "the last fixed-digit index")
    check(hi, pr.Paths(sc, rays, seeds, 2, 3, dom, sample_base=base - 1).radiance(2), "the first general index")
    check(far, pr.Paths(sc, rays[:64], seeds[:64], 1, 3, dom, sample_base=2 ** 32 - 2 ** 20 - 1).radiance(1),
          "the largest sample_base")


@pytest.mark.parametrize("ctx", ["cornell", "spheres", "triangles"])
def test_after_update_scene_the_result_is_a_new_contexts(ctx):
    import update_scenes
    from gpuraytracer_amd import SphereGPU
    name, opt, _, _ = CONTEXTS[ctx]
    s = scene_of(name)
    if s.n_spheres:  # the spheres move
        sph = (SphereGPU * s.n_spheres)()
        ctypes.memmove(ctypes.addressof(sph), ctypes.addressof(s.spheres), ctypes.sizeof(sph))
        np.frombuffer(sph, np.float32).reshape(-1, 20)[:, 0:3] += np.array([0.1, 0.05, -0.1], np.float32)
        moved = Scene(s.camera, s.materials, s.vertices, s.light, sph)
    else:  # everything but the room's walls and the light moves
        tri = ray_sets._tri_vertices(s)
        keep = np.zeros(len(tri), bool)
        keep[:12] = keep[34:36] = True
        tri[~keep] += np.array([0.15, 0.0, -0.1], np.float32)
        moved = update_scenes.with_vertices(s, tri)
    rays, _, seeds, _ = set_of(name)
    with Renderer(s, options=Options(**opt)) as r:
        before = r.trace_paths(rays, spp=5, seeds=seeds)
        r.update_scene(moved)
        got, (t, ids) = r.trace_paths(rays, spp=5, seeds=seeds, first_hits=True)
        assert not pr.same_words(before, got)
    with Renderer(moved, options=Options(**opt)) as r2:
        want, (wt, wi) = r2.trace_paths(rays, spp=5, seeds=seeds, first_hits=True)
    check(got, want, "radiance after the update")
    check(t, wt, "first-hit t after the update")
    assert np.array_equal(ids, wi)


def test_argument_checks():
    rays, _, seeds, _ = set_of("cornell")
    n = 8
    r8 = np.ascontiguousarray(rays[:n])
    s8 = np.ascontiguousarray(seeds[:n])
    rad = np.zeros((n, 4), np.float32)
    hits = np.zeros((n, 2), np.int32)
    P = ctypes.c_void_p

    def ptr(a):
        return None if a is None else a.ctypes.data_as(P)

    with renderer("cornell") as r:
        r.trace_rays(r8)
        before = r.last_launch()

        def call(n_rays=n, rays_=r8, rad_=rad, params=True, **fields):
            p = PathParamsC()
            lib.rt_path_params_default(ctypes.byref(p))
            for k, v in fields.items():
                setattr(p, k, v)
            st = lib.rt_trace_paths(r._ctx, ctypes.byref(p) if params else None, ptr(rays_), ptr(s8), n_rays,
                                    ptr(rad_), ptr(hits))
            return st, lib.rt_last_error(r._ctx).decode()

        assert call()[0] == 0
        assert "path_query_kernel" in r.last_launch()["kernel"]
        r.trace_rays(r8)
        # n == 0: RT_OK without a launch, whatever the pointers
        assert call(n_rays=0, rays_=None, rad_=None, params=False)[0] == 0
        assert r.last_launch() == before
        for kw, word in [(dict(n_rays=2 ** 31 + 1), "n > 2^31"),
                         (dict(params=False), "params"),
                         (dict(rays_=None), "rays"),
                         (dict(rad_=None), "radiance"),
                         (dict(spp=0), "spp"),
                         (dict(spp=2 ** 24 + 1), "spp"),
                         (dict(bounces=5), "bounces"),
                         (dict(lanes_per_ray=4), "lanes_per_ray"),
                         (dict(lanes_per_ray=2), "lanes_per_ray"),
                         (dict(sample_base=2 ** 32 - 2 ** 20, spp=1), "sample_base"),
                         (dict(sample_base=2 ** 32 - 2 ** 20 - 2 ** 24 + 1, spp=2 ** 24), "sample_base"),
                         (dict(flags=0x2), "flags"),
                         (dict(flags=0x100), "flags"),
                         (dict(reserved=1), "reserved")]:
            st, msg = call(**kw)
            assert st == RT_ERR_INVALID_ARG and "rt_trace_paths" in msg and word in msg, (kw, st, msg)
            assert r.last_launch() == before, kw
        assert call(spp=2 ** 24, bounces=0)[0] == 0  # the largest spp: no sample loop without bounces
        with pytest.raises(RtError) as e:
            r.trace_paths(r8, spp=0)
        assert e.value.status == RT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            r.trace_paths(r8[:, :7])
        with pytest.raises(ValueError):
            r.trace_paths(r8, seeds=s8[:3])
