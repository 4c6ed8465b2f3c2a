"""GPU: the first-hit feature buffers (Renderer.render_aov / rt_render_aov)
against tests/aov_ref.py, bit for bit: floats as uint32 views, ids exactly.

Every record layout and acceleration structure renders the same frames; each
case asserts all three buffers, the kernel instantiation (rt_last_launch), one
lane per pixel and that the launcher requested exactly the layout's staged
bytes (plus the Halton table where the launch fills it).  The per-sample
reference of a frame is computed once and shared by the cases of that frame
(spp 1 is its first sample)."""
import ctypes
import functools

import numpy as np
import pytest

import aov_ref as ar
import oracle_lib
import sphere_edge_scenes as ses
from gpuraytracer_amd import Options, Renderer, Scene, _native, lib, seed_splitmix

pytestmark = pytest.mark.gpu
W, H = 64, 48
PAIR, TRI, CLU, TAB = 112, 48, 112, 4 * 729  # bytes: pair, triangle, box-cluster record; Halton table of dimension 1
KEYS = ("albedo", "normal_depth", "first_hit")

SCENES = {
    "cornell": lambda: Scene.cornell_box(W, H),
    "cornell70": lambda: Scene.cornell_box(70, 45),                  # partial tiles on both axes
    "cornell40": lambda: Scene.cornell_box(40, 24),
    "boxes1": lambda: Scene.random_boxes(W, H, 4, seed=1),
    "boxes2": lambda: Scene.random_boxes(W, H, 4, seed=2),
    "spheres": lambda: Scene.random_spheres(W, H, 200, seed=42),
    "spheres129": lambda: Scene.random_spheres(W, H, 129, seed=5),   # one leaf of 129 with sphere_leaf_max 129
    "lattice": lambda: ses.build("lattice", W, H),                   # tangent neighbours, ties in t
    "tri400": lambda: Scene.random_triangles(W, H, 400),
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def np_scene(name):
    return ar.np_scene(scene_of(name))


@functools.lru_cache(maxsize=None)
def seeds_of(name, kind="splitmix"):
    s = scene_of(name)
    if kind == "splitmix":
        sd = seed_splitmix(s.width, s.height)
    elif kind == "u32":  # full range: seed + n wraps
        sd = np.random.default_rng(77).integers(0, 2 ** 32, (s.height, s.width), dtype=np.uint64).astype(np.uint32)
        sd[0, 0], sd[1, 5], sd[7, 3] = 0xFFFFFFFF, 0xFFFFFFFE, 0
    else:  # ("top", top, spp): largest Halton index = top, spread over the top digits
        _, top, spp = kind
        sd = np.random.default_rng(top).integers(top - spp + 1 - 400000, top - spp + 2, (s.height, s.width),
                                                 dtype=np.int64)
        sd[5, 9] = top - spp + 1
        sd = sd.astype(np.uint32)
    sd.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def hits_of(name, seeds, spp, sample_base=0, row_start=0, row_step=1, center=False):
    h = ar.sample_hits(np_scene(name), None if center else seeds_of(name, seeds), spp, sample_base, row_start,
                       row_step, 0, center)
    for v in h.values():
        v.setflags(write=False)
    return h


def reference(name, seeds, spp, full_spp=None, **kw):
    """The buffers of ``spp`` samples; ``full_spp``: take them from the cached
    per-sample reference of that many samples."""
    h = hits_of(name, seeds, full_spp or spp, **kw)
    return ar.buffers(None, None, spp, hits={k: v[:spp] for k, v in h.items()})


def staged_bytes(layout, info):
    return {0: TRI * info["n_triangles"], 1: PAIR * info["n_triangle_pairs"], 7: PAIR * info["n_triangle_pairs"],
            6: PAIR * info["n_triangle_pairs"] + CLU * info["n_box_clusters"]}.get(layout, 0)


def check_launch(r, name, layout, spp, rows, small=True):
    s = scene_of(name)
    L = r.last_launch()
    sph = "true" if s.n_spheres > 0 else "false"
    tables = layout == 6 and small and spp >= 8  # halton_tables_on at one lane per pixel
    assert L["kernel"] == f"rt::aov_kernel<{layout}, {sph}, {'true' if small else 'false'}>", L
    assert L["lanes_per_pixel"] == 1 and L["block_threads"] == 256, L
    assert L["small_index"] == int(small) and L["halton_tables"] == int(tables), L
    assert L["grid_x"] == -(-s.width // 16) and L["grid_y"] == -(-rows // 16), L
    assert L["lds_bytes"] == staged_bytes(layout, s.describe()) + (TAB if tables else 0), L


def check_buffers(got, want, what, keys=KEYS):
    assert set(got) == set(keys), (what, sorted(got))
    for k in keys:
        assert ar.same(got[k], want[k]), f"{what} {k}: " + ar.first_difference(got[k], want[k])


def check(r, name, layout, spp, seeds="splitmix", full_spp=None, small=True, **kw):
    got = r.render_aov(spp=spp, **kw)
    want = reference(name, seeds, spp, full_spp, **{k: v for k, v in kw.items() if k != "row_count"})
    check_buffers(got, want, f"{name} spp={spp} {kw}")
    check_launch(r, name, layout, spp, want["albedo"].shape[0], small)


@pytest.mark.parametrize("spp", [1, 17])
@pytest.mark.parametrize("layout_opt,layout", [("auto", 6), ("pairs", 1), ("single", 0), ("global", 2),
                                               ("pairsmem", 4), ("bvh", 5), ("sorted", 1)])
def test_cornell_every_layout(layout_opt, layout, spp):
    """The 36 triangles through every record layout; the path-sorting pair
    layout is a render kernel, its context renders AOVs through layout 1.
    17 spp fills the Halton table in the box-cluster layout, 1 spp does not."""
    with Renderer(scene_of("cornell"), seeds=seeds_of("cornell"), options=Options(layout=layout_opt)) as r:
        check(r, "cornell", layout, spp, full_spp=17)


@pytest.mark.parametrize("name", ["boxes1", "boxes2"])
def test_random_boxes_clusters(name):
    """Turned boxes inside the room: oblique cluster axes in the camera mask."""
    assert scene_of(name).describe()["n_box_clusters"] == 6
    with Renderer(scene_of(name), seeds=seeds_of(name)) as r:
        check(r, name, 6, 9)


def test_sphere_kernel_layout():
    with Renderer(scene_of("spheres"), seeds=seeds_of("spheres")) as r:
        check(r, "spheres", 7, 17)
        check(r, "spheres", 7, 1, full_spp=17)


def test_sphere_big_leaf_takes_the_pair_layout():
    """A leaf of 129 spheres has no leaf-box entry: layout 1 with the 32-B-node walk."""
    opt = Options(sphere_leaf_max=129)
    assert scene_of("spheres129").describe(opt)["kernel_layout"] == 1
    with Renderer(scene_of("spheres129"), seeds=seeds_of("spheres129"), options=opt) as r:
        check(r, "spheres129", 1, 3)


def test_sphere_lattice_ties():
    with Renderer(scene_of("lattice"), seeds=seeds_of("lattice")) as r:
        check(r, "lattice", 7, 3)


def test_triangle_bvh_scene():
    with Renderer(scene_of("tri400"), seeds=seeds_of("tri400")) as r:
        check(r, "tri400", 5, 2)


@pytest.mark.parametrize("layout_opt,layout", [("auto", 6), ("pairs", 1), ("bvh", 5)])
def test_partial_tiles_rows_and_sample_base(layout_opt, layout):
    """70x45 (partial tiles on both axes; the camera mask is computed before
    lanes leave), spp 5; then rows 1, 4, 7, ... from sample 1000."""
    with Renderer(scene_of("cornell70"), seeds=seeds_of("cornell70"), options=Options(layout=layout_opt)) as r:
        check(r, "cornell70", layout, 5)
        check(r, "cornell70", layout, 5, sample_base=1000, row_start=1, row_step=3)
        # a row_count below the partition's rows: the first rows of the same partition
        got = r.render_aov(spp=5, sample_base=1000, row_start=1, row_step=3, row_count=4)
        want = reference("cornell70", "splitmix", 5, sample_base=1000, row_start=1, row_step=3)
        check_buffers(got, {k: v[:4] for k, v in want.items()}, "row_count=4")
        check_launch(r, "cornell70", layout, 5, 4)


@pytest.mark.parametrize("layout_opt,layout", [("auto", 6), ("pairs", 1)])
def test_full_range_seeds_wrap(layout_opt, layout):
    """uint32 seeds up to 2^32 - 1: seed + n wraps, the generic Halton loop."""
    with Renderer(scene_of("cornell40"), seeds=seeds_of("cornell40", "u32"), options=Options(layout=layout_opt)) as r:
        check(r, "cornell40", layout, 5, seeds="u32", small=False)


@pytest.mark.parametrize("top", [3 ** 13 - 1, 3 ** 13])
def test_halton_index_bound_edges(top):
    """Largest index 3^13 - 1: fixed digits, and at 32 samples per lane the
    LDS table of dimension 1; 3^13: the generic loop, no table."""
    kind = ("top", top, 32)
    with Renderer(scene_of("cornell40"), seeds=seeds_of("cornell40", kind)) as r:
        check(r, "cornell40", 6, 32, seeds=kind, small=top < 3 ** 13)


def test_center_form_is_the_id_buffer():
    s = scene_of("cornell")
    with Renderer(s) as r:
        got = r.render_aov(center=True)
        check_launch(r, "cornell", 6, 1, H)
    assert np.array_equal(got["first_hit"]["id"], oracle_lib.primary_ids(s))
    check_buffers(got, reference("cornell", None, 1, center=True), "center")
    with Renderer(s, options=Options(layout="bvh")) as r:
        got = r.render_aov(center=True, sample_base=12345)  # sample_base is ignored
    check_buffers(got, reference("cornell", None, 1, center=True), "center bvh")


def _raw_context(scene):
    ctx = ctypes.c_void_p()
    assert lib.rt_create(ctypes.byref(scene.desc()), ctypes.byref(ctx)) == 0
    return ctx


def _raw_call(ctx, hit, spp=1, flags=0, **kw):
    p, b = _native.AovParams(), _native.AovBuffers()
    p.spp, p.flags = spp, flags
    for k, v in kw.items():
        setattr(p, k, v)
    if hit is not None:
        b.first_hit = hit.ctypes.data
    return lib.rt_render_aov(ctx, ctypes.byref(p), ctypes.byref(b))


def test_center_form_needs_no_seeds():
    s = scene_of("cornell")
    ctx = _raw_context(s)  # no rt_set_seeds / rt_fill_seeds
    try:
        hit = np.empty((H, W), ar.HIT_DTYPE)
        assert _raw_call(ctx, hit, flags=_native.RT_AOV_CENTER) == 0
        assert np.array_equal(hit["id"], oracle_lib.primary_ids(s))
        assert _raw_call(ctx, hit) == 5  # RT_ERR_STATE: jittered, no seeds
        assert b"seeds" in lib.rt_last_error(ctx)
    finally:
        lib.rt_destroy(ctx)


def test_buffer_subsets():
    want = reference("cornell", "splitmix", 17)
    with Renderer(scene_of("cornell"), seeds=seeds_of("cornell")) as r:
        got = r.render_aov(spp=17, albedo=False, normal_depth=False)
        check_buffers(got, want, "first_hit only", ("first_hit",))
        got = r.render_aov(spp=17, normal_depth=False, first_hit=False)
        check_buffers(got, want, "albedo only", ("albedo",))
        got = r.render_aov(spp=17, albedo=False, first_hit=False)
        check_buffers(got, want, "normal_depth only", ("normal_depth",))


def test_device_tensors_on_a_stream():
    import torch
    want = reference("cornell", "splitmix", 17)
    with Renderer(scene_of("cornell"), seeds=seeds_of("cornell")) as r:
        dev = torch.device("cuda", r.device)
        out = {"albedo": torch.empty((H, W, 4), dtype=torch.float32, device=dev),
               "normal_depth": torch.empty((H, W, 4), dtype=torch.float32, device=dev),
               "first_hit": torch.empty((H, W, 2), dtype=torch.int32, device=dev)}
        stream = torch.cuda.Stream(dev)
        r.render_aov(spp=17, out=out, stream=stream)
        stream.synchronize()
        check_launch(r, "cornell", 6, 17, H)
        got = {"albedo": out["albedo"].cpu().numpy(), "normal_depth": out["normal_depth"].cpu().numpy(),
               "first_hit": np.ascontiguousarray(out["first_hit"].cpu().numpy()).view(ar.HIT_DTYPE)[..., 0]}
        check_buffers(got, want, "device")
        only = {"first_hit": torch.zeros((H, W, 2), dtype=torch.int32, device=dev)}
        r.render_aov(spp=17, out=only)  # torch's current stream, waited for
        assert torch.equal(only["first_hit"], out["first_hit"])


def test_error_statuses():
    s = scene_of("cornell")
    hit = np.empty((H, W), ar.HIT_DTYPE)
    with Renderer(s) as r:
        ctx = r._ctx
        p, b = _native.AovParams(), _native.AovBuffers()
        p.spp = 1
        b.first_hit = hit.ctypes.data
        assert lib.rt_render_aov(ctx, None, ctypes.byref(b)) == 1 and b"params" in lib.rt_last_error(ctx)
        assert lib.rt_render_aov(ctx, ctypes.byref(p), None) == 1 and b"buffers" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, None) == 1 and b"all three" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, spp=0) == 1 and b"spp" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, spp=2 ** 24 + 1) == 1 and b"spp" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, spp=2, flags=_native.RT_AOV_CENTER) == 1 and b"CENTER" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, flags=0x800) == 1 and b"flag" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, flags=_native.RT_RAYS_ANY) == 1
        assert _raw_call(ctx, hit, row_start=H) == 1 and b"row" in lib.rt_last_error(ctx)
        assert _raw_call(ctx, hit, row_start=1, row_step=3, row_count=17) == 1  # 16 rows in that partition
        assert _raw_call(ctx, hit) == 0
