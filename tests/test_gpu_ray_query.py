"""GPU: the batched ray queries (Renderer.trace_rays / rt_trace_rays) against
the numpy restatement's id-ordered scan, bit for bit: ``t`` as uint32 views,
``id`` exactly.  Every record layout and acceleration structure gets the same
few thousand rays of tests/ray_sets.py -- incoherent rays and segments (B, C),
the chosen rays (D: tmax / tmin exactly at a hit, shared edges, rays in a
face's plane, origins on a face or inside a sphere, tangent rays, +0 / -0
directions) and rays outside the exactness domain mixed into the waves (E).

Each case states the kernel instantiation it checked (rt_last_launch) and
that the launcher requested exactly the layout's staging bytes.  The
reference of a scene is computed once and shared by the contexts of that
scene."""
import ctypes
import functools

import numpy as np
import pytest

import ray_sets as rs
import sphere_edge_scenes as ses
from gpuraytracer_amd import Options, Renderer, Scene, _native, lib

pytestmark = pytest.mark.gpu
W, H = 64, 48
CHUNK = _native.RT_RAYS_CHUNK
PAIR, TRI, CLU = 112, 48, 112  # bytes of a pair, triangle and box-cluster record

SCENES = {
    "cornell": lambda: Scene.cornell_box(W, H),
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
    return rs.np_scene(scene_of(name))


@functools.lru_cache(maxsize=None)
def rays_of(name, which):
    B, C = rs.sets_bc()
    if which == "B":
        return B
    if which == "C":
        return C
    if which == "D":
        return rs.set_d(scene_of(name), B, reference(name, "B", False), pairs=scene_of(name).describe()["n_triangle_pairs"] > 0)
    assert which == "E"
    return rs.set_e(B, scene_of(name).ray_domain())


@functools.lru_cache(maxsize=None)
def reference(name, which, any_hit):
    t, ids = rs.reference(np_scene(name), rays_of(name, which), any_hit)
    t.setflags(write=False)
    ids.setflags(write=False)
    return t, ids


def kernel_name(layout, sph, any_hit):
    return f"rt::ray_query_kernel<{layout}, {'true' if sph else 'false'}, {'true' if any_hit else 'false'}>"


def staged_bytes(layout, info):
    return {0: TRI * info["n_triangles"], 1: PAIR * info["n_triangle_pairs"], 7: PAIR * info["n_triangle_pairs"],
            6: PAIR * info["n_triangle_pairs"] + CLU * info["n_box_clusters"]}.get(layout, 0)


def check(r, name, layout, which, any_hit=False, exact=False):
    """One query of a ray set on the context ``r`` against the reference, and
    the launch it made."""
    rays = rays_of(name, which)
    got = r.trace_rays(rays, any_hit=any_hit, exact=exact)
    want = reference(name, which, any_hit)
    assert rs.same(got, want), f"{name} {which} any={any_hit} exact={exact}: " + rs.first_difference(got, want)
    L = r.last_launch()
    sph = scene_of(name).n_spheres > 0
    assert L["kernel"] == kernel_name(layout, sph, any_hit), L
    assert L["block_threads"] == 256 and L["grid_x"] == -(-len(rays) // CHUNK) and L["grid_y"] == 1, L
    assert L["lds_bytes"] == staged_bytes(layout, scene_of(name).describe()), L


def check_all(r, name, layout, sets=("B", "C", "D", "E")):
    for which in sets:
        check(r, name, layout, which)
        check(r, name, layout, which, any_hit=True)
    check(r, name, layout, "B", exact=True)
    check(r, name, layout, "B", any_hit=True, exact=True)


@pytest.mark.parametrize("layout_opt,layout", [("auto", 6), ("pairs", 1), ("single", 0), ("global", 2),
                                               ("pairsmem", 4), ("bvh", 5), ("sorted", 1)])
def test_cornell_every_layout(layout_opt, layout):
    """The 36 triangles through every record layout; the path-sorting pair
    layout is a render kernel, its context answers queries through layout 1."""
    with Renderer(scene_of("cornell"), options=Options(layout=layout_opt)) as r:
        check_all(r, "cornell", layout)


@pytest.mark.parametrize("name", ["boxes1", "boxes2"])
def test_random_boxes_clusters(name):
    """Turned boxes inside the room: oblique cluster axes, rays that start
    between boxes, inside none and on their faces."""
    assert scene_of(name).describe()["n_box_clusters"] == 6
    with Renderer(scene_of(name)) as r:
        check_all(r, name, 6)


def test_sphere_kernel_layout():
    with Renderer(scene_of("spheres")) as r:
        check_all(r, "spheres", 7)


def test_sphere_lattice_ties():
    with Renderer(scene_of("lattice")) as r:
        check_all(r, "lattice", 7)


def test_sphere_big_leaf_takes_the_pair_layout():
    """A leaf of 129 spheres has no leaf-box entry: layout 1 with the 32-B-node walk."""
    opt = Options(sphere_leaf_max=129)
    assert scene_of("spheres129").describe(opt)["kernel_layout"] == 1
    with Renderer(scene_of("spheres129"), options=opt) as r:
        check_all(r, "spheres129", 1)


@pytest.mark.parametrize("opt", [{"tri_build": "host"}, {"tri_build": "lbvh"}, {"tri_build": "gpusah"},
                                 {"tri_build": "host", "tri_leaf_max": 4}, {"tri_build": "gpusah", "tri_leaf_max": 4}],
                         ids=lambda o: "-".join(str(v) for v in o.values()))
def test_triangle_bvh_builders(opt):
    """400 random triangles, just above the 384-triangle threshold: the three
    builders, and leaves of up to 4 triangles."""
    with Renderer(scene_of("tri400"), options=Options(**opt)) as r:
        assert r.build_info()["tri_bvh_build"] == _native.TRI_BUILDS[opt["tri_build"]]
        check_all(r, "tri400", 5, sets=("B", "C", "E"))


@pytest.mark.parametrize("walk", ["free", "sorted"])
@pytest.mark.parametrize("name,layout", [("spheres", 7), ("tri400", 5)])
def test_render_schedulers_do_not_change_a_query(name, layout, walk):
    """walk_scheduler is a render choice: the query of a free or sorted context
    runs the lockstep layout's kernel and gives its bytes."""
    rays = rays_of(name, "B")
    with Renderer(scene_of(name)) as r:
        base = [r.trace_rays(rays, any_hit=a) for a in (False, True)]
        base_kernels = []
        for a in (False, True):
            r.trace_rays(rays[:64], any_hit=a)
            base_kernels.append(r.last_launch()["kernel"])
    with Renderer(scene_of(name), options=Options(walk=walk)) as r:
        for k, a in enumerate((False, True)):
            got = r.trace_rays(rays, any_hit=a)
            assert rs.same(got, base[k]) and rs.same(got, reference(name, "B", a))
            assert r.last_launch()["kernel"] == base_kernels[k] == kernel_name(layout, name == "spheres", a)
        check(r, name, layout, "E")


@pytest.mark.parametrize("name,layout", [("cornell", 6), ("spheres", 7), ("tri400", 5)])
def test_ray_counts_and_grid_shapes(name, layout):
    """n = 1, 63, 65, one past a workgroup's chunk, and 0 (no launch): a prefix
    of a ray set gives the prefix of its answers, whatever the grid."""
    B = rays_of(name, "B")
    E = rays_of(name, "E")
    with Renderer(scene_of(name)) as r:
        check(r, name, layout, "B")
        before = r.last_launch()
        t, ids = r.trace_rays(B[:0])
        assert len(t) == 0 and len(ids) == 0 and r.last_launch() == before  # n == 0: no launch
        assert lib.rt_trace_rays(r._ctx, None, 0, 0, None) == 0
        for any_hit in (False, True):
            for n in (1, 63, 65, CHUNK + 1):
                got = r.trace_rays(B[:n], any_hit=any_hit)
                want = tuple(a[:n] for a in reference(name, "B", any_hit))
                assert rs.same(got, want), (n, any_hit, rs.first_difference(got, want))
                assert r.last_launch()["grid_x"] == -(-n // CHUNK)
            # a tail wave of out-of-domain rays only, and one that mixes both kinds
            for lo, hi in ((512, 513), (512, 576), (500, 577)):
                got = r.trace_rays(E[lo:hi], any_hit=any_hit)
                want = tuple(a[lo:hi] for a in reference(name, "E", any_hit))
                assert rs.same(got, want), (lo, hi, any_hit, rs.first_difference(got, want))


def test_argument_errors():
    B = rays_of("cornell", "B")
    hits = np.empty((4, 2), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with Renderer(scene_of("cornell")) as r:
        for args, what in [((p(B), 4, 0x400, p(hits)), b"flag"), ((p(B), 4, 0x2, p(hits)), b"flag"),
                           ((None, 4, 0, p(hits)), b"null"), ((p(B), 4, 0, None), b"null"),
                           ((p(B), 2**31 + 1, 0, p(hits)), b"2^31")]:
            assert lib.rt_trace_rays(r._ctx, *args) == 1, args
            assert what in lib.rt_last_error(r._ctx), lib.rt_last_error(r._ctx)
        assert lib.rt_trace_rays_async(r._ctx, None, 4, 0, p(hits), None) == 1
        with pytest.raises(_native.RtError):
            r.last_launch()  # nothing was launched
        t, ids = r.trace_rays(B[:4])
        assert rs.same((t, ids), tuple(a[:4] for a in reference("cornell", "B", False)))
        assert r.last_kernel_ms() > 0.0


@pytest.mark.parametrize("name,layout", [("cornell", 6), ("spheres", 7)])
def test_device_pointers_and_streams(name, layout):
    """Torch tensors take the device path: the same bytes as host pointers,
    through the synchronous call, through rt_trace_rays with RT_OUT_DEVICE, and
    through the async call on a non-null stream."""
    import torch
    rays = np.concatenate([rays_of(name, "B")[:1500], rays_of(name, "E")])
    with Renderer(scene_of(name)) as r:
        for any_hit in (False, True):
            host = r.trace_rays(rays, any_hit=any_hit)
            want = tuple(np.concatenate([a[:1500], b]) for a, b in zip(reference(name, "B", any_hit),
                                                                       reference(name, "E", any_hit)))
            assert rs.same(host, want), rs.first_difference(host, want)
            d_rays = torch.from_numpy(rays).cuda()
            t, ids = r.trace_rays(d_rays, any_hit=any_hit)
            assert t.is_cuda and t.dtype == torch.float32 and ids.dtype == torch.int32
            assert rs.same((t.cpu().numpy(), ids.cpu().numpy()), host)
            assert r.last_launch()["kernel"] == kernel_name(layout, name == "spheres", any_hit)
            # the C entry point with RT_OUT_DEVICE (blocks on the context's own stream)
            out = torch.full((len(rays), 2), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            flags = _native.RT_OUT_DEVICE | (_native.RT_RAYS_ANY if any_hit else 0)
            assert lib.rt_trace_rays(r._ctx, ctypes.c_void_p(d_rays.data_ptr()), len(rays), flags,
                                     ctypes.c_void_p(out.data_ptr())) == 0
            o = out.cpu().numpy()
            assert rs.same((o[:, 0].view(np.float32), o[:, 1]), host)
            # asynchronously on a stream of the caller's
            s = torch.cuda.Stream()
            out2 = torch.full((len(rays), 2), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                t2, id2 = r.trace_rays(d_rays, any_hit=any_hit, out=out2, stream=s)
            s.synchronize()
            assert t2.data_ptr() == out2.data_ptr()
            assert rs.same((t2.cpu().numpy(), id2.cpu().numpy()), host)


@pytest.mark.parametrize("name,first,last", [("cornell", 10, 34), ("boxes1", 10, 58)])
@pytest.mark.parametrize("layout_opt,layout", [("auto", 6), ("bvh", 5), ("pairs", 1)])
def test_rays_in_the_plane_of_an_oblique_face(name, first, last, layout_opt, layout):
    """The stated limit of the accelerated layouts (the
    premise): a ray that lies in an oblique face's plane to rounding can be
    accepted by that face's triangles on rounding residues, anywhere along the
    ray -- no padded box bounds such a hit.  RT_RAYS_EXACT answers these rays
    like the scan; the accelerated layouts differ from it ONLY on rays where
    the scan's own answer rests on such a residue hit, and only by dropping it.
    Measured on an MI355X, closest / any: Cornell (1,453 rays, 16 of them with a
    residue hit) layouts 6 and 5: 5 / 1 rays differ; 4 boxes (7,077 rays, 150):
    layout 6 37 / 8, layout 5 34 / 6; layout 1 (no box decides a closest hit,
    and the segment boxes of its any-hit kept every residue hit): 0 / 0."""
    scene = scene_of(name)
    rays = rs.in_plane_random(scene, range(first, last))
    sc = np_scene(name)
    residue = rs.residue_hits(sc, rays)
    assert rs.in_domain(rays, scene.ray_domain()).all() and residue.any()
    with Renderer(scene, options=Options(layout=layout_opt)) as r:
        for any_hit in (False, True):
            want = rs.reference(sc, rays, any_hit)
            exact = r.trace_rays(rays, any_hit=any_hit, exact=True)
            assert rs.same(exact, want), rs.first_difference(exact, want)
            t, ids = r.trace_rays(rays, any_hit=any_hit)
            assert r.last_launch()["kernel"] == kernel_name(layout, False, any_hit)
            bad = (t.view(np.uint32) != want[0].view(np.uint32)) | (ids != want[1])
            print(f"{name} layout {layout} any={any_hit}: {int(bad.sum())} of {len(rays)} rays differ "
                  f"({int(residue.sum())} rays with a residue hit)")
            assert not (bad & ~residue).any(), rs.first_difference((t[~residue], ids[~residue]),
                                                                  (want[0][~residue], want[1][~residue]))
            if any_hit:
                assert np.all(ids[bad] == 0)      # a dropped residue hit, never an invented one
            else:
                assert np.all(t[bad] > want[0][bad])
