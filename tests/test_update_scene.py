"""CPU: the entry points of rt_update_scene exist with the layout the header
states, argument errors come back as a status without a device, and the host
restatement of the refit (``Scene.tri_bvh_refit_host``, rt_scene.cpp
refit_tri_bvh_host) is right:

  * a refit onto unchanged triangles gives the build's dump byte for byte --
    the builders pad and round the fp32 min of a subtree, the refit takes the
    min of padded and rounded leaf planes, and both are the same halves because
    padding and rounding are monotone;
  * a refit onto the scenes of tests/update_scenes.py passes the node-by-node
    checker (tests/tri_bvh_tree.py), keeps ``perm`` and every escape / leaf
    word of the build, carries the updated scene's records and margin, and the
    float64 walk of the refitted tree equals brute force.

tests/test_gpu_update_scene.py holds the device refit (rt_refit.hip) to the
same results."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tri_bvh_scenes as ts
import tri_bvh_tree as tt
import update_scenes as us
from gpuraytracer_amd import Options, Scene, _native, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = {"host": Options(tri_build="host"), "host_leaf4": Options(tri_build="host", tri_leaf_max=4, tri_leaf_cost=2.0)}
IDENTITY = ["tiny1", "tiny2", "tiny3", "soup385", "soup1025", "grid", "same600", "far", "past_half"]
WALKED = ["tiny3", "soup385", "grid", "same600", "far"]
ARRAYS = ("nodes", "sorted", "perm", "isect")


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def built(name, builder):
    return ts.build(name).tri_bvh_host(HOST[builder])


@functools.lru_cache(maxsize=None)
def refitted(name, kind, builder):
    return ts.build(name).tri_bvh_refit_host(us.build(name, kind), HOST[builder])


def test_symbols_and_layout():
    for name in ("rt_update_scene", "rt_update_info", "rt_debug_tri_bvh_refit_host"):
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    assert ctypes.sizeof(_native.UpdateStats) == 32
    assert lib.rt_abi_version() == 11 and _native.ABI_VERSION == 11


def test_header_compiles_as_c99_with_the_stated_sizes():
    src = ('#include "rtpt.h"\n'
           "_Static_assert(sizeof(rt_update_stats) == 32, \"rt_update_stats\");\n"
           "_Static_assert(RTPT_ABI_VERSION == 11, \"abi\");\n"
           "_Static_assert(RT_UPDATE_REBUILD == 0x1u, \"flag\");\n"
           "int (*p_update)(rt_ctx*, const rt_scene_desc*, uint32_t) = rt_update_scene;\n"
           "int (*p_info)(const rt_ctx*, rt_update_stats*) = rt_update_info;\n"
           "int (*p_refit)(const rt_scene_desc*, const rt_create_options*, const rt_scene_desc*, rt_tri_bvh_dump*) =\n"
           "    rt_debug_tri_bvh_refit_host;\n")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tu.c")
        with open(path, "w") as f:
            f.write(src)
        cc = os.environ.get("CC", "cc")
        # C11 only for _Static_assert in this file; the header itself is checked as C99 below
        subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", path,
                               "-o", os.path.join(tmp, "tu.o")])
        with open(path, "w") as f:
            f.write('#include "rtpt.h"\nint use(void) { rt_update_stats s; return (int)sizeof(s) + (int)RT_UPDATE_REBUILD; }\n')
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                               path])


def test_null_arguments_return_a_status_without_a_device():
    desc = ts.build("tiny1").desc()
    assert lib.rt_update_scene(None, ctypes.byref(desc), 0) == 1
    assert b"null" in lib.rt_last_error(None)
    assert lib.rt_update_scene(None, None, 0) == 1
    info = _native.UpdateStats()
    assert lib.rt_update_info(None, ctypes.byref(info)) == 1
    dump = _native.TriBvhDump()
    assert lib.rt_debug_tri_bvh_refit_host(None, None, ctypes.byref(desc), ctypes.byref(dump)) == 1
    assert lib.rt_debug_tri_bvh_refit_host(ctypes.byref(desc), None, None, ctypes.byref(dump)) == 1
    assert lib.rt_debug_tri_bvh_refit_host(ctypes.byref(desc), None, ctypes.byref(desc), None) == 1


def test_refit_host_refuses_another_triangle_count():
    a, b = ts.build("tiny3").desc(), ts.build("tiny2").desc()
    dump = _native.TriBvhDump()
    assert lib.rt_debug_tri_bvh_refit_host(ctypes.byref(a), None, ctypes.byref(b), ctypes.byref(dump)) == 1
    assert b"n_triangles" in lib.rt_last_error(None)
    bad = Options(tri_leaf_max=129).c()
    assert lib.rt_debug_tri_bvh_refit_host(ctypes.byref(a), ctypes.byref(bad), ctypes.byref(a), ctypes.byref(dump)) == 1


@pytest.mark.parametrize("builder", list(HOST))
@pytest.mark.parametrize("name", IDENTITY)
def test_refit_onto_the_same_triangles_is_the_build(name, builder):
    want, got = built(name, builder), refitted(name, "same", builder)
    assert got["nodes_per_layout"] == want["nodes_per_layout"] and got["leaf_max"] == want["leaf_max"]
    assert got["margin"].tobytes() == want["margin"].tobytes()
    for k in ARRAYS:
        if not same_bytes(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])[0]
            raise AssertionError(f"{name} {builder}: {k} differs first at {tuple(int(v) for v in bad)}: "
                                 f"{got[k][tuple(bad)]!r} for {want[k][tuple(bad)]!r}")


@pytest.mark.parametrize("builder", list(HOST))
@pytest.mark.parametrize("kind", us.MOVED)
@pytest.mark.parametrize("name", IDENTITY)
def test_refit_onto_moved_triangles(name, kind, builder):
    was, got = built(name, builder), refitted(name, kind, builder)
    tt.check(got)
    assert same_bytes(got["perm"], was["perm"])
    assert same_bytes(got["nodes"][..., 3], was["nodes"][..., 3]), "an escape or leaf word changed"
    fresh = us.build(name, kind).tri_bvh_host(HOST[builder])
    assert same_bytes(got["isect"], fresh["isect"])
    assert got["margin"].tobytes() == fresh["margin"].tobytes()
    assert got["leaf_max"] == was["leaf_max"] and got["nodes_per_layout"] == was["nodes_per_layout"]


def random_rays(tri, count=600, seed=5):
    """As tests/test_tri_bvh_tree.py random_rays, for the vertices ``tri``."""
    rng = np.random.default_rng(seed)
    v = tri.astype(np.float64)
    lo, hi = v.min((0, 1)), v.max((0, 1))
    size = np.maximum(hi - lo, 0.5)
    o = rng.uniform(lo - 0.1 * size, hi + 0.1 * size, (count, 3))
    k = rng.integers(0, len(v), count)
    b = rng.dirichlet((1, 1, 1), count)
    aim = np.einsum("rv,rva->ra", b, v[k]) - o
    d = np.where((np.arange(count) % 4 == 0)[:, None], aim, rng.uniform(-1, 1, (count, 3)))
    d[::7, 0] = 0.0
    d[3::14, 2] = -0.0
    rays = np.empty((count, 8))
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-3, d, 1e9
    return rays


@pytest.mark.parametrize("kind", us.MOVED)
@pytest.mark.parametrize("name", WALKED)
def test_walk_of_the_refitted_tree_equals_brute_force(name, kind):
    rays = random_rays(us.vertices(name, kind))
    for builder in HOST:
        d = refitted(name, kind, builder)
        hits = tt.hit_matrix(d["isect"], rays)
        bt, bi = tt.brute(d, rays, hits)
        wt, wi = tt.walk(d, rays, hits)
        bad = np.flatnonzero((wt != bt) | (wi != bi))
        assert len(bad) == 0, (name, kind, builder, len(bad), int(bad[0]), wt[bad[0]], wi[bad[0]], bt[bad[0]], bi[bad[0]])
        # the rays must mean something: a tenth of them hit (nothing hits the zero-area triangles of collapse)
        assert kind == "collapse" or (bi >= 0).sum() >= len(rays) // 10, (name, kind, int((bi >= 0).sum()))


def test_update_scenes_keep_counts_and_move_the_camera():
    for kind in us.KINDS:
        a, b = ts.build("soup385"), us.build("soup385", kind)
        assert (b.n_triangles, b.width, b.height) == (a.n_triangles, a.width, a.height)
        assert (kind == "same") == (tuple(b.camera.position) == tuple(a.camera.position))
    assert np.abs(us.vertices("far", "to_far")).max() > 65504
    assert isinstance(us.build("grid", "shift"), Scene)
