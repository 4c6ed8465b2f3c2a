"""GPU: the trees the three triangle-BVH builders make -- the host binned SAH
(uploaded), the Morton LBVH (rt_lbvh.hip) and the batched binned SAH
(rt_gsah.hip), the SAH builds also with leaves of up to 4 triangles -- read
back with ``Renderer.tri_bvh()`` and checked node by node
(tests/tri_bvh_tree.py), on the scenes of tests/tri_bvh_scenes.py.  A render
or a ray query of random small triangles passes on any tree whose boxes are
conservative for the rays it happens to trace; the checker does not depend on
rays, and the grazing rays of set G run along the box faces themselves.

Per builder and scene: the checker, then sets B, C, E and G of
tests/ray_sets.py, closest and any-hit, bit-equal to the numpy scan through
the layout-5 query kernel (``soup20k``: the checker only, 79 workgroups of
256 threads).  The reference of a scene is computed once and shared by the
builders.

``past_half`` (vertices out to 7e4, past the largest finite fp16): every
builder accepts it, planes past 65504 become +-inf in the outward rounding,
the trees pass the checker and the queries equal the scan (outcome B of the
feature's issue)."""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_sets as rs
import tri_bvh_scenes as ts
import tri_bvh_tree as tt
from gpuraytracer_amd import RenderParams, Renderer, RtError, Scene, _native, seed_splitmix
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

BUILDERS = {
    "host": dict(tri_build="host"),
    "lbvh": dict(tri_build="lbvh"),
    "gpusah": dict(tri_build="gpusah"),
    "host_leaf4": dict(tri_build="host", tri_leaf_max=4, tri_leaf_cost=2.0),
    "gpusah_leaf4": dict(tri_build="gpusah", tri_leaf_max=4, tri_leaf_cost=2.0),
}
QUERIED = [n for n in ts.NAMES if n != "soup20k"]


def context(name, builder):
    return Renderer(ts.build(name), options=ts.options(name, **BUILDERS[builder]))


@functools.lru_cache(maxsize=None)
def rays_of(name, which):
    B, C = rs.sets_bc()
    if which == "G":
        return rs.set_g(ts.build(name))[0]
    return {"B": B, "C": C}[which] if which in "BC" else rs.set_e(B, ts.build(name).ray_domain())


@functools.lru_cache(maxsize=None)
def references(name):
    """{(set, any_hit): (t, id)}: one id-ordered scan per kind of query over the
    scene's four sets back to back (the scan treats every ray by itself)."""
    sets = [rays_of(name, which) for which in "BCEG"]
    cuts = np.cumsum([len(s) for s in sets])[:-1]
    sc, rays = rs.np_scene(ts.build(name)), np.concatenate(sets)
    out = {}
    for any_hit in (False, True):
        t, ids = rs.reference(sc, rays, any_hit)
        for which, tt_, ii in zip("BCEG", np.split(t, cuts), np.split(ids, cuts)):
            tt_.setflags(write=False)
            ii.setflags(write=False)
            out[which, any_hit] = (tt_, ii)
    return out


def reference(name, which, any_hit):
    return references(name)[which, any_hit]


def checked_dump(r, name, builder):
    info = r.build_info()
    assert info["tri_bvh_build"] == _native.TRI_BUILDS[BUILDERS[builder]["tri_build"]], info
    d = r.tri_bvh()
    n = len(ts.triangles(name))
    assert d["n_triangles"] == n
    assert d["leaf_max"] == (1 if builder == "lbvh" else BUILDERS[builder].get("tri_leaf_max", 1)), d["leaf_max"]
    if d["leaf_max"] == 1:
        assert d["nodes_per_layout"] == 2 * n - 1
    tt.check(d, expect_nodes=info["tri_bvh_nodes"])
    return d


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ts.NAMES)
def test_tree_and_queries(name, builder):
    with context(name, builder) as r:
        checked_dump(r, name, builder)
        if name not in QUERIED:
            return
        for which in "BCEG":
            for any_hit in (False, True):
                got = r.trace_rays(rays_of(name, which), any_hit=any_hit)
                want = reference(name, which, any_hit)
                assert rs.same(got, want), f"{name} {builder} {which} any={any_hit}: " + rs.first_difference(got, want)
                kernel = r.last_launch()["kernel"]
                assert kernel == f"rt::ray_query_kernel<5, false, {'true' if any_hit else 'false'}>", kernel


def test_a_context_without_a_tree_says_so():
    """The Cornell box takes an LDS layout and builds no triangle BVH: RT_ERR_STATE."""
    with Renderer(Scene.cornell_box(ts.W, ts.H)) as r:
        assert r.build_info()["tri_bvh_build"] == 0
        with pytest.raises(RtError) as e:
            r.tri_bvh()
    assert e.value.status == 5


@pytest.mark.parametrize("leaf4", [False, True])
@pytest.mark.parametrize("name", ["tiny1", "soup385", "soup1025", "grid", "far"])
def test_host_upload_is_the_host_build(name, leaf4):
    """What a host-build context holds on the device is Scene.tri_bvh_host(), byte for byte."""
    builder = "host_leaf4" if leaf4 else "host"
    opt = ts.options(name, **BUILDERS[builder])
    with Renderer(ts.build(name), options=opt) as r:
        dev = r.tri_bvh()
    host = ts.build(name).tri_bvh_host(opt)
    assert sorted(dev) == sorted(host)
    for k, v in host.items():
        assert np.array_equal(np.asarray(v).view(np.uint8) if isinstance(v, np.ndarray) else v,
                              np.asarray(dev[k]).view(np.uint8) if isinstance(v, np.ndarray) else dev[k]), k


@pytest.mark.parametrize("builder", ["lbvh", "gpusah"])
def test_gpu_builds_are_deterministic(builder):
    """Both GPU builders claim a deterministic build: two builds, the same bytes."""
    dumps = []
    for _ in range(2):
        with context("soup1024", builder) as r:
            dumps.append(r.tri_bvh())
    for k in ("nodes", "sorted", "perm", "isect"):
        assert dumps[0][k].tobytes() == dumps[1][k].tobytes(), k
    assert dumps[0]["nodes_per_layout"] == dumps[1]["nodes_per_layout"]


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    out = oracle_lib.render(ts.build(name), seed_splitmix(ts.W, ts.H), 2, 3)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("builder", ["host", "lbvh", "gpusah"])
@pytest.mark.parametrize("name", ["grid", "cell", "far", "same600"])
def test_render_against_the_oracle(name, builder):
    with Renderer(ts.build(name), seeds=seed_splitmix(ts.W, ts.H), options=ts.options(name, **BUILDERS[builder])) as r:
        out = r.render(RenderParams(spp=2, bounces=3))
    assert_parity(out, oracle_frame(name), f"{name} {builder}")
