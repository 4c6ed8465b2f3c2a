"""CPU: the node-by-node checker of the triangle BVH (tests/tri_bvh_tree.py) on
the host binned-SAH build (``Scene.tri_bvh_host``, rt_scene.cpp build_tri_sah)
for the scenes of tests/tri_bvh_scenes.py -- the smallest trees, counts round a
block edge, a flat grid, 600 triangles in one Morton cell, 600 copies of one
triangle, coordinates where an fp16 step is units wide or past the largest
finite fp16.  The scene compiler accepts every count from 1 up, so the tiny
scenes start at one triangle.

The checker is itself checked: eight mutations of a valid dump, each of which
a wrong builder could produce without a render noticing, must be named by the
right invariant.  tests/test_gpu_tri_bvh_tree.py runs the same checker on the
trees the two GPU builders make.

``past_half`` (vertices out to 7e4): the scene compiles, planes past 65504
round outward to +-inf, which is conservative; the tree passes the checker and
the walk equals brute force (outcome B of the feature's issue)."""
import functools

import numpy as np
import pytest

import ray_sets as rs
import tri_bvh_scenes as ts
import tri_bvh_tree as tt
from gpuraytracer_amd import Options

LEAF = {1: Options(tri_build="host"), 4: Options(tri_build="host", tri_leaf_max=4, tri_leaf_cost=2.0)}
WALKED = [n for n in ts.NAMES if n != "soup20k"]  # soup20k: structure only


@functools.lru_cache(maxsize=None)
def host_dump(name, leaf):
    d = ts.build(name).tri_bvh_host(LEAF[leaf])
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def mutable(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", ts.NAMES)
def test_host_build_passes_the_checker(name, leaf):
    d = host_dump(name, leaf)
    n = len(ts.triangles(name))
    assert d["n_triangles"] == n and d["leaf_max"] == leaf
    assert d["nodes_per_layout"] == 2 * n - 1 if leaf == 1 else d["nodes_per_layout"] <= 2 * n - 1
    tt.check(d)


def test_dump_entry_point_sizes_and_errors():
    """rt_debug_tri_bvh_host: NULL buffers give the counts without a build,
    NULL arguments and a scene without triangles come back as a status."""
    import ctypes

    from gpuraytracer_amd import Scene, _native, lib
    scene = ts.build("soup385")
    desc = scene.desc()
    d = _native.TriBvhDump()
    assert lib.rt_debug_tri_bvh_host(ctypes.byref(desc), None, ctypes.byref(d)) == 0
    assert (d.n_triangles, d.nodes_per_layout, d.leaf_max) == (385, 0, 1)
    assert np.float32(d.margin) == host_dump("soup385", 1)["margin"]
    assert lib.rt_debug_tri_bvh_host(None, None, ctypes.byref(d)) == 1
    assert lib.rt_debug_tri_bvh_host(ctypes.byref(desc), None, None) == 1
    assert lib.rt_debug_tri_bvh(None, ctypes.byref(d)) == 1
    bad = Options(tri_leaf_max=129).c()
    assert lib.rt_debug_tri_bvh_host(ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(d)) == 1
    empty = Scene.random_spheres(ts.W, ts.H, 4).desc()
    empty.n_triangles = 0
    assert lib.rt_debug_tri_bvh_host(ctypes.byref(empty), None, ctypes.byref(d)) == 1
    assert b"no triangles" in lib.rt_last_error(None)


def random_rays(name, count=2000, seed=3):
    """A quarter aimed at a point of a random triangle, the rest in random directions,
    from origins in the scene's bounds grown by a tenth; every seventh ray has
    a zero direction component."""
    rng = np.random.default_rng(seed)
    v = ts.triangles(name).astype(np.float64)
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


@pytest.mark.parametrize("name", WALKED)
def test_walk_equals_brute_force(name):
    rays = random_rays(name)
    for leaf in (1, 4):
        d = host_dump(name, leaf)
        hits = tt.hit_matrix(d["isect"], rays)
        bt, bi = tt.brute(d, rays, hits)
        wt, wi = tt.walk(d, rays, hits)
        bad = np.flatnonzero((wt != bt) | (wi != bi))
        assert len(bad) == 0, (name, leaf, len(bad), int(bad[0]), wt[bad[0]], wi[bad[0]], bt[bad[0]], bi[bad[0]])
        assert (bi >= 0).sum() >= len(rays) // 10, (name, int((bi >= 0).sum()))


# ---- negative controls -------------------------------------------------------------

def half_step(bits, up):
    """The fp16 next to ``bits`` (uint16) in value: one step up or down."""
    bits = int(bits)
    if bits & 0x7FFF == 0:
        return 0x0001 if up else 0x8001
    neg = bool(bits & 0x8000)
    return bits + 1 if up != neg else bits - 1


def set_half(nodes, o, i, slot, bits):
    w, sh = slot // 2, 16 * (slot % 2)
    nodes[o, i, w] = (int(nodes[o, i, w]) & ~(0xFFFF << sh)) | (int(bits) << sh)


def get_half(nodes, o, i, slot):
    return (int(nodes[o, i, slot // 2]) >> (16 * (slot % 2))) & 0xFFFF


def a_leaf(d, o):
    """A leaf entry of layout o, past the first few."""
    leaves = np.flatnonzero((d["nodes"][o, :, 3] & tt.INNER) == 0)
    return int(leaves[len(leaves) // 3])


def expect(d, invariant, **where):
    with pytest.raises(tt.TreeError) as e:
        tt.check(d)
    assert e.value.invariant == invariant, str(e.value)
    for k, v in where.items():
        assert getattr(e.value, k) == v, (k, v, str(e.value))


def test_control_hi_plane_one_step_down():
    """What round-to-nearest in place of round-up does to half the planes."""
    d = mutable(host_dump("soup1024", 1))
    o, a = 0, 1
    i = a_leaf(d, o)
    set_half(d["nodes"], o, i, 3 + a, half_step(get_half(d["nodes"], o, i, 3 + a), up=False))
    expect(d, 5, layout=o, entry=i)


def test_control_lo_plane_one_step_up():
    d = mutable(host_dump("soup1024", 1))
    o, a = 0, 2
    i = a_leaf(d, o)
    set_half(d["nodes"], o, i, a, half_step(get_half(d["nodes"], o, i, a), up=True))
    expect(d, 5, layout=o, entry=i)


def test_control_near_far_swapped_in_layout_5():
    d = mutable(host_dump("soup1024", 1))
    i = a_leaf(d, 5)
    near, far = get_half(d["nodes"], 5, i, 0), get_half(d["nodes"], 5, i, 3)
    set_half(d["nodes"], 5, i, 0, far)
    set_half(d["nodes"], 5, i, 3, near)
    expect(d, 4, layout=5, entry=i)


@pytest.mark.parametrize("delta", [1, -1])
def test_control_escape_off_by_one(delta):
    d = mutable(host_dump("soup1024", 1))
    inner = np.flatnonzero((d["nodes"][3, :, 3] & tt.INNER) != 0)
    i = int(inner[len(inner) // 2])
    d["nodes"][3, i, 3] = int(d["nodes"][3, i, 3]) + delta
    expect(d, 2, layout=3)


def test_control_leaf_word_duplicated():
    """A leaf missing from one layout (another is there twice)."""
    d = mutable(host_dump("soup1024", 1))
    leaves = np.flatnonzero((d["nodes"][6, :, 3] & tt.INNER) == 0)
    d["nodes"][6, leaves[10], 3] = d["nodes"][6, leaves[20], 3]
    expect(d, 3, layout=6)


def test_control_perm_entries_swapped():
    d = mutable(host_dump("soup1024", 1))
    d["perm"][[5, 9]] = d["perm"][[9, 5]]
    expect(d, 1, triangle=5)


def test_control_inner_box_is_its_first_childs():
    """A refit that missed the second child."""
    d = mutable(host_dump("soup1024", 1))
    for o in range(8):
        d["nodes"][o, 0, :3] = d["nodes"][o, 1, :3]
    expect(d, 6, layout=0, entry=0)


def test_control_children_not_reversed():
    """Layout 2 written in the child order of layout 5 (its own planes and
    escapes): a valid tree, the same tree, in the wrong order for its octant."""
    d = mutable(host_dump("soup1024", 1))
    total = d["nodes_per_layout"]
    src = d["nodes"][5].copy()
    h = tt.halves(src[None])[0]
    for a in range(3):  # octant 5 -> octant 2: every axis flips its near and far slots
        h[:, [a, 3 + a]] = h[:, [3 + a, a]]
    h = h.astype(np.uint32)
    src[:, 0], src[:, 1], src[:, 2] = h[:, 0] | h[:, 1] << 16, h[:, 2] | h[:, 3] << 16, h[:, 4] | h[:, 5] << 16
    inner = (src[:, 3] & tt.INNER) != 0
    src[inner, 3] -= np.uint32(3 * total)
    d["nodes"][2] = src
    expect(d, 7)


def test_controls_start_from_a_valid_tree():
    tt.check(mutable(host_dump("soup1024", 1)))


# ---- the grazing rays --------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup385", "grid", "far"])
def test_grazing_rays_hit_what_they_aim_at(name):
    """Set G means something only if its rays hit: at least half of them must
    reach their own triangle in the numpy scan."""
    scene = ts.build(name)
    rays, target = rs.set_g(scene)
    assert len(rays) == 6 * scene.n_triangles
    _, ids = rs.reference(rs.np_scene(scene), rays)
    share = float(np.mean(ids == target))
    print(f"{name}: {share:.3f} of {len(rays)} grazing rays hit their triangle")
    assert share >= 0.5, (name, share)
