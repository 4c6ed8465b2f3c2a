"""GPU: the sphere BVH walks on the inputs where such walks go wrong, bit for
bit against the C oracle -- the hand-built scenes of
tests/sphere_edge_scenes.py (a ray origin inside a sphere, nested, tangent and
duplicate spheres, coincident centroids, a one-node tree, negative, zero, tiny,
huge and non-finite radii, an emissive sphere), leaves around the 128-sphere
limit of the leaf-box entry, median splits, and the 0x7FFF-entry limit of the
compact table.

Every case first asks ``describe()`` for the kernel layout of its options,
checks it is the one the case is meant to exercise (BEFORE anything is
launched: a scene without a leaf-box table must not reach the sphere kernel),
renders, and then checks ``last_launch()`` ran exactly that kernel: the
lockstep sphere kernel (layout 7), its free (8) and sorted (10) forms, or the
pair kernel with the 32-B-node walk (1).
"""
import pytest

import oracle_lib
import sphere_edge_scenes as ses
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, KEY = 32, 20, 4, 3, 3
WALKS = ["auto", "free", "sorted"]
SPHERE_LAYOUT = {"auto": 7, "free": 8, "sorted": 10}
# describe()'s kernel_layout -> (kernel function, its GEO template argument)
KERNEL = {1: ("path_trace_kernel", 1), 7: ("path_trace_kernel", 7), 8: ("path_free_kernel", 7),
          10: ("path_trace_sorted_kernel", 7)}
NO_LEAF_BOX = ("nan_single", "nonfinite")  # scenes whose tree has a non-finite box

_scenes, _refs = {}, {}


def scene_of(key, width=W, height=H):
    """``key``: a name of the edge-scene table, or a sphere count n for
    random_spheres(width, height, n, seed=5 at 32 x 20, seed=9 at 16 x 8)."""
    k = (key, width, height)
    if k not in _scenes:
        if isinstance(key, str):
            _scenes[k] = ses.build(key, width, height)
        else:
            _scenes[k] = Scene.random_spheres(width, height, key, seed=5 if width == W else 9)
    return _scenes[k]


def reference(key, spp, bounces, width=W, height=H):
    """The oracle's image, computed once per (scene, spp, bounces)."""
    k = (key, spp, bounces, width, height)
    if k not in _refs:
        ref = oracle_lib.render(scene_of(key, width, height), seed_splitmix(width, height, key=KEY), spp, bounces)
        ref.setflags(write=False)
        _refs[k] = ref
    return _refs[k]


def run_case(key, expect, spp=SPP, bounces=BOUNCES, width=W, height=H, **opt):
    """Render scene ``key`` with the options ``opt``; ``expect`` is the kernel
    layout the case must exercise.  Returns last_launch()."""
    s = scene_of(key, width, height)
    options = Options(**opt)
    predicted = s.describe(options)["kernel_layout"]
    assert predicted == expect, (key, opt, predicted)   # before any launch
    with Renderer(s, seeds=seed_splitmix(width, height, key=KEY), options=options) as r:
        out = r.render(RenderParams(spp=spp, bounces=bounces))
        info = r.last_launch()
    fn, geo = KERNEL[expect]
    assert info["kernel"].startswith(f"rt::{fn}<{bounces}, {geo}, true, "), (key, opt, info)
    print(f"KERNEL {key} spp={spp} bounces={bounces} {opt}: {info['kernel']}")
    assert_parity(out, reference(key, spp, bounces, width, height), f"{key} {opt} spp {spp} bounces {bounces}")
    return info


def sphere_or_pair(key, walk):
    return 1 if key in NO_LEAF_BOX else SPHERE_LAYOUT[walk]


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ses.NAMES)
def test_edge_scene_every_walk(name, walk):
    run_case(name, sphere_or_pair(name, walk), walk=walk)


@pytest.mark.parametrize("name", ses.NAMES)
def test_edge_scene_32_byte_node_walk(name):
    run_case(name, 1, layout="pairs")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", ["camera_inside", "lattice", "concentric"])
def test_edge_scene_16_lanes_per_pixel(name, walk):
    """spp 16: the lockstep sphere kernel splits a pixel's samples over 16
    lanes (the free and sorted kernels keep one lane per pixel)."""
    info = run_case(name, SPHERE_LAYOUT[walk], spp=16, walk=walk)
    assert info["lanes_per_pixel"] == (16 if walk == "auto" else 1), info


# the free-running kernel needs bounces >= 1: bounce 0 with auto and sorted only
BOUNCE_CASES = [(b, w) for b in (0, 1, 4) for w in WALKS if not (b == 0 and w == "free")]


@pytest.mark.parametrize("bounces,walk", BOUNCE_CASES)
@pytest.mark.parametrize("name", ["camera_inside", "emissive"])
def test_edge_scene_bounce_counts(name, bounces, walk):
    run_case(name, SPHERE_LAYOUT[walk], bounces=bounces, walk=walk)


# (spheres, sphere_leaf_max, sphere kernel?): the leaf-box entry holds count - 1 in 7 bits
LEAF_CASES = [(127, 128, True), (128, 128, True), (129, 128, True), (300, 64, True),
              (129, 129, False), (150, 200, False), (300, 200, False), (255, 255, False)]


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("n,leaf,sphere_kernel", LEAF_CASES)
def test_leaf_sizes_around_the_entry_limit(n, leaf, sphere_kernel, walk):
    """Leaves of up to 128 spheres run the sphere kernels; a tree with a
    larger leaf has no leaf-box table and runs the pair kernel, whose 32-B
    node holds up to 255 spheres."""
    info = run_case(n, SPHERE_LAYOUT[walk] if sphere_kernel else 1, sphere_leaf_max=leaf, walk=walk)
    assert (", 7, " in info["kernel"]) == sphere_kernel, info
    assert info["kernel"].startswith("rt::path_trace_kernel<3, 1, ") == (not sphere_kernel), info


@pytest.mark.parametrize("walk", WALKS)
def test_lattice_in_leaves_of_128(walk):
    """343 spheres with many equal coordinates in leaves of up to 128."""
    run_case("lattice", SPHERE_LAYOUT[walk], sphere_leaf_max=128, walk=walk)


@pytest.mark.parametrize("key", ["lattice", "concentric", 300])
def test_median_splits(key):
    run_case(key, 7, sphere_median=True)


@pytest.mark.parametrize("n,layout", [(16384, 7), (16385, 1)])
def test_compact_table_entry_limit(n, layout):
    """32767 entries per layout fit the compact table's escape field; 32769
    do not, and the scene runs the pair kernel."""
    run_case(n, layout, spp=1, bounces=2, width=16, height=8)
