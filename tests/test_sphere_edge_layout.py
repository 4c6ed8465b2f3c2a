"""CPU: the kernel choice for sphere scenes at the limits of the compact
tables, and the checker itself on the degenerate scenes of
tests/sphere_edge_scenes.py.

* ``describe()`` must name the sphere kernel (layout 7, free 8, sorted 10)
  only when every table its walks read exists: the leaf-box entry stores
  ``count - 1`` in 7 bits, so a tree with a leaf of more than 128 spheres, or
  with a non-finite node box, has no leaf-box table and takes the pair kernel
  (layout 1) with the 32-B-node walk.
* The compact table holds at most 0x7FFF entries per layout.
* The C oracle equals its numpy restatement on every scene, so the root rule,
  negative radii and non-finite radii of the checker are pinned before the GPU
  is compared with it (tests/test_gpu_sphere_edges.py).
"""
import numpy as np
import pytest

import oracle_lib
import sphere_edge_scenes as ses
from gpuraytracer_amd import Options, Scene, seed_splitmix

PAIR_BYTES = 6 * 112  # the room's 6 pair records, staged by the pair and the sphere kernels alike
# (spheres of random_spheres(32, 20, n, seed=5), sphere_leaf_max) -> lockstep layout
LEAF_CASES = [(127, 128, 7), (128, 128, 7), (129, 128, 7),
              (129, 129, 1), (150, 200, 1), (300, 200, 1), (255, 255, 1)]
SORT_BYTES = 16 * 1097  # the sorted kernel's path buffers (tests/test_abi.py)


def check_layouts(scene, lockstep, **opt):
    """describe() for the three walk schedulers: the sphere kernel in all of
    them or in none, with the LDS bytes of the kernel it names."""
    info = scene.describe(Options(**opt))
    assert info["kernel_layout"] == lockstep, info
    assert info["kernel_lds_bytes"] == PAIR_BYTES, info
    assert info["sphere_kernel_lds_bytes"] == (PAIR_BYTES if lockstep == 7 else 0), info
    assert scene.describe(Options(walk="lockstep", **opt))["kernel_layout"] == lockstep
    free = scene.describe(Options(walk="free", **opt))
    srt = scene.describe(Options(walk="sorted", **opt))
    if lockstep == 7:
        assert (free["kernel_layout"], free["kernel_lds_bytes"]) == (8, PAIR_BYTES), free
        assert (srt["kernel_layout"], srt["kernel_lds_bytes"]) == (10, SORT_BYTES + PAIR_BYTES), srt
    else:
        assert (free["kernel_layout"], free["kernel_lds_bytes"]) == (1, PAIR_BYTES), free
        assert (srt["kernel_layout"], srt["kernel_lds_bytes"]) == (1, PAIR_BYTES), srt
    for i in (free, srt):
        assert i["sphere_kernel_lds_bytes"] == info["sphere_kernel_lds_bytes"], i


@pytest.mark.parametrize("n,leaf,layout", LEAF_CASES)
def test_layout_at_the_leaf_count_limit(n, leaf, layout):
    """A leaf of up to 128 spheres fits the leaf-box entry; with
    sphere_leaf_max > 128 and enough spheres the builder makes a larger leaf
    and the scene takes the pair kernel."""
    check_layouts(Scene.random_spheres(32, 20, n, seed=5), layout, sphere_leaf_max=leaf)


@pytest.mark.parametrize("name", ["nan_single", "nonfinite"])
def test_layout_with_a_non_finite_box(name):
    """A NaN radius leaves its leaf box non-finite (nan_single: the root leaf,
    refused only by the leaf-box table; nonfinite: an inner box as well)."""
    check_layouts(ses.build(name, 32, 20), 1)


@pytest.mark.parametrize("name", [n for n in ses.NAMES if n not in ("nan_single", "nonfinite")])
def test_layout_of_the_finite_edge_scenes(name):
    s = ses.build(name, 32, 20)
    check_layouts(s, 7)
    nodes = s.describe()["n_sphere_nodes"]
    assert nodes == 2 * len(ses.ROWS[name]) - 1
    if name == "lattice":  # leaves of up to 128 of the 343: still the sphere kernel
        check_layouts(s, 7, sphere_leaf_max=128)
        check_layouts(s, 7, sphere_median=True)


def test_single_sphere_is_a_root_leaf():
    assert ses.build("single", 32, 20).describe()["n_sphere_nodes"] == 1
    assert ses.build("two", 32, 20).describe()["n_sphere_nodes"] == 3


@pytest.mark.parametrize("n,nodes,layout", [(16384, 32767, 7), (16385, 32769, 1)])
def test_layout_at_the_entry_count_limit(n, nodes, layout):
    """The compact table's escape field holds entry indices up to 0x7FFF per
    layout: 16384 one-sphere leaves make 32767 entries, one more sphere 32769."""
    s = Scene.random_spheres(16, 8, n, seed=9)
    assert s.describe()["n_sphere_nodes"] == nodes
    check_layouts(s, layout)


def test_the_room_is_the_documented_one():
    r = ses.room(32, 20)
    assert r.n_triangles == 12 and r.n_spheres == 0
    assert tuple(r.camera.position) == ses.CAMERA
    assert tuple(np.float32(v) for v in r.light.center) == tuple(np.float32(v) for v in ses.LIGHT)
    assert (r.camera.direction.x, r.camera.direction.y) == (0.0, 0.0) and r.camera.direction.z < 0.0


@pytest.mark.parametrize("name", ses.NAMES)
def test_oracle_equals_numpy_restatement(name):
    import pt_oracle_np as P
    rows = ses.ROWS[name][::7] if name == "lattice" else None
    s = ses.build(name, 16, 10, rows)
    sd = seed_splitmix(16, 10, key=3)
    out = oracle_lib.render(s, sd, 2, 3)
    sc = P.Scene(s.camera, s.materials, s.light, s.vertices, s.spheres)
    ref = P.render(sc, sd, 2, 3)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), name


# pixels (of 32 x 20) each scene changes against the empty room at 4 spp, 3
# bounces, seed_splitmix(32, 20, key=3): the C oracle's own count
CHANGED = {"single": 364, "two": 342, "camera_inside": 640, "room_inside": 281, "concentric": 244,
           "neg_zero_tiny": 236, "lattice": 559, "emissive": 279, "cover_light": 580, "huge": 529,
           "nonfinite": 140, "nan_single": 0}


@pytest.fixture(scope="module")
def empty_room():
    sd = seed_splitmix(32, 20, key=3)
    return sd, oracle_lib.render(ses.room(32, 20), sd, 4, 3)


@pytest.mark.parametrize("name", ses.NAMES)
def test_scene_is_finite_and_changes_the_image(name, empty_room):
    """Keeps a scene from degenerating into one that tests nothing: the
    oracle's image is finite and differs from the empty room's (nan_single:
    equal bit for bit, a NaN radius is never hit)."""
    sd, empty = empty_room
    out = oracle_lib.render(ses.build(name, 32, 20), sd, 4, 3)
    assert np.isfinite(out).all()
    changed = int((out.view(np.uint32) != empty.view(np.uint32)).any(axis=-1).sum())
    assert (changed > 0) == (name != "nan_single"), changed
    assert changed == CHANGED[name], changed
