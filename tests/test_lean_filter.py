"""CPU: the lean paths of the box-cluster filter (gpuraytracer_amd/csrc/
rt_cluorder.hpp) checked by a small C++ program linked against
librtpt.so and the oracle (tests/native/lean_filter_check.cpp).  The program
runs the kernel's own per-lane filter text over more than 200,000 rays per
scene -- closest queries from surface points in cosine-weighted directions,
from points on the room's walls and on the bounds of its shrunk box, in
directions with exactly zero components, and shadow segments to points drawn on
the light -- and asserts, with no tolerance:
  * every pair with a triangle the oracle's test accepts is a lean candidate,
  * far_lo never exceeds the t of an accepted hit on a far candidate,
  * the query over the candidates returns the brute force's (t, id) / boolean.
The kinds the scene compiler reports (rt_debug_cluster_kinds) are asserted per
scene, and two wrong filters must be caught: the turned-box products applied to
a tilted box, and the light skip applied to an emissive quad 5e-4 below the
sampling plane.  The GPU side: tests/test_gpu_lean_filter.py."""
import os
import shutil
import subprocess

import pytest

from closest_order_scenes import write_scene_file
from conftest import native_toolchain
from lean_filter_scenes import CONTAINER, INSIDE, OWN_LIGHT, SINGLE, TURNED, kinds, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = scenes()
ROOM = CONTAINER | INSIDE
LIGHT = SINGLE | OWN_LIGHT

# The kind bits (8 container, 16 single face, 32 turned, 64 shrunk box, 128 own
# light) of every cluster, sorted.  A box at 0 or 90 degrees has world axes and
# room inside: a container, never "turned".  In second_emitter only the light
# itself is an own-light cluster; in light_minus_zero nothing is.
EXPECTED = {
    "cornell": sorted([ROOM, TURNED, TURNED, LIGHT]),
    "turned_0deg": sorted([ROOM, ROOM, LIGHT]),
    "turned_90deg": sorted([ROOM, ROOM, LIGHT]),
    "turned_y_minus": sorted([ROOM, TURNED, LIGHT]),
    "turned_x": sorted([ROOM, TURNED, LIGHT]),
    "turned_z": sorted([ROOM, TURNED, LIGHT]),
    "tilted": sorted([ROOM, 0, LIGHT]),
    "outside": sorted([ROOM, TURNED, LIGHT]),
    "second_emitter": sorted([ROOM, SINGLE, TURNED, LIGHT]),
    "light_minus_zero": sorted([ROOM, TURNED, SINGLE]),
    "boxes1": sorted([ROOM, 0, LIGHT]),
    "boxes2": sorted([ROOM, 0, 0, LIGHT]),
    "boxes3": sorted([ROOM, 0, 0, 0, LIGHT]),
    "boxes4": sorted([ROOM, 0, 0, 0, 0, LIGHT]),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    cxx, san, lib = native_toolchain(cxx)
    orc = os.environ.get("RTPT_SAN_DIR") or os.path.join(ROOT, "oracle")
    if not os.path.exists(os.path.join(orc, "liboracle.so")):
        pytest.skip("oracle/liboracle.so not built")
    out = tmp_path_factory.mktemp("lean") / "lean_filter_check"
    # all three items, also those the kernel does not ship (rt_cluorder.hpp RT_CLU_LEAN_ITEMS)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-DRT_CLU_LEAN_ITEMS=7", *san,
                           "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gpuraytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "lean_filter_check.cpp"),
                           "-L", lib, "-lrtpt", f"-Wl,-rpath,{lib}",
                           "-L", orc, "-loracle", f"-Wl,-rpath,{orc}", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_scenes")
    files = {}
    for name, make in SCENES.items():
        files[name] = str(d / (name + ".bin"))
        write_scene_file(make(), files[name])
    return files


def run(checker, path, seed=1, mode=0):
    return subprocess.run([checker, path, str(seed), str(mode)], capture_output=True, text=True, timeout=300)


def counts(stdout):
    return {k: int(v) for k, v in (w.split("=") for w in stdout.split()[1:])}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_reported_kinds(name):
    assert kinds(SCENES[name]()) == EXPECTED[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_lean_candidates_hold_every_accepted_hit(checker, scene_files, name):
    r = run(checker, scene_files[name])
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    c = counts(r.stdout)
    assert c["closest"] + c["shadow"] >= 200_000, r.stdout
    assert c["occluded"] > 0, r.stdout
    # the exit-only path is taken, and the wall and bound origins make it fall back
    assert c["exit-only"] > 0 and c["full"] > 0, r.stdout
    # every shadow query passes over the light's own cluster, or none does
    assert c["own-skipped"] == (c["shadow"] if OWN_LIGHT in [k & OWN_LIGHT for k in EXPECTED[name]] else 0), r.stdout
    if name == "outside":
        # path-like rays that start on the box in front of the room are outside the container
        assert c["A-full"] > 1000, r.stdout
    elif name in ("boxes1", "tilted"):
        # inside the room a path-like ray leaves it from inside, but for the few
        # origins within the shrink of a second wall (an edge of the room)
        assert c["A-full"] <= c["A-exit-only"] // 1000, r.stdout
    elif name == "cornell":
        # the same, and the origins this check draws under the boxes' bottom
        # faces, which lie in the floor (4 of 36 triangles, either side)
        assert c["A-exit-only"] > 5 * c["A-full"], r.stdout


def test_turned_products_on_a_tilted_box_are_caught(checker, scene_files):
    r = run(checker, scene_files["tilted"], mode=1)
    assert r.returncode == 1 and ("MISSING" in r.stdout or "FAR_LO" in r.stdout), r.stdout + r.stderr


def test_light_skip_below_the_sampling_plane_is_caught(checker, scene_files):
    r = run(checker, scene_files["second_emitter"], mode=2)
    assert r.returncode == 1 and "MISSING class" in r.stdout, r.stdout + r.stderr
