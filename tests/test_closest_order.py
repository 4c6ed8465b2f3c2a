"""CPU: the ordered and culled closest query of the box-cluster kernel
(gpuraytracer_amd/csrc/rt_cluorder.hpp) checked by a small C++
program linked against librtpt.so and the oracle
(tests/native/closest_order_check.cpp): over path-like rays, rays from the box
faces and rays grazing silhouettes, edges, corners and the padded planes, the
query that tests the entry-side candidates first and culls the exit-side ones
by the hit found returns the (t, id) of the id-ordered strict-'<' brute force
with the reference's triangle test, bit for bit.  Two wrong queries must be
caught: one that drops the far candidates after any near hit, one that forms
the far bound without the filter's slack.  The GPU side:
tests/test_gpu_closest_order.py."""
import os
import shutil
import subprocess

import pytest

from closest_order_scenes import NO_CLUSTERS, scenes, write_scene_file
from conftest import native_toolchain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = scenes()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    cxx, san, lib = native_toolchain(cxx)
    orc = os.environ.get("RTPT_SAN_DIR") or os.path.join(ROOT, "oracle")
    if not os.path.exists(os.path.join(orc, "liboracle.so")):
        pytest.skip("oracle/liboracle.so not built")
    out = tmp_path_factory.mktemp("clo") / "closest_order_check"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", *san, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "gpuraytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "closest_order_check.cpp"),
                           "-L", lib, "-lrtpt", f"-Wl,-rpath,{lib}",
                           "-L", orc, "-loracle", f"-Wl,-rpath,{orc}", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("clo_scenes")
    files = {}
    for name, make in SCENES.items():
        files[name] = str(d / (name + ".bin"))
        write_scene_file(make(), files[name])
    return files


def run(checker, path, seed, mode=0):
    return subprocess.run([checker, path, str(seed), str(mode)], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_ordered_query_equals_brute_force(checker, scene_files, name):
    r = run(checker, scene_files[name], 1)
    assert r.returncode == 0, r.stdout + r.stderr
    if name in NO_CLUSTERS:
        assert r.stdout.startswith("no clusters"), r.stdout
    else:
        assert r.stdout.startswith("ok"), r.stdout
        # the cull is exercised: rays with near and far candidates, some culled
        assert int(r.stdout.split("far culled ")[1].split()[0]) > 0, r.stdout


def test_dropping_far_after_a_near_hit_is_caught(checker, scene_files):
    r = run(checker, scene_files["protruding"], 1, mode=1)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, r.stdout + r.stderr


def test_far_bound_without_slack_is_caught(checker, scene_files):
    r = run(checker, scene_files["protruding"], 1, mode=2)
    assert r.returncode == 1 and "MISMATCH class C" in r.stdout, r.stdout + r.stderr
