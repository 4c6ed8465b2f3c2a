#!/usr/bin/env python3
"""CPU count of the candidate rounds of the box-cluster kernel's closest
queries at bounces 1 and 2: rounds per wave and lanes per
round for the single-mask order and for the ordered and culled one, over
Cornell and the Scene.random_boxes scenes.  Compiles tools/closest_rounds.cpp
(the kernel's own per-lane classification, rt_cluorder.hpp) against the built
librtpt.so and oracle/liboracle.so; needs no GPU.
  python tools/closest_round_stats.py [--waves 20000] [--out FILE.json]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from closest_order_scenes import write_scene_file  # noqa: E402
from gpuraytracer_amd import Scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cxx = shutil.which("g++") or shutil.which("c++")
    pkg, orc = os.path.join(ROOT, "gpuraytracer_amd"), os.path.join(ROOT, "oracle")
    scenes = {"cornell": Scene.cornell_box(1920, 1080)}
    for n in range(1, 5):
        scenes[f"random_boxes_{n}"] = Scene.random_boxes(1920, 1080, n, seed=3)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "closest_rounds")
        subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(pkg, "csrc"), os.path.join(ROOT, "tools", "closest_rounds.cpp"),
                               "-L", pkg, "-lrtpt", f"-Wl,-rpath,{pkg}", "-L", orc, "-loracle",
                               f"-Wl,-rpath,{orc}", "-o", exe])
        for name, s in scenes.items():
            path = os.path.join(tmp, name + ".bin")
            write_scene_file(s, path)
            r = subprocess.run([exe, path, str(a.seed), str(a.waves)], capture_output=True, text=True)
            res[name] = json.loads(r.stdout)
            assert r.returncode == 0, (name, r.stdout, r.stderr)
    for name, d in res.items():
        for b in ("bounce1", "bounce2"):
            q = d[b]
            print(f"{name:16s} {b}: live {q['live_lanes_per_wave']:5.1f}  rounds/wave "
                  f"{q['single_mask']['rounds_per_wave']:.2f} -> {q['ordered']['rounds_per_wave']:.2f}  "
                  f"lanes/round {q['single_mask']['lanes_per_round']:.1f} -> {q['ordered']['lanes_per_round']:.1f}  "
                  f"tests/lane {q['single_mask']['pair_tests_per_lane']:.2f} -> "
                  f"{q['ordered']['pair_tests_per_lane']:.2f}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
