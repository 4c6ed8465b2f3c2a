#!/usr/bin/env python3
"""CPU count of the bounce-0 occluder masks (rt_shaft.hpp) over
a Cornell frame in 4x4 tiles, through rt_debug_shadow_candidates:
    python tools/shadow_mask_stats.py [W H]
Prints the histogram of mask sizes (pairs), the share of empty masks among the
tiles whose camera mask holds a pair that is neither the light nor the ceiling,
the same for tiles whose camera mask holds one pair (the only waves the kernel
decides), the share of tiles where nothing is decided, and for K = 1, 2, 3 the
share of the tiles with a decided non-empty mask whose mask holds at most K
pairs (the masks RT_SHD_SHORT = K tests directly)."""
import collections
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gpuraytracer_amd import Scene  # noqa: E402
from gpuraytracer_amd._native import lib  # noqa: E402


def main():
    W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
    s = Scene.cornell_box(W, H)
    n = s.n_triangles
    desc = s.desc()
    cam, occ, avail = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)(), ctypes.c_int32()
    light = {k // 2 for k in range(n) if s.materials[k].emissive.x or s.materials[k].emissive.y
             or s.materials[k].emissive.z}
    ys = [max(s.vertices[3 * k + v].y for v in range(3)) for k in range(n)]
    top = max(ys)
    ceiling = {k // 2 for k in range(n) if min(s.vertices[3 * k + v].y for v in range(3)) == top} - light
    hist, tiles, unavailable, lit, lit_empty, lit_empty_one = collections.Counter(), 0, 0, 0, 0, 0
    one_pair_hist = collections.Counter()  # mask sizes of the tiles the kernel decides
    for y0 in range(0, H, 4):
        for x0 in range(0, W, 4):
            rect = (x0, x0 + 3, y0, y0 + 3)
            assert lib.rt_debug_camera_candidates(ctypes.byref(desc), *rect, cam) == 0
            assert lib.rt_debug_shadow_candidates(ctypes.byref(desc), *rect, occ, ctypes.byref(avail)) == 0
            tiles += 1
            if not avail.value:
                unavailable += 1
                continue
            size = int(np.frombuffer(occ, np.uint8)[0::2].sum())
            hist[size] += 1
            seen = set(np.flatnonzero(np.frombuffer(cam, np.uint8)[0::2]).tolist())
            if len(seen) == 1 and not seen <= light:
                one_pair_hist[size] += 1
            if seen - light - ceiling:
                lit += 1
                lit_empty += size == 0
                lit_empty_one += size == 0 and len(seen) == 1  # the kernel decides one-pair waves only
    # RT_SHD_SHORT = K: the tiles whose bounce-0 shadow queries
    # run at all (a decided, non-empty mask; the kernel decides one-camera-pair
    # waves only) and the share of them a direct test of masks of <= K pairs covers
    queried = sum(c for size, c in one_pair_hist.items() if size > 0)
    short = {K: sum(c for size, c in one_pair_hist.items() if 0 < size <= K) for K in (1, 2, 3)}
    print(json.dumps({"W": W, "H": H, "tiles": tiles, "unavailable": unavailable,
                      "one_camera_pair_mask_size_histogram": dict(sorted(one_pair_hist.items())),
                      "lit_tiles_with_a_decided_nonempty_mask": queried,
                      "short_mask_tiles_by_K": short,
                      "short_mask_share_of_those_by_K": {K: c / max(queried, 1) for K, c in short.items()},
                      "short_mask_share_of_all_tiles_by_K": {K: c / tiles for K, c in short.items()},
                      "unavailable_share": unavailable / tiles, "mask_size_histogram": dict(sorted(hist.items())),
                      "tiles_with_a_lit_surface": lit, "of_those_empty": lit_empty, "of_those_empty_with_one_camera_pair": lit_empty_one,
                      "empty_share": lit_empty / max(lit, 1), "light_pairs": sorted(light),
                      "ceiling_pairs": sorted(ceiling)}))


if __name__ == "__main__":
    main()
