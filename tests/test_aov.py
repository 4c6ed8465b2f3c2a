"""CPU: the C-ABI surface of the first-hit feature buffers (rt_render_aov) and
the reference the GPU tests compare against (tests/aov_ref.py).

The surface: both entry points declared and bound, the two 24-byte structs in
ctypes and in a C99 program, RT_AOV_CENTER, the unchanged ABI version, status
codes for null contexts.  The reference: its centre ids against the C
oracle's pto_primary_ids, and floors that make the GPU inputs worth running --
frames with all-miss pixels, partly covered pixels, pixels whose samples see
several primitives, light hits and sphere hits."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import aov_ref as ar
import gpuraytracer_amd as g
import oracle_lib
from gpuraytracer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48


def test_header_declares_both_entry_points():
    text = open(os.path.join(ROOT, "include", "rtpt.h")).read()
    assert "int rt_render_aov(rt_ctx* ctx, const rt_aov_params* params, const rt_aov_buffers* buffers);" in text
    assert "int rt_render_aov_async(" in text
    for name in ("rt_render_aov", "rt_render_aov_async"):
        assert name in _native.SIGNATURES and hasattr(g.lib, name)
    assert "presence of the symbol" in " ".join(text.split())  # how a caller detects the feature at ABI 11


def test_struct_sizes_ctypes():
    assert ctypes.sizeof(_native.AovParams) == 24 and ctypes.sizeof(_native.AovBuffers) == 24
    assert [n for n, _ in _native.AovParams._fields_] == ["spp", "sample_base", "row_start", "row_step",
                                                          "row_count", "flags"]
    assert _native.AovBuffers.normal_depth.offset == 8 and _native.AovBuffers.first_hit.offset == 16


def test_struct_sizes_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "aov.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rtpt.h"
int main(void) {
    if (sizeof(rt_aov_params) != 24 || sizeof(rt_aov_buffers) != 24) return 1;
    if (offsetof(rt_aov_params, flags) != 20 || offsetof(rt_aov_buffers, first_hit) != 16) return 2;
    if (RT_AOV_CENTER != 0x400u || RTPT_ABI_VERSION != 11) return 3;
    rt_aov_params p = {1, 0, 0, 1, 0, RT_AOV_CENTER};
    rt_aov_buffers b = {NULL, NULL, NULL};
    if (rt_render_aov(NULL, &p, &b) != RT_ERR_INVALID_ARG) return 4;
    if (rt_render_aov_async(NULL, &p, &b, NULL) != RT_ERR_INVALID_ARG) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "aov"
    libdir = os.path.join(ROOT, "gpuraytracer_amd")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lrtpt", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-500:])


def test_center_flag_and_abi_version():
    assert _native.RT_AOV_CENTER == 0x400 and g.RT_AOV_CENTER == 0x400
    assert g.lib.rt_abi_version() == 11 and g.ABI_VERSION == 11


def test_null_context_calls_return_status():
    p, b = _native.AovParams(), _native.AovBuffers()
    p.spp = 1
    assert g.lib.rt_render_aov(None, ctypes.byref(p), ctypes.byref(b)) == 1
    assert b"null" in g.lib.rt_last_error(None)
    assert g.lib.rt_render_aov_async(None, ctypes.byref(p), ctypes.byref(b), None) == 1
    assert g.lib.rt_render_aov(None, None, None) == 1


def test_center_ids_equal_the_c_oracle():
    scene = g.Scene.cornell_box(W, H)
    ref = ar.buffers(ar.np_scene(scene), None, 1, center=True)
    ids = oracle_lib.primary_ids(scene)
    assert np.array_equal(ref["first_hit"]["id"], ids)
    hit = ids >= 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(ref["albedo"][..., 3], hit.astype(np.float32))  # coverage of one centre ray
    assert np.array_equal(ref["first_hit"]["t"][~hit], np.full((~hit).sum(), 1000.0, np.float32))
    assert np.array_equal(ref["normal_depth"][..., 3][hit], ref["first_hit"]["t"][hit])


@functools.lru_cache(maxsize=None)
def hits_of(name, w, h, spp):
    scene = g.Scene.cornell_box(w, h) if name == "cornell" else g.Scene.random_spheres(w, h, 200, seed=42)
    return scene, ar.sample_hits(ar.np_scene(scene), g.seed_splitmix(w, h), spp)


def _pixel_stats(ids):
    """Pixels without a hit, partly covered pixels, and pixels whose samples
    give more than one id (a miss's -1 counts as one)."""
    cov = (ids >= 0).sum(0)
    return {"all_miss": int((cov == 0).sum()), "partial": int(((cov > 0) & (cov < ids.shape[0])).sum()),
            "mixed": int((ids.min(0) != ids.max(0)).sum())}


def test_floors_cornell():
    """64x48 x 17 spp, seeds splitmix(0x5EED00000000): measured 312 all-miss
    pixels, 208 partly covered, 686 with more than one id, 260 light-hit
    samples, 23 distinct ids."""
    _, h = hits_of("cornell", W, H, 17)
    s = _pixel_stats(h["ids"])
    light = int(((h["ids"] == 34) | (h["ids"] == 35)).sum())
    print(s, light, len(np.unique(h["ids"][h["ids"] >= 0])))
    assert s["all_miss"] >= 100 and s["partial"] >= 100 and s["mixed"] >= 500
    assert light >= 100


def test_floors_spheres():
    """200 spheres (seed 42), 64x48 x 17 spp: measured 9,494 sphere-hit
    samples and 1,212 pixels with more than one id."""
    scene, h = hits_of("spheres", W, H, 17)
    s = _pixel_stats(h["ids"])
    sph = int((h["ids"] >= scene.n_triangles).sum())
    print(s, sph)
    assert sph >= 5000 and s["mixed"] >= 500


def test_floor_partial_tiles_frame():
    """70x45 x 5 spp Cornell: measured 214 partly covered pixels."""
    _, h = hits_of("cornell", 70, 45, 5)
    s = _pixel_stats(h["ids"])
    print(s)
    assert s["partial"] >= 100


def test_reference_sums_and_miss_convention():
    """The buffers are the in-order sums of the per-sample records over spp,
    and skipping a miss changes nothing: a miss's record is all +0 and no sum
    is ever -0."""
    scene, h = hits_of("cornell", W, H, 17)
    ref = ar.buffers(None, None, 17, hits=h)
    miss = h["ids"] < 0
    assert not h["a"][miss].any() and not h["N"][miss].any()
    cov = (~miss).sum(0).astype(np.float32) / np.float32(17)
    assert np.array_equal(ref["albedo"][..., 3], cov)
    for k in ("albedo", "normal_depth"):
        assert not (np.signbit(ref[k]) & (ref[k] == 0)).any()
    assert np.array_equal(ref["first_hit"]["id"], h["ids"][0])
