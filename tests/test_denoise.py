"""CPU: the C-ABI surface of the denoiser (rt_denoise) and the numpy
restatement of its arithmetic contract (tests/denoise_ref.py)
that the GPU tests compare against bit for bit.

The surface: both entry points and both structs declared and bound, their
sizes in ctypes and in a C99 program, the defaults, the unchanged ABI version,
status codes for null contexts.  The restatement: what it must do on frames
whose answer is known without it, and the quality it has to reach on a real
low-spp render against a converged one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aov_ref as ar
import denoise_ref as dr
import gpuraytracer_amd as g
import oracle_lib
from gpuraytracer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H = 24, 16


def test_header_declares_both_entry_points_and_structs():
    text = " ".join(open(os.path.join(ROOT, "include", "rtpt.h")).read().split())
    assert "int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_buffers* buffers);" in text
    assert "int rt_denoise_async(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_buffers* buffers_dev, void* hip_stream);" in text
    assert "void rt_denoise_params_default(rt_denoise_params* params);" in text
    assert "} rt_denoise_params;" in text and "} rt_denoise_buffers;" in text
    assert "presence of the symbol rt_denoise" in text  # how a caller detects the feature at ABI 11


def test_ctypes_table_and_struct_sizes():
    for name in ("rt_denoise", "rt_denoise_async", "rt_denoise_params_default"):
        assert name in _native.SIGNATURES and hasattr(g.lib, name)
    assert ctypes.sizeof(_native.DenoiseParams) == 32 and ctypes.sizeof(_native.DenoiseBuffers) == 40
    assert [n for n, _ in _native.DenoiseParams._fields_] == ["iterations", "normal_power_log2", "sigma_luminance",
                                                              "sigma_depth", "depth_floor", "flags", "reserved"]
    assert [n for n, _ in _native.DenoiseBuffers._fields_] == ["color_a", "color_b", "albedo", "normal_depth", "out"]
    assert _native.DenoiseBuffers.out.offset == 32 and _native.DenoiseParams.flags.offset == 20
    assert g.DenoiseParams is _native.DenoiseParams and g.DenoiseBuffers is _native.DenoiseBuffers


def test_struct_sizes_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "denoise.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rtpt.h"
int main(void) {
    if (sizeof(rt_denoise_params) != 32 || sizeof(rt_denoise_buffers) != 40) return 1;
    if (offsetof(rt_denoise_buffers, out) != 32) return 2;
    if (RTPT_ABI_VERSION != 11) return 3;
    rt_denoise_params p;
    rt_denoise_params_default(&p);
    if (p.iterations != 5 || p.normal_power_log2 != 7 || p.sigma_luminance != 4.0f || p.sigma_depth != 1.0f ||
        p.depth_floor != 0.01f || p.flags != 0 || p.reserved[0] != 0 || p.reserved[1] != 0) return 6;
    rt_denoise_buffers b = {NULL, NULL, NULL, NULL, NULL};
    if (rt_denoise(NULL, &p, &b) != RT_ERR_INVALID_ARG) return 4;
    if (rt_denoise_async(NULL, &p, &b, NULL) != RT_ERR_INVALID_ARG) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "denoise"
    libdir = os.path.join(ROOT, "gpuraytracer_amd")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lrtpt", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-500:])


def test_defaults():
    p = _native.DenoiseParams()
    p.iterations, p.flags, p.reserved[1] = 99, 7, 3  # overwritten
    g.lib.rt_denoise_params_default(ctypes.byref(p))
    assert (p.iterations, p.normal_power_log2, p.flags, list(p.reserved)) == (5, 7, 0, [0, 0])
    assert (f32(p.sigma_luminance), f32(p.sigma_depth), f32(p.depth_floor)) == (f32(4.0), f32(1.0), f32(0.01))
    assert dr.DEFAULTS == dict(iterations=5, normal_power_log2=7, sigma_luminance=4.0, sigma_depth=1.0,
                               depth_floor=0.01)
    assert g.lib.rt_abi_version() == 11 and g.ABI_VERSION == 11


def test_null_context_calls_return_status():
    p, b = _native.DenoiseParams(), _native.DenoiseBuffers()
    g.lib.rt_denoise_params_default(ctypes.byref(p))
    assert g.lib.rt_denoise(None, ctypes.byref(p), ctypes.byref(b)) == 1
    assert b"null" in g.lib.rt_last_error(None)
    assert g.lib.rt_denoise_async(None, ctypes.byref(p), ctypes.byref(b), None) == 1
    assert g.lib.rt_denoise(None, None, None) == 1


# ---- properties of the restatement on synthetic 24x16 buffers -----------------

def _frames(seed, coverage):
    rng = np.random.default_rng(seed)
    ca = rng.uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    cb = rng.uniform(0.0, 2.0, (H, W, 4)).astype(f32)
    al = rng.uniform(0.05, 1.0, (H, W, 4)).astype(f32)
    al[..., 3] = coverage
    n = rng.normal(size=(H, W, 3))
    nd = np.empty((H, W, 4), f32)
    nd[..., :3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(f32)
    nd[..., 3] = rng.uniform(1.0, 5.0, (H, W)).astype(f32)
    return ca, cb, al, nd


def test_all_miss_frame_is_the_mean_of_the_halves():
    ca, cb, al, nd = _frames(1, 0.0)
    out = dr.denoise(ca, cb, al, nd)
    want = np.concatenate([(ca[..., :3] + cb[..., :3]) * f32(0.5), ca[..., 3:]], -1)
    assert dr.same(out, want), dr.first_difference(out, want)


def test_single_hit_pixel_returns_itself():
    cov = np.zeros((H, W), f32)
    cov[7, 11] = 0.25
    ca, cb, al, nd = _frames(2, cov)
    out = dr.denoise(ca, cb, al, nd)
    want = np.concatenate([(ca[..., :3] + cb[..., :3]) * f32(0.5), ca[..., 3:]], -1)
    am = np.maximum(al[7, 11, :3], f32(2.0 ** -10))
    ia = f32(1.0) / am
    # the centre tap alone: D' = (w * D) * (1 / w) with w = 9/64, once per iteration
    d = (ca[7, 11, :3] * ia + cb[7, 11, :3] * ia) * f32(0.5)
    k = f32(0.375) * f32(0.375)
    for _ in range(5):
        d = (k * d) * (f32(1.0) / k)
    want[7, 11, :3] = d * am
    assert dr.same(out, want), dr.first_difference(out, want)
    assert np.allclose(out[7, 11, :3], (ca[7, 11, :3] + cb[7, 11, :3]) * f32(0.5), rtol=1e-5)


def test_constant_demodulated_colour_is_kept():
    """Ca == Cb == c * albedo: D is the constant c everywhere (up to the
    rounding of the division), V = 0, and a normalised weighted mean of a
    constant is the constant: the output stays within 4 ulp of the input."""
    ca, _, al, nd = _frames(3, 1.0)
    c = f32(0.7)
    ca[..., :3] = c * al[..., :3]
    out = dr.denoise(ca, ca.copy(), al, nd)
    ulp = np.abs(out[..., :3].view(np.int32).astype(np.int64) - ca[..., :3].view(np.int32).astype(np.int64))
    print("max ulp", ulp.max())
    assert ulp.max() <= 4
    assert np.array_equal(out[..., 3], ca[..., 3])


# ---- quality on a real low-spp render -----------------------------------------

def test_quality_cornell_160x120():
    """Cornell 160x120, 3 bounces, default seeds: halves of 2 spp at
    sample_base 0 and 2, AOVs of the 4 samples, reference 2048 spp at
    sample_base 1000.  RMSE over all pixels and rgb in float64; the defaults
    must give RMSE(denoised) <= 0.4 * RMSE(mean of the halves)."""
    w, h = 160, 120
    scene = g.Scene.cornell_box(w, h)
    seeds = g.seed_splitmix(w, h)
    ca = oracle_lib.render(scene, seeds, 2, 3, sample_base=0)
    cb = oracle_lib.render(scene, seeds, 2, 3, sample_base=2)
    aov = ar.buffers(ar.np_scene(scene), seeds, 4)
    ref = oracle_lib.render(scene, seeds, 2048, 3, sample_base=1000, threads=os.cpu_count())
    out = dr.denoise(ca, cb, aov["albedo"], aov["normal_depth"])
    noisy = (ca[..., :3] + cb[..., :3]) * f32(0.5)

    def rmse(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))

    rn, rd = rmse(noisy), rmse(out[..., :3])
    print(f"RMSE noisy {rn:.4f} denoised {rd:.4f} ratio {rd / rn:.3f}")
    assert rd <= 0.4 * rn
