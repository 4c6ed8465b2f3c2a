"""CPU: the C-ABI surface of temporal reprojection (rt_reproject), the host
function rt_reproject_host against the numpy restatement of the contract
(tests/reproject_ref.py) bit for bit, the stand-alone
sanitizer program, and the quality the accumulation has to reach on an
orbiting camera against a converged render."""
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
import pose_scenes as ps
import reproject_cases as rc
import reproject_ref as rr
from gpuraytracer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- interface -------------------------------------------------------------------

def test_header_declares_the_entry_points_and_structs():
    text = " ".join(open(os.path.join(ROOT, "include", "rtpt.h")).read().split())
    assert ("int rt_reproject(rt_ctx* ctx, const rt_reproject_params* params, const CameraGPU* prev_camera, "
            "const rt_reproject_buffers* buffers);") in text
    assert ("int rt_reproject_async(rt_ctx* ctx, const rt_reproject_params* params, const CameraGPU* prev_camera, "
            "const rt_reproject_buffers* buffers_dev, void* hip_stream);") in text
    assert ("int rt_reproject_host(const CameraGPU* camera, const CameraGPU* prev_camera, "
            "const rt_reproject_params* params, const rt_reproject_buffers* buffers);") in text
    assert "void rt_reproject_params_default(rt_reproject_params* params);" in text
    assert "} rt_reproject_params;" in text and "} rt_reproject_buffers;" in text
    assert "presence of the symbol rt_reproject" in text  # how a caller detects the feature at ABI 11
    assert "is not compensated" in text                     # moving geometry is out of scope, and said so


def test_ctypes_table_and_struct_sizes():
    for name in ("rt_reproject", "rt_reproject_async", "rt_reproject_host", "rt_reproject_params_default"):
        assert name in _native.SIGNATURES and hasattr(g.lib, name)
    assert ctypes.sizeof(_native.ReprojectParams) == 32 and ctypes.sizeof(_native.ReprojectBuffers) == 80
    assert [n for n, _ in _native.ReprojectParams._fields_] == ["max_history", "normal_cos_min", "plane_rel",
                                                                "weight_min", "flags", "reserved"]
    assert [n for n, _ in _native.ReprojectBuffers._fields_] == ["color", "history", "hit", "normal_depth",
                                                                 "prev_hit", "prev_normal_depth", "out"]
    assert _native.ReprojectParams.flags.offset == 16 and _native.ReprojectBuffers.out.offset == 64
    assert g.ReprojectParams is _native.ReprojectParams and g.ReprojectBuffers is _native.ReprojectBuffers


def test_struct_sizes_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "reproject.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rtpt.h"
int main(void) {
    if (sizeof(rt_reproject_params) != 32 || sizeof(rt_reproject_buffers) != 80) return 1;
    if (offsetof(rt_reproject_buffers, hit) != 32 || offsetof(rt_reproject_buffers, out) != 64) return 2;
    if (RTPT_ABI_VERSION != 11) return 3;
    rt_reproject_params p;
    rt_reproject_params_default(&p);
    if (p.max_history != 32 || p.normal_cos_min != 0.9f || p.plane_rel != 0.0078125f || p.weight_min != 0.0625f ||
        p.flags != 0 || p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return 6;
    rt_reproject_buffers b = {{NULL, NULL}, {NULL, NULL}, NULL, NULL, NULL, NULL, {NULL, NULL}};
    if (rt_reproject(NULL, &p, NULL, &b) != RT_ERR_INVALID_ARG) return 4;
    if (rt_reproject_async(NULL, &p, NULL, &b, NULL) != RT_ERR_INVALID_ARG) return 5;
    if (rt_reproject_host(NULL, NULL, &p, &b) != RT_ERR_INVALID_ARG) return 7;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "reproject"
    libdir = os.path.join(ROOT, "gpuraytracer_amd")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lrtpt", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-500:])


def test_defaults():
    p = _native.ReprojectParams()
    p.max_history, p.flags, p.reserved[2] = 99, 7, 3  # overwritten
    g.lib.rt_reproject_params_default(ctypes.byref(p))
    assert (p.max_history, p.flags, list(p.reserved)) == (32, 0, [0, 0, 0])
    assert (f32(p.normal_cos_min), f32(p.plane_rel), f32(p.weight_min)) == (f32(0.9), f32(2.0 ** -7), f32(0.0625))
    assert rr.DEFAULTS == dict(max_history=32, normal_cos_min=0.9, plane_rel=2.0 ** -7, weight_min=0.0625)
    assert g.lib.rt_abi_version() == 11 and g.ABI_VERSION == 11


def test_null_context_calls_return_status():
    p, b = _native.ReprojectParams(), _native.ReprojectBuffers()
    g.lib.rt_reproject_params_default(ctypes.byref(p))
    assert g.lib.rt_reproject(None, ctypes.byref(p), None, ctypes.byref(b)) == 1
    assert b"null" in g.lib.rt_last_error(None)
    assert g.lib.rt_reproject_async(None, ctypes.byref(p), None, ctypes.byref(b), None) == 1
    assert g.lib.rt_reproject(None, None, None, None) == 1


def _host_call(camera, prev, p, b):
    st = g.lib.rt_reproject_host(ctypes.byref(camera) if camera is not None else None,
                                 ctypes.byref(prev) if prev is not None else None,
                                 ctypes.byref(p) if p is not None else None,
                                 ctypes.byref(b) if b is not None else None)
    return st, g.lib.rt_last_error(None).decode()


def test_host_function_argument_errors_name_the_field():
    w, h = 8, 6
    scene = g.Scene.cornell_box(w, h)
    frames = [np.zeros((h, w, 4), f32) for _ in range(8)]
    hits = [np.zeros((h, w), ar.HIT_DTYPE) for _ in range(2)]

    def good():
        p, b = _native.ReprojectParams(), _native.ReprojectBuffers()
        g.lib.rt_reproject_params_default(ctypes.byref(p))
        for k in range(2):
            b.color[k], b.history[k], b.out[k] = (frames[3 * k + i].ctypes.data for i in range(3))
        b.normal_depth, b.prev_normal_depth = frames[6].ctypes.data, frames[7].ctypes.data
        b.hit, b.prev_hit = hits[0].ctypes.data, hits[1].ctypes.data
        return p, b

    p, b = good()
    assert _host_call(scene.camera, None, p, b)[0] == 0
    assert _host_call(scene.camera, scene.camera, p, b)[0] == 0

    def bad(what, camera=scene.camera, prev=None, edit=None, params=True, buffers=True):
        p, b = good()
        if edit:
            edit(p, b)
        st, msg = _host_call(camera, prev, p if params else None, b if buffers else None)
        assert st == 1 and what in msg and msg.startswith("rt_reproject_host: "), (what, st, msg)

    bad("params is null", params=False)
    bad("buffers is null", buffers=False)
    bad("camera is null", camera=None)
    for name in ("hit", "normal_depth", "prev_hit", "prev_normal_depth"):
        bad(f"{name} is null", edit=lambda p, b, n=name: setattr(b, n, None))
    for name in ("color", "history", "out"):
        def null0(p, b, n=name):
            getattr(b, n)[0] = None
        bad(f"{name}[0] is null", edit=null0)

        def null1(p, b, n=name):
            getattr(b, n)[1] = None
        bad("color[1], history[1] and out[1]", edit=null1)
    nan = float("nan")
    for field, values, what in (("max_history", (0, 65537), "max_history must be in [1, 65536]"),
                                ("normal_cos_min", (-1.5, 1.5, nan), "normal_cos_min must be in [-1, 1]"),
                                ("plane_rel", (-1e-9, nan), "plane_rel must be >= 0"),
                                ("weight_min", (0.0, -1.0, 1.5, nan), "weight_min must be in (0, 1]"),
                                ("flags", (1, 2, 0x400), "unknown flag bits")):   # the host form takes no flag
        for v in values:
            bad(what, edit=lambda p, b, f=field, v=v: setattr(p, f, v))
    for k in range(3):
        def res(p, b, k=k):
            p.reserved[k] = 1
        bad("reserved must be 0", edit=res)

    def cam(**kw):
        c = g.CameraGPU.from_buffer_copy(scene.camera)
        for k, v in kw.items():
            if k == "res":
                c.resolution.x, c.resolution.y = v
            elif k == "fov":
                c.horizontalFov = v
            else:
                f = getattr(c, k)
                f.x, f.y, f.z = v
        return c

    bad("prev_camera: resolution differs", prev=cam(res=(w + 1, h)))
    bad("prev_camera: camera resolution must be positive", prev=cam(res=(0, h)))
    bad("prev_camera: camera resolution.x < resolution.y", prev=cam(res=(h, w)))
    bad("prev_camera: camera vectors must be finite", prev=cam(position=(nan, 0, 0)))
    bad("prev_camera: camera direction", prev=cam(direction=(0, 0, 0)))
    bad("prev_camera: camera up", prev=cam(up=(0, 0, -1), direction=(0, 0, -2)))
    bad("prev_camera: camera horizontalFov", prev=cam(fov=float("inf")))
    bad("camera: camera direction", camera=cam(direction=(0, 0, 0)))
    # one-plane and the limits of every range pass
    p, b = good()
    b.color[1] = b.history[1] = b.out[1] = None
    p.max_history, p.normal_cos_min, p.plane_rel, p.weight_min = 65536, -1.0, float("inf"), 1.0
    assert _host_call(scene.camera, None, p, b)[0] == 0


def test_scene_compile_uses_the_same_camera_messages():
    """compile_scene and rt_reproject_host share one camera function: the
    scene compile reports the same texts (rt_scene_describe)."""
    scene = g.Scene.cornell_box(8, 6)
    bad = ps.posed(scene, direction=(0, 0, 0))
    info = _native.SceneInfo()
    assert g.lib.rt_scene_describe(ctypes.byref(bad.desc()), ctypes.byref(info)) == 1
    scene_msg = g.lib.rt_last_error(None).decode()
    p, b = _native.ReprojectParams(), _native.ReprojectBuffers()
    g.lib.rt_reproject_params_default(ctypes.byref(p))
    x = np.zeros((6, 8, 4), f32)
    hz = np.zeros((6, 8), ar.HIT_DTYPE)
    b.color[0] = b.history[0] = b.normal_depth = b.prev_normal_depth = x.ctypes.data
    b.out[0] = np.zeros_like(x).ctypes.data
    b.hit = b.prev_hit = hz.ctypes.data
    st, msg = _host_call(scene.camera, bad.camera, p, b)
    assert st == 1 and msg == "rt_reproject_host: prev_camera: " + scene_msg


# ---- the host function against the reference -------------------------------------

def _both(cur, prev, color, history, bufs, **kw):
    hit, nd, phit, pnd = bufs
    got = g.reproject_host(cur, prev, color, history, hit, nd, phit, pnd, **kw)
    stats = {}
    want = rr.reproject(cur, prev, color, history, hit, nd, phit, pnd, stats=stats, **kw)
    return got, want, stats


@pytest.mark.parametrize("name", list(rc.PAIRS))
def test_pose_pairs_bit_for_bit_and_reuse_bands(name):
    prev, cur = rc.pair_scenes(name)
    color, history = rc.planes(11)
    got, want, st = _both(cur.camera, prev.camera, color, history, rc.centre_buffers(name))
    for k in range(2):
        assert rr.same(got[k], want[k]), f"{name} plane {k}: " + rr.first_difference(got[k], want[k])
    n_hit, n_reused = int(st["hit"].sum()), int(st["reused"].sum())
    band = rc.PAIRS[name][3]
    print(f"{name}: hit {n_hit} reused {n_reused} share {n_reused / max(n_hit, 1):.3f} "
          f"behind {int(st['behind'].sum())} off-frame {int(st['off_frame'].sum())}")
    # every history alpha is >= 1: reuse is visible as out.a > 1
    assert np.array_equal(want[0][..., 3] > 1, st["reused"])
    if band is None:
        assert n_hit == 0
        for k in range(2):
            assert np.array_equal(want[k][..., :3], color[k][..., :3]) and np.all(want[k][..., 3] == 1)
        return
    assert n_hit > 0
    share = n_reused / n_hit
    assert band[0] <= share <= band[1], (name, share, band)
    if name == "wide_to_cornell":
        assert st["behind"].sum() > 0 and st["off_frame"].sum() > 0
    if name == "down_to_up":
        assert st["behind"].sum() > 0


@pytest.mark.parametrize("w,h", rc.SMALL)
def test_small_frames(w, h):
    prev, cur = rc.pair_scenes("shift", w, h)
    color, history = rc.planes(w * 100 + h, w, h)
    got, want, st = _both(cur.camera, prev.camera, color, history, rc.centre_buffers("shift", w, h))
    for k in range(2):
        assert rr.same(got[k], want[k]), f"{w}x{h} plane {k}: " + rr.first_difference(got[k], want[k])
    if w >= 17:
        assert st["reused"].sum() >= 0.5 * st["hit"].sum()


def test_variants():
    prev, cur = rc.pair_scenes("shift")
    bufs = rc.centre_buffers("shift")
    color, history = rc.planes(5)
    two, want2, st = _both(cur.camera, prev.camera, color, history, bufs)
    reused = st["reused"]
    assert reused.sum() > 1000
    # one plane: plane 0 of the two-plane call
    one, want1, _ = _both(cur.camera, prev.camera, color[:1], history[:1], bufs)
    assert len(one) == 1 and rr.same(one[0], two[0]) and rr.same(want1[0], want2[0])
    # out aliasing color
    alias = [c.copy() for c in color]
    hit, nd, phit, pnd = bufs
    g.reproject_host(cur.camera, prev.camera, alias, history, hit, nd, phit, pnd, out=alias)
    for k in range(2):
        assert rr.same(alias[k], two[k])
    # max_history 1: n = 1, al = 1, out = fma(1, cur - h, h): cur within the rounding of (cur - h) + h
    got, want, _ = _both(cur.camera, prev.camera, color, history, bufs, max_history=1)
    for k in range(2):
        assert rr.same(got[k], want[k])
        assert np.all(got[k][..., 3] == 1)
        err = np.abs(got[k][..., :3].astype(np.float64) - color[k][..., :3])
        # |h| < 2 and |cur - h| < 2: one rounding of cur - h (<= 2^-24 * 2) and one of the fma (<= 2^-24 * 2)
        assert err.max() <= 2.0 ** -22
        assert np.array_equal(got[k][~reused], np.concatenate([color[k][..., :3], np.ones_like(color[k][..., 3:])], -1)[~reused])
    # max_history 65536: no cap binds (history lengths <= 40), n = m + 1
    got, want, _ = _both(cur.camera, prev.camera, color, history, bufs, max_history=65536)
    for k in range(2):
        assert rr.same(got[k], want[k])
    assert got[0][..., 3].max() > 33
    assert two[0][..., 3].max() == 32    # the default cap binds on these histories
    # weight_min 1: only a sum of weights that reaches 1 reuses
    got, want, st1 = _both(cur.camera, prev.camera, color, history, bufs, weight_min=1.0)
    for k in range(2):
        assert rr.same(got[k], want[k])
    assert 0 < st1["reused"].sum() < reused.sum()
    # the camera did not move: prev NULL is prev == cur
    same_bufs = rc.centre_buffers("same")
    a = g.reproject_host(prev.camera, None, color, history, *same_bufs)
    b = g.reproject_host(prev.camera, prev.camera, color, history, *same_bufs)
    for k in range(2):
        assert rr.same(a[k], b[k])


# ---- totality --------------------------------------------------------------------

@pytest.mark.parametrize("params", list(rc.ADVERSARIAL_PARAMS))
@pytest.mark.parametrize("plausible", [False, True])
def test_adversarial_buffers(params, plausible):
    """Any bytes give a defined result and no read leaves the frame: the
    host result equals the reference wherever the reference is not NaN and is
    NaN where it is."""
    A = rc.adversarial(rc.W, rc.H, plausible)
    scene = rc.base_scene("cornell")
    kw = rc.ADVERSARIAL_PARAMS[params]
    reusing = 0
    for prev in (None, rc.shifted(scene).camera, ps.view(scene, "behind_left").camera):
        bufs = (A["hit"], A["normal_depth"], A["prev_hit"], A["prev_normal_depth"])
        got, want, st = _both(scene.camera, prev, A["color"], A["history"], bufs, **kw)
        for k in range(2):
            assert rr.same_or_nan(got[k], want[k]), rr.first_difference(got[k], want[k])
        reusing += int(st["reused"].sum())
    print(f"{params} plausible={plausible}: {reusing} reusing pixels")
    if params == "loose":
        assert reusing > 0   # the set reaches the taps and the blend


def test_adversarial_tables_hold_what_the_contract_names():
    t = np.array(rc.T_BITS, np.uint32).view(f32)
    assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any() and f32(1e30) in t and f32(-5) in t
    assert f32(0) in t and (np.abs(t[np.isfinite(t)]) < np.finfo(f32).tiny).sum() == 2  # 0 and a denormal
    assert set(np.array(rc.ID_BITS, np.uint32).view(np.int32).tolist()) >= {-1, 0, 35, 2 ** 31 - 1, -2 ** 31}
    n = np.array(rc.N_BITS, np.uint32).view(f32)
    assert np.isnan(n).any() and f32(0) in n and f32(1e30) in n
    a = np.array(rc.ALPHA_BITS, np.uint32).view(f32)
    assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any()


# ---- the stand-alone sanitizer program --------------------------------------------

def test_standalone_sanitizer_program(tmp_path):
    """tools/reproject_host_check.cpp: its own main, the host objects built
    with -fsanitize=address,undefined, nothing loaded into Python."""
    out = subprocess.run(["make", "-s", "-C", ROOT, "reproject-check", "ASAN=" + str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-1000:], out.stderr[-2000:])
    assert out.returncode == 0 and "0 failures" in out.stdout


# ---- quality ----------------------------------------------------------------------

def test_quality_orbiting_cornell():
    """Cornell 96x72, 3 bounces, 8 frames of 1+1 spp at sample_base 2 * frame,
    the eye at (9 sin a, 0.3 sin 2a, 9 cos a) looking at the origin, a = 0.05 *
    frame; reference 2048 spp at the last pose.  Measured with this reference
    (DESIGN.md §3.31): last frame 0.0638, accumulated 0.0207 (ratio 0.325),
    denoised last frame 0.0275, denoised accumulated 0.0149 (ratio 0.544)."""
    w, h, frames = 96, 72, 8
    base = g.Scene.cornell_box(w, h)
    seeds = g.seed_splitmix(w, h)

    def pose(f):
        a = 0.05 * f
        return ps.posed(base, eye=(9 * np.sin(a), 0.3 * np.sin(2 * a), 9 * np.cos(a)), look_at=(0, 0, 0))

    prev = None
    for f in range(frames):
        s = pose(f)
        ca = oracle_lib.render(s, seeds, 1, 3, sample_base=2 * f)
        cb = oracle_lib.render(s, seeds, 1, 3, sample_base=2 * f + 1)
        c = ar.buffers(ar.np_scene(s), None, 1, center=True)
        if prev is None:
            acc = [ca, cb]
        else:
            acc = rr.reproject(s.camera, prev["camera"], [ca, cb], prev["acc"], c["first_hit"], c["normal_depth"],
                               prev["hit"], prev["nd"])
            if f == 1:  # the host function computes the same planes
                got = g.reproject_host(s.camera, prev["camera"], [ca, cb], prev["acc"], c["first_hit"],
                                       c["normal_depth"], prev["hit"], prev["nd"])
                assert rr.same(got[0], acc[0]) and rr.same(got[1], acc[1])
            print(f"frame {f}: reused {np.mean(acc[0][..., 3][c['first_hit']['id'] >= 0] > 1):.3f} of the hit pixels")
        prev = dict(camera=s.camera, acc=acc, hit=c["first_hit"], nd=c["normal_depth"])
    aov = ar.buffers(ar.np_scene(s), seeds, 2, sample_base=2 * (frames - 1))
    ref = oracle_lib.render(s, seeds, 2048, 3, sample_base=1000, threads=os.cpu_count())

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))

    last = rmse((ca + cb) * f32(0.5))
    accum = rmse((acc[0] + acc[1]) * f32(0.5))
    den_last = rmse(dr.denoise(ca, cb, aov["albedo"], aov["normal_depth"]))
    den_acc = rmse(dr.denoise(acc[0], acc[1], aov["albedo"], aov["normal_depth"]))
    print(f"RMSE last {last:.4f} accumulated {accum:.4f} ({accum / last:.3f}) "
          f"denoised last {den_last:.4f} denoised accumulated {den_acc:.4f} ({den_acc / den_last:.3f})")
    assert accum <= 0.45 * last
    assert den_acc <= 0.7 * den_last
