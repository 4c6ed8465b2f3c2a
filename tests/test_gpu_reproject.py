"""GPU: temporal reprojection (Renderer.reproject / render_temporal,
rt_reproject) against its numpy restatement tests/reproject_ref.py, bit for
bit on uint32 views.

The pose pairs and small frames of tests/test_reproject.py with the feature
buffers of the device's own render_aov(center=True), both plane counts, the
adversarial buffers under the NaN rule, the host / device / stream paths with
aliasing outputs, a scene update between the frames, the render_temporal
pipeline against the same calls made by hand, the error statuses and the
launch report."""
import ctypes

import numpy as np
import pytest

import denoise_ref as dr
import pose_scenes as ps
import reproject_cases as rc
import reproject_ref as rr
from gpuraytracer_amd import RenderParams, Renderer, RtError, _native, lib

pytestmark = pytest.mark.gpu
f32 = np.float32


def centre(r):
    b = r.render_aov(center=True, albedo=False)
    return b["first_hit"], b["normal_depth"]


def check(got, cur, prev, color, history, bufs, what, rule=rr.same, **kw):
    want = rr.reproject(cur, prev, color, history, *bufs, **kw)
    assert len(got) == len(want)
    for k in range(len(want)):
        assert rule(np.asarray(got[k]), want[k]), f"{what} plane {k} {kw}: " + rr.first_difference(got[k], want[k])
    return want


def launch_is(r, planes, w, h):
    L = r.last_launch()
    assert L["kernel"] == f"rt::reproject_kernel<{planes}>", L
    assert L["grid_x"] == -(-w // 16) and L["grid_y"] == -(-h // 16) and L["block_threads"] == 256, L
    assert L["lds_bytes"] == 0 and L["lanes_per_pixel"] == 1, L
    assert r.last_kernel_ms() > 0


# ---- parity ----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.PAIRS))
def test_pose_pairs(name):
    prev, cur = rc.pair_scenes(name)
    with Renderer(prev) as r:
        phit, pnd = centre(r)
    color, history = rc.planes(21)
    with Renderer(cur) as r:
        hit, nd = centre(r)
        bufs = (hit, nd, phit, pnd)
        two = r.reproject(color, history, *bufs, prev_camera=prev.camera)
        launch_is(r, 2, cur.width, cur.height)
        check(two, cur.camera, prev.camera, color, history, bufs, name)
        one = r.reproject(color[0], history[0], *bufs, prev_camera=prev.camera)
        launch_is(r, 1, cur.width, cur.height)
        assert len(one) == 1 and rr.same(one[0], two[0])


@pytest.mark.parametrize("w,h", rc.SMALL)
def test_small_frames(w, h):
    prev, cur = rc.pair_scenes("shift", w, h)
    with Renderer(prev) as r:
        phit, pnd = centre(r)
    color, history = rc.planes(w * 100 + h, w, h)
    with Renderer(cur) as r:
        bufs = centre(r) + (phit, pnd)
        for planes in (2, 1):
            got = r.reproject(color[:planes], history[:planes], *bufs, prev_camera=prev.camera)
            launch_is(r, planes, w, h)
            check(got, cur.camera, prev.camera, color[:planes], history[:planes], bufs, f"{w}x{h}")


@pytest.mark.parametrize("plausible", [False, True])
def test_adversarial_buffers(plausible):
    A = rc.adversarial(rc.W, rc.H, plausible)
    scene = rc.base_scene("cornell")
    bufs = (A["hit"], A["normal_depth"], A["prev_hit"], A["prev_normal_depth"])
    with Renderer(scene) as r:
        for params, kw in rc.ADVERSARIAL_PARAMS.items():
            for prev in (None, rc.shifted(scene).camera, ps.view(scene, "behind_left").camera):
                for planes in (2, 1):
                    got = r.reproject(A["color"][:planes], A["history"][:planes], *bufs, prev_camera=prev, **kw)
                    check(got, scene.camera, prev, A["color"][:planes], A["history"][:planes], bufs,
                          f"adversarial {params}", rule=rr.same_or_nan, **kw)


# ---- paths -----------------------------------------------------------------------

def dev_hit(h):
    import torch
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int32).reshape(h.shape + (2,))).cuda()


def test_host_device_and_stream_paths_and_aliasing():
    import torch
    prev, cur = rc.pair_scenes("shift")
    with Renderer(prev) as r:
        phit, pnd = centre(r)
    color, history = rc.planes(31)
    with Renderer(cur) as r:
        hit, nd = centre(r)
        bufs = (hit, nd, phit, pnd)
        want = check(r.reproject(color, history, *bufs, prev_camera=prev.camera), cur.camera, prev.camera, color,
                     history, bufs, "host")
        # host, out aliasing color
        alias = [c.copy() for c in color]
        got = r.reproject(alias, history, *bufs, prev_camera=prev.camera, out=alias)
        assert got[0] is alias[0] and all(rr.same(alias[k], want[k]) for k in range(2))
        # device tensors on the current stream
        dcol = [torch.from_numpy(c).cuda() for c in color]
        dhis = [torch.from_numpy(c).cuda() for c in history]
        dbuf = (dev_hit(hit), torch.from_numpy(nd).cuda(), dev_hit(phit), torch.from_numpy(pnd).cuda())
        got = r.reproject(dcol, dhis, *dbuf, prev_camera=prev.camera)
        assert all(rr.same(got[k].cpu().numpy(), want[k]) for k in range(2))
        assert all(rr.same(dcol[k].cpu().numpy(), color[k]) for k in range(2))   # inputs untouched
        # a non-null stream, out aliasing color, one plane and two
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        acol = [c.clone() for c in dcol]
        torch.cuda.synchronize()
        got = r.reproject(acol, dhis, *dbuf, prev_camera=prev.camera, out=acol, stream=s)
        one = r.reproject(dcol[1], dhis[1], *dbuf, prev_camera=prev.camera, stream=s)
        s.synchronize()
        assert got[0] is acol[0] and all(rr.same(acol[k].cpu().numpy(), want[k]) for k in range(2))
        assert rr.same(one[0].cpu().numpy(), want[1])
        launch_is(r, 1, cur.width, cur.height)
        # tensors of another shape or type are refused before the call
        with pytest.raises(ValueError):
            r.reproject(dcol, dhis, dbuf[0].float(), *dbuf[1:], prev_camera=prev.camera)
        with pytest.raises(ValueError):
            r.reproject(dcol, dhis[:1], *dbuf, prev_camera=prev.camera)


# ---- scene updates ---------------------------------------------------------------

def test_after_update_scene_the_context_camera_is_the_new_pose():
    prev, cur = rc.pair_scenes("to_diag_roll")
    color, history = rc.planes(41)
    with Renderer(prev) as r:
        phit, pnd = centre(r)
        r.update_scene(cur)
        bufs = centre(r) + (phit, pnd)
        got = r.reproject(color, history, *bufs, prev_camera=prev.camera)
        want = check(got, cur.camera, prev.camera, color, history, bufs, "updated")
        share = np.mean(want[0][..., 3][bufs[0]["id"] >= 0] > 1)
        assert 0.3 <= share <= 0.8, share
        # without prev_camera the old frame is taken as seen from the new pose: another result
        still = r.reproject(color, history, *bufs)
        check(still, cur.camera, None, color, history, bufs, "updated, unmoved")
        assert not rr.same(still[0], got[0])


# ---- pipeline --------------------------------------------------------------------

def test_render_temporal_equals_the_calls_made_by_hand():
    base = rc.base_scene("cornell")
    poses = [ps.posed(base, eye=(9 * np.sin(a), 0.3 * np.sin(2 * a), 9 * np.cos(a)), look_at=(0, 0, 0))
             for a in (0.0, 0.05, 0.1)]
    p = RenderParams(spp=2, bounces=3, sample_base=6)
    with Renderer(poses[0]) as r, Renderer(poses[0]) as q:
        state, hand = None, None
        for f, s in enumerate(poses):
            if f:
                r.update_scene(s)
                q.update_scene(s)
            img, state = r.render_temporal(p, state)
            assert state["frame"] == f
            # by hand, through the host paths of a second context
            ca = q.render(RenderParams(spp=1, bounces=3, sample_base=6 + 2 * f))
            cb = q.render(RenderParams(spp=1, bounces=3, sample_base=6 + 2 * f + 1))
            hit, nd = centre(q)
            acc = [ca, cb] if hand is None else q.reproject([ca, cb], hand["acc"], hit, nd, hand["hit"], hand["nd"],
                                                            prev_camera=hand["camera"])
            aov = q.render_aov(spp=2, sample_base=6 + 2 * f, first_hit=False)
            want = q.denoise(acc[0], acc[1], aov["albedo"], aov["normal_depth"])
            assert all(rr.same(state["out"][k].cpu().numpy(), acc[k]) for k in range(2)), f
            assert rr.same(img.cpu().numpy(), want), f
            if f:
                assert np.mean(acc[0][..., 3] > 1) > 0.5   # history is reused
                ref = rr.reproject(s.camera, hand["camera"], [ca, cb], hand["acc"], hit, nd, hand["hit"], hand["nd"])
                assert rr.same(acc[0], ref[0]) and rr.same(acc[1], ref[1])
                assert dr.same(want, dr.denoise(acc[0], acc[1], aov["albedo"], aov["normal_depth"]))
            hand = dict(acc=acc, hit=hit, nd=nd, camera=s.camera)
        planes, _ = r.render_temporal(p, state, denoise=False)   # the accumulated planes themselves
        assert len(planes) == 2 and float(planes[0][..., 3].max()) == 4.0
        for bad in (RenderParams(spp=3), RenderParams(spp=2, row_step=2), RenderParams(spp=2, fp16=True)):
            with pytest.raises(ValueError):
                r.render_temporal(bad)


# ---- errors ----------------------------------------------------------------------

def test_error_statuses_name_the_field():
    scene = rc.base_scene("cornell")
    color, history = rc.planes(51)
    with Renderer(scene) as r:
        hit, nd = centre(r)
        ok = dict(color=color, history=history, hit=hit, normal_depth=nd, prev_hit=hit, prev_normal_depth=nd)
        r.reproject(**ok)
        for kw, what in ((dict(max_history=0), "max_history"), (dict(max_history=65537), "max_history"),
                         (dict(normal_cos_min=float("nan")), "normal_cos_min"), (dict(plane_rel=-1.0), "plane_rel"),
                         (dict(weight_min=0.0), "weight_min"), (dict(weight_min=float("nan")), "weight_min")):
            with pytest.raises(RtError) as e:
                r.reproject(**ok, **kw)
            assert e.value.status == 1 and what in str(e.value) and "rt_reproject: " in str(e.value)
        wrong = ps.posed(rc.base_scene("cornell", 70, 45)).camera
        for cam, what in ((wrong, "prev_camera: resolution"),
                          (ps.posed(scene, direction=(0, 0, 0)).camera, "prev_camera: camera direction")):
            with pytest.raises(RtError) as e:
                r.reproject(**ok, prev_camera=cam)
            assert e.value.status == 1 and what in str(e.value)
        # the raw entry points: null pointers, a mixed plane 1, flags, reserved
        p, b = _native.ReprojectParams(), _native.ReprojectBuffers()
        lib.rt_reproject_params_default(ctypes.byref(p))
        out = [np.empty_like(color[0]) for _ in range(2)]

        def fill():
            for k in range(2):
                b.color[k], b.history[k], b.out[k] = color[k].ctypes.data, history[k].ctypes.data, out[k].ctypes.data
            b.hit = b.prev_hit = hit.ctypes.data
            b.normal_depth = b.prev_normal_depth = nd.ctypes.data

        def status(pp=p, bb=b):
            st = lib.rt_reproject(r._ctx, ctypes.byref(pp) if pp is not None else None, None,
                                  ctypes.byref(bb) if bb is not None else None)
            return st, lib.rt_last_error(r._ctx).decode()

        fill()
        assert status()[0] == 0
        assert status(pp=None) == (1, "rt_reproject: params is null")
        assert status(bb=None) == (1, "rt_reproject: buffers is null")
        for name in ("hit", "normal_depth", "prev_hit", "prev_normal_depth"):
            setattr(b, name, None)
            assert status() == (1, f"rt_reproject: {name} is null")
            fill()
        for name in ("color", "history", "out"):
            getattr(b, name)[0] = None
            assert status() == (1, f"rt_reproject: {name}[0] is null")
            fill()
            getattr(b, name)[1] = None
            assert status()[0] == 1 and "color[1], history[1] and out[1]" in status()[1]
            fill()
        p.flags = 0x2
        assert status() == (1, "rt_reproject: unknown flag bits")
        p.flags = 0
        p.reserved[1] = 5
        assert status() == (1, "rt_reproject: reserved must be 0")
        p.reserved[1] = 0
        assert status()[0] == 0
        assert lib.rt_reproject_async(r._ctx, None, None, ctypes.byref(b), None) == 1
