"""Reference of temporal reprojection (rt_reproject) -- TEST
INFRASTRUCTURE ONLY.

A numpy restatement of the contract's steps 1-6, vectorised over the frame,
built on the numpy restatement of ``pathTrace`` (oracle/pt_oracle_np.py: its
``V``, ``dot`` and ``fma32``) and the camera rays of tests/aov_ref.py
(``camera_rays`` at jitter 0.5, 0.5: the ray of RT_AOV_CENTER).  Every
operation is fp32 and the fma's are the contract's; the comparisons against
it are bit for bit, or by the NaN rule of ``same_or_nan`` on adversarial
buffers.
"""
from __future__ import annotations

import numpy as np

import aov_ref as ar
import pt_oracle_np as onp

f32 = np.float32
DEFAULTS = dict(max_history=32, normal_cos_min=0.9, plane_rel=2.0 ** -7, weight_min=0.0625)


class Camera:
    """The constants of one CameraGPU, as the scene compile makes them."""

    def __init__(self, camera):
        sc = onp.Scene(camera, b"", np.zeros(16, f32).tobytes(), b"")
        self.W, self.H = sc.W, sc.H
        self.pos, self.u, self.v, self.w, self.halfW, self.halfH = sc.pos, sc.u, sc.v, sc.w, sc.halfW, sc.halfH


def _v(a):
    return onp.V(a[..., 0], a[..., 1], a[..., 2])


def _dirs(cam, xs, ys):
    half = np.full(xs.shape, 0.5, f32)
    return ar.camera_rays(cam, xs, ys, half, half)[1]


def reproject(camera, prev_camera, color, history, hit, normal_depth, prev_hit, prev_normal_depth,
              max_history=32, normal_cos_min=0.9, plane_rel=2.0 ** -7, weight_min=0.0625, stats=None):
    """The output planes (a list, one per colour plane).  ``camera`` /
    ``prev_camera``: CameraGPU (prev None: the camera did not move); ``color`` /
    ``history``: lists of (H, W, 4) float32; ``hit`` / ``prev_hit``: (H, W)
    structured (t, id).  ``stats``: a dict that receives the masks ``hit``,
    ``reused``, ``behind`` (zc <= 0 among the hit pixels) and ``off_frame``
    (in front, projected outside the gate) of the frame."""
    cam = Camera(camera)
    prev = cam if prev_camera is None else Camera(prev_camera)
    W, H = cam.W, cam.H
    assert (prev.W, prev.H) == (W, H)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = np.ascontiguousarray(hit["t"]).astype(f32)
    ids = np.ascontiguousarray(hit["id"]).astype(np.int32)
    pt = np.ascontiguousarray(prev_hit["t"]).astype(f32)
    pid = np.ascontiguousarray(prev_hit["id"]).astype(np.int32)
    nd = np.asarray(normal_depth, f32)
    pnd = np.asarray(prev_normal_depth, f32)
    N = _v(nd)
    fW, fH = f32(W), f32(H)
    with np.errstate(all="ignore"):
        is_hit = ids >= 0                                               # step 1
        d = _dirs(cam, xx, yy)                                          # step 2
        X = onp.V(cam.pos.x + d.x * t, cam.pos.y + d.y * t, cam.pos.z + d.z * t)
        q = X - prev.pos                                                # step 3
        zc = -onp.dot(q, prev.w).reshape(H, W)
        a = onp.dot(q, prev.u).reshape(H, W) / zc
        b = onp.dot(q, prev.v).reshape(H, W) / zc
        fx = (((a / prev.halfW) + f32(1.0)) * f32(0.5)) * fW - f32(0.5)
        fy = ((f32(1.0) - (b / prev.halfH)) * f32(0.5)) * fH - f32(0.5)
        r = np.sqrt(onp.dot(q, q).reshape(H, W))
        ndd = onp.dot(N, d).reshape(H, W)                               # step 4
        ndq = onp.dot(N, q).reshape(H, W)
        side = ((ndd < 0) & (ndq < 0)) | ((ndd >= 0) & (ndq >= 0))
        front = zc > 0
        inside = (fx >= f32(-1.0)) & (fx < fW) & (fy >= f32(-1.0)) & (fy < fH)
        gate = is_hit & side & front & inside
        fxg, fyg = np.where(gate, fx, f32(0.0)), np.where(gate, fy, f32(0.0))
        flx, fly = np.floor(fxg), np.floor(fyg)                         # step 5
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = fxg - flx, fyg - fly
        lim = f32(plane_rel) * r
        n_planes = len(color)
        sw = np.zeros((H, W), f32)
        c = [[np.zeros((H, W), f32) for _ in range(3)] for _ in range(n_planes)]
        l = [np.zeros((H, W), f32) for _ in range(n_planes)]
        for j in (0, 1):
            for i in (0, 1):
                bw = (wx if i else f32(1.0) - wx) * (wy if j else f32(1.0) - wy)
                xt, yt = x0 + i, y0 + j
                ok = gate & (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
                xc, yc = np.where(ok, xt, 0), np.where(ok, yt, 0)
                ok &= pid[yc, xc] == ids
                Nt = _v(pnd[yc, xc])
                ok &= onp.dot(N, Nt).reshape(H, W) >= f32(normal_cos_min)
                dp = _dirs(prev, xc, yc)
                tt = pt[yc, xc]
                Xp = onp.V(prev.pos.x + dp.x * tt, prev.pos.y + dp.y * tt, prev.pos.z + dp.z * tt)
                ok &= np.abs(onp.dot(N, Xp - X).reshape(H, W)) <= lim
                sw = np.where(ok, sw + bw, sw)
                for k in range(n_planes):
                    h = np.asarray(history[k], f32)[yc, xc]
                    for ch in range(3):
                        c[k][ch] = np.where(ok, onp.fma32(bw, h[..., ch], c[k][ch]).reshape(H, W), c[k][ch])
                    l[k] = np.where(ok, onp.fma32(bw, h[..., 3], l[k]).reshape(H, W), l[k])
        reuse = gate & (sw >= f32(weight_min))                          # step 6
        rw = f32(1.0) / np.where(reuse, sw, f32(1.0))
        mh = f32(max_history)
        outs = []
        for k in range(n_planes):
            cur = np.asarray(color[k], f32)
            m1 = l[k] * rw + f32(1.0)
            n = np.where(m1 < mh, m1, mh)
            al = f32(1.0) / n
            out = np.empty((H, W, 4), f32)
            for ch in range(3):
                h = c[k][ch] * rw
                out[..., ch] = np.where(reuse, onp.fma32(al, cur[..., ch] - h, h).reshape(H, W), cur[..., ch])
            out[..., 3] = np.where(reuse, n, f32(1.0))
            outs.append(out)
    if stats is not None:
        stats.update(hit=is_hit, reused=reuse, behind=is_hit & ~front, off_frame=is_hit & front & ~inside)
    return outs


def same(got, want):
    g = np.ascontiguousarray(got, f32)
    return g.shape == want.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def same_or_nan(got, want):
    """Equal bits wherever the reference is not NaN, NaN where it is NaN."""
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(w)
    return g.shape == w.shape and bool(np.all(np.isnan(g[nan]))) and \
        np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def first_difference(got, want):
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    bad = ((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))).any(-1)
    idx = np.argwhere(bad)
    if not len(idx):
        return "equal"
    y, x = idx[0]
    return f"{len(idx)} pixels differ, first at y {y}, x {x}: got {g[y, x]}, want {w[y, x]}"
