"""Reference of the variance-guided a-trous denoiser (rt_denoise, DESIGN.md
§3.23) -- TEST INFRASTRUCTURE ONLY.

The numpy restatement of the arithmetic contract: fp32 throughout, every
``fmaf`` of the contract through ``pt_oracle_np.fma32``, ``exp_pt`` through
``pt_oracle_mis_np._exp``, division and square root correctly rounded (numpy's
float32 ``/`` and ``sqrt``).  Whole frames: every array is (H, W, 4) float32.

All comparisons against it are bit for bit (``same`` compares uint32 views).
"""
from __future__ import annotations

import numpy as np

import pt_oracle_mis_np as mnp
from pt_oracle_np import fma32

f32 = np.float32
DEFAULTS = dict(iterations=5, normal_power_log2=7, sigma_luminance=4.0, sigma_depth=1.0, depth_floor=0.01)
ALBEDO_FLOOR = f32(2.0 ** -10)
G3 = [f32(0.25), f32(0.5), f32(0.25)]
B5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]


def shifted(a, dx, dy):
    """``a`` at (x + dx, y + dy) for every pixel (zero outside the frame) and
    the in-frame mask."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    x0, x1 = max(0, -dx), min(W, W - dx)
    y0, y1 = max(0, -dy), min(H, H - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def lum(v):
    return fma32(v[..., 2], f32(0.0722), fma32(v[..., 1], f32(0.7152), v[..., 0] * f32(0.2126)))


def g3(v, hit):
    """3x3 binomial mean of ``v`` over the hit pixels in the frame; 0 at a
    non-hit pixel."""
    s = np.zeros(v.shape, f32)
    sw = np.zeros(v.shape, f32)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            k = G3[j + 1] * G3[i + 1]
            vq, ok = shifted(v, i, j)
            hq, _ = shifted(hit, i, j)
            m = ok & hq
            sw = np.where(m, sw + k, sw)
            s = np.where(m, fma32(k, vq, s), s)
    with np.errstate(all="ignore"):
        return np.where(hit, s * (f32(1.0) / sw), f32(0.0)).astype(f32)


def slope(Z, hit, axis):
    """gx (axis 0) / gy (axis 1): the one-sided depth difference of smaller
    magnitude among the hit neighbours, forward on a tie, 0 without one."""
    d = (1, 0) if axis == 0 else (0, 1)
    zf, okf = shifted(Z, d[0], d[1])
    hf, _ = shifted(hit, d[0], d[1])
    zb, okb = shifted(Z, -d[0], -d[1])
    hb, _ = shifted(hit, -d[0], -d[1])
    pf, pb = okf & hf, okb & hb
    f = zf - Z
    b = Z - zb
    both = np.where(np.abs(f) <= np.abs(b), f, b)
    return np.where(pf & pb, both, np.where(pf, f, np.where(pb, b, f32(0.0)))).astype(f32)


def denoise(color_a, color_b, albedo, normal_depth, iterations=5, normal_power_log2=7, sigma_luminance=4.0,
            sigma_depth=1.0, depth_floor=0.01):
    Ca = np.ascontiguousarray(color_a, f32)
    Cb = np.ascontiguousarray(color_b, f32)
    A = np.ascontiguousarray(albedo, f32)
    ND = np.ascontiguousarray(normal_depth, f32)
    assert Ca.ndim == 3 and Ca.shape[2] == 4 and Ca.shape == Cb.shape == A.shape == ND.shape
    sl, sd, fl = f32(sigma_luminance), f32(sigma_depth), f32(depth_floor)
    hit = A[..., 3] > 0
    N, Z = ND[..., :3], ND[..., 3]

    # prepare
    am = np.maximum(A[..., :3], ALBEDO_FLOOR)
    ia = f32(1.0) / am
    Da = Ca[..., :3] * ia
    Db = Cb[..., :3] * ia
    D = (Da + Db) * f32(0.5)
    hl = (lum(Da) - lum(Db)) * f32(0.5)
    V = g3(hl * hl, hit)
    gx, gy = slope(Z, hit, 0), slope(Z, hit, 1)

    for it in range(iterations):
        s = 1 << it
        L = lum(D)
        gv = g3(V, hit)
        il = f32(1.0) / fma32(sl, np.sqrt(gv), f32(1e-4))
        sw = np.zeros(V.shape, f32)
        sv = np.zeros(V.shape, f32)
        sc = np.zeros(D.shape, f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                k = B5[j + 2] * B5[i + 2]
                Dq, ok = shifted(D, i * s, j * s)
                Vq, _ = shifted(V, i * s, j * s)
                if i == 0 and j == 0:
                    w = np.full(V.shape, k, f32)
                    m = hit
                else:
                    Nq, _ = shifted(N, i * s, j * s)
                    Zq, _ = shifted(Z, i * s, j * s)
                    hq, _ = shifted(hit, i * s, j * s)
                    Lq, _ = shifted(L, i * s, j * s)
                    m = hit & ok & hq
                    dn = fma32(N[..., 2], Nq[..., 2], fma32(N[..., 1], Nq[..., 1], N[..., 0] * Nq[..., 0]))
                    wn = np.maximum(dn, f32(0.0))
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    sp = np.abs(fma32(gx, f32(i * s), gy * f32(j * s)))
                    e = np.abs(Z - Zq) * (f32(1.0) / fma32(sd, sp, fl))
                    e = fma32(np.abs(L - Lq), il, e)
                    w = (k * wn) * mnp._exp(-np.minimum(e, f32(87.0)))
                    w = np.where(m, w, f32(0.0)).astype(f32)  # keeps what is not counted finite
                sw = np.where(m, sw + w, sw)
                sv = np.where(m, fma32(w * w, Vq, sv), sv)
                sc = np.where(m[..., None], fma32(w[..., None], Dq, sc), sc)
        with np.errstate(all="ignore"):
            r = f32(1.0) / sw
            D = np.where(hit[..., None], sc * r[..., None], D).astype(f32)
            V = np.where(hit, sv * (r * r), V).astype(f32)

    out = np.empty_like(Ca)
    out[..., :3] = np.where(hit[..., None], D * am, (Ca[..., :3] + Cb[..., :3]) * f32(0.5))
    out[..., 3] = Ca[..., 3]
    return out


def same(got, want):
    g = np.ascontiguousarray(got, f32)
    return g.shape == want.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def first_difference(got, want):
    bad = (np.ascontiguousarray(got, f32).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(-1)
    idx = np.argwhere(bad)
    if not len(idx):
        return "equal"
    y, x = idx[0]
    return f"{len(idx)} pixels differ, first at y {y}, x {x}: got {got[y, x]}, want {want[y, x]}"
