"""References of adaptive sampling (rt_render_counts, rt_plan_samples; DESIGN.md
§3.27) -- TEST INFRASTRUCTURE ONLY.

``SampleFrames`` is the reference for any map of per-pixel totals: the oracle
renders one frame per sample index at ``spp = 1`` (one sample's radiance
exactly), and ``image`` adds them in ascending index, in float32, into the
pixels whose total is past that index, then divides by ``float32(total)`` (0
where the total is 0).  That is the oracle's own in-order sum, so pixel p
equals the oracle's render at ``spp = total_p``.  The frames are rendered once
and shared by every map of one scene.

``plan`` restates the planner's contract in numpy: fp32 up to the weight q
(``denoise_ref.lum`` with its ``fma32``), integers from there.

All comparisons are bit for bit (uint32 views).
"""
from __future__ import annotations

import numpy as np

import oracle_lib
from denoise_ref import lum, shifted

f32 = np.float32


class SampleFrames:
    """The oracle's single-sample frames of one scene, seeds and bounce count
    from ``sample_base`` on, for the rows of one partition."""

    def __init__(self, scene, seeds, bounces, sample_base=0, row_start=0, row_step=1, row_count=0):
        self.scene, self.seeds, self.bounces, self.base = scene, seeds, bounces, sample_base
        self.rows = dict(row_start=row_start, row_step=row_step, row_count=row_count)
        self.frames = []

    def frame(self, n):
        while len(self.frames) <= n:
            k = len(self.frames)
            f = oracle_lib.render(self.scene, self.seeds, 1, self.bounces, sample_base=self.base + k, **self.rows)
            self.frames.append(np.ascontiguousarray(f[..., :3]))
        return self.frames[n]

    def sums(self, totals):
        """(rows, W, 3) float32: each pixel's in-order sum of its first ``totals`` samples."""
        t = np.asarray(totals, np.uint32)
        s = np.zeros(t.shape + (3,), f32)
        for n in range(int(t.max(initial=0))):
            s = np.where((t > n)[..., None], s + self.frame(n), s).astype(f32)
        return s

    def image(self, totals):
        """(rows, W, 4) float32: sum / float32(total), alpha 1; colour +0 where the total is 0."""
        t = np.asarray(totals, np.uint32)
        s = self.sums(t)
        out = np.ones(t.shape + (4,), f32)
        with np.errstate(all="ignore"):
            out[..., :3] = np.where((t > 0)[..., None], s / t.astype(f32)[..., None], f32(0.0))
        return out


def weights(first, all, relative=False, luminance_floor=0.01):
    """Steps 1-4 of the contract: q per pixel, uint32 in [1, 2^24 + 1]."""
    F, A = np.ascontiguousarray(first, f32), np.ascontiguousarray(all, f32)
    with np.errstate(all="ignore"):
        la = lum(A)
        el = np.abs(la - lum(F))
        r = (el / (la + f32(luminance_floor))).astype(f32) if relative else el
        r = np.where(r >= 0, r, f32(0.0)).astype(f32)  # NaN: 0
        return (np.minimum(r * f32(65536.0), f32(16777216.0)).astype(np.uint32) + np.uint32(1)).astype(np.uint32)


def plan(first, all, budget, count_min=0, count_max=1 << 24, radius=1, relative=False, luminance_floor=0.01):
    """(counts uint32 (rows, W), stats dict): the whole contract."""
    q = weights(first, all, relative, luminance_floor)
    m = q.copy()
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            m = np.maximum(m, shifted(q, i, j)[0])  # outside the tile: 0 < every q
    Q = int(m.astype(np.uint64).sum())
    share = np.uint64(count_min) + (np.uint64(budget) * m.astype(np.uint64)) // np.uint64(Q)
    capped = share > np.uint64(count_max)
    counts = np.where(capped, np.uint64(count_max), share).astype(np.uint32)
    stats = dict(weight_sum=Q, samples=int(counts.astype(np.uint64).sum()), count_max_seen=int(counts.max()),
                 at_cap=int(capped.sum()))
    return counts, stats


def same_words(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize and np.array_equal(
        g.view(np.uint32) if g.dtype.itemsize == 4 else g, w.view(np.uint32) if w.dtype.itemsize == 4 else w)


def first_difference(got, want):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(np.shape(want))
    w = np.ascontiguousarray(want).view(np.uint32)
    bad = g != w
    if bad.ndim == 3:
        bad = bad.any(-1)
    idx = np.argwhere(bad)
    if not len(idx):
        return "equal"
    y, x = idx[0]
    return f"{len(idx)} pixels differ, first at y {y}, x {x}: got {np.asarray(got)[y, x]}, want {np.asarray(want)[y, x]}"
