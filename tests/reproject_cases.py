"""Inputs of tests/test_reproject.py and tests/test_gpu_reproject.py: the pose
pairs of the reprojection contract with the band each one's
reuse share must stay in, the small frames, random colour / history planes and
the deterministic adversarial generator that tools/reproject_host_check.cpp
states in C++ (same seed rule, same tables, same draw order)."""
import functools

import numpy as np

import aov_ref as ar
import pose_scenes as ps
from gpuraytracer_amd import Scene

f32 = np.float32
W, H = ps.W, ps.H
SHIFT = (0.1, 0.05, 0.0)
SMALL = [(1, 1), (2, 1), (17, 16), (33, 17), (70, 45)]   # W >= H: the integer aspect ratio


@functools.lru_cache(maxsize=None)
def base_scene(kind, w=W, h=H):
    return Scene.cornell_box(w, h) if kind == "cornell" else Scene.random_spheres(w, h, 40, seed=42)


def shifted(scene):
    c = scene.camera.position
    return ps.posed(scene, eye=(c.x + SHIFT[0], c.y + SHIFT[1], c.z + SHIFT[2]))


def _pose(kind, name, w=W, h=H):
    s = base_scene(kind, w, h)
    return shifted(s) if name == "shifted" else ps.view(s, name)


# name: (scene, previous pose, current pose, band of the reused share of the hit pixels)
PAIRS = {
    "same": ("cornell", "cornell", "cornell", (0.99, 1.0)),
    "shift": ("cornell", "cornell", "shifted", (0.9, 1.0)),
    "shift_spheres": ("spheres", "cornell", "shifted", (0.9, 1.0)),
    "to_diag_roll": ("cornell", "cornell", "diag_roll", (0.3, 0.8)),
    "wide_to_cornell": ("cornell", "wide", "cornell", (0.5, 0.9)),
    "down_to_up": ("cornell", "straight_down", "up_from_floor", (0.02, 0.3)),
    "into_tall_box": ("cornell", "cornell", "inside_tall_box", (0.0, 0.0)),
    "away_to_cornell": ("cornell", "away", "cornell", (0.0, 0.0)),
    "to_away": ("cornell", "cornell", "away", None),   # no hit pixel: out == (cur.rgb, 1) everywhere
}


def pair_scenes(name, w=W, h=H):
    kind, prev, cur, _ = PAIRS[name]
    return _pose(kind, prev, w, h), _pose(kind, cur, w, h)


@functools.lru_cache(maxsize=None)
def _centre(kind, pose, w, h):
    b = ar.buffers(ar.np_scene(_pose(kind, pose, w, h)), None, 1, center=True)
    return b["first_hit"], b["normal_depth"]


def centre_buffers(name, w=W, h=H):
    """(hit, normal_depth, prev_hit, prev_normal_depth) of a pair from the numpy AOV reference."""
    kind, prev, cur, _ = PAIRS[name]
    return _centre(kind, cur, w, h) + _centre(kind, prev, w, h)


def planes(seed, w=W, h=H):
    """Two colour and two history planes: rgb in [0, 2), colour alpha 1,
    history lengths 1..40 (some above the default cap of 32)."""
    rng = np.random.default_rng(seed)
    color = [rng.uniform(0.0, 2.0, (h, w, 4)).astype(f32) for _ in range(2)]
    history = [rng.uniform(0.0, 2.0, (h, w, 4)).astype(f32) for _ in range(2)]
    for c in color:
        c[..., 3] = 1.0
    for hs in history:
        hs[..., 3] = rng.integers(1, 41, (h, w)).astype(f32)
    return color, history


# ---- the adversarial generator (tools/reproject_host_check.cpp) -----------------
_M = (1 << 64) - 1
T_BITS = [0x40400000, 0x41100000, 0x7FC00000, 0x7F800000, 0xFF800000, 0x7149F2CA, 0xC0A00000, 0x00000000, 0x00000001]
ID_BITS = [0, 7, 35, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000]
N_BITS = [0x00000000, 0x3F800000, 0xBF800000, 0x3F19999A, 0x7FC00000, 0x7149F2CA]
RGB_BITS = [0x3E800000, 0x3FC00000, 0x3F000000, 0x7FC00000, 0x7F800000, 0xFF800000]
ALPHA_BITS = [0x3F800000, 0x40E00000, 0x42000000, 0x7FC00000, 0x7F800000, 0xFF800000, 0xC0400000, 0x00000000,
              0x7149F2CA]
PLAUSIBLE = [2, 3, 4, 3, 3]   # the leading finite, tame entries of the five tables


def adversarial_seed(w, h):
    return 0x5EED0000 + w * 1000 + h


def adversarial(w, h, plausible=False):
    """dict(hit, normal_depth, prev_hit, prev_normal_depth, color, history):
    per pixel, row-major, the draws (t, id), (N.xyz, w) of this frame, the same
    of the previous frame, color[0], color[1], history[0], history[1]; a draw is
    table[(splitmix64() >> 33) % len]."""
    state = [adversarial_seed(w, h)]

    def pick(n):
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & _M
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
        return ((z ^ (z >> 31)) >> 33) % n

    tabs = [T_BITS, ID_BITS, N_BITS, RGB_BITS, ALPHA_BITS]

    def draw(which):
        tab = tabs[which]
        return tab[pick(PLAUSIBLE[which] if plausible else len(tab))]

    n = w * h
    hits = [np.empty((n, 2), np.uint32) for _ in range(2)]
    nds = [np.empty((n, 4), np.uint32) for _ in range(2)]
    cols = [np.empty((n, 4), np.uint32) for _ in range(4)]
    for p in range(n):
        for k in range(2):
            hits[k][p] = (draw(0), draw(1))
            nds[k][p] = (draw(2), draw(2), draw(2), draw(0))
        for b in range(4):
            cols[b][p] = (draw(3), draw(3), draw(3), draw(4))
    as_hit = lambda a: np.ascontiguousarray(a).view(ar.HIT_DTYPE).reshape(h, w)  # noqa: E731
    as_f = lambda a: np.ascontiguousarray(a).view(f32).reshape(h, w, 4)          # noqa: E731
    return dict(hit=as_hit(hits[0]), normal_depth=as_f(nds[0]), prev_hit=as_hit(hits[1]),
                prev_normal_depth=as_f(nds[1]), color=[as_f(cols[0]), as_f(cols[1])],
                history=[as_f(cols[2]), as_f(cols[3])])


# the parameter sets of the adversarial runs (the C++ program's def, loose, tight)
ADVERSARIAL_PARAMS = {
    "default": {},
    "loose": dict(normal_cos_min=-1.0, plane_rel=1e30, weight_min=2.0 ** -20, max_history=65536),
    "tight": dict(weight_min=1.0, max_history=1),
}
