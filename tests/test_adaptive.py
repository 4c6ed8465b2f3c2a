"""CPU: the sample planner's host function (rt_plan_samples_host) against its
numpy restatement (tests/adaptive_ref.py), bit for bit; its argument checks;
and the quality of the whole scheme, simulated with the oracle: a pilot, the
plan and the per-pixel in-order sums against uniform sampling of the same mean
count.  No GPU."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import oracle_lib
from gpuraytracer_amd import PlanParams, PlanStats, RT_PLAN_RELATIVE, Scene, lib, plan_samples_host

f32 = np.float32


def images(rows, W, seed, special=False):
    rng = np.random.default_rng(seed)
    a = rng.random((rows, W, 4), dtype=f32) * f32(2.0)
    f = (a + rng.normal(0.0, 0.05, (rows, W, 4)).astype(f32)).astype(f32)
    if special:  # NaN, +-inf, -0 and huge values, in either image and any channel
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38, -3e38, 1e-40], f32)
        for img in (f, a):
            k = rng.integers(0, rows * W * 4, size=max(4, rows * W // 3))
            img.reshape(-1)[k] = vals[rng.integers(0, len(vals), size=k.size)]
    return f, a


def check(f, a, **kw):
    got, gs = plan_samples_host(f, a, return_stats=True, **kw)
    want, ws = ar.plan(f, a, **kw)
    assert got.dtype == np.uint32 and np.array_equal(got, want), ar.first_difference(got, want)
    assert gs == ws, (gs, ws)
    pixels = got.size
    assert gs["samples"] == int(got.astype(np.uint64).sum()) <= pixels * kw.get("count_min", 0) + kw["budget"]
    assert got.max() <= kw.get("count_max", 1 << 24) and got.min() >= kw.get("count_min", 0)
    return got, gs


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("special", [False, True])
def test_host_plan_equals_numpy(relative, radius, special):
    f, a = images(21, 37, 7 + radius, special)
    check(f, a, budget=8 * 21 * 37, radius=radius, relative=relative, count_max=64)
    check(f, a, budget=100_000, radius=radius, relative=relative, count_min=3, count_max=4000, luminance_floor=0.5)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (16, 16), (17, 33)])
def test_small_and_thin_tiles(shape):
    f, a = images(*shape, seed=3, special=True)
    for radius in (0, 1, 2):
        for relative in (False, True):
            check(f, a, budget=1000, radius=radius, relative=relative)
            check(f, a, budget=(1 << 38) - 1, radius=radius, relative=relative)  # the share past 2^32 on 1 x 1


def test_budget_extremes_with_every_weight_at_its_ceiling():
    """q = 2^24 + 1 everywhere: budget * m is the largest 64-bit product."""
    a = np.full((5, 7, 4), 1e30, f32)
    f = np.zeros_like(a)
    assert (ar.weights(f, a) == (1 << 24) + 1).all()
    got, st = check(f, a, budget=(1 << 38) - 1)
    assert (got == 1 << 24).all() and st["at_cap"] == 35  # the share, (2^38 - 1) / 35, is past the default cap
    got, st = check(f, a, budget=35 * 1000 + 17)
    assert (got == 1000).all() and st["at_cap"] == 0 and st["weight_sum"] == 35 * ((1 << 24) + 1)
    got, st = check(f, a, budget=(1 << 38) - 1, count_max=1000)
    assert (got == 1000).all() and st["at_cap"] == 35 and st["count_max_seen"] == 1000
    got, st = check(f, a, budget=0, count_min=2)
    assert (got == 2).all() and st["samples"] == 70
    # equal weights share the budget equally, rounded down
    got, _ = check(np.ones((4, 4, 4), f32), np.ones((4, 4, 4), f32), budget=100)
    assert (got == 6).all()


def test_count_min_equals_count_max():
    f, a = images(8, 8, 5)
    got, st = check(f, a, budget=10_000, count_min=7, count_max=7)
    assert (got == 7).all() and st["samples"] == 7 * 64
    got, st = check(f, a, budget=0, count_min=7, count_max=7)
    assert (got == 7).all() and st["at_cap"] == 0  # no share was cut


def test_dilation_spreads_the_largest_weight():
    a = np.zeros((9, 9, 4), f32)
    f = np.zeros_like(a)
    a[4, 4, :3] = 1.0
    for radius in (0, 1, 2):
        got, _ = check(f, a, budget=10_000, radius=radius)
        hot = got > got.min()
        assert hot.sum() == (2 * radius + 1) ** 2 and hot[4 - radius:5 + radius, 4 - radius:5 + radius].all()


def raw_plan(width, p, n):
    f = np.zeros((n, 4), f32)
    c = np.zeros(n, np.uint32)
    st = PlanStats()
    return lib.rt_plan_samples_host(width, ctypes.byref(p), f.ctypes.data_as(ctypes.c_void_p),
                                    f.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(st))


def default_params(rows=2):
    p = PlanParams()
    lib.rt_plan_params_default(ctypes.byref(p))
    p.rows = rows
    return p


def test_defaults():
    p = default_params(0)
    assert (p.budget, p.count_min, p.count_max, p.radius, p.rows, p.flags) == (0, 0, 1 << 24, 1, 0, 0)
    assert p.luminance_floor == f32(0.01) and tuple(p.reserved) == (0, 0)
    assert raw_plan(3, default_params(), 6) == 0


@pytest.mark.parametrize("field,value", [
    ("count_min", (1 << 24) + 1),          # > count_max
    ("count_max", (1 << 24) + 1),
    ("budget", 1 << 38),
    ("radius", 3),
    ("flags", RT_PLAN_RELATIVE | 0x4000),  # an unknown bit
    ("flags", 0x1),                        # RT_OUT_DEVICE: not on the host
    ("reserved0", 1),
    ("reserved1", 1),
    ("rows", 0),
])
def test_invalid_arguments(field, value):
    p = default_params()
    if field.startswith("reserved"):
        p.reserved[int(field[-1])] = value
    else:
        setattr(p, field, value)
    assert raw_plan(3, p, 6) == 1, field  # RT_ERR_INVALID_ARG
    assert lib.rt_last_error(None)


@pytest.mark.parametrize("floor", [0.0, -1.0, float("nan")])
def test_relative_mode_needs_a_positive_floor(floor):
    p = default_params()
    p.luminance_floor = floor
    assert raw_plan(3, p, 6) == 0  # absolute mode does not read it
    p.flags = RT_PLAN_RELATIVE
    assert raw_plan(3, p, 6) == 1
    p.count_min, p.count_max = 5, 4
    assert raw_plan(3, default_params(), 6) == 0 and raw_plan(0, default_params(), 6) == 1


def test_null_pointers():
    p = default_params()
    c = np.zeros(6, np.uint32)
    assert lib.rt_plan_samples_host(3, None, c.ctypes.data, c.ctypes.data, c.ctypes.data, None) == 1
    assert lib.rt_plan_samples_host(3, ctypes.byref(p), None, c.ctypes.data, c.ctypes.data, None) == 1
    assert lib.rt_plan_samples(None, ctypes.byref(p), None, None, None, None) == 1
    assert lib.rt_render_counts(None, None, None, None, None) == 1


def rmse(img, ref):
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_adaptive_beats_uniform_sampling(k):
    """Cornell 96 x 72, 3 bounces, against 2048 spp at sample_base 1000: a 4 + 4
    pilot, budget 8 samples per pixel, radius 1, absolute mode, count_max 64,
    with the shipped planner and the oracle's in-order sums.  The comparator is
    uniform sampling at round(mean total) spp.  Measured RMSE ratios for
    k = 1, 2, 3: 0.778, 0.761, 0.790 (mean totals 15.53, 15.51, 15.54; no
    share was cut by the cap)."""
    W, H = 96, 72
    scene = Scene.cornell_box(W, H)
    seeds = oracle_lib.seeds(W, H, key=0x5EED00000000 + 7919 * k)
    ref = oracle_lib.render(scene, seeds, 2048, 3, sample_base=1000)
    first = oracle_lib.render(scene, seeds, 4, 3)
    both = oracle_lib.render(scene, seeds, 8, 3)
    counts, stats = plan_samples_host(first, both, budget=8 * W * H, radius=1, count_max=64, return_stats=True)
    totals = counts + np.uint32(8)
    frames = ar.SampleFrames(scene, seeds, 3)
    assert ar.same_words(frames.image(np.full((H, W), 8, np.uint32)), both)  # the reference is the oracle's sum
    adaptive = frames.image(totals)
    mean = float(totals.mean())
    uniform = oracle_lib.render(scene, seeds, int(round(mean)), 3)
    ratio = rmse(adaptive, ref) / rmse(uniform, ref)
    print(f"key {k}: mean total {mean:.2f}, uniform spp {int(round(mean))}, at_cap {stats['at_cap']}, "
          f"RMSE ratio {ratio:.3f}")
    assert mean <= 16.0
    assert ratio <= 0.9, ratio
