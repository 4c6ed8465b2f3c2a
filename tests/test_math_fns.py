"""CPU: the host side of rt_debug_math_values / rt_debug_math_sums (DESIGN.md
§3.24) -- the x86 compile of the scalar functions the kernels share with the
host -- on the edge inputs of tests/math_fn_domains.py plus a fixed stride
through every domain: bit for bit against the restatements the project
already has, within a measured error of float64 numpy, and the two checksums
against their definition.  tests/test_gpu_math_fns.py then holds the gfx950
compile to this host side over every function's whole domain."""
import ctypes

import numpy as np
import pytest

import gpuraytracer_amd as g
import math_fn_domains as dom
import oracle_lib
import pt_oracle_mis_np
import pt_oracle_np
from gpuraytracer_amd import _native

f32 = np.float32
NAN32, NAN16 = 0x7FC00000, 0x7E00


@pytest.fixture(scope="module")
def inputs():
    """fn -> (input patterns, host result patterns): edges + stride, computed once."""
    out = {}
    for fn in dom.SCALAR_FNS:
        x = np.unique(np.concatenate([dom.edge_inputs(fn), dom.stride_inputs(fn)]))
        assert x.size >= 1 << 16
        got = g.math_values(fn, x)
        x.setflags(write=False)
        got.setflags(write=False)
        out[fn] = (x, got)
    return out


def canon32(a):
    a = np.asarray(a, f32)
    return np.where(np.isnan(a), np.uint32(NAN32), a.view(np.uint32)).astype(np.uint32)


def canon16(h):
    h = np.asarray(h, np.uint16).astype(np.uint32)
    return np.where((h & 0x7FFF) > 0x7C00, np.uint32(NAN16), h).astype(np.uint32)


def restated(fn, x):
    """The project's numpy / oracle restatement of fn on the patterns x."""
    v = x.view(f32)
    with np.errstate(all="ignore"):
        if fn in ("sin", "cos"):
            return canon32(pt_oracle_np.sincos(v)[fn == "cos"])
        if fn == "log":
            return canon32(pt_oracle_mis_np._log(v))
        if fn == "exp":
            return canon32(pt_oracle_mis_np._exp(v))
        if fn == "pow_gamma":
            return canon32(pt_oracle_mis_np.pow_pt(v, f32(1.0) / f32(2.2)))
        if fn == "sqrt":
            return canon32(np.sqrt(v))
        if fn == "rcp":
            return canon32(f32(1.0) / v)
        if fn == "f2h":
            return canon16(v.astype(np.float16).view(np.uint16))
        if fn == "h2f":
            return canon32(x.astype(np.uint16).view(np.float16).astype(f32))
        if fn == "tonemap":
            a = np.zeros((x.size, 4), f32)
            a[:, 0] = x.astype(np.uint16).view(np.float16).astype(f32)
            return oracle_lib.tonemap(a)[:, 0].astype(np.uint32)
        if fn == "mis_unit":
            return canon32(pt_oracle_mis_np._unit(pt_oracle_mis_np._u32_hash(x)))
    raise KeyError(fn)


def first_difference(x, got, want):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    k = bad[0]
    return f"{bad.size} of {x.size} differ; first at input 0x{int(x[k]):08x}: 0x{int(got[k]):08x} != 0x{int(want[k]):08x}"


@pytest.mark.parametrize("fn", dom.SCALAR_FNS)
def test_host_values_equal_the_restatements(inputs, fn):
    x, got = inputs[fn]
    assert first_difference(x, got, restated(fn, x)) is None


def test_tonemap_takes_the_low_half_only(inputs):
    """Bytes and halves are zero-extended, and H2F / TONEMAP read the low 16 bits."""
    x, got = inputs["tonemap"]
    assert got.max() <= 255 and inputs["f2h"][1].max() <= 0xFFFF
    assert np.array_equal(g.math_values("tonemap", x | np.uint32(0xABCD0000)), got)


HALTON_STRIDE = np.arange(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32) + np.uint32(40503)


@pytest.mark.parametrize("dim", range(24))
def test_host_halton_equals_the_restatements(dim):
    """The host's reference loop against pt_oracle_np.halton (edges + a stride of
    2^16 indices through all of 2^32) and, on the edges, the C oracle's."""
    edges = dom.halton_edge_indices(dim)
    i = np.unique(np.concatenate([edges, HALTON_STRIDE]))
    got = g.math_values("halton_loop", i, dim=dim)
    assert first_difference(i, got, canon32(pt_oracle_np.halton(i, dim))) is None
    # the call sites' 2*pi*u stays inside sincos_pt's [0, 6.28318548f]: in the
    # dimensions that feed it, a sample whose digits are all b - 1 may round up
    # to 1.0f, not above (dimensions 5 and 15 reach 1.0000001f)
    if dim in dom.SINCOS_DIMS:
        assert got.view(f32).min() >= 0.0 and got.view(f32).max() <= 1.0
    mine = g.math_values("halton_loop", edges, dim=dim).view(f32)
    assert [float(v) for v in mine] == [oracle_lib.halton(int(k), dim) for k in edges]


# ---- accuracy against float64 ----------------------------------------------
# The input set is fixed (edges + stride), so the largest error is one number;
# the constants are that number, measured here against float64 numpy and
# rounded up to two significant digits (also in DESIGN.md §3.4 / §3.11).
MAX_ABS_ERR = {"sin": 8.0e-8, "cos": 8.7e-8}          # measured 7.9792e-08, 8.6358e-08
MAX_ULP_ERR = {"log": 0.75, "exp": 1.0, "pow_gamma": 44.0}  # measured 0.7484, 0.9956, 43.2926


def _exact(fn, v):
    v = v.astype(np.float64)
    with np.errstate(all="ignore"):
        if fn == "pow_gamma":
            return np.power(v, float(f32(1.0) / f32(2.2)))
        return {"sin": np.sin, "cos": np.cos, "log": np.log, "exp": np.exp}[fn](v)


@pytest.mark.parametrize("fn", list(MAX_ABS_ERR))
def test_sincos_absolute_error(inputs, fn):
    x, got = inputs[fn]
    err = np.abs(got.view(f32).astype(np.float64) - _exact(fn, x.view(f32)))
    k = int(np.argmax(err))
    print(f"{fn}: max abs error {err[k]:.4e} at 0x{int(x[k]):08x} over {x.size} inputs")
    assert err[k] <= MAX_ABS_ERR[fn]


@pytest.mark.parametrize("fn", list(MAX_ULP_ERR))
def test_log_exp_pow_error_in_ulps(inputs, fn):
    """Error in units of the float32 spacing at the exact value.  pow_pt returns
    0 for x <= 2^-100 by design (rt_math.h): there the exact value is below
    2^-45 and the bound is that, absolutely."""
    x, got = inputs[fn]
    v, r = x.view(f32), got.view(f32).astype(np.float64)
    exact = _exact(fn, v)
    if fn == "pow_gamma":
        cut = v <= np.uint32(dom.POW_CUT).view(f32)
        assert np.all(r[cut] == 0.0) and np.all(exact[cut] < 2.0 ** -45)
        x, r, exact = x[~cut], r[~cut], exact[~cut]
    ulp = np.spacing(np.abs(exact).astype(f32)).astype(np.float64)
    err = np.abs(r - exact) / ulp
    k = int(np.argmax(err))
    print(f"{fn}: max error {err[k]:.4f} ulp at 0x{int(x[k]):08x} over {x.size} inputs")
    assert err[k] <= MAX_ULP_ERR[fn]


# ---- the checksums ----------------------------------------------------------
def sums_np(out, chunk_log2):
    """rt_debug_math_sums from the outputs, by its definition (mod 2^64)."""
    out = np.asarray(out, np.uint32).astype(np.uint64)
    res = []
    for lo in range(0, out.size, 1 << chunk_log2):
        o = out[lo:lo + (1 << chunk_log2)]
        w = 2 * np.arange(o.size, dtype=np.uint64) + np.uint64(1)
        res.append((o.sum(dtype=np.uint64), (o * w).sum(dtype=np.uint64)))
    return np.array(res, np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("fn", dom.SCALAR_FNS + ("halton_loop",))
def test_sums_equal_their_definition(fn):
    """One full chunk and a partial last one, from the host's own values."""
    dim = 5 if fn == "halton_loop" else 0
    first = 0x1234 if fn == "halton_loop" else dom.DOMAINS[fn][-1][0]
    count = (1 << 12) + 1001
    out = g.math_values(fn, first + np.arange(count, dtype=np.uint64), dim=dim)
    s = g.math_sums(fn, first, count, 12, dim=dim)
    assert s.shape == (2, 2) and np.array_equal(s, sums_np(out, 12))
    assert np.array_equal(g.math_sums(fn, first, 1 << 12, 12, dim=dim), s[:1])


def test_sums_reach_the_last_pattern():
    s = g.math_sums("mis_unit", 0xFFFFFF00, 0x100, 6)
    out = g.math_values("mis_unit", 0xFFFFFF00 + np.arange(0x100, dtype=np.uint64))
    assert np.array_equal(s, sums_np(out, 6))


def test_sums_negative_controls():
    """The checksums see what they are for: one output moved by 1 ulp changes
    both; two unequal outputs swapped keep the first and change the second."""
    out = g.math_values("sin", dom.stride_inputs("sin", 1 << 10))[:1 << 10]
    base = sums_np(out, 10)
    moved = out.copy()
    moved[517] += 1
    assert np.all(sums_np(moved, 10) != base)
    swapped = out.copy()
    assert swapped[3] != swapped[900]
    swapped[[3, 900]] = swapped[[900, 3]]
    s = sums_np(swapped, 10)
    assert s[0, 0] == base[0, 0] and s[0, 1] != base[0, 1]


@pytest.mark.parametrize("chunk_log2", [6, 12, 16])
def test_sums_do_not_depend_on_the_thread_count(chunk_log2):
    """Chunks below, at and above the piece a host thread takes at a time."""
    count = (3 << 16) + 77
    one = g.math_sums("log", dom.FLT_MIN, count, chunk_log2, host_threads=1)
    for threads in (2, 5, 16):
        assert np.array_equal(g.math_sums("log", dom.FLT_MIN, count, chunk_log2, host_threads=threads), one)


def test_argument_errors():
    lib, fns = g.lib, _native.MATH_FNS
    buf = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    out = (ctypes.c_uint32 * 4)()
    sums = (ctypes.c_uint64 * 8)()

    def values(fn, where=0, n=4, i=buf, o=out):
        return lib.rt_debug_math_values(fn, where, i, n, o), lib.rt_last_error(None)

    def sums_(fn, where=0, first=0, count=64, log2=6, threads=1, s=sums):
        return lib.rt_debug_math_sums(fn, where, first, count, log2, threads, s), lib.rt_last_error(None)

    assert values(fns["sin"])[0] == 0 and sums_(fns["sin"])[0] == 0
    assert values(fns["sin"], n=0, i=None, o=None)[0] == 0  # nothing to do
    for call in (values, sums_):
        for fn, where, word in [(14, 0, b"rt_math_fn"), (0xFF, 0, b"rt_math_fn"), (1 << 13, 0, b"rt_math_fn"),
                                (fns["sin"], 2, b"where"), (fns["sin"] | 3 << 8, 0, b"dimension"),
                                (fns["halton_loop"] | 24 << 8, 0, b"dimension"),
                                (fns["halton_small"] | 2 << 8, 0, b"reference loop"),
                                (fns["halton_tab"] | 2 << 8, 0, b"reference loop"),
                                (fns["halton_tab"] | 6 << 8, 1, b"table"),
                                (fns["halton_tab"], 1, b"table")]:
            status, msg = call(fn, where)
            assert status == 1 and word in msg, (call.__name__, fn, where, msg)
    assert values(fns["sin"], i=None) == (1, b"null argument")
    assert values(fns["sin"], o=None) == (1, b"null argument")
    assert values(fns["sin"], n=(1 << 24) + 1)[0] == 1
    big = (ctypes.c_uint32 * 4)(1, 2, 3 ** 13, 4)
    assert values(fns["halton_small"] | 1 << 8, 1, i=big) == (1, b"RT_MATH_HALTON_SMALL / _TAB index >= 3^13")
    assert sums_(fns["halton_tab"] | 1 << 8, 1, first=3 ** 13 - 64, count=65)[0] == 1
    assert sums_(fns["sin"], s=None) == (1, b"null argument")
    assert sums_(fns["sin"], log2=5)[0] == 1 and sums_(fns["sin"], log2=32)[0] == 1
    assert b"chunk_log2" in lib.rt_last_error(None)
    assert sums_(fns["sin"], first=0xFFFFFFFF, count=2) == (1, b"first_bits + count > 2^32")
    assert sums_(fns["sin"], first=0xFFFFFFFF, count=1)[0] == 0
    assert sums_(fns["sin"], threads=0)[0] == 1 and sums_(fns["sin"], threads=257)[0] == 1
    assert b"host_threads" in lib.rt_last_error(None)
    with pytest.raises(ValueError):
        g.math_values("tan", [0])
