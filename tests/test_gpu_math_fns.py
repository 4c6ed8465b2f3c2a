"""GPU: every scalar function the kernels share with the host, the half
conversions of the image epilogue and the three device Halton forms, gfx950
compile against x86 compile, bit for bit over the function's WHOLE documented
domain (tests/math_fn_domains.py).  Both sides reduce every
2^16 consecutive inputs to two 64-bit checksums (rt_debug_math_sums); on a
mismatch the first differing chunk is fetched value by value from both sides
and the assertion names the first input on which they differ."""
import os
import time

import numpy as np
import pytest

import gpuraytracer_amd as g
import math_fn_domains as dom

pytestmark = pytest.mark.gpu

CHUNK_LOG2 = 16
THREADS = min(16, len(os.sched_getaffinity(0)))


def sums_difference(fn, first, count, dim=0, host_fn=None):
    """None when the device sums of fn over first .. first + count - 1 equal the
    host sums of host_fn (default fn), chunk for chunk; else a message that
    names the first differing input."""
    host_fn = host_fn or fn
    t0 = time.perf_counter()
    dev = g.math_sums(fn, first, count, CHUNK_LOG2, "device", dim)
    t1 = time.perf_counter()
    host = g.math_sums(host_fn, first, count, CHUNK_LOG2, "host", dim, THREADS)
    t2 = time.perf_counter()
    print(f"{fn}[{dim}] 0x{first:08x}+{count}: device {t1 - t0:.3f} s, host {t2 - t1:.3f} s on {THREADS} threads")
    bad = np.flatnonzero((dev != host).any(axis=1))
    if bad.size == 0:
        return None
    c = int(bad[0])
    lo = first + (c << CHUNK_LOG2)
    x = lo + np.arange(min(1 << CHUNK_LOG2, first + count - lo), dtype=np.uint64)
    d, h = g.math_values(fn, x, "device", dim), g.math_values(host_fn, x, "host", dim)
    k = np.flatnonzero(d != h)
    if k.size == 0:
        return f"{fn}[{dim}]: the sums of chunk {c} (from 0x{lo:08x}) differ, its values do not"
    j = int(k[0])
    return (f"{fn}[{dim}]: {bad.size} of {dev.shape[0]} chunks differ; first input 0x{int(x[j]):08x}: "
            f"device 0x{int(d[j]):08x}, host 0x{int(h[j]):08x} ({k.size} inputs of its chunk differ)")


def values_difference(fn, x, dim=0, host_fn=None):
    d, h = g.math_values(fn, x, "device", dim), g.math_values(host_fn or fn, x, "host", dim)
    k = np.flatnonzero(d != h)
    if k.size == 0:
        return None
    return (f"{fn}[{dim}]: {k.size} of {x.size} edge inputs differ; first 0x{int(x[k[0]]):08x}: "
            f"device 0x{int(d[k[0]]):08x}, host 0x{int(h[k[0]]):08x}")


CASES = dom.full_domain_cases()


@pytest.mark.parametrize("fn,first,count", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_device_equals_host_over_the_whole_domain(fn, first, count):
    assert sums_difference(fn, first, count) is None


@pytest.mark.parametrize("fn", dom.SCALAR_FNS)
def test_device_equals_host_on_the_edge_inputs(fn):
    assert values_difference(fn, dom.edge_inputs(fn)) is None


@pytest.mark.parametrize("dim", range(24))
def test_halton_forms_equal_the_host_loop(dim):
    """Every device form of dimension dim over every index below 3^13 (what
    halton_small / halton_tab serve), the loop also just above it and at the
    top of the 32-bit indices; then the edge indices value by value."""
    small = dom.SMALL_INDEX_MAX
    forms = ["halton_loop", "halton_small"] + (["halton_tab"] if dim in dom.TAB_DIMS else [])
    found = [sums_difference(fn, 0, small, dim, "halton_loop") for fn in forms]
    found.append(sums_difference("halton_loop", small, 1 << 16, dim))
    found.append(sums_difference("halton_loop", (1 << 32) - (1 << 20), 1 << 20, dim))
    found.append(values_difference("halton_loop", dom.halton_edge_indices(dim), dim))
    found += [values_difference(fn, dom.halton_edge_indices(dim, small), dim, "halton_loop") for fn in forms[1:]]
    found = [m for m in found if m]  # every form is checked before the test fails
    assert not found, "\n".join(found)


def test_table_dimensions_match_the_library():
    """dom.TAB_DIMS restates rt_halton.hpp kTabDigits: the library refuses
    halton_tab exactly for the other dimensions."""
    for dim in range(24):
        if dim in dom.TAB_DIMS:
            g.math_values("halton_tab", [0, 1], "device", dim)
        else:
            with pytest.raises(g.RtError):
                g.math_values("halton_tab", [0, 1], "device", dim)
