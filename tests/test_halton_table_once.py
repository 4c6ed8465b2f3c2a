"""CPU: the Halton low-digit tables of the box-cluster kernel (rt_halton.hpp,
DESIGN.md §3.3) through the host entry point rt_debug_halton_table, which runs
the header's fill_halton_table<D> on the host: the source a context's one-time
fill kernel runs on the device.

Every entry of every tabulated dimension is compared bit for bit (uint32 views)
with the numpy restatement of the reference loop, pt_oracle_np.halton: for
v < b^k the loop's sum after v's own digits is its sum after k digit steps (the
steps past v's last digit add f * 0 = +0 to a sum that is never -0)."""
import ctypes

import numpy as np

import pt_oracle_np
from gpuraytracer_amd._native import lib

# primes[D]^digits of rt_halton.hpp kTabDigits, D = 1..5 and 7..10
SIZES = {1: 3 ** 6, 2: 5 ** 4, 3: 7 ** 3, 4: 11 ** 2, 5: 13 ** 2, 7: 19 ** 2, 8: 23 ** 2, 9: 29 ** 2, 10: 31 ** 2}
TOTAL = 729 + 625 + 343 + 121 + 169 + 361 + 529 + 841 + 961


def host_table():
    n = ctypes.c_uint32()
    off, size = (ctypes.c_uint32 * 24)(), (ctypes.c_uint32 * 24)()
    assert lib.rt_debug_halton_table(None, 0, ctypes.byref(n), off, size) == 0
    tab = np.full(n.value, np.nan, np.float32)
    assert lib.rt_debug_halton_table(tab.ctypes.data_as(ctypes.c_void_p), tab.size, ctypes.byref(n), None, None) == 0
    return tab, list(off), list(size)


def test_sizes_and_offsets():
    tab, off, size = host_table()
    assert tab.size == TOTAL == sum(SIZES.values())
    assert [int(pt_oracle_np.PRIMES[d]) for d in SIZES] == [3, 5, 7, 11, 13, 19, 23, 29, 31]
    at = 0
    for d in range(24):
        assert size[d] == SIZES.get(d, 0), d
        assert off[d] == at, d
        at += size[d]
    assert at == TOTAL


def test_capacity_is_checked():
    n = ctypes.c_uint32()
    short = np.zeros(TOTAL - 1, np.float32)
    assert lib.rt_debug_halton_table(short.ctypes.data_as(ctypes.c_void_p), short.size, ctypes.byref(n), None, None) != 0
    assert n.value == TOTAL and not short.any()


def test_every_entry_is_the_reference_loop():
    tab, off, size = host_table()
    assert not np.isnan(tab).any()
    for d, n in SIZES.items():
        ref = pt_oracle_np.halton(np.arange(n, dtype=np.uint32), d)
        got = tab[off[d]:off[d] + n]
        diff = got.view(np.uint32) != ref.view(np.uint32)
        assert not diff.any(), (d, np.flatnonzero(diff)[:6].tolist())
