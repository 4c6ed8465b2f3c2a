"""The table behind tests/test_math_fns.py (CPU) and tests/test_gpu_math_fns.py
(GPU): every function of rt_debug_math_values / rt_debug_math_sums (DESIGN.md
§3.24) with its documented domain, as inclusive ranges of 32-bit input
patterns, and the edge inputs where a host and a device compile could part:
ties of the range reductions, denormals, the half overflow edge, NaNs, the
last digits of large Halton indices.  Inputs only; no expected values."""
import numpy as np

from pt_oracle_np import PRIMES


def bits(x):
    """The pattern of the float32 nearest to x."""
    return int(np.array(x, np.float64).astype(np.float32).view(np.uint32))


def around(pattern, r):
    """The 2r + 1 patterns centred on ``pattern`` (clipped to 32 bits)."""
    return np.arange(max(0, pattern - r), min(0xFFFFFFFF, pattern + r) + 1, dtype=np.uint64)


FLT_MIN, FLT_MAX, INF = 0x00800000, 0x7F7FFFFF, 0x7F800000
DENORM_MIN, DENORM_MAX = 0x00000001, 0x007FFFFF
SIGN = 0x80000000
TWO_PI = 0x40C90FDB          # 6.28318548f
MINUS_87 = 0xC2AE0000        # -87.0f
POW_CUT = bits(7.88860905e-31)  # 2^-100: pow_pt's x <= cut gives 0
SMALL_INDEX_MAX = 3 ** 13    # rt_halton.hpp kSmallIndexMax
TAB_DIMS = (1, 2, 3, 4, 5, 7, 8, 9, 10)  # rt_halton.hpp kTabDigits > 0
# Halton dimensions whose sample u reaches sincos_pt as 2*pi*u: 4 + 5b of the
# path tracer (rt_kernel.hip shade, rt_free.hpp), 2 and 4 of the MIS table
SINCOS_DIMS = (2, 4, 9, 14)
GENERIC = [0, SIGN, DENORM_MIN, DENORM_MAX, FLT_MIN, FLT_MAX, INF, 0x3F800000, 0x7FC00000, 0x7F800001]

# fn -> inclusive ranges of input patterns: the documented domain (rt_math.h)
DOMAINS = {
    "sin": [(0, TWO_PI)],
    "cos": [(0, TWO_PI)],
    "log": [(FLT_MIN, FLT_MAX)],
    "exp": [(0, 0), (SIGN, MINUS_87)],
    "pow_gamma": [(0, 0x3F800000)],
    "sqrt": [(0, 0xFFFFFFFF)],
    "rcp": [(0, 0xFFFFFFFF)],
    "f2h": [(0, 0xFFFFFFFF)],
    "h2f": [(0, 0xFFFF)],
    "tonemap": [(0, 0xFFFF)],
    "mis_unit": [(0, 0xFFFFFFFF)],
}
SCALAR_FNS = tuple(DOMAINS)


def in_domain(fn, patterns):
    p = np.unique(np.asarray(patterns, np.uint64))
    keep = np.zeros(p.shape, bool)
    for lo, hi in DOMAINS[fn]:
        keep |= (p >= lo) & (p <= hi)
    return p[keep].astype(np.uint32)


def _sincos_edges():
    e = [around(0, 64), around(TWO_PI, 64), around(DENORM_MAX, 64)]
    for k in range(1, 9):  # the quadrant and octant boundaries
        e.append(around(bits(k * np.pi / 4), 64))
    c = float(np.float32(0.636619772))
    for n in range(4):  # rintf ties: x * 0.636619772f = n + 0.5
        e.append(around(bits((n + 0.5) / c), 64))
    return np.concatenate(e)


def _exp_edges():
    e = [around(SIGN, 16), around(MINUS_87, 16), around(SIGN | DENORM_MAX, 16), [0]]
    log2e = float(np.float32(1.44269504088896341))
    for m in range(0, -127, -1):  # floorf ties: x * log2e + 0.5 = m
        e.append(around(bits((m - 0.5) / log2e), 16))
    return np.concatenate(e)


def _log_edges():
    e = [around(FLT_MIN, 16), around(FLT_MAX, 16), around(0x3F800000, 64)]
    man = bits(0.707106781) & 0x007FFFFF
    for ex in range(1, 255):  # the m < 0.707106781f switch at every exponent
        e.append(around((ex << 23) | man, 16))
    return np.concatenate(e)


def _pow_edges():
    return np.concatenate([around(0, 16), around(DENORM_MAX, 16), around(POW_CUT, 64), around(0x3F800000, 64),
                           around(bits(0.5), 16)])


def _f2h_edges():
    h = np.arange(0, 0x7C00, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    mid = ((lo + hi) / 2).astype(np.float32)  # exact: 12 significant bits
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    m = mid.view(np.uint32).astype(np.uint64)
    pos = np.concatenate([
        m - 1, m, m + 1,                                       # every half-way point with its neighbours
        h.view(np.float16).astype(np.float32).view(np.uint32)[:0x401].astype(np.uint64),  # the half subnormals, 2^-14
        around(bits(2.0 ** -25), 4), around(bits(2.0 ** -24), 4), around(bits(2.0 ** -14), 4),
        [bits(65504.0), 0x477FEFFF, bits(65520.0), bits(65536.0), INF, FLT_MAX, DENORM_MIN, DENORM_MAX, FLT_MIN, 0],
        [0x7F800001, 0x7F801000, 0x7F802000, 0x7FA00000, 0x7FC00000, 0x7FC00001, 0x7FFFE000, 0x7FFFFFFF],  # NaNs
    ]).astype(np.uint64)
    return np.concatenate([pos, pos | SIGN])


def _cr_edges():  # sqrt_cr / rcp_cr: the short forms' [2^-100, 2^100) switch
    pos = np.concatenate([GENERIC, around(0x0D800000, 8), around(0x71800000, 8), around(FLT_MIN, 8),
                          around(0x3F800000, 8), around(INF, 8), around(bits(2.0 ** 126), 8)]).astype(np.uint64)
    return np.concatenate([pos, pos | SIGN])


def _half_in_edges():
    pos = np.array([0, 1, 0x3FF, 0x400, 0x3BFF, 0x3C00, 0x7BFF, 0x7C00, 0x7C01, 0x7DFF, 0x7E00, 0x7FFF], np.uint64)
    return np.concatenate([pos, pos | 0x8000])


_EDGES = {
    "sin": _sincos_edges, "cos": _sincos_edges, "log": _log_edges, "exp": _exp_edges, "pow_gamma": _pow_edges,
    "sqrt": _cr_edges, "rcp": _cr_edges, "f2h": _f2h_edges, "h2f": _half_in_edges, "tonemap": _half_in_edges,
    "mis_unit": lambda: np.concatenate([around(0, 64), around(SIGN, 64), around(0xFFFFFFFF, 64),
                                        around(1 << 24, 8), around(1 << 16, 8)]),
}


def edge_inputs(fn):
    """Edge input patterns of a scalar function, inside its domain, sorted."""
    return in_domain(fn, np.concatenate([np.asarray(_EDGES[fn](), np.uint64), GENERIC,
                                         [lo for lo, _ in DOMAINS[fn]], [hi for _, hi in DOMAINS[fn]]]))


def stride_inputs(fn, at_least=1 << 16):
    """A fixed stride through every range of the domain, >= at_least inputs in all."""
    size = sum(hi - lo + 1 for lo, hi in DOMAINS[fn])
    step = max(1, size // at_least)
    return np.concatenate([np.arange(lo, hi + 1, step, dtype=np.uint64) for lo, hi in DOMAINS[fn]]).astype(np.uint32)


def halton_edge_indices(dim, limit=1 << 32):
    """0, 1, b^k - 1, b^k, b^k + 1 for every k that fits, 3^13 - 1, 3^13,
    2^20 - 1, 2^32 - 1; below ``limit``."""
    b = int(PRIMES[dim])
    e = {0, 1, SMALL_INDEX_MAX - 1, SMALL_INDEX_MAX, (1 << 20) - 1, (1 << 32) - 1}
    p = b
    while p - 1 < 1 << 32:
        e.update((p - 1, p, p + 1))
        p *= b
    return np.array(sorted(i for i in e if i < min(limit, 1 << 32)), np.uint32)


# The GPU cases: (id, fn, first pattern, count), a full-domain row of DOMAINS
# split where one case would run too long
def full_domain_cases(split=1 << 32):
    cases = []
    for fn in SCALAR_FNS:
        for lo, hi in DOMAINS[fn]:
            parts = -(-(hi - lo + 1) // split)
            for k in range(parts):
                a = lo + k * split
                n = min(split, hi - a + 1)
                cases.append((f"{fn}-{a:08x}", fn, a, n))
    return cases
