// rt_mathcheck.hpp — what rt_debug_math_values / rt_debug_math_sums evaluate
// (include/rtpt.h): one definition of "function fn on input
// pattern b", compiled for x86 into rt_api_host.cpp and for gfx950 into
// rt_mathcheck.hip.  The two compiles differ only where the library's host
// and device code differ: sqrt_cr / rcp_cr (rt_math.h) and the half
// conversions (__float2half_rn / __half2float against rt_half.h).  The Halton
// forms are device templates (rt_halton.hpp) and live in rt_mathcheck.hip; the
// host has the reference loop of rt_api_host.cpp.
#pragma once

#include <hip/hip_runtime.h>
#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#endif
#include <stdint.h>

#include "../../include/rtpt.h"
#include "rt_half.h"
#include "rt_math.h"

namespace rt {

// NaN signs and payloads differ between x86 and gfx950: one pattern for all
RT_HD uint32_t canon_f32(float v) {
    const uint32_t b = f2u(v);
    return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : b;
}
RT_HD uint32_t canon_f16(uint32_t h) { return (h & 0x7FFFu) > 0x7C00u ? 0x7E00u : h; }

RT_HD uint32_t math_f2h(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half_as_ushort(__float2half_rn(x));
#else
    return to_half(x);
#endif
}
RT_HD float math_h2f(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half((unsigned short)h));
#else
    return from_half((uint16_t)h);
#endif
}

// The scalar (non-Halton) functions: FN is an rt_math_fn below RT_MATH_HALTON_LOOP.
template <uint32_t FN>
RT_HD uint32_t math_eval(uint32_t b) {
    static_assert(FN < RT_MATH_HALTON_LOOP, "Halton forms: rt_mathcheck.hip / halton_host");
    if constexpr (FN == RT_MATH_SIN || FN == RT_MATH_COS) {
        float s, c;
        sincos_pt(u2f(b), &s, &c);
        return canon_f32(FN == RT_MATH_SIN ? s : c);
    } else if constexpr (FN == RT_MATH_LOG) {
        return canon_f32(log_pt(u2f(b)));
    } else if constexpr (FN == RT_MATH_EXP) {
        return canon_f32(exp_pt(u2f(b)));
    } else if constexpr (FN == RT_MATH_POW_GAMMA) {
        return canon_f32(pow_pt(u2f(b), 1.0f / 2.2f));
    } else if constexpr (FN == RT_MATH_SQRT) {
        return canon_f32(sqrt_cr(u2f(b)));
    } else if constexpr (FN == RT_MATH_RCP) {
        return canon_f32(rcp_cr(u2f(b)));
    } else if constexpr (FN == RT_MATH_F2H) {
        return canon_f16(math_f2h(u2f(b)));
    } else if constexpr (FN == RT_MATH_H2F) {
        return canon_f32(math_h2f(b & 0xFFFFu));
    } else if constexpr (FN == RT_MATH_TONEMAP) {
        return tonemap_channel(math_h2f(b & 0xFFFFu));
    } else {
        return canon_f32(mis_unit(mis_hash(b)));
    }
}

constexpr uint32_t kMathFnCount = RT_MATH_HALTON_TAB + 1;
constexpr uint32_t kMathChunkLog2Min = 6, kMathChunkLog2Max = 31;

// Device side (rt_mathcheck.hip): host arrays in and out, the current device,
// its null stream, synchronous.  The arguments were validated by the caller
// (rt_api_host.cpp): fn below kMathFnCount, D < 24 (a table dimension for _TAB),
// indices of _SMALL / _TAB below math_small_index_max().
bool math_dim_has_table(uint32_t D);
uint32_t math_small_index_max();
hipError_t math_values_device(uint32_t fn, uint32_t D, const uint32_t* in, uint32_t n, uint32_t* out);
hipError_t math_sums_device(uint32_t fn, uint32_t D, uint32_t first, uint64_t count, uint32_t chunk_log2,
                            uint64_t* sums);

}  // namespace rt
