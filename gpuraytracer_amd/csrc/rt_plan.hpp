// rt_plan.hpp — the sample planner's per-pixel arithmetic (include/rtpt.h
// rt_plan_samples), written once for the device kernels
// (rt_adaptive.hip) and the host function (rt_api_host.cpp
// rt_plan_samples_host).  Steps 1-4 of the contract are fp32 under the
// arithmetic contract of rt_math.h; from the weight q on everything is
// integer, a maximum or an order-free sum.
#pragma once

#include "rt_math.h"

namespace rt {

constexpr uint32_t kPlanRelative = 0x800u;       // RT_PLAN_RELATIVE
constexpr uint32_t kPlanRadiusMax = 2;           // dilation radius at most
constexpr uint32_t kPlanCountMax = 1u << 24;     // counts stay exact as a sum's .w
constexpr uint64_t kPlanBudgetEnd = 1ull << 38;  // budget * q < 2^63

// Steps 1-4: the weight q in [1, 2^24 + 1] of a pixel from its pilot colours,
// `first` (the first half of the pilot's samples) and `all` (all of them).
RT_HD uint32_t plan_weight(float fr, float fg, float fb, float ar, float ag, float ab, bool relative, float floor) {
    const float la = lum(ar, ag, ab);
    const float el = fabsf(la - lum(fr, fg, fb));
    float r = relative ? el / (la + floor) : el;
    r = (r >= 0.0f) ? r : 0.0f;  // NaN: 0
    return 1u + (uint32_t)fminf(r * 65536.0f, 16777216.0f);
}

// Step 7: the count of a pixel of dilated weight m, before the cap (64 bit:
// budget < 2^38 and m <= 2^24 + 1, and the share is at most the budget).
RT_HD uint64_t plan_share(uint64_t budget, uint32_t m, uint64_t Q, uint32_t count_min) {
    return (uint64_t)count_min + (budget * (uint64_t)m) / Q;
}

}  // namespace rt
