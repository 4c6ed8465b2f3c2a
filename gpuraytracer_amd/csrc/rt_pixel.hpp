// rt_pixel.hpp — what the per-pixel kernels share about pixels: the camera ray
// through a pixel, the XCD-aware tile order of the workgroups and the mapping
// of a workgroup's threads to the pixels of its tile (rt_kernel.hip,
// rt_free.hpp, rt_aov.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_math.h"

namespace rt {
namespace {

// generateCameraRay (sampling.metal:125-157): the direction through pixel
// (fx, fy) jittered by (jx, jy).  IEEE: the triangle-BVH kernel's
// normalize_ieee (rt_math.h).  P: any kernel's arguments (halfW, halfH).
template <bool IEEE = false, typename PT>
__device__ __forceinline__ f3 camera_dir(const PT& P, f3 cu, f3 cv, f3 cw, float fW, float fH, float fx,
                                         float fy, float jx, float jy) {
    const float sx = ((fx + jx) / fW) * 2.0f - 1.0f;
    const float ty = -(((fy + jy) / fH) * 2.0f - 1.0f);
    const float sh = sx * P.halfW, th = ty * P.halfH;
    return IEEE ? normalize_ieee((cu * sh + cv * th) - cw) : normalize((cu * sh + cv * th) - cw);
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs in
// dispatch order (p = blockIdx.y * gridDim.x + blockIdx.x; MI355X_MICROARCH.md
// "Workgroup dispatch"), so the tiles are dealt in runs of kXcdRun: the run
// of neighbouring tiles that share the 128-B lines of the seed rows goes
// through ONE XCD's L2 (seed reads 4x -> 1x the seed bytes), while the runs
// still interleave over the XCDs, which keeps the cheap and the expensive
// image regions evenly spread (contiguous bands per XCD ran 7 % slower).
// Speed only: every tile is rendered exactly once.
__device__ __forceinline__ void xcd_tile(uint32_t& bx, uint32_t& by) {
    constexpr uint32_t kXcdRun = 4;  // runs of 0 (plain order) / 16: 158.9 / 157.6 vs 158.4 ms on config 4
    const uint32_t n = gridDim.x * gridDim.y, full = n / (8u * kXcdRun + (kXcdRun == 0)) * (8u * kXcdRun);
    const uint32_t p = blockIdx.y * gridDim.x + blockIdx.x;
    uint32_t t = p;
    if (kXcdRun > 0 && p < full) {
        const uint32_t xcd = p % 8u, k = p / 8u;
        t = ((k / kXcdRun) * 8u + xcd) * kXcdRun + k % kXcdRun;
    }
    bx = t % gridDim.x;
    by = t / gridDim.x;
}

// The pixel of thread t in tile (bx, by): a wave holds 64/L pixels, kWX wide
// and kWY high, L consecutive lanes each; a workgroup is WR x WC waves.  x is
// the column, j the row of the launch's row partition.  The render kernel
// (rt_kernel.hip pixel_of) states the same mapping in place.
template <uint32_t L, uint32_t WR, uint32_t WC>
__device__ __forceinline__ void tile_pixel(uint32_t t, uint32_t bx, uint32_t by, uint32_t kWX, uint32_t kWY,
                                           uint32_t& x, uint32_t& j) {
    const uint32_t lane = t & 63u, wave = t >> 6, pix = lane / L;
    x = bx * (WR * kWX) + (wave % WR) * kWX + (pix % kWX);
    j = by * (WC * kWY) + (wave / WR) * kWY + (pix / kWX);
}

}  // namespace
}  // namespace rt
