// rt_wavemask.hpp — the beam of a wave's camera rays, for the kernels that form
// the per-wave camera mask of the box-cluster layout themselves (DESIGN.md
// §3.16, §3.29): rt_kernel.hip wave_masks_kernel, rt_counts.hpp
// path_counts_kernel, rt_aov.hip aov_kernel.  The lane tests and ballots behind
// it stay spelled out in each kernel: through a shared routine the kernels
// compile to other instructions (tools/isa_diff.sh).
#pragma once

#include "rt_beam.hpp"
#include "rt_kernel.hpp"
#include "rt_trace.hpp"

namespace rt {
namespace {

// The beam of a wave's camera rays: its pixels are columns wx0 .. wx0 + kWX - 1
// and partition rows wj0 .. wj0 + kWY - 1 of P (KParams or AovParams).
template <typename PT>
__device__ __forceinline__ Beam wave_beam(const PT& P, uint32_t wx0, uint32_t wj0, uint32_t kWX, uint32_t kWY) {
    const float y0 = (float)(P.row_start + wj0 * P.row_step);
    const float y1 = (float)(P.row_start + (wj0 + kWY - 1u) * P.row_step);
    return make_beam(ld_f3(P.cam_pos), ld_f3(P.cam_u), ld_f3(P.cam_v), ld_f3(P.cam_w), P.halfW, P.halfH, (float)P.W,
                     (float)P.H, (float)wx0, (float)(wx0 + kWX - 1u), y0, y1);
}

}  // namespace
}  // namespace rt
