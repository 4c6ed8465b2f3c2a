// rt_reproject.hip — temporal reprojection under a moving camera
// (include/rtpt.h rt_reproject; the arithmetic contract is DESIGN.md §3.31,
// restated in numpy by tests/reproject_ref.py and compared bit for bit).
//
// For every pixel that hit something, the world point of its centre ray is
// projected into the previous frame's camera and the previous frame's
// accumulated colour is gathered there bilinearly, from the taps that show the
// same primitive with a like normal near the pixel's tangent plane; the
// frame's own colour is then blended in by the gathered history length.  The
// per-pixel function is rt_reproject.hpp's, shared with rt_reproject_host.
//
//   * one lane per pixel, a workgroup is a 16x16 tile, a wave four rows of it:
//     the frame's own texels are read as runs of 16 consecutive texels;
//   * PLANES = 1 or 2 colour planes share one set of tap tests;
//   * both cameras' constants are kernel arguments;
//   * a tap costs 8 B (its hit record), then 16 B (its normal) when the id
//     matches, then 16 B per plane when it is valid: a tap of another
//     primitive skips its camera ray.  No LDS: the taps of a tile are not a
//     tile of the previous frame (profiles/r24/reproject.md);
//   * the tap corner is the one place where data reaches an address: it is
//     formed after the gates that bound it, and every tap is tested against
//     the frame before it is read (rt_reproject.hpp);
//   * out[k] may be color[k]: each lane reads its own pixel before it writes
//     that pixel.  A history plane is read at other pixels: it must not
//     overlap an output.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "rt_kernel.hpp"
#include "rt_reproject.hpp"

namespace rt {
namespace {

constexpr uint32_t kThreads = kReprojectTile * kReprojectTile;

template <int PLANES>
__global__ __launch_bounds__(kThreads) void reproject_kernel(ReprojectArgs A) {
    const int32_t x = (int32_t)(blockIdx.x * kReprojectTile + (threadIdx.x & (kReprojectTile - 1u)));
    const int32_t y = (int32_t)(blockIdx.y * kReprojectTile + threadIdx.x / kReprojectTile);
    if (x >= A.W || y >= A.H) return;
    reproject_pixel<PLANES>(A, x, y);
}

}  // namespace

hipError_t launch_reproject(const ReprojectArgs& A, uint32_t planes, hipStream_t stream, LaunchInfo* info) {
    if (A.W <= 0 || A.H <= 0 || planes < 1 || planes > 2) return hipErrorInvalidValue;
    const dim3 grid(((uint32_t)A.W + kReprojectTile - 1) / kReprojectTile,
                    ((uint32_t)A.H + kReprojectTile - 1) / kReprojectTile);
    const dim3 block(kThreads);
    if (planes == 2)
        hipLaunchKernelGGL(reproject_kernel<2>, grid, block, 0, stream, A);
    else
        hipLaunchKernelGGL(reproject_kernel<1>, grid, block, 0, stream, A);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && info)
        fill_launch_info(*info, 1, false, false, kThreads, grid, 0, "rt::reproject_kernel<%u>", planes);
    return e;
}

}  // namespace rt
