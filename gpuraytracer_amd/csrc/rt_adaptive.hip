// rt_adaptive.hip — the sample planner (include/rtpt.h rt_plan_samples; the
// contract is DESIGN.md §3.27, restated in numpy by tests/adaptive_ref.py and
// in plain C++ by rt_plan_samples_host, all compared bit for bit).
//
// From the two images of a pilot render -- `first`, the mean of its first h
// samples, and `all`, the mean of all 2h -- one sample count per pixel:
//
//   plan_weights_kernel  (first, all) -> counts = m, the dilated weight: a
//                        workgroup takes 16x16 tiles in a grid-stride loop; it
//                        computes the weight q (rt_plan.hpp plan_weight) of a
//                        tile and a halo of `radius` pixels into LDS, a texel
//                        outside the image as 0 (q >= 1 inside), takes the
//                        maximum over each pixel's (2 radius + 1)^2
//                        neighbourhood, and adds the sum of its tiles to Q
//                        with one 64-bit atomicAdd
//   plan_counts_kernel   counts = min(count_max, count_min + budget * m / Q)
//                        in place (grid-stride), and the statistics: per
//                        workgroup one atomicAdd each for the samples and the
//                        capped pixels, one atomicMax for the largest count
// At most kPlanGroups workgroups per launch: a few thousand atomics on one
// address instead of one per tile (32,400 at 1080p).
//
// Everything after q is integer, a maximum or a sum of integers: the order of
// the atomics cannot change a result.  No address depends on data.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "rt_kernel.hpp"
#include "rt_plan.hpp"

namespace rt {
namespace {

constexpr int kT = (int)kPlanTile;
constexpr uint32_t kThreads = kPlanTile * kPlanTile;
constexpr int kPitchMax = kT + 2 * (int)kPlanRadiusMax;
constexpr uint32_t kPlanGroups = 2048;

// Sum over the workgroup (every thread calls it); the result is valid in thread 0.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) scratch[wave] = v;
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x == 0)
        for (uint32_t w = 0; w < kThreads / 64u; ++w) s += scratch[w];
    __syncthreads();  // scratch may be used again
    return s;
}
__device__ __forceinline__ uint32_t block_max(uint32_t v, unsigned long long* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_down(v, off));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) scratch[wave] = v;
    __syncthreads();
    uint32_t s = 0;
    if (threadIdx.x == 0)
        for (uint32_t w = 0; w < kThreads / 64u; ++w) s = max(s, (uint32_t)scratch[w]);
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kThreads) void plan_weights_kernel(PlanParams A) {
    __shared__ uint32_t q_s[kPitchMax * kPitchMax];
    __shared__ unsigned long long red_s[kThreads / 64u];
    const int tx = (int)(threadIdx.x & (kPlanTile - 1u)), ty = (int)(threadIdx.x / kPlanTile);
    const int R = (int)A.radius, pitch = kT + 2 * R, n = pitch * pitch;  // R <= kPlanRadiusMax: n <= kPitchMax^2
    const bool relative = (A.flags & kPlanRelative) != 0u;
    const uint32_t tiles_x = ((uint32_t)A.W + kPlanTile - 1u) / kPlanTile;
    const uint32_t tiles = tiles_x * (((uint32_t)A.rows + kPlanTile - 1u) / kPlanTile);
    unsigned long long mine = 0ull;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // uniform over the workgroup (barriers)
        const int x0 = (int)(tile % tiles_x) * kT, y0 = (int)(tile / tiles_x) * kT;
        for (int k = (int)threadIdx.x; k < n; k += (int)kThreads) {
            const int ly = k / pitch, lx = k - ly * pitch;
            const int gx = x0 - R + lx, gy = y0 - R + ly;
            uint32_t q = 0u;  // outside the tile of rows x W pixels: below every weight
            if ((unsigned)gx < (unsigned)A.W && (unsigned)gy < (unsigned)A.rows) {
                const size_t p = (size_t)gy * (size_t)A.W + (size_t)gx;
                const float4 f = A.first[p], a = A.all[p];
                q = plan_weight(f.x, f.y, f.z, a.x, a.y, a.z, relative, A.luminance_floor);
            }
            q_s[k] = q;
        }
        __syncthreads();
        const int x = x0 + tx, y = y0 + ty;
        if (x < A.W && y < A.rows) {
            const int c = (ty + R) * pitch + tx + R;
            uint32_t m = 0u;
            for (int j = -R; j <= R; ++j)
                for (int i = -R; i <= R; ++i) m = max(m, q_s[c + j * pitch + i]);
            A.counts[(size_t)y * (size_t)A.W + (size_t)x] = m;
            mine += m;
        }
        __syncthreads();  // q_s is staged again
    }
    const unsigned long long s = block_sum(mine, red_s);
    if (threadIdx.x == 0) atomicAdd(&A.acc->weight_sum, s);
}

__global__ __launch_bounds__(kThreads) void plan_counts_kernel(PlanParams A) {
    __shared__ unsigned long long red_s[kThreads / 64u];
    const size_t n = (size_t)A.W * (size_t)A.rows;
    const unsigned long long Q = A.acc->weight_sum;  // complete: the launch before this one
    unsigned long long sum = 0ull, ncapped = 0ull;
    uint32_t largest = 0u;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (size_t)gridDim.x * kThreads) {
        const unsigned long long share = plan_share(A.budget, A.counts[p], Q, A.count_min);
        const bool capped = share > (unsigned long long)A.count_max;
        const uint32_t c = capped ? A.count_max : (uint32_t)share;
        A.counts[p] = c;
        sum += c;
        ncapped += capped ? 1u : 0u;
        largest = max(largest, c);
    }
    const unsigned long long samples = block_sum(sum, red_s);
    const unsigned long long ncap = block_sum(ncapped, red_s);
    const uint32_t cmax = block_max(largest, red_s);
    if (threadIdx.x == 0) {
        atomicAdd(&A.acc->samples, samples);
        atomicAdd(&A.acc->at_cap, (uint32_t)ncap);
        atomicMax(&A.acc->count_max_seen, cmax);
    }
}

}  // namespace

hipError_t launch_plan(const PlanParams& P, hipStream_t stream, LaunchInfo* info) {
    if (P.W <= 0 || P.rows <= 0 || P.radius > kPlanRadiusMax || !P.acc) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(P.acc, 0, sizeof(PlanStats), stream);
    if (e != hipSuccess) return e;
    const uint64_t tiles = (uint64_t)(((uint32_t)P.W + kPlanTile - 1) / kPlanTile) *
                           (((uint32_t)P.rows + kPlanTile - 1) / kPlanTile);
    if (tiles > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(tiles < kPlanGroups ? tiles : kPlanGroups));
    hipLaunchKernelGGL(plan_weights_kernel, grid, dim3(kThreads), 0, stream, P);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t n = (size_t)P.W * (size_t)P.rows;
    const size_t blocks = (n + kThreads - 1) / kThreads;
    const dim3 grid2((uint32_t)(blocks < kPlanGroups ? blocks : kPlanGroups));
    hipLaunchKernelGGL(plan_counts_kernel, grid2, dim3(kThreads), 0, stream, P);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (info) fill_launch_info(*info, 1, false, false, kThreads, grid2, 0, "rt::plan_counts_kernel");
    return hipSuccess;
}

}  // namespace rt
