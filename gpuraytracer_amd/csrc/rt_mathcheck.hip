// rt_mathcheck.hip — device side of rt_debug_math_values / rt_debug_math_sums
// (include/rtpt.h): the scalar functions the kernels share
// with the host (rt_math.h), the half conversions of the image epilogue and
// the three Halton forms (rt_halton.hpp), each in a kernel of its own, so a
// test can hold the gfx950 compile of every one of them to the x86 compile bit
// for bit over its whole domain.  Built with the library's HIPFLAGS, like every
// other device TU: what is checked is the contract under the shipped flags.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "rt_kernel.hpp"
#include "rt_halton.hpp"
#include "rt_mathcheck.hpp"

namespace rt {
namespace {

// One Halton form at a compile-time dimension, called as the path-tracing
// kernels call it (halton_dim, rt_halton.hpp).
template <uint32_t FN, uint32_t D>
__device__ __forceinline__ float halton_form(uint32_t i, const float* tab) {
    if constexpr (FN == RT_MATH_HALTON_LOOP) {
        return halton_dim<D, false>(i);
    } else if constexpr (FN == RT_MATH_HALTON_SMALL) {
        return halton_dim<D, true>(i);
    } else if constexpr (kTabDigits[D] > 0) {
        return halton_dim<D, true, true>(i, tab);
    } else {
        return 0.0f;  // no table for D: refused by the caller
    }
}

template <uint32_t FN>
__device__ __forceinline__ float halton_at(uint32_t i, uint32_t D, const float* tab) {
    switch (D) {  // wave-uniform
#define RT_CASE(d) case d: return halton_form<FN, d>(i, tab);
        RT_CASE(0) RT_CASE(1) RT_CASE(2) RT_CASE(3) RT_CASE(4) RT_CASE(5) RT_CASE(6) RT_CASE(7)
        RT_CASE(8) RT_CASE(9) RT_CASE(10) RT_CASE(11) RT_CASE(12) RT_CASE(13) RT_CASE(14) RT_CASE(15)
        RT_CASE(16) RT_CASE(17) RT_CASE(18) RT_CASE(19) RT_CASE(20) RT_CASE(21) RT_CASE(22) RT_CASE(23)
#undef RT_CASE
    }
    return 0.0f;
}

template <uint32_t FN>
__device__ __forceinline__ uint32_t eval_device(uint32_t b, uint32_t D, const float* tab) {
    if constexpr (FN < RT_MATH_HALTON_LOOP)
        return math_eval<FN>(b);
    else
        return canon_f32(halton_at<FN>(b, D, tab));
}

constexpr uint32_t tab_floats(uint32_t FN) { return FN == RT_MATH_HALTON_TAB ? kHaltonTabFloats : 1u; }

// The low-digit tables in LDS, filled by the whole workgroup at the path-tracing
// kernels' block size as they fill them (fill_halton_tables, then a barrier).
template <uint32_t FN>
__device__ __forceinline__ void stage_tables(float* tab) {
    if constexpr (FN == RT_MATH_HALTON_TAB) {
        fill_halton_tables(tab, threadIdx.x, kBlockThreads);
        __syncthreads();
    }
}

template <uint32_t FN>
__global__ __launch_bounds__(kBlockThreads) void math_values_kernel(uint32_t D, const uint32_t* __restrict__ in,
                                                                    uint32_t n, uint32_t* __restrict__ out) {
    __shared__ float tab[tab_floats(FN)];
    stage_tables<FN>(tab);
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < n; j += gridDim.x * kBlockThreads)
        out[j] = eval_device<FN>(in[j], D, tab);
}

// One workgroup per chunk of 2^chunk_log2 inputs first + j: the two checksums of
// rt_debug_math_sums, summed per lane, then across the wave, then one 64-bit
// atomic add per wave and sum (integer sums mod 2^64: any order gives the
// same value).  sums was zeroed by the caller.
template <uint32_t FN>
__global__ __launch_bounds__(kBlockThreads) void math_sums_kernel(uint32_t D, uint32_t first, uint64_t count,
                                                                  uint32_t chunk_log2,
                                                                  unsigned long long* __restrict__ sums) {
    __shared__ float tab[tab_floats(FN)];
    stage_tables<FN>(tab);
    const uint64_t base = (uint64_t)blockIdx.x << chunk_log2;  // < count: the grid is ceil(count / chunk)
    const uint64_t left = count - base, chunk = 1ull << chunk_log2;
    const uint32_t n = (uint32_t)(left < chunk ? left : chunk);  // <= 2^31
    const uint32_t b0 = first + (uint32_t)base;                  // first + count <= 2^32: no wrap below
    unsigned long long s0 = 0, s1 = 0;
    for (uint32_t j = threadIdx.x; j < n; j += kBlockThreads) {
        const unsigned long long o = eval_device<FN>(b0 + j, D, tab);
        s0 += o;
        s1 += o * (2ull * j + 1ull);
    }
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off);
        s1 += __shfl_down(s1, off);
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&sums[2 * (size_t)blockIdx.x], s0);
        atomicAdd(&sums[2 * (size_t)blockIdx.x + 1], s1);
    }
}

template <uint32_t FN>
void launch_values(uint32_t D, const uint32_t* d_in, uint32_t n, uint32_t* d_out) {
    uint32_t blocks = (n + kBlockThreads - 1) / kBlockThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(math_values_kernel<FN>, dim3(blocks), dim3(kBlockThreads), 0, 0, D, d_in, n, d_out);
}

template <uint32_t FN>
void launch_sums(uint32_t D, uint32_t first, uint64_t count, uint32_t chunk_log2, uint32_t chunks,
                 unsigned long long* d_sums) {
    hipLaunchKernelGGL(math_sums_kernel<FN>, dim3(chunks), dim3(kBlockThreads), 0, 0, D, first, count, chunk_log2,
                       d_sums);
}

// fn (validated below kMathFnCount) -> f(its value as a compile-time constant)
template <typename F>
void for_fn(uint32_t fn, F&& f) {
    switch (fn) {
        case RT_MATH_SIN: f(std::integral_constant<uint32_t, RT_MATH_SIN>{}); break;
        case RT_MATH_COS: f(std::integral_constant<uint32_t, RT_MATH_COS>{}); break;
        case RT_MATH_LOG: f(std::integral_constant<uint32_t, RT_MATH_LOG>{}); break;
        case RT_MATH_EXP: f(std::integral_constant<uint32_t, RT_MATH_EXP>{}); break;
        case RT_MATH_POW_GAMMA: f(std::integral_constant<uint32_t, RT_MATH_POW_GAMMA>{}); break;
        case RT_MATH_SQRT: f(std::integral_constant<uint32_t, RT_MATH_SQRT>{}); break;
        case RT_MATH_RCP: f(std::integral_constant<uint32_t, RT_MATH_RCP>{}); break;
        case RT_MATH_F2H: f(std::integral_constant<uint32_t, RT_MATH_F2H>{}); break;
        case RT_MATH_H2F: f(std::integral_constant<uint32_t, RT_MATH_H2F>{}); break;
        case RT_MATH_TONEMAP: f(std::integral_constant<uint32_t, RT_MATH_TONEMAP>{}); break;
        case RT_MATH_MIS_UNIT: f(std::integral_constant<uint32_t, RT_MATH_MIS_UNIT>{}); break;
        case RT_MATH_HALTON_LOOP: f(std::integral_constant<uint32_t, RT_MATH_HALTON_LOOP>{}); break;
        case RT_MATH_HALTON_SMALL: f(std::integral_constant<uint32_t, RT_MATH_HALTON_SMALL>{}); break;
        default: f(std::integral_constant<uint32_t, RT_MATH_HALTON_TAB>{}); break;
    }
}

}  // namespace

bool math_dim_has_table(uint32_t D) { return D < 24 && kTabDigits[D] > 0; }
uint32_t math_small_index_max() { return kSmallIndexMax; }

hipError_t math_values_device(uint32_t fn, uint32_t D, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (n == 0) return hipSuccess;
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    uint32_t* d = nullptr;  // n inputs, then n outputs
    hipError_t e = hipMalloc((void**)&d, 2 * bytes);
    if (e != hipSuccess) return e;
    if ((e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice)) == hipSuccess) {
        for_fn(fn, [&](auto F) { launch_values<decltype(F)::value>(D, d, n, d + n); });
        if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
            e = hipMemcpy(out, d + n, bytes, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    return e;
}

hipError_t math_sums_device(uint32_t fn, uint32_t D, uint32_t first, uint64_t count, uint32_t chunk_log2,
                            uint64_t* sums) {
    if (count == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)((count + (1ull << chunk_log2) - 1) >> chunk_log2);
    const size_t bytes = 2 * (size_t)chunks * sizeof(unsigned long long);
    unsigned long long* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, bytes);
    if (e != hipSuccess) return e;
    if ((e = hipMemset(d, 0, bytes)) == hipSuccess) {
        for_fn(fn, [&](auto F) { launch_sums<decltype(F)::value>(D, first, count, chunk_log2, chunks, d); });
        if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
            e = hipMemcpy(sums, d, bytes, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    return e;
}

}  // namespace rt
