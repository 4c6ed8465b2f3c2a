// rt_denoise.hip — variance-guided edge-avoiding a-trous denoiser for low-spp
// renders (include/rtpt.h rt_denoise; the arithmetic contract is DESIGN.md
// §3.23, restated in numpy by tests/denoise_ref.py and compared bit for bit).
//
// Inputs: two renders of half the samples each (colour a, b), and the albedo /
// normal_depth feature buffers of all samples (rt_render_aov).  The filter runs
// on albedo-demodulated colour D; its luminance weight is scaled by a per-pixel
// variance V estimated from the difference of the halves, and V is filtered
// with the squared weights alongside D.
//
//   prepare_kernel     (a, b, albedo) -> t0 = (D.rgb, Vraw)    Vraw = -1 marks a
//                      pixel without coverage: taps skip it, it keeps its texel
//   variance_kernel    t0 -> t1 = (D.rgb, g3(Vraw))            3x3 binomial
//   atrous_kernel<LDS> one 5x5 pass at `step` pixels between taps, t1 -> t0 ->
//                      t1 ...; the last pass multiplies the albedo back and
//                      writes `out` (a pixel without coverage: the mean of the
//                      halves) instead of a texel
//
//   * one lane per pixel, a workgroup is a 16x16 tile, a wave four rows of it:
//     every tap of a wave reads four runs of 16 consecutive 16-B texels;
//   * a tap costs two 16-B reads, (D, V) and (N, Z); the per-pixel terms -- the
//     depth slopes, g3(V) and the luminance scale -- are computed once;
//   * LDS = true: the workgroup stages the texels of its tile and a halo of
//     2 * step pixels (denoise_lds_bytes, rt_kernel.hpp), a texel outside the
//     frame as a no-coverage texel; LDS = false reads global memory, a tap
//     outside the frame by a bounds test, its workgroups in XCD bands
//     (xcd_band_tile).  Both forms run the same arithmetic; steps 1, 2 and 4
//     are staged, measured against both neighbours (profiles/r16/denoise.md);
//   * no index depends on data: nothing a buffer holds can move a read;
//   * `out` may be colour a or b: only the last pass reads them again, each
//     lane its own pixel, before it writes that pixel.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "rt_kernel.hpp"

namespace rt {
namespace {

constexpr int kT = (int)kDenoiseTile;
constexpr uint32_t kThreads = kDenoiseTile * kDenoiseTile;
constexpr float kAlbedoFloor = 0x1p-10f;
constexpr float kNoCoverage = -1.0f;  // V of a pixel without coverage (V >= 0 otherwise)

// lum: rt_math.h (shared with the sample planner)
__device__ __forceinline__ bool covered(float v) { return v >= 0.0f; }

// The texels around one pixel in global memory; outside the frame a texel reads
// as no coverage.
struct GlobalTexels {
    const float4* dv;
    const float4* nz;
    int W, H, x, y;
    __device__ __forceinline__ bool inside(int dx, int dy) const {
        return (unsigned)(x + dx) < (unsigned)W && (unsigned)(y + dy) < (unsigned)H;
    }
    __device__ __forceinline__ size_t at(int dx, int dy) const { return (size_t)(y + dy) * (size_t)W + (size_t)(x + dx); }
    __device__ __forceinline__ float v(int dx, int dy) const { return inside(dx, dy) ? dv[at(dx, dy)].w : kNoCoverage; }
    __device__ __forceinline__ float z(int dx, int dy) const { return inside(dx, dy) ? nz[at(dx, dy)].w : 0.0f; }
    __device__ __forceinline__ float4 DV(int dx, int dy) const {
        return inside(dx, dy) ? dv[at(dx, dy)] : make_float4(0.0f, 0.0f, 0.0f, kNoCoverage);
    }
    __device__ __forceinline__ float4 NZ(int dx, int dy) const {
        return inside(dx, dy) ? nz[at(dx, dy)] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
};

// The same around one pixel of a staged tile: every tap lies in the halo.
struct LdsTexels {
    const float4* dv;
    const float4* nz;
    int pitch, c;  // texels per staged row; this pixel's texel
    __device__ __forceinline__ float v(int dx, int dy) const { return dv[c + dy * pitch + dx].w; }
    __device__ __forceinline__ float z(int dx, int dy) const { return nz[c + dy * pitch + dx].w; }
    __device__ __forceinline__ float4 DV(int dx, int dy) const { return dv[c + dy * pitch + dx]; }
    __device__ __forceinline__ float4 NZ(int dx, int dy) const { return nz[c + dy * pitch + dx]; }
};

// g3 of §3.23 at a covered pixel: the 3x3 binomial mean of V over the covered
// pixels in the frame.  v9: V of the 3x3 neighbourhood, row by row.
__device__ __forceinline__ float g3(const float (&v9)[9]) {
    constexpr float G[3] = {0.25f, 0.5f, 0.25f};
    float s = 0.0f, sw = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float k = G[j] * G[i];
            const float v = v9[3 * j + i];
            if (covered(v)) {
                sw += k;
                s = fmaf(k, v, s);
            }
        }
    return s * rcp_cr(sw);
}

// One-sided depth difference of smaller magnitude among the covered
// neighbours, the forward one on a tie, 0 without one.
__device__ __forceinline__ float depth_slope(float zp, bool pf, float zf, bool pb, float zb) {
    const float f = zf - zp, b = zp - zb;
    if (pf && pb) return fabsf(f) <= fabsf(b) ? f : b;
    return pf ? f : pb ? b : 0.0f;
}

// Workgroups are dealt round-robin over the 8 XCDs in dispatch order
// (p = blockIdx.y * gridDim.x + blockIdx.x): XCD x filters the x-th of eight
// contiguous runs of tiles in row-major order, so that the taps of neighbouring
// tiles go through one XCD's L2.  For the passes that read global memory only:
// 1080p Cornell, 5 passes 0.557 -> 0.448 ms with it on every pass, the step-8
// and step-16 passes 0.125 -> 0.095 and 0.181 -> 0.096 ms, the staged passes
// 3 % slower (profiles/r16/denoise.md).  Speed only: every tile is filtered once.
#ifndef RT_DENOISE_XCD_BANDS
#define RT_DENOISE_XCD_BANDS 1
#endif
__device__ __forceinline__ void xcd_band_tile(uint32_t& bx, uint32_t& by) {
    const uint32_t n = gridDim.x * gridDim.y, q = n / 8u, r = n % 8u;
    const uint32_t p = by * gridDim.x + bx, xcd = p % 8u, k = p / 8u;
    const uint32_t t = xcd * q + min(xcd, r) + k;  // XCD x holds q + (x < r) tiles
    bx = t % gridDim.x;
    by = t / gridDim.x;
}

struct AtrousArgs {
    const float4* src;           // (D, V) of the previous pass
    const float4* normal_depth;
    float4* dst;                 // (D, V) of this pass; unused by the last pass
    const float4* color_a;       // the last pass only
    const float4* color_b;
    const float4* albedo;
    float4* out;
    int32_t W, H;
    int32_t step;
    uint32_t normal_power_log2;
    float sigma_luminance, sigma_depth, depth_floor;
    uint32_t last;
};

// One pixel of one pass: the new (D, V) of a covered pixel.
template <class Texels>
__device__ __forceinline__ float4 atrous_pixel(const Texels& T, const float4 Tp, const float4 Np, const AtrousArgs& A) {
    constexpr float B[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int s = A.step;
    float v9[9];
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) v9[3 * (j + 1) + (i + 1)] = (i == 0 && j == 0) ? Tp.w : T.v(i, j);
    const float gv = g3(v9);
    const float il = rcp_cr(fmaf(A.sigma_luminance, sqrt_cr(gv), 1e-4f));
    const float gx = depth_slope(Np.w, covered(v9[5]), T.z(1, 0), covered(v9[3]), T.z(-1, 0));
    const float gy = depth_slope(Np.w, covered(v9[7]), T.z(0, 1), covered(v9[1]), T.z(0, -1));
    const float Lp = lum(Tp.x, Tp.y, Tp.z);

    float sw = 0.0f, sv = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const float k = B[j + 2] * B[i + 2];
            float4 Tq;
            float w;
            if (i == 0 && j == 0) {
                Tq = Tp;
                w = k;
            } else {
                Tq = T.DV(i * s, j * s);
                if (!covered(Tq.w)) continue;
                const float4 Nq = T.NZ(i * s, j * s);
                const float dn = fmaf(Np.z, Nq.z, fmaf(Np.y, Nq.y, Np.x * Nq.x));
                float wn = fmaxf(dn, 0.0f);
                for (uint32_t n = 0; n < A.normal_power_log2; ++n) wn = wn * wn;
                const float slope = fabsf(fmaf(gx, (float)(i * s), gy * (float)(j * s)));
                float e = fabsf(Np.w - Nq.w) * rcp_cr(fmaf(A.sigma_depth, slope, A.depth_floor));
                e = fmaf(fabsf(Lp - lum(Tq.x, Tq.y, Tq.z)), il, e);
                w = (k * wn) * exp_pt(-fminf(e, 87.0f));
            }
            sw += w;
            sv = fmaf(w * w, Tq.w, sv);
            sr = fmaf(w, Tq.x, sr);
            sg = fmaf(w, Tq.y, sg);
            sb = fmaf(w, Tq.z, sb);
        }
    }
    const float r = rcp_cr(sw);
    return make_float4(sr * r, sg * r, sb * r, sv * (r * r));
}

__device__ __forceinline__ void atrous_store(const AtrousArgs& A, size_t p, float4 R) {
    if (!A.last) {
        A.dst[p] = R;
        return;
    }
    const float4 ca = A.color_a[p];
    if (covered(R.w)) {
        const float4 al = A.albedo[p];
        A.out[p] = make_float4(R.x * fmaxf(al.x, kAlbedoFloor), R.y * fmaxf(al.y, kAlbedoFloor),
                               R.z * fmaxf(al.z, kAlbedoFloor), ca.w);
    } else {
        const float4 cb = A.color_b[p];
        A.out[p] = make_float4((ca.x + cb.x) * 0.5f, (ca.y + cb.y) * 0.5f, (ca.z + cb.z) * 0.5f, ca.w);
    }
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void denoise_atrous_kernel(AtrousArgs A) {
    const int tx = (int)(threadIdx.x & (kDenoiseTile - 1u)), ty = (int)(threadIdx.x / kDenoiseTile);
    uint32_t bx = blockIdx.x, by = blockIdx.y;
    if constexpr (!LDS && RT_DENOISE_XCD_BANDS) xcd_band_tile(bx, by);
    const int x0 = (int)bx * kT, y0 = (int)by * kT;
    const int x = x0 + tx, y = y0 + ty;
    if constexpr (LDS) {
        extern __shared__ float4 lds[];
        const int halo = 2 * A.step, pitch = kT + 2 * halo, n = pitch * pitch;  // denoise_lds_bytes: 32 B * n
        float4* ldv = lds;
        float4* lnz = lds + n;
        for (int k = (int)threadIdx.x; k < n; k += (int)kThreads) {
            const int ly = k / pitch, lx = k - ly * pitch;
            const int gx = x0 - halo + lx, gy = y0 - halo + ly;
            float4 dv = make_float4(0.0f, 0.0f, 0.0f, kNoCoverage), nz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if ((unsigned)gx < (unsigned)A.W && (unsigned)gy < (unsigned)A.H) {
                const size_t q = (size_t)gy * (size_t)A.W + (size_t)gx;
                dv = A.src[q];
                nz = A.normal_depth[q];
            }
            ldv[k] = dv;
            lnz[k] = nz;
        }
        __syncthreads();
        if (x >= A.W || y >= A.H) return;  // no barrier below
        const LdsTexels T{ldv, lnz, pitch, (ty + halo) * pitch + tx + halo};
        const float4 Tp = T.DV(0, 0);
        const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
        atrous_store(A, p, covered(Tp.w) ? atrous_pixel(T, Tp, T.NZ(0, 0), A) : Tp);
    } else {
        if (x >= A.W || y >= A.H) return;
        const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
        const GlobalTexels T{A.src, A.normal_depth, A.W, A.H, x, y};
        const float4 Tp = A.src[p];
        atrous_store(A, p, covered(Tp.w) ? atrous_pixel(T, Tp, A.normal_depth[p], A) : Tp);
    }
}

__global__ __launch_bounds__(kThreads) void denoise_prepare_kernel(const float4* color_a, const float4* color_b,
                                                                   const float4* albedo, float4* dst, int W, int H) {
    const int x = (int)blockIdx.x * kT + (int)(threadIdx.x & (kDenoiseTile - 1u));
    const int y = (int)blockIdx.y * kT + (int)(threadIdx.x / kDenoiseTile);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 a = color_a[p], b = color_b[p], al = albedo[p];
    const float ir = rcp_cr(fmaxf(al.x, kAlbedoFloor)), ig = rcp_cr(fmaxf(al.y, kAlbedoFloor)),
                ib = rcp_cr(fmaxf(al.z, kAlbedoFloor));
    const float ar = a.x * ir, ag = a.y * ig, ab = a.z * ib;
    const float br = b.x * ir, bg = b.y * ig, bb = b.z * ib;
    const float hl = (lum(ar, ag, ab) - lum(br, bg, bb)) * 0.5f;
    dst[p] = make_float4((ar + br) * 0.5f, (ag + bg) * 0.5f, (ab + bb) * 0.5f, al.w > 0.0f ? hl * hl : kNoCoverage);
}

__global__ __launch_bounds__(kThreads) void denoise_variance_kernel(const float4* src, float4* dst, int W, int H) {
    const int x = (int)blockIdx.x * kT + (int)(threadIdx.x & (kDenoiseTile - 1u));
    const int y = (int)blockIdx.y * kT + (int)(threadIdx.x / kDenoiseTile);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const GlobalTexels T{src, nullptr, W, H, x, y};
    float4 Tp = src[p];
    if (covered(Tp.w)) {
        float v9[9];
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int i = -1; i <= 1; ++i) v9[3 * (j + 1) + (i + 1)] = (i == 0 && j == 0) ? Tp.w : T.v(i, j);
        Tp.w = g3(v9);
    }
    dst[p] = Tp;
}

}  // namespace

hipError_t launch_denoise(const DenoiseParams& P, hipStream_t stream, LaunchInfo* info) {
    if (P.W <= 0 || P.H <= 0 || P.iterations == 0 || P.iterations > 6) return hipErrorInvalidValue;
    const dim3 grid(((uint32_t)P.W + kDenoiseTile - 1) / kDenoiseTile, ((uint32_t)P.H + kDenoiseTile - 1) / kDenoiseTile);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(denoise_prepare_kernel, grid, block, 0, stream, P.color_a, P.color_b, P.albedo, P.scratch[0],
                       P.W, P.H);
    hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, P.scratch[0], P.scratch[1], P.W, P.H);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if constexpr (denoise_lds_bytes(RT_DENOISE_LDS_MAX_STEP) > 64u * 1024u) {  // past the default limit of a launch
        static const hipError_t raised =
            hipFuncSetAttribute(reinterpret_cast<const void*>(&denoise_atrous_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)denoise_lds_bytes(RT_DENOISE_LDS_MAX_STEP));
        if (raised != hipSuccess) return raised;
    }
    AtrousArgs A{};
    A.normal_depth = P.normal_depth;
    A.color_a = P.color_a;
    A.color_b = P.color_b;
    A.albedo = P.albedo;
    A.out = P.out;
    A.W = P.W;
    A.H = P.H;
    A.normal_power_log2 = P.normal_power_log2;
    A.sigma_luminance = P.sigma_luminance;
    A.sigma_depth = P.sigma_depth;
    A.depth_floor = P.depth_floor;
    for (uint32_t it = 0; it < P.iterations; ++it) {
        const uint32_t step = 1u << it;
        A.src = P.scratch[(it + 1u) & 1u];
        A.dst = P.scratch[it & 1u];
        A.step = (int32_t)step;
        A.last = it + 1u == P.iterations ? 1u : 0u;
        const size_t lds = denoise_lds_bytes(step);
        if (lds)
            hipLaunchKernelGGL(denoise_atrous_kernel<true>, grid, block, lds, stream, A);
        else
            hipLaunchKernelGGL(denoise_atrous_kernel<false>, grid, block, 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (A.last && info)
            fill_launch_info(*info, 1, false, false, kThreads, grid, lds, "rt::denoise_atrous_kernel<%s>",
                             lds ? "true" : "false");
    }
    return hipSuccess;
}

}  // namespace rt
