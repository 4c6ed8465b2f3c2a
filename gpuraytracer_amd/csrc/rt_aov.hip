// rt_aov.hip — first-hit feature buffers (include/rtpt.h rt_render_aov;
// DESIGN.md §3.22): what the camera rays of the beauty samples see.  For every
// pixel the kernel rebuilds the camera rays of pathTrace (seed + n, Halton
// dimensions 0 and 1, generateCameraRay), runs bounce 0's closest query of the
// path kernel on each (closest_hit<GEO, SPH, CULL> with the per-wave camera
// mask of the box-cluster layout, unchanged) and sums, in sample order,
//   albedo        (diffuse.rgb, 1)  of the primitive hit,
//   normal_depth  (N.xyz, t)        N: the triangle record's normal / the
//                                   sphere normal of shade(),
// a miss adding nothing; each sum is divided by (float)spp.  first_hit is
// (t, id) of the launch's first sample, a miss (tmax, -1) as rt_trace_rays.
//
//   * one lane per pixel: a wave is an 8x8 tile, a workgroup 2x2 waves in the
//     XCD-aware tile order of the render (rt_pixel.hpp);
//   * the workgroup stages its layout's records once (stage_records) and, when
//     every lane runs enough samples (halton_tables_on), the low-digit table
//     of Halton dimension 1: aov_lds_bytes (rt_kernel.hpp);
//   * N and diffuse come from the shading records of the render (tri_shade
//     rows 0-3, sph_shade), read on a hit only; buffers that are null (wave-
//     uniform, from the arguments) cost neither loads nor sums;
//   * one 16-B store per lane and colour buffer, 8 B for first_hit;
//   * the result of a pixel does not depend on the layout, the grid or the
//     other pixels of its wave: the query's answer is the id-ordered scan's
//      and the sums are per lane.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "rt_kernel.hpp"
#include "rt_halton.hpp"
#include "rt_beam.hpp"
#include "rt_pixel.hpp"
#include "rt_trace.hpp"
#include "rt_wavemask.hpp"

namespace rt {
namespace {

static_assert(tab_offset(1) == 0 && tab_offset(2) == kAovTabLdsFloats, "dimension 1's table comes first");

template <int GEO, bool SPH, bool SMALL>
__global__ __launch_bounds__(kBlockThreads) void aov_kernel(AovParams P) {
    constexpr uint32_t WR = 2, WC = 2, kWX = 8, kWY = 8;  // the render's L = 1 tiling
    extern __shared__ float4 lds[];
    SceneView sv;
    const SceneTables& T = P.tab;
    const bool center = (P.flags & kAovCenter) != 0u;
    if constexpr (geo_staged(GEO)) {  // aov_lds_bytes: the records, the box clusters, then the table
        stage_records<GEO, kBlockThreads>(lds, T);
        if constexpr (GEO == kGeoPairClu) {
            if (halton_tables_on(GEO, SMALL, P.spp, 1u)) {  // wave-uniform
                const StagedF4<uint32_t> n = staged_f4(GEO, T.nT, T.nP, T.nC);
                float* tab = reinterpret_cast<float*>(lds + n.rec + n.clu);
                fill_halton_table<1>(tab, threadIdx.x, kBlockThreads);
                sv.htab = tab;
            }
        }
        __syncthreads();
    }
    bind_scene<GEO, SPH>(sv, T, lds);

    uint32_t bx, by;
    xcd_tile(bx, by);
    if constexpr (RT_CAM_CAND && GEO == kGeoPairClu) {
        // The pairs this wave's camera rays can hit (rt_beam.hpp, DESIGN.md
        // §3.16), as in the render kernel's prologue: the footprint is the
        // wave's 8x8 pixel rectangle, lane k tests pair k and the ballot is the
        // mask.  Before any lane leaves: a ballot only sees active lanes.
        if (sv.nP - 1u < 32u) {  // wave-uniform: 1..32 pairs, else cluster_query
            const uint32_t wave = wave_uniform(threadIdx.x >> 6);
            const uint32_t wx0 = bx * (WR * kWX) + (wave % WR) * kWX;
            const uint32_t wj0 = by * (WC * kWY) + (wave / WR) * kWY;
            const Beam beam = wave_beam(P, wx0, wj0, kWX, kWY);
            // the camera mask of wave_masks_kernel, spelled out (tools/isa_diff.sh)
            const uint32_t k = threadIdx.x & 63u;
            const uint32_t kc = min(k, sv.nP - 1u);  // lanes past the last pair re-test it (discarded)
            const bool keep = !beam_excludes_pair(beam, reinterpret_cast<const float*>(sv.pair + kPairF4 * kc));
            sv.cam_mask = wave_uniform((uint32_t)__builtin_amdgcn_ballot_w64(k < sv.nP && keep));
            sv.cam_avail = true;
        }
    }
    uint32_t x, j;
    tile_pixel<1u, WR, WC>(threadIdx.x, bx, by, kWX, kWY, x, j);
    if (x >= (uint32_t)P.W || j >= P.row_count) return;  // no barrier below
    const uint32_t y = P.row_start + j * P.row_step;
    const size_t px = (size_t)j * (size_t)P.W + x;
    uint32_t seed = 0u;
    if (!center) seed = P.seeds[(size_t)y * (size_t)P.W + x] + P.sample_base;  // raytrace.metal:37

    const bool want_a = P.albedo != nullptr, want_n = P.normal_depth != nullptr;  // wave-uniform
    const f3 cu = ld_f3(P.cam_u), cv = ld_f3(P.cam_v), cw = ld_f3(P.cam_w);
    const float fW = (float)P.W, fH = (float)P.H, fx = (float)x, fy = (float)y;
    f3 sa{0.0f, 0.0f, 0.0f}, sn{0.0f, 0.0f, 0.0f};
    float sh = 0.0f, st = 0.0f;
    uint2 first = make_uint2(__float_as_uint(1000.0f), 0xFFFFFFFFu);  // a miss: tmax, bit for bit
    for (uint32_t n = 0; n < P.spp; ++n) {
        float jx = 0.5f, jy = 0.5f;
        if (!center) {  // wave-uniform
            const uint32_t i = seed + n;                                               // seed + (sample_base + n)
            jx = halton_dim<0, SMALL>(i);                                              // raytrace.metal:39-40
            jy = halton_dim<1, SMALL, GEO == kGeoPairClu>(i, sv.htab);
        }
        f3 d = camera_dir<GEO == kGeoTriBvh>(P, cu, cv, cw, fW, fH, fx, fy, jx, jy);
        f3 o = ld_f3(P.cam_pos);
        float t = 1000.0f;                                                             // sampling.metal:154-155
        const int id = closest_hit<GEO, SPH, true, 0>(sv, o, d, 0.001f, &t);          // bounce 0 of the path kernel
        if (id < 0) continue;  // a miss adds +0 to sums that are never -0: nothing
        if (n == 0) first = make_uint2(__float_as_uint(t), (uint32_t)id);
        if (!SPH || (uint32_t)id < sv.nT) {
            const float4* rec = P.tri_shade + 4 * id;
            if (want_a) {
                sa = sa + f3{rec[1].w, rec[2].w, rec[3].w};
                sh = sh + 1.0f;
            }
            if (want_n) {
                const float4 s0 = rec[0];
                sn = sn + f3{s0.x, s0.y, s0.z};
                st = st + t;
            }
        } else {
            const float4* rec = P.sph_shade + 3 * ((uint32_t)id - sv.nT);
            if (want_a) {
                const float4 s0 = rec[0];
                sa = sa + f3{s0.x, s0.y, s0.z};
                sh = sh + 1.0f;
            }
            if (want_n) {
                const float4 S = rec[2];
                sn = sn + normalize((o + d * t) - f3{S.x, S.y, S.z});  // shade()'s sphere normal
                st = st + t;
            }
        }
    }
    const float fs = (float)P.spp;
    if (want_a) P.albedo[px] = make_float4(sa.x / fs, sa.y / fs, sa.z / fs, sh / fs);
    if (want_n) P.normal_depth[px] = make_float4(sn.x / fs, sn.y / fs, sn.z / fs, st / fs);
    if (P.first_hit) P.first_hit[px] = first;
}

thread_local LaunchInfo g_last_aov;

template <int GEO, bool SPH, bool SMALL>
hipError_t launch_k(const AovParams& P, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid((P.W + kTile - 1) / kTile, (P.row_count + kTile - 1) / kTile);
    fill_launch_info(g_last_aov, 1, halton_tables_on(GEO, SMALL, P.spp, 1u), SMALL, kBlockThreads, grid, lds_bytes,
                     "rt::aov_kernel<%d, %s, %s>", GEO, SPH ? "true" : "false", SMALL ? "true" : "false");
    hipLaunchKernelGGL((aov_kernel<GEO, SPH, SMALL>), grid, dim3(kBlockThreads), lds_bytes, stream,
                       P);  // aov_lds_bytes of the layout
    return hipGetLastError();
}

template <int GEO, bool SPH>
hipError_t launch_h(const AovParams& P, hipStream_t stream) {
    const bool small = P.max_index < kSmallIndexMax;
    const size_t lds = aov_lds_bytes(GEO, P.tab.nT, P.tab.nP, P.tab.nC, halton_tables_on(GEO, small, P.spp, 1u));
    return small ? launch_k<GEO, SPH, true>(P, lds, stream) : launch_k<GEO, SPH, false>(P, lds, stream);
}

}  // namespace

hipError_t launch_aov(const AovParams& P, SceneMem mem, hipStream_t stream, LaunchInfo* info) {
    if (P.spp == 0 || P.W <= 0 || P.row_count == 0) return hipErrorInvalidValue;
    const KernelChoice kc = choose_kernel(P.tab, P.sph_compact != 0u, 3, mem, kWalkLockstep);
    const hipError_t e = dispatch_layout(ray_query_layout(kc.layout), P.tab.nS, [&](auto g, auto sph) {
        return launch_h<decltype(g)::value, decltype(sph)::value>(P, stream);
    });
    if (info) *info = g_last_aov;
    return e;
}

}  // namespace rt
