// rt_rays.hip — batched ray queries (include/rtpt.h rt_trace_rays): the exact
// closest-hit and any-hit queries of the render kernels (rt_trace.hpp
// closest_hit / any_hit, unchanged) for the caller's own rays, through the
// record layout and the acceleration structures of the context.
//
//   * a workgroup stages its layout's records in LDS once (pair or triangle
//     records, then the box clusters; no Halton tables) and loops over a
//     contiguous chunk of kRayChunk rays: a wave reads 64 consecutive rays
//     (2 KB) per pass, two 16-B loads per lane, and stores 8 B per hit;
//   * nothing is assumed about the coherence of a wave's rays: closest_hit
//     without CULL, any_hit without PACKET, no camera or shadow masks;
//   * rays inside the exactness domain (rt_raydomain.h) take
//     the accelerated layout.  Its walks decide their leaf rounds by ballots
//     and its cluster paths branch wave-uniformly, so all 64 lanes stay active
//     through it: a tail lane past n and a lane whose own ray is outside the
//     domain run a copy of the wave's first in-domain ray and discard the
//     result.  Every other ray then takes the id-ordered loop over the global
//     records (tri_test in id order; the spheres in leaf order, ranked by
//     (t, id) through sph_perm), which is what RT_RAYS_EXACT asks for every ray;
//   * the one limit of the accelerated layouts is theirs in the render kernels
//     too: a ray lying in an oblique triangle's plane to
//     rounding can be accepted on residues anywhere along the ray, where no
//     padded box bounds the hit; RT_RAYS_EXACT answers it like the scan;
//   * no value taken from a ray is used as an index, and the result of a ray
//     does not depend on the grid shape or on the other rays of its wave.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "rt_kernel.hpp"
#include "rt_trace.hpp"

namespace rt {
namespace {

// The id-ordered scan with strict '<'  over the global
// records: the definition of every answer.  ANY: *id >= 0 on the first
// accepted hit.  *best enters as the ray's tmax.
template <bool ANY>
__device__ __forceinline__ void exact_scan(const SceneTables& T, f3 o, f3 d, float tmin, float tmax,
                                           float* best, int* id) {
    for (uint32_t k = 0; k < T.nT; ++k) {
        float t;
        if (tri_test(T.tri_isect[3 * k], T.tri_isect[3 * k + 1], T.tri_isect[3 * k + 2], o, d, tmin, *best, &t)) {
            *id = (int)k;
            if (ANY) return;
            *best = t;
        }
    }
    const float a = dot(d, d);
    for (uint32_t k = 0; k < T.nS; ++k) {  // leaf order: ranked by (t, id)
        float t;
        if (sph_test(T.sph_isect[k], o, d, a, tmin, tmax, &t)) {
            if (ANY) {
                *id = 0;
                return;
            }
            const int sid = (int)(T.nT + T.sph_perm[k]);
            if (t < *best || (t == *best && sid < *id)) {
                *best = t;
                *id = sid;
            }
        }
    }
}

template <int GEO, bool SPH, bool ANY>
__global__ __launch_bounds__(kBlockThreads) void ray_query_kernel(RayQueryParams P) {
    extern __shared__ float4 lds[];
    SceneView sv;
    const SceneTables& T = P.tab;
    if constexpr (geo_staged(GEO)) {  // ray_query_lds_bytes: the records, then the box clusters
        stage_records<GEO, kBlockThreads>(lds, T);
        __syncthreads();
    }
    bind_scene<GEO, SPH>(sv, T, lds);

    const bool accel = (P.flags & kRaysExact) == 0u;
    const uint64_t base = (uint64_t)blockIdx.x * kRayChunk;
    for (uint32_t pass = 0; pass < kRayChunk / kBlockThreads; ++pass) {
        const uint64_t w0 = base + pass * kBlockThreads + (threadIdx.x & ~63u);
        if (w0 >= P.n) break;  // wave-uniform: nothing left for this wave (no barrier below)
        const uint64_t i = base + pass * kBlockThreads + threadIdx.x;
        const bool live = i < P.n;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (live) {
            r0 = P.rays[2 * (size_t)i];
            r1 = P.rays[2 * (size_t)i + 1];
        }
        const f3 o{r0.x, r0.y, r0.z}, d{r1.x, r1.y, r1.z};
        const float tmin = r0.w, tmax = r1.w;
        const bool in = live && accel && ray_in_domain(P.dom, o, d, tmin, tmax);
        float best = tmax;
        int id = -1;
        const unsigned long long inmask = __builtin_amdgcn_ballot_w64(in);
        if (inmask != 0ull) {  // wave-uniform
            // the substitution, spelled out here and in path_query_kernel: through a shared routine
            // every instantiation of both kernels compiles differently (tools/isa_diff.sh)
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)inmask) - 1);
            f3 qo{in ? o.x : lane_copy(o.x, src), in ? o.y : lane_copy(o.y, src), in ? o.z : lane_copy(o.z, src)};
            f3 qd{in ? d.x : lane_copy(d.x, src), in ? d.y : lane_copy(d.y, src), in ? d.z : lane_copy(d.z, src)};
            const float qtmin = in ? tmin : lane_copy(tmin, src);
            const float qtmax = in ? tmax : lane_copy(tmax, src);
            float qbest = qtmax;
            int qid = -1;
            if constexpr (!ANY) {
                qid = closest_hit<GEO, SPH, /*CULL*/ false>(sv, qo, qd, qtmin, &qbest);
            } else if constexpr (GEO == kGeoPairClu) {
                // any_hit's cluster query without the shade()-only rule for the light's own cluster
                cluster_query<true, true, false, false, false>(sv, qo, qd, qtmin, &qbest, &qid);
            } else {
                // the box of [o, o + d*tmax]: tmin >= 0 in the domain, so it bounds every acceptable point
                const f3 e = qo + qd * qtmax;
                const f3 lo{fminf(qo.x, e.x), fminf(qo.y, e.y), fminf(qo.z, e.z)};
                const f3 hi{fmaxf(qo.x, e.x), fmaxf(qo.y, e.y), fmaxf(qo.z, e.z)};
                qid = any_hit<GEO, SPH, /*PACKET*/ false>(sv, qo, qd, qtmin, qtmax, lo, hi) ? 0 : -1;
            }
            if (in) {
                best = qbest;
                id = qid;
            }
        }
        if (live && !in) exact_scan<ANY>(T, o, d, tmin, tmax, &best, &id);
        if (live) {
            uint2 h;
            if (ANY) {
                h.x = 0u;
                h.y = id >= 0 ? 1u : 0u;
            } else {
                h.x = id >= 0 ? __float_as_uint(best) : __float_as_uint(tmax);  // a miss: tmax, bit for bit
                h.y = (uint32_t)id;
            }
            P.hits[(size_t)i] = h;
        }
    }
}

thread_local LaunchInfo g_last_rays;

template <int GEO, bool SPH, bool ANY>
hipError_t launch_q(const RayQueryParams& P, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid((uint32_t)(((uint64_t)P.n + kRayChunk - 1) / kRayChunk));
    fill_launch_info(g_last_rays, 0, false, false, kBlockThreads, grid, lds_bytes, "rt::ray_query_kernel<%d, %s, %s>",
                     GEO, SPH ? "true" : "false", ANY ? "true" : "false");
    hipLaunchKernelGGL((ray_query_kernel<GEO, SPH, ANY>), grid, dim3(kBlockThreads), lds_bytes, stream,
                       P);  // ray_query_lds_bytes of the layout
    return hipGetLastError();
}

template <int GEO, bool SPH>
hipError_t launch_a(const RayQueryParams& P, size_t lds_bytes, hipStream_t stream) {
    return (P.flags & kRaysAny) ? launch_q<GEO, SPH, true>(P, lds_bytes, stream)
                                : launch_q<GEO, SPH, false>(P, lds_bytes, stream);
}

}  // namespace

hipError_t launch_ray_query(const RayQueryParams& P, SceneMem mem, hipStream_t stream, LaunchInfo* info) {
    if (P.n == 0 || P.n > 0x80000000u) return hipErrorInvalidValue;
    const KernelChoice kc = choose_kernel(P.tab, P.sph_compact != 0u, 3, mem, kWalkLockstep);
    const int geo = ray_query_layout(kc.layout);
    const size_t lds = ray_query_lds_bytes(geo, P.tab.nT, P.tab.nP, P.tab.nC);
    const hipError_t e = dispatch_layout(geo, P.tab.nS, [&](auto g, auto sph) {
        return launch_a<decltype(g)::value, decltype(sph)::value>(P, lds, stream);
    });
    if (info) *info = g_last_rays;
    return e;
}

}  // namespace rt
