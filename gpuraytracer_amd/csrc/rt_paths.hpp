// rt_paths.hpp — path-traced radiance along the caller's own rays
// (include/rtpt.h rt_trace_paths): included by rt_kernel.hip
// inside namespace rt after rt_counts.hpp, so that every existing kernel and
// launcher stays where it is.
//
// path_query_kernel is the render's bounce chain (shade, FusedChain,
// BounceChain) entered at bounce 0 with the closest hit of a ray the caller
// gives, in the chunked form of ray_query_kernel (rt_rays.hip):
//   * a workgroup stages its layout's records once (and the context's Halton
//     tables, box-cluster layout, when halton_tables_on) and loops over a
//     contiguous chunk of rays, NT / L rays per pass;
//   * per ray: the two 16-B halves, the exactness domain (rt_raydomain.h), and
//     the first segment once -- closest_hit without CULL and with the ray's own
//     tmin and tmax, the answer of rt_trace_rays.  As there, all 64 lanes stay
//     active through that query: a tail lane past n and a lane whose ray is
//     outside the domain run a copy of the wave's first in-domain ray and
//     discard the result;
//   * per sample n of [sample_base, sample_base + spp): i = seed + n, acc = 0,
//     thr = 1, and the chain from (id, t): FusedChain<0> where trace_path would
//     fuse, otherwise shade<0> and BounceChain<1>.  Bounce 0 is shaded without
//     COH (rt_kernel.hip shade): nothing is assumed about the coherence of a
//     wave's rays, and sv.cam_avail / sv.shd_avail stay false.  Dimensions 0
//     and 1 (the camera jitter) are not drawn;
//   * L = 1: one lane per ray adds its samples in order.  L = 16: the 16 lanes
//     of a DPP row share a ray, round r traces samples r * 16 + k, and the
//     row's leader adds them in order with row_sum_counts (rt_counts.hpp): the
//     count is spp for a ray with a first hit and 0 for every other one (past
//     n, outside the domain, a miss: its sum stays +0), so the 16 lanes of a
//     ray enter and leave every add together and no add reads another ray's
//     lane;
//   * radiance[r] = (sum / (float)spp, 1); a ray outside the domain gets
//     (0, 0, 0, 0) and first_hits[r] = (tmax bits, -1).
// A wave only touches the LDS slots of its own rays, so the ray loop needs no
// barrier and a wave past n leaves it alone.  No value taken from a ray or a
// seed is used as an index, and a ray's result does not depend on the grid
// shape or on the other rays of its wave.

namespace {

// The render's bounce chain from the closest hit (id, t) of s.o, s.d.
template <int B, int GEO, bool SPH, bool SMALL>
__device__ __forceinline__ void trace_from_hit(const KParams& P, const SceneView& sv, PathState& s, int id,
                                               float t) {
    if constexpr (B == 0) {
        return;
    } else if constexpr (geo_pairs(GEO) && !SPH && B > 1) {  // as trace_path
        FusedChain<0, B, GEO, SMALL, /*COH*/ false>::run(P, sv, s, id, t);
    } else {
        if (shade<0, B, GEO, SPH, SMALL, false, GEO == kGeoSphLds, /*COH*/ false>(P, sv, s, id, t))
            BounceChain<1, B, GEO, SPH, SMALL>::run(P, sv, s);
    }
}

constexpr int kPathMiss = -1, kPathUntraced = -2;  // a first segment without a hit

}  // namespace

template <int B, int GEO, bool SPH, bool SMALL, int L>
__global__ __launch_bounds__(block_threads(GEO), lockstep_min_waves(GEO, SPH))
void path_query_kernel(KParams P, const float4* __restrict__ rays, const uint32_t* __restrict__ seeds,
                       float4* __restrict__ radiance, uint2* __restrict__ hits, uint32_t n, uint32_t chunk,
                       uint64_t seed_key, RayDomain dom) {
    static_assert(L == 1 || L == 16, "the query forms: one lane or one DPP row per ray");
    constexpr uint32_t NT = block_threads(GEO), RPP = NT / L;  // rays per pass
    extern __shared__ float4 lds[];
    SceneView sv;
    __shared__ float sph_stash[GEO == kGeoSphLds ? 6 * kSphBlockThreads : 1];
    const bool tab = path_query_tables_on(GEO, SMALL, P.spp, L);  // halton_tables_on, inlined
    RT_LDS_GUARD(staged_end(GEO, P, tab));
    stage_scene<GEO, SPH, NT>(sv, P, lds, sph_stash, tab);

    // per ray, in LDS so that they are not live across the walks: seed +
    // sample_base, the first hit, and at L = 16 the running sum
    __shared__ uint32_t seed_s[RPP];
    __shared__ int id_s[RPP];
    __shared__ float t_s[RPP];
    __shared__ float lum_s[L > 1 ? 3 * RPP : 1];
    const uint32_t base = blockIdx.x * chunk;  // < n <= 2^31
    for (uint32_t p0 = 0; p0 < chunk; p0 += RPP) {
        if (base + p0 + (threadIdx.x & ~63u) / L >= n) break;  // wave-uniform: nothing left for this wave
        {
            const uint32_t slot = threadIdx.x / L, sub = threadIdx.x % L;
            const uint32_t i = base + p0 + slot;
            const bool live = i < n;
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
            if (live) {
                r0 = rays[2 * (size_t)i];
                r1 = rays[2 * (size_t)i + 1];
            }
            const f3 o{r0.x, r0.y, r0.z}, d{r1.x, r1.y, r1.z};
            const float tmin = r0.w, tmax = r1.w;
            const bool in = live && ray_in_domain(dom, o, d, tmin, tmax);
            float best = tmax;
            int id = in ? kPathMiss : kPathUntraced;
            const unsigned long long inmask = __builtin_amdgcn_ballot_w64(in);
            if (inmask != 0ull) {  // wave-uniform
                // the substitution of ray_query_kernel (rt_rays.hip), spelled out (tools/isa_diff.sh)
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)inmask) - 1);
                f3 qo{in ? o.x : lane_copy(o.x, src), in ? o.y : lane_copy(o.y, src), in ? o.z : lane_copy(o.z, src)};
                f3 qd{in ? d.x : lane_copy(d.x, src), in ? d.y : lane_copy(d.y, src), in ? d.z : lane_copy(d.z, src)};
                const float qtmin = in ? tmin : lane_copy(tmin, src);
                float qbest = in ? tmax : lane_copy(tmax, src);
                const int qid = closest_hit<GEO, SPH, /*CULL*/ false, 1>(sv, qo, qd, qtmin, &qbest);
                if (in && qid >= 0) {
                    best = qbest;
                    id = qid;
                }
            }
            if (sub == 0) {
                uint32_t sr;
                if (seeds) {
                    sr = live ? seeds[i] : 0u;
                } else {  // rt_fill_seeds' value for pixel i (fill_seeds_kernel)
                    uint64_t z = seed_key + i + 0x9E3779B97F4A7C15ULL;
                    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
                    sr = (uint32_t)(z ^ (z >> 31));
                }
                seed_s[slot] = (sr & 0xFFFFFu) + P.sample_base;
                id_s[slot] = id;
                t_s[slot] = best;
                if (L > 1) lum_s[3 * slot] = lum_s[3 * slot + 1] = lum_s[3 * slot + 2] = 0.0f;
                // a miss and an untraced ray: tmax, bit for bit
                if (hits && live) hits[i] = make_uint2(__float_as_uint(best), (uint32_t)(id >= 0 ? id : -1));
            }
        }
        f3 lum{0.0f, 0.0f, 0.0f};
        for (uint32_t r = 0; B > 0; ++r) {
            uint32_t t = threadIdx.x;
            asm volatile("" : "+v"(t));
            const uint32_t slot = t / L, sub = t % L;
            const int id = id_s[slot];
            const uint32_t cp = id >= 0 ? P.spp : 0u;  // the ray's L lanes hold the same count
            // wave-uniform: ceil(spp / L) rounds while a ray of the wave has a first hit
            if (__builtin_amdgcn_ballot_w64(r * L < cp) == 0ull) break;
            const uint32_t ns = r * L + sub;
            PathState s;
            s.acc = f3{0.0f, 0.0f, 0.0f};
            if (ns < cp) {  // per lane: no work past the ray's last sample
                const size_t i = (size_t)(base + p0 + slot);
                const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
                s.o = f3{r0.x, r0.y, r0.z};
                s.d = f3{r1.x, r1.y, r1.z};
                s.i = seed_s[slot] + ns;  // seed + (sample_base + n)
                s.thr = f3{1.0f, 1.0f, 1.0f};
                trace_from_hit<B, GEO, SPH, SMALL>(P, sv, s, id, t_s[slot]);
                if (L == 1) lum = lum + s.acc;
            }
            if (L > 1) {
                // every lane of the wave is here again: the L lanes of a ray take
                // each add of the sum together (row_sum_counts)
                uint32_t t2 = threadIdx.x;
                asm volatile("" : "+v"(t2));
                const uint32_t sub2 = t2 % L, slot2 = t2 / L;
                f3 acc{lum_s[3 * slot2], lum_s[3 * slot2 + 1], lum_s[3 * slot2 + 2]};
                row_sum_counts<L, 0>::run(acc, s.acc, r * L, id_s[slot2] >= 0 ? P.spp : 0u);
                if (sub2 == 0) {
                    lum_s[3 * slot2] = acc.x;
                    lum_s[3 * slot2 + 1] = acc.y;
                    lum_s[3 * slot2 + 2] = acc.z;
                }
            }
        }
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const uint32_t slot = t / L;
        const uint32_t i = base + p0 + slot;
        if (t % L == 0 && i < n) {
            if (L > 1) lum = f3{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
            const float fs = (float)P.spp;
            radiance[i] = id_s[slot] == kPathUntraced ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)
                                                      : make_float4(lum.x / fs, lum.y / fs, lum.z / fs, 1.0f);
        }
    }
}

namespace {

// Rays a workgroup traces: passes of NT / L rays, one pass while that still
// gives kPathGroups workgroups, eight at most (the staging is then shared by
// more rays).  A ray's result does not depend on it.
constexpr uint32_t kPathGroups = 2048, kPathPassesMax = 8;

template <int B, int GEO, bool SPH, bool SMALL, int L>
hipError_t launch_paths_tl(const KParams& P, const PathQueryArgs& A, hipStream_t stream) {
    constexpr uint32_t RPP = block_threads(GEO) / L;
    const uint64_t want = ((uint64_t)A.n + (uint64_t)RPP * kPathGroups - 1) / ((uint64_t)RPP * kPathGroups);
    const uint32_t passes = want > kPathPassesMax ? kPathPassesMax : (uint32_t)want;
    const uint32_t chunk = passes * RPP;
    const dim3 grid((uint32_t)(((uint64_t)A.n + chunk - 1) / chunk));
    const size_t lds_bytes =
        path_query_lds_bytes(GEO, P.nT, P.nP, P.nC, path_query_tables_on(GEO, SMALL, P.spp, (uint32_t)L));
    if (GEO == kGeoSphLds) {
        const hipError_t e = allow_lds((const void*)path_query_kernel<B, GEO, SPH, SMALL, L>, lds_bytes);
        if (e != hipSuccess) return e;
    }
    note_launch<B, GEO, SPH, SMALL, L>("path_query_kernel", P, grid, block_threads(GEO), lds_bytes);
    hipLaunchKernelGGL((path_query_kernel<B, GEO, SPH, SMALL, L>), grid, dim3(block_threads(GEO)), lds_bytes, stream,
                       P, A.rays, A.seeds, A.radiance, A.hits, A.n, chunk, A.seed_key, A.dom);
    return hipGetLastError();
}

// Lanes per ray.  Fixed-digit indices: 16 when asked for, or by the automatic
// rule (path_auto_lanes16, measured: profiles/r21/paths.md); one lane per ray
// otherwise, and always for the general Halton form.
template <int B, int GEO, bool SPH>
hipError_t launch_paths_h(const KParams& P, const PathQueryArgs& A, hipStream_t stream) {
    if (P.max_index < kSmallIndexMax) {
        const bool l16 = P.lanes == 16u || (P.lanes == 0u && path_auto_lanes16(P.spp, A.n));
        return l16 ? launch_paths_tl<B, GEO, SPH, true, 16>(P, A, stream)
                   : launch_paths_tl<B, GEO, SPH, true, 1>(P, A, stream);
    }
    return launch_paths_tl<B, GEO, SPH, false, 1>(P, A, stream);
}

}  // namespace

hipError_t launch_path_query(const KParams& P, const PathQueryArgs& A, uint32_t bounces, SceneMem mem,
                             hipStream_t stream, LaunchInfo* info) {
    if (!A.rays || !A.radiance || A.n == 0 || A.n > 0x80000000u || P.spp == 0) return hipErrorInvalidValue;
    const SceneTables T = tables_of(P);
    // the lockstep form of the context's layout, as a ray query takes it
    const int geo = ray_query_layout(choose_kernel(T, P.sph_lds != nullptr, bounces, mem, kWalkLockstep).layout);
    const hipError_t e = dispatch_bounces(bounces, [&](auto b) {
        return dispatch_layout(geo, P.nS, [&](auto g, auto sph) {
            return launch_paths_h<decltype(b)::value, decltype(g)::value, decltype(sph)::value>(P, A, stream);
        });
    });
    if (info) *info = g_last;
    return e;
}
