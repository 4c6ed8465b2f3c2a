// rt_kernel.hip — gfx950 path-tracing kernel (the hot path) and its launcher.
//
// Rebuilds `kernel pathTrace` (RTrace/raytrace.metal:11-111) for CDNA4:
//   * the scene's intersection records (shared-edge triangle pairs, box
//     clusters) and the Halton low-digit tables are staged into LDS once per
//     workgroup; the sphere and triangle BVHs are read from global memory
//     (L2-resident); shading records are fetched from global only on a hit (the
//     box-cluster kernel knows a light from the launch's light mask,
//     DESIGN.md §3.21);
//   * L = 4 or 16 lanes per pixel: a wave traces 64/L pixels (a 4x4 or 2x2
//     tile, or one row of interleaved rows), lane `sub` traces samples
//     n = r*L + sub, and the colours are summed at the pixel's leader in
//     sample order (DPP row shifts or ds_bpermute) -- the additions of one
//     lane per pixel, so the result is unchanged;
//   * the bounce loop is unrolled at compile time (template B) so every Halton
//     dimension, hence every base, is a constant: the digit steps run in float
//     (floor(x*c), fma(q, -b, x): exact for indices < 3^13, rt_halton.hpp);
//   * camera constants are precomputed on the host once (same contract ops);
//   * the per-pixel result is one coalesced float4 / half4 / uchar4 store.
// Arithmetic follows the contract of rt_math.h / DESIGN.md §3 so the result is
// bit-identical to the CPU oracle.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <stddef.h>
#include <stdio.h>
#ifdef RT_LDS_CHECK
#include <hsa/hsa.h>
#endif

#include "rt_kernel.hpp"
#include "rt_halton.hpp"
#include "rt_beam.hpp"
#include "rt_shaft.hpp"
#include "rt_pixel.hpp"
#include "rt_trace.hpp"
#include "rt_wavemask.hpp"

namespace rt {

// -DRT_LDS_CHECK diagnostic builds: before staging, every kernel checks that
// the end of what its staging loops write (computed from the kernel's own
// loop bounds) lies within the dynamic LDS of its dispatch
// (hsa_kernel_dispatch_packet_t.group_segment_size, byte 28 = static +
// dynamic LDS).  A short allocation records the end in g_lds_overflow and the
// workgroup returns before writing anything; rt_render then fails with
// RT_ERR_LAUNCH (lds_check_result).  Production builds compile it out: the
// launcher requests staged_lds_bytes (rt_kernel.hpp), the same terms.
#ifdef RT_LDS_CHECK
__device__ uint32_t g_lds_overflow;
__device__ __forceinline__ bool lds_short(size_t end) {
    // word 7 (byte 28) of the AQL packet: group_segment_size (static_assert below)
    const uint32_t grp = ((const uint32_t*)__builtin_amdgcn_dispatch_ptr())[7];
    const size_t dyn = grp - __builtin_amdgcn_groupstaticsize();
    if (end <= dyn) return false;
    if (threadIdx.x == 0) atomicMax(&g_lds_overflow, (uint32_t)end);
    return true;
}
static_assert(offsetof(hsa_kernel_dispatch_packet_t, group_segment_size) == 28, "AQL packet layout");
#define RT_LDS_GUARD(end)            \
    do {                             \
        if (lds_short(end)) return;  \
    } while (0)
#else
#define RT_LDS_GUARD(end) ((void)0)
#endif
// The end a lockstep path kernel guards: its layout's records and clusters, and
// the Halton tables where its launcher's request holds them (`tables`: the
// render and the counts launchers request staged_lds_bytes, which has them for
// every box-cluster launch; the path query's only when the launch copies them).
__device__ __forceinline__ size_t staged_end(int geo, const KParams& P, bool tables) {
    const StagedF4<size_t> n = staged_f4<size_t>(geo, P.nT, P.nP, P.nC);
    return 16 * (n.rec + n.clu) + (tables ? 4 * (size_t)kHaltonTabLdsFloats : (size_t)0);
}

namespace {

// -DRT_CENSUS=k: VALU census builds of the box-cluster (Cornell) kernel
// (tools/census.sh).  Build k runs phase k a second time on opaque copies of
// its inputs (the compiler cannot reuse the first result) and discards the
// result through an opaque sink, under the same lanes and control flow: the
// SQ_INSTS_VALU difference to the plain build is the phase's dynamic VALU.
// 1 camera ray (Halton dims 0-1 + generateCameraRay), 2 closest-hit queries,
// 3 shadow queries, 4 Halton dims 2-5 of the bounces, 5 the rest of the
// shading arithmetic (light sample, NEE term, cosine direction), 6 the
// in-order pixel sums.  Timing-invalid by construction; never shipped.
#ifndef RT_CENSUS
#define RT_CENSUS 0
#endif
template <typename T>
__device__ __forceinline__ T cz(T v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ f3 cz(f3 v) { return f3{cz(v.x), cz(v.y), cz(v.z)}; }
__device__ __forceinline__ void cz_sink(float v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void cz_sink(f3 v) {
    cz_sink(v.x);
    cz_sink(v.y);
    cz_sink(v.z);
}

struct PathState {
    f3 o, d, acc, thr;
    uint32_t i;  // Halton index seed + n
};

// One bounce b of raytrace.metal:47-101.  Returns false when the path ends.
// Shading of a hit (id, t) at bounce b: raytrace.metal:55-101.  Returns false
// when the path ends (light hit).
// FUSE (pair layout, triangles only): the shadow query of bounce b and the
// closest hit of bounce b+1 run as one pass over the records
// (fused_shadow_closest); the next hit is returned in *nid / *nt.
// STASH (the one-wave sphere kernel): contrib and the next direction wait in
// the per-lane LDS stash sv.xstash across the shadow walk.
// COH: the wave's rays are the coherent camera rays of a tile, the render
// kernels' bounce 0: the triangle BVH's shadow query walks as a wave packet
// and keeps every lane.  The path-query kernel (rt_paths.hpp) shades the
// caller's rays at bounce 0 without it.
template <int b, int B, int GEO, bool SPH, bool SMALL, bool FUSE = false, bool STASH = false,
          bool COH = (b == 0)>
__device__ __forceinline__ bool shade(const KParams& P, const SceneView& sv, PathState& s, int id,
                                      float t, int* nid = nullptr, float* nt = nullptr) {
    f3 N, right, fwd, diffuse;
    // The box-cluster kernel (at most 31 pairs, ids < 62): the
    // light flag is bit id of the launch's light mask (one 64-bit shift), so
    // the gather of the record does not wait for a first load of its flag
    // word: a light lane reads its emissive row and ends, the others the
    // three other rows and the last colour word in one stage.
    if constexpr (GEO == kGeoPairClu && !SPH) {
        if ((P.light_mask >> (uint32_t)id) & 1ull) {        // :57-60 light: overwrite, stop
            const float4 s3 = P.tri_shade[4 * id + 3];
            s.acc = f3{s3.x, s3.y, s3.z};
            return false;
        }
        const float4* sh = P.tri_shade + 4 * id;
        const float4 s0 = sh[0], s1 = sh[1], s2 = sh[2];
        N = f3{s0.x, s0.y, s0.z};
        right = f3{s1.x, s1.y, s1.z};
        fwd = f3{s2.x, s2.y, s2.z};
        diffuse = f3{s1.w, s2.w, sh[3].w};
    } else if (!SPH || (uint32_t)id < sv.nT) {
        const float4* sh = P.tri_shade + 4 * id;
        const float4 s0 = sh[0];
        const float4 s3 = sh[3];
        if (s0.w != 0.0f) {                                 // :57-60 light: overwrite, stop
            s.acc = f3{s3.x, s3.y, s3.z};
            return false;
        }
        const float4 s1 = sh[1], s2 = sh[2];
        N = f3{s0.x, s0.y, s0.z};
        right = f3{s1.x, s1.y, s1.z};
        fwd = f3{s2.x, s2.y, s2.z};
        diffuse = f3{s1.w, s2.w, s3.w};
    } else {
        const uint32_t k = (uint32_t)id - sv.nT;
        const float4* sh = P.sph_shade + 3 * k;
        const float4 s0 = sh[0];
        if (s0.w != 0.0f) {
            const float4 s1 = sh[1];
            s.acc = f3{s1.x, s1.y, s1.z};
            return false;
        }
        const float4 S = sh[2];
        N = normalize((s.o + s.d * t) - f3{S.x, S.y, S.z});
        shading_frame(N, &right, &fwd);
        diffuse = f3{s0.x, s0.y, s0.z};
    }
    f3 p = (s.o + s.d * t) + N * 1e-3f;              // :67

#if RT_CENSUS == 4
    {
        const uint32_t i2 = cz(s.i);
        float h = halton_dim<2 + 5 * b, SMALL, GEO == kGeoPairClu>(i2, sv.htab) +
                  halton_dim<3 + 5 * b, SMALL, GEO == kGeoPairClu>(i2, sv.htab);
        if (b + 1 < B)
            h = h + halton_dim<4 + 5 * b, SMALL, GEO == kGeoPairClu>(i2, sv.htab) +
                halton_dim<5 + 5 * b, SMALL, GEO == kGeoPairClu>(i2, sv.htab);
        cz_sink(h);
    }
#endif
    // sampleAreaLight (sampling.metal:198-236), dims 2+5b, 3+5b (:72-74)
    const float ux = halton_dim<2 + 5 * b, SMALL, GEO == kGeoPairClu>(s.i, sv.htab) * 2.0f - 1.0f;
    const float uy = halton_dim<3 + 5 * b, SMALL, GEO == kGeoPairClu>(s.i, sv.htab) * 2.0f - 1.0f;
#if RT_CENSUS == 5
    {
        const f3 o2 = cz(s.o), dd = cz(s.d), N2 = cz(N), r2 = cz(right), f2 = cz(fwd), df = cz(diffuse);
        const float t2 = cz(t), ux2 = cz(ux), uy2 = cz(uy);
        const f3 p2 = (o2 + dd * t2) + N2 * 1e-3f;
        const f3 q2 = (ld_f3(P.light_center) + f3{0.25f, 0.0f, 0.0f} * ux2) + f3{0.0f, 0.0f, 0.25f} * uy2;
        f3 L2 = q2 - p2;
        const float dist2 = length(L2);
        const float inv2 = 1.0f / fmaxf(dist2, 1e-3f);
        L2 = L2 * inv2;
        f3 lc2 = ld_f3(P.light_color) * (inv2 * inv2);
        lc2 = lc2 * saturate(dot(-L2, f3{0.0f, -1.0f, 0.0f}));
        lc2 = lc2 * saturate(dot(N2, L2));
        const f3 c2 = lc2 * (cz(s.thr) * df);
        cz_sink(c2);
        cz_sink(f3{fminf(p2.x, q2.x), fminf(p2.y, q2.y), fminf(p2.z, q2.z)});
        cz_sink(f3{fmaxf(p2.x, q2.x), fmaxf(p2.y, q2.y), fmaxf(p2.z, q2.z)});
        if (b + 1 < B) {
            float sp2, cp2;
            sincos_pt(6.28318548f * cz(ux), &sp2, &cp2);
            const float ct2 = sqrtf(cz(uy));
            const float st2 = sqrtf(1.0f - ct2 * ct2);
            cz_sink((r2 * (st2 * cp2) + N2 * ct2) + f2 * (st2 * sp2));
        }
    }
#endif
    const f3 lcen = ld_f3(P.light_center);
    // q = center + (0.25,0,0)*ux + (0,0,0.25)*uy (sampling.metal:208-213).  The
    // zero terms (0*ux, 0*uy: +-0, ux and uy are finite and never -0) drop out
    // exactly: lcen.x + 0.25ux is never -0, so adding +-0 keeps it, and
    // lcen.y (lcen.z) + +-0 is lcen.y (lcen.z) unless that is -0 -- the
    // host's light_plain flag; otherwise the literal form
    f3 q;
    if (P.light_plain)
        q = f3{lcen.x + 0.25f * ux, lcen.y, lcen.z + 0.25f * uy};
    else
        q = (lcen + f3{0.25f, 0.0f, 0.0f} * ux) + f3{0.0f, 0.0f, 0.25f} * uy;
    f3 L = q - p;
    // the short correctly rounded forms (rt_math.h) except in the triangle-BVH
    // kernel, where their uniform branches cost spills (scratch 16 -> 36 B)
    constexpr bool CR = GEO != kGeoTriBvh;
    const float dist = CR ? length(L) : length_ieee(L);
    const float inv = CR ? rcp_cr(fmaxf(dist, 1e-3f)) : 1.0f / fmaxf(dist, 1e-3f);
    L = L * inv;
    f3 lc = ld_f3(P.light_color) * (inv * inv);
    // dot(-L, (0,-1,0)) = fma(-L.z, 0, fma(-L.y, -1, -L.x * 0)) is L.y exactly
    // when L.y != 0; when L.y is +-0 either form gives a zero, which makes the
    // light term zero (no shadow query, +0 added: the same result)
    lc = lc * saturate(L.y);
    lc = lc * saturate(dot(N, L));                         // :75
    s.thr = s.thr * diffuse;                               // :76
    // the light term lc * throughput (:87-89) and the next direction (:93-100)
    // are formed BEFORE the shadow query: the same operations, but the shading
    // frame N/right/fwd and lc are dead during the walk (6-9 fewer live VGPRs)
    const f3 contrib = lc * s.thr;
    const f3 seg_lo{fminf(p.x, q.x), fminf(p.y, q.y), fminf(p.z, q.z)};
    const f3 seg_hi{fmaxf(p.x, q.x), fmaxf(p.y, q.y), fmaxf(p.z, q.z)};
    f3 d2{0.0f, 0.0f, 0.0f};
    if (b + 1 < B) {                                       // last direction never traced
        const float cu = halton_dim<4 + 5 * b, SMALL, GEO == kGeoPairClu>(s.i, sv.htab);           // :93-94
        const float cv = halton_dim<5 + 5 * b, SMALL, GEO == kGeoPairClu>(s.i, sv.htab);
        float sp, cp;
        sincos_pt(6.28318548f * cu, &sp, &cp);             // sampling.metal:40-48
        const float ct = CR ? sqrt_cr(cv) : sqrtf(cv);
        const float st = CR ? sqrt_cr(1.0f - ct * ct) : sqrtf(1.0f - ct * ct);
        d2 = (right * (st * cp) + N * ct) + fwd * (st * sp);  // sampling.metal:65
    }
    if (FUSE && b + 1 < B) {
        const FusedHit h = fused_shadow_closest(sv, p, L, dist - 1e-3f, seg_lo, seg_hi, d2);
        if (!h.occluded) s.acc = s.acc + contrib;          // :79-89
        s.d = d2;
        s.o = p;                                           // :99-100
        *nid = h.id;
        *nt = h.t;
        return true;
    }
    // A zero light term (the light behind the surface or behind its own plane,
    // a black material) adds +0 to acc whatever the shadow query says: acc is a
    // sum of non-negative terms starting at +0, so acc + 0 == acc bit for bit,
    // and such lanes skip the query (whole waves do, e.g. camera rays on the
    // ceiling): Cornell +4.3 %, 1000 spheres +1.8 %, 100k triangles +2.5 %.
    // Bounce-0 shadow rays of the triangle BVH walk as wave packets and keep
    // every lane (skipping there: 100k triangles -8 %).
    const bool lit = (GEO == kGeoTriBvh && COH) || contrib.x != 0.0f || contrib.y != 0.0f ||
                     contrib.z != 0.0f;
    if constexpr (STASH) {
        // the sphere kernel parks contrib and the next direction in a per-lane
        // LDS stash across the shadow walk (read back through an opaque lane
        // index, so they are not kept in registers): at 64 VGPRs (8 waves/SIMD)
        // they were 5-6 spilled VGPRs, 24-28 B of scratch per lane (round 4)
        constexpr uint32_t SS = kSphBlockThreads;  // stash stride
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        float* st = sv.xstash;
        st[t] = contrib.x;
        st[SS + t] = contrib.y;
        st[2 * SS + t] = contrib.z;
        if (b + 1 < B) {
            st[3 * SS + t] = d2.x;
            st[4 * SS + t] = d2.y;
            st[5 * SS + t] = d2.z;
        }
        const bool occluded =
            lit && any_hit<GEO, SPH, COH && !SPH>(sv, p, L, 0.0f, dist - 1e-3f, seg_lo, seg_hi);  // :79-85
        uint32_t t2 = threadIdx.x;
        asm volatile("" : "+v"(t2));
        if (lit && !occluded)                              // :87-89
            s.acc = s.acc + f3{st[t2], st[SS + t2], st[2 * SS + t2]};
        if (b + 1 < B) {
            s.d = f3{st[3 * SS + t2], st[4 * SS + t2], st[5 * SS + t2]};
            s.o = p;                                       // :99-100
        }
        return true;
    }
#if RT_CENSUS == 3
    if (lit) {
        f3 p2 = cz(p), L2 = cz(L);
        cz_sink(any_hit<GEO, SPH, COH && !SPH>(sv, p2, L2, 0.0f, cz(dist) - 1e-3f, cz(seg_lo), cz(seg_hi)) ? 1.0f
                                                                                                            : 0.0f);
    }
#endif
    if (lit && !any_hit<GEO, SPH, COH && !SPH>(sv, p, L, 0.0f, dist - 1e-3f, seg_lo, seg_hi))  // :79-85
        s.acc = s.acc + contrib;                           // :87-89
    if (b + 1 < B) {
        s.d = d2;
        s.o = p;                                           // :99-100
    }
    return true;
}

// One bounce b of raytrace.metal:47-101.  Returns false when the path ends.
// The triangle-BVH kernel runs WITHOUT the LDS stash of shade(): with it the
// kernel has no scratch (63 VGPRs) but ran 778 vs 846 Msamples/s on 100k
// triangles (round 5, profiles/r5/ab_results.md); without it 18 VGPRs spill
// (16 B of scratch per lane, L2-resident)
template <int b, int B, int GEO, bool SPH, bool SMALL>
__device__ __forceinline__ bool bounce(const KParams& P, const SceneView& sv, PathState& s) {
    float t = 1000.0f;                                      // max_distance (sampling.metal:155)
    // Camera rays of an 8x8 tile are coherent: cull with their segment boxes.
    const int id = closest_hit<GEO, SPH, b == 0, (b == 0 ? 0 : 1)>(sv, s.o, s.d, 0.001f, &t);  // min_distance :154
#if RT_CENSUS == 2
    {
        f3 o2 = cz(s.o), d2 = cz(s.d);
        float t2 = cz(1000.0f);
        const int id2 = closest_hit<GEO, SPH, b == 0, (b == 0 ? 0 : 1)>(sv, o2, d2, 0.001f, &t2);
        cz_sink(t2 + (float)id2);
    }
#endif
    if (id < 0) return false;                               // :51-53
    return shade<b, B, GEO, SPH, SMALL, false, GEO == kGeoSphLds>(P, sv, s, id, t);
}

template <int b, int B, int GEO, bool SPH, bool SMALL>
struct BounceChain {
    __device__ __forceinline__ static void run(const KParams& P, const SceneView& sv,
                                               PathState& s) {
#ifdef RT_STATS
        if constexpr (!SPH && GEO != kGeoTriBvh) {  // slots 16-31: the per-lane BVH walks' otherwise
            // lane-slot accounting of the triangle kernels (tools/kernel_stats.py):
            // shader-clock cycles of this bounce per wave, and the same weighted
            // by the lanes whose path is still alive when it starts (16+b, 20+b)
            const unsigned long long t0 = clock64();
            const unsigned long long live = (unsigned long long)__popcll(__ballot(1));
            const bool ok = bounce<b, B, GEO, SPH, SMALL>(P, sv, s);
            const unsigned long long dt = clock64() - t0;
            RT_STAT(16 + b, dt);
            RT_STAT(20 + b, dt * live);
            if (!ok) return;
            BounceChain<b + 1, B, GEO, SPH, SMALL>::run(P, sv, s);
            return;
        }
#endif
        if (!bounce<b, B, GEO, SPH, SMALL>(P, sv, s)) return;
        BounceChain<b + 1, B, GEO, SPH, SMALL>::run(P, sv, s);
    }
};
template <int B, int GEO, bool SPH, bool SMALL>
struct BounceChain<B, B, GEO, SPH, SMALL> {
    __device__ __forceinline__ static void run(const KParams&, const SceneView&, PathState&) {}
};

// Fused bounce chain: enters bounce b with the closest hit (id, t) of its ray.
template <int b, int B, int GEO, bool SMALL, bool COH = (b == 0)>
struct FusedChain {
    __device__ __forceinline__ static void run(const KParams& P, const SceneView& sv,
                                               PathState& s, int id, float t) {
        int nid = -1;
        float nt = 0.0f;
        if (!shade<b, B, GEO, false, SMALL, true, false, COH>(P, sv, s, id, t, &nid, &nt)) return;
        if (b + 1 < B && nid >= 0) FusedChain<b + 1, B, GEO, SMALL>::run(P, sv, s, nid, nt);
    }
};
template <int B, int GEO, bool SMALL, bool COH>
struct FusedChain<B, B, GEO, SMALL, COH> {
    __device__ __forceinline__ static void run(const KParams&, const SceneView&, PathState&, int,
                                               float) {}
};

// The pair layouts (triangles only) fuse the shadow query of bounce b with the
// closest hit of bounce b + 1 (fused_shadow_closest).  The box-cluster kernel
// does not: its fused candidate rounds measured 5 % slower on Cornell 1080p
// (DESIGN.md §5).
template <int B, int GEO, bool SPH, bool SMALL>
__device__ __forceinline__ void trace_path(const KParams& P, const SceneView& sv, PathState& s) {
    if (geo_pairs(GEO) && !SPH && B > 1) {
        float t = 1000.0f;                                  // sampling.metal:155
        const int id = closest_hit<GEO, false, true, 0>(sv, s.o, s.d, 0.001f, &t);
        if (id >= 0) FusedChain<0, B, GEO, SMALL>::run(P, sv, s, id, t);
    } else {
        BounceChain<0, B, GEO, SPH, SMALL>::run(P, sv, s);
    }
}

// In-order sum of the L colours of a pixel's lanes at its group leader, with
// DPP row shifts (row_shl:k: lane i reads lane i + k of its 16-lane row).  The
// sphere kernel keeps ds_bpermute shuffles (its DPP form spilled 3 more VGPRs:
// 2,715 vs 2,724 Msamples/s).
template <int k>
__device__ __forceinline__ float row_shl(float v) {
    if constexpr (k == 0) {
        return v;
    } else {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + k, 0xF, 0xF, false));
    }
}
template <int L, int k>
struct row_sum_in_order {
    __device__ __forceinline__ static void run(f3& acc, f3 c, uint32_t n0, uint32_t spp) {
        if (n0 + (uint32_t)k < spp)  // wave-uniform: the round's last samples may be past spp
            acc = acc + f3{row_shl<k>(c.x), row_shl<k>(c.y), row_shl<k>(c.z)};
        row_sum_in_order<L, k + 1>::run(acc, c, n0, spp);
    }
};
template <int L>
struct row_sum_in_order<L, L> {
    __device__ __forceinline__ static void run(f3&, f3, uint32_t, uint32_t) {}
};

// The pixel store (raytrace.metal:109): float4(luminance, 1) as rgba32F, as
// the reference's rgba16F texture (renderer.swift:74-82), or that texture
// tonemapped to the reference's 8-bit image (RTrace/image.swift:35-65: fp16
// read-back, then rt::tonemap_channel) -- 16, 8 or 4 bytes, one store.
__device__ __forceinline__ void store_pixel(const KParams& P, size_t o, float r, float g, float b) {
    if (P.flags & kOutRgba8) {
        const uint8_t cr = tonemap_channel(__half2float(__float2half_rn(r)));
        const uint8_t cg = tonemap_channel(__half2float(__float2half_rn(g)));
        const uint8_t cb = tonemap_channel(__half2float(__float2half_rn(b)));
        reinterpret_cast<uchar4*>(P.out)[o] = make_uchar4(cr, cg, cb, 255);
    } else if (P.flags & kOutFp16) {
        ushort4 h;
        h.x = __half_as_ushort(__float2half_rn(r));
        h.y = __half_as_ushort(__float2half_rn(g));
        h.z = __half_as_ushort(__float2half_rn(b));
        h.w = __half_as_ushort(__float2half_rn(1.0f));
        reinterpret_cast<ushort4*>(P.out)[o] = h;
    } else {
        reinterpret_cast<float4*>(P.out)[o] = make_float4(r, g, b, 1.0f);
    }
}

// The end of a pixel (raytrace.metal:106-109): its running sum to P.sum, the
// mean over all samples so far to the image.
__device__ __forceinline__ void finish_pixel(const KParams& P, size_t o, f3 lum) {
    if (P.sum) P.sum[o] = make_float4(lum.x, lum.y, lum.z, (float)P.samples_total);
    if (P.out) {
        const float fs = (float)P.samples_total;                 // :106
        const float r = lum.x / fs, g = lum.y / fs, bl = lum.z / fs;
        store_pixel(P, o, r, g, bl);
    }
}

// ---- sorted-path variant ----------------------------------------------------
// Between bounces the 256 paths of a workgroup are counting-sorted through LDS
// by the octant of their next direction, dead paths last (9 buckets).  Waves
// then hold live rays of one octant: the wave-level segment culling of
// closest_hit works for bounce rays too, and finished paths no longer idle
// lanes.  Each path carries its owner pixel; at the end of a sample every path
// hands its accumulatedColor to its owner through LDS, and the owner adds it
// to its running sum in sample order n = 0, 1, ... exactly as before.
constexpr uint32_t kSortBuckets = 9;
// LDS layout of the sorted kernel: fixed offsets (in float4) from the dynamic
// LDS base, scene records after them.
constexpr uint32_t kSortA = 0;                            // (o.xyz, thr.x)   [256]
constexpr uint32_t kSortB = kBlockThreads;                // (d.xyz, thr.y)   [256]
constexpr uint32_t kSortC = 2 * kBlockThreads;            // (acc.xyz, thr.z) [256]
constexpr uint32_t kSortD = 3 * kBlockThreads;            // uint2 (i, owner)  [256]
constexpr uint32_t kSortLum = kSortD + kBlockThreads / 2;  // float sum x[256], y[256], z[256]
constexpr uint32_t kSortCnt = kSortLum + 3 * kBlockThreads / 4;  // uint [bucket][wave]
constexpr uint32_t kSortF4 = kSortCnt + (kSortBuckets * 4 + 3) / 4;

__device__ __forceinline__ uint32_t sort_octant(f3 d) {
    return (d.x > 0.0f ? 4u : 0u) | (d.y > 0.0f ? 2u : 0u) | (d.z > 0.0f ? 1u : 0u);
}

// Counting sort of the workgroup's live paths by the octant of their next
// direction (buckets 0-7); dead paths (bucket 8) are dropped — they have
// already handed their colour to their pixel.  All 256 threads must call it
// (two barriers).  Afterwards lanes tid < n_live hold a path: o, d, i and owner
// are reloaded here, thr/acc later by load_thr_acc (same slot, valid until the
// next sort), which keeps them out of registers during the intersection loops.
__device__ __forceinline__ void sort_paths(float4* lds, PathState& s, uint32_t& owner,
                                           bool& alive) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t* counts = reinterpret_cast<uint32_t*>(lds + kSortCnt);
    const uint32_t key = alive ? sort_octant(s.d) : 8u;
    uint32_t my_count = 0, slot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSortBuckets - 1; ++k) {
        const unsigned long long m = __ballot(key == k);
        if (lane == k) my_count = (uint32_t)__popcll(m);
        if (key == k) slot = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    }
    if (lane < kSortBuckets - 1) counts[lane * 4u + wave] = my_count;
    __syncthreads();
    // Exclusive scan of the 32 counts in (bucket, wave) order, redundantly in
    // every wave (lanes 32-63 repeat lanes 0-31): entry (key, wave) is where
    // this wave's paths of bucket `key` start.
    const uint32_t idx = lane & 31u;
    const uint32_t c = counts[idx];
    uint32_t v = c;
#pragma unroll
    for (uint32_t off = 1; off < 32; off <<= 1) {
        const uint32_t t = __shfl_up(v, off);
        if (idx >= off) v += t;
    }
    const uint32_t live = __shfl(v, 31);
    slot += __shfl(v - c, (int)(key * 4u + wave));
    if (alive) {
        lds[kSortA + slot] = make_float4(s.o.x, s.o.y, s.o.z, s.thr.x);
        lds[kSortB + slot] = make_float4(s.d.x, s.d.y, s.d.z, s.thr.y);
        lds[kSortC + slot] = make_float4(s.acc.x, s.acc.y, s.acc.z, s.thr.z);
        reinterpret_cast<uint2*>(lds + kSortD)[slot] = make_uint2(s.i, owner);
    }
    // thr/acc now live in LDS only (reloaded by load_thr_acc): end their
    // register live ranges here.
    s.thr = f3{0.0f, 0.0f, 0.0f};
    s.acc = f3{0.0f, 0.0f, 0.0f};
    __syncthreads();
    alive = tid < live;
    if (alive) {
        const float4 a = lds[kSortA + tid], bq = lds[kSortB + tid];
        const uint2 dd = reinterpret_cast<const uint2*>(lds + kSortD)[tid];
        s.o = f3{a.x, a.y, a.z};
        s.d = f3{bq.x, bq.y, bq.z};
        s.i = dd.x;
        owner = dd.y;
    }
}

__device__ __forceinline__ void load_thr_acc(const float4* lds, PathState& s) {
    const uint32_t tid = threadIdx.x;
    const float4 c = lds[kSortC + tid];
    s.thr = f3{lds[kSortA + tid].w, lds[kSortB + tid].w, c.w};
    s.acc = f3{c.x, c.y, c.z};
}

// A finished path adds its accumulatedColor to its pixel's running sum in LDS
// (raytrace.metal:103).  Each pixel gets exactly one path per sample and
// samples are separated by barriers, so the additions keep the order n.
__device__ __forceinline__ void deliver(float4* lds, uint32_t owner, f3 acc) {
    float* sum = reinterpret_cast<float*>(lds + kSortLum);
    sum[owner] = sum[owner] + acc.x;
    sum[kBlockThreads + owner] = sum[kBlockThreads + owner] + acc.y;
    sum[2 * kBlockThreads + owner] = sum[2 * kBlockThreads + owner] + acc.z;
}

// GEO: kGeoPairLds (pair records in LDS, wave-culled loops), kGeoTriBvh
// (triangle BVH: camera rays as wave packets, bounce rays per lane) or
// kGeoSphLds (the room's pairs in LDS + the leaf-box sphere BVH).  For the BVH
// scenes the sort is what the lockstep kernels lack: the waves of a bounce
// walk rays of ONE direction octant, i.e. ONE of the eight BVH layouts.
template <int b, int B, int GEO, bool SPH, bool SMALL>
struct SortedChain {
    __device__ __forceinline__ static void run(const KParams& P, const SceneView& sv, float4* lds,
                                               PathState& s, uint32_t& owner, bool& alive) {
        if (b > 0) sort_paths(lds, s, owner, alive);
        if (alive) {
            float t = 1000.0f;                                   // sampling.metal:154-155
            constexpr bool cull = GEO == kGeoTriBvh ? b == 0 : true;
            const int id = closest_hit<GEO, SPH, cull, (b == 0 ? 0 : 1)>(sv, s.o, s.d, 0.001f, &t);
            if (b > 0) load_thr_acc(lds, s);
            alive = id >= 0 && shade<b, B, GEO, SPH, SMALL>(P, sv, s, id, t);
            if (!alive || b + 1 == B) deliver(lds, owner, s.acc);
        }
        SortedChain<b + 1, B, GEO, SPH, SMALL>::run(P, sv, lds, s, owner, alive);
    }
};
template <int B, int GEO, bool SPH, bool SMALL>
struct SortedChain<B, B, GEO, SPH, SMALL> {
    __device__ __forceinline__ static void run(const KParams&, const SceneView&, float4*,
                                               PathState&, uint32_t&, bool&) {}
};


}  // namespace

constexpr int kMinWavesPerEu = 8;     // 8 waves/SIMD (<= 64 VGPRs): +4.5% measured over 7
constexpr int kMinWavesPerEuSph = 8;  // sphere kernel: 7 / 6 waves 162.2 / 176.3 ms vs 154.3
// box-cluster kernel: 7 waves/SIMD runs as fast as 8 and spills 6 VGPRs
// instead of 30 (HBM traffic 146 MB instead of 19 GB per 1080p launch)
#ifndef RT_CLU_WAVES
#define RT_CLU_WAVES 7
#endif
constexpr int kMinWavesPerEuClu = RT_CLU_WAVES;
// L lanes per pixel (1, 4 or 16: more lanes when the launch has few pixels,
// e.g. one GPU's share of a multi-GPU frame): lane `sub` of a pixel's
// group traces samples n = r*L + sub of round r, and after every round the L
// colours are shuffled within the wave and added to the pixel's sum in sample
// order n — the same sequence of fp32 additions as one lane per pixel.
// Workgroup size: one wave for the sphere kernel (rt_kernel.hpp
// kSphBlockThreads), 256 threads (2x2 waves) otherwise -- the box-cluster
// kernel at 128 / 64 / 512 threads ran 40.1 / 68.9 / 27.8 ms vs 26.2 (its 22 KB
// of Halton tables per workgroup then cap the waves per CU), the
// triangle-BVH kernel at 64 / 128 threads 204.3 / 192.1 ms vs 180.7.
constexpr uint32_t block_threads(int geo) { return geo == kGeoSphLds ? kSphBlockThreads : kBlockThreads; }
constexpr uint32_t waves_per_row(int geo) { return block_threads(geo) >= 128 ? 2u : 1u; }
constexpr uint32_t waves_per_col(int geo) { return block_threads(geo) / 64u / waves_per_row(geo); }

#ifndef RT_TRI_WAVES
#define RT_TRI_WAVES 8
#endif
// The waves per SIMD the lockstep path kernels (render, counts, path query) are
// compiled for.
constexpr int lockstep_min_waves(int geo, bool sph) {
    return sph ? kMinWavesPerEuSph
               : (geo == kGeoPairClu ? kMinWavesPerEuClu : (geo == kGeoTriBvh ? RT_TRI_WAVES : kMinWavesPerEu));
}

// THE staging prologue of the lockstep path kernels (render, counts, path
// query), after the kernel's RT_LDS_GUARD: the workgroup's NT threads stage the
// layout's intersection records once, then, for the box-cluster layout when
// `tab` (the kernel's halton_tables_on), a copy of the context's Halton tables
// (filled once, rt_create_ex: a copy, not a fill); one barrier; sv bound to the
// scene (bind_scene).  sph_stash: the kernel's per-lane LDS stash of shade()
// (the sphere kernel).
template <int GEO, bool SPH, uint32_t NT>
__device__ __forceinline__ void stage_scene(SceneView& sv, const KParams& P, float4* lds, float* sph_stash, bool tab) {
    const SceneTables T = tables_of(P);
    if (geo_staged(GEO)) {
        const StagedF4<uint32_t> n = staged_f4(GEO, T.nT, T.nP, T.nC);
        stage_records<GEO, NT>(lds, T);
        if (GEO == kGeoSphLds) sv.xstash = sph_stash;
        if (GEO == kGeoPairClu) {
            const uint32_t tab0 = n.rec + n.clu;
            sv.htab = tab ? reinterpret_cast<const float*>(lds + tab0) : nullptr;
            if (tab) copy_halton_tables<NT>(reinterpret_cast<float*>(lds + tab0), P.halton_tab, threadIdx.x);
        }
        __syncthreads();
    }
    bind_scene<GEO, SPH>(sv, T, lds);
}

template <int B, int GEO, bool SPH, bool SMALL, int L = 1>
__global__ __launch_bounds__(block_threads(GEO), lockstep_min_waves(GEO, SPH))
void path_trace_kernel(KParams P) {
    constexpr uint32_t NT = block_threads(GEO), WR = waves_per_row(GEO), WC = waves_per_col(GEO);
    extern __shared__ float4 lds[];
    SceneView sv;
    __shared__ float sph_stash[GEO == kGeoSphLds ? 6 * kSphBlockThreads : 1];
    RT_LDS_GUARD(staged_end(GEO, P, GEO == kGeoPairClu));
    stage_scene<GEO, SPH, NT>(sv, P, lds, sph_stash, halton_tables_on(GEO, SMALL, P.spp, L));

    // wave = 64/L pixels: 8x8 (L=1), 4x4 (L=4), 2x2 (L=16), or one row of 64/L
    // pixels for interleaved rows (launcher's wave_w); workgroup = 2x2 waves
    const uint32_t kWX = (L == 1) ? 8u : P.wave_w, kWY = (64u / L) / kWX;
    uint32_t bx, by;
    xcd_tile(bx, by);
    // tile_pixel (rt_pixel.hpp) for L lanes per pixel, spelled out: through the
    // helper the compiler orders the operands of one add differently
    // (tools/isa_diff.sh)
    auto pixel_of = [&](uint32_t t, uint32_t& x, uint32_t& j) {
        const uint32_t lane = t & 63u, wave = t >> 6, pix = lane / L;
        x = bx * (WR * kWX) + (wave % WR) * kWX + (pix % kWX);
        j = by * (WC * kWY) + (wave / WR) * kWY + (pix / kWX);
    };
    // Per-lane constants (pixel coordinates, lane roles) are recomputed from an
    // opaque copy of threadIdx.x where they are used, and the seed is kept in
    // LDS: otherwise the compiler hoists them out of the sample loop and spills
    // them to scratch for the whole launch (36 B/lane of scratch writes).
    // Only for the box-cluster and LDS-sphere kernels: the triangle-BVH walk
    // kernel (global-memory nodes) ran 16 % slower with the opaque copies
    // (325 vs 281 ms, 10k triangles) and spills about as much without them.
    constexpr bool kRemat = GEO == kGeoPairClu || GEO == kGeoSphLds;
    auto opaque_tid = []() {
        uint32_t t = threadIdx.x;
        if constexpr (kRemat) asm volatile("" : "+v"(t));
        return t;
    };
    {
        uint32_t x, j;
        pixel_of(threadIdx.x, x, j);
        if (x >= (uint32_t)P.W || j >= P.row_count) return;  // a pixel's L lanes leave together
    }
    __shared__ uint32_t seed_s[NT];        // seed + sample_base of the lane's pixel
    __shared__ float lum_s[L > 1 ? 3 * (NT / L) : 1];
    f3 lum{0.0f, 0.0f, 0.0f};                                    // :32
    {
        const uint32_t t = threadIdx.x, sub = t % L;
        uint32_t x, j;
        pixel_of(t, x, j);
        const uint32_t y = P.row_start + j * P.row_step;
        seed_s[t] = P.seeds[(size_t)y * (size_t)P.W + x] + P.sample_base;  // raytrace.metal:37
        if (P.accumulate) {
            const float4 prev = P.sum[(size_t)j * (size_t)P.W + x];
            lum = f3{prev.x, prev.y, prev.z};
        }
        // L > 1: the pixel's running sum lives in LDS (its group leader adds to
        // it), which keeps three VGPRs free across the path traversal
        const uint32_t slot = t / L;
        if (L > 1 && sub == 0) {
            lum_s[3 * slot] = lum.x;
            lum_s[3 * slot + 1] = lum.y;
            lum_s[3 * slot + 2] = lum.z;
        }
    }
    if constexpr (RT_CAM_CAND && GEO == kGeoPairClu) {
        // The pairs this wave's camera rays can hit and the pairs that can
        // occlude its bounce-0 shadow rays: fixed by
        // the scene, the camera and the wave's pixel rectangle, so they come
        // from the context's table (wave_masks_kernel below),
        // one entry per wave in wave row-major order, one scalar load.  Placed
        // after the seed staging: loaded before it, the L = 4 and L = 16 forms
        // at 3 and 4 bounces spill a VGPR inside the sample loop.
        if (sv.nP - 1u < 32u) {  // wave-uniform: 1..32 pairs, else no table: cluster_query as before
            const uint32_t wave = wave_uniform(threadIdx.x >> 6);
            const uint32_t wx = bx * WR + wave % WR, wy = by * WC + wave / WR;
            const uint4 m = P.wave_masks[wave_uniform(wy * (gridDim.x * WR) + wx)];
            sv.cam_mask = wave_uniform(m.x);
            sv.cam_avail = true;
            if constexpr (RT_SHD_CAND) {
                sv.shd_mask = wave_uniform(m.y);
                sv.shd_cskip = wave_uniform(m.z);
                sv.shd_avail = wave_uniform(m.w) != 0u;
            }
        }
    }
    const f3 cu = ld_f3(P.cam_u), cv = ld_f3(P.cam_v), cw = ld_f3(P.cam_w);
    const float fW = (float)P.W, fH = (float)P.H;
    uint32_t rounds = (P.spp + (L - 1)) / L;
    // A wave whose camera mask is empty hits nothing (the mask holds the free
    // pairs too, and this form has no spheres): every sample adds (+0, +0, +0)
    // to the pixel's sum.  It skips the sample loop and the epilogue adds +0
    // once, which leaves the bits that spp such additions leave.
    constexpr bool kDeadSkip = RT_CAM_CAND && RT_DEAD_SKIP && GEO == kGeoPairClu && !SPH;
    bool dead = false;
    if constexpr (kDeadSkip) {
        dead = sv.cam_avail && sv.cam_mask == 0u;  // wave-uniform
        if (dead) rounds = 0u;
    }
    for (uint32_t r = 0; r < rounds; ++r) {                      // :34
#ifdef RT_STATS
        const unsigned long long t_round = clock64();  // slot 24: cycles of whole rounds
#endif
        const uint32_t t = opaque_tid(), sub = t % L;
        // a lane past the last sample re-traces the last one (discarded below):
        // no divergent branch around the path
        const uint32_t n = (L == 1) ? r : min(r * L + sub, P.spp - 1u);
        PathState s;
        s.acc = f3{0.0f, 0.0f, 0.0f};
        {
            uint32_t x, j;
            pixel_of(t, x, j);
            const float fx = (float)x, fy = (float)(P.row_start + j * P.row_step);
            s.i = seed_s[t] + n;                                 // seed + (sample_base + n)
            const float jx = halton_dim<0, SMALL>(s.i);                                // :39-40
            const float jy = halton_dim<1, SMALL, GEO == kGeoPairClu>(s.i, sv.htab);
            s.d = camera_dir<GEO == kGeoTriBvh>(P, cu, cv, cw, fW, fH, fx, fy, jx, jy);
            s.o = ld_f3(P.cam_pos);
            s.thr = f3{1.0f, 1.0f, 1.0f};
#if RT_CENSUS == 1
            {
                const uint32_t i2 = cz(s.i);
                const float jx2 = halton_dim<0, SMALL>(i2);
                const float jy2 = halton_dim<1, SMALL, GEO == kGeoPairClu>(i2, sv.htab);
                cz_sink(camera_dir(P, cu, cv, cw, fW, fH, cz(fx), cz(fy), jx2, jy2));
            }
#endif
#ifndef RT_TIMING_NO_TRACE  // timing-only A/B (tools/ab_kernel.sh): camera, Halton jitter and sums alone
            trace_path<B, GEO, SPH, SMALL>(P, sv, s);                       // :47-102
#else
            s.acc = s.d;
#endif
        }
        if (L == 1) {
            lum = lum + s.acc;                                   // :103
        } else if (L <= 16 && !SPH) {
            // a pixel's L lanes are consecutive lanes of one 16-lane DPP row
            // (L = 4: groups at 0, 4, 8, 12; L = 16: the whole row), so its
            // leader reads sample r*L + k from lane +k with a row shift fused
            // into the add (v_add_f32_dpp row_shl:k) -- the same additions in
            // sample order, no LDS-pipe traffic.  Only the leaders' sums are kept.
            const uint32_t t2 = opaque_tid(), sub2 = t2 % L, slot = t2 / L;
            f3 acc{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
#if RT_CENSUS == 6
            {
                f3 a2 = cz(acc);
                row_sum_in_order<L, 0>::run(a2, cz(s.acc), r * L, P.spp);
                cz_sink(a2);
            }
#endif
            row_sum_in_order<L, 0>::run(acc, s.acc, r * L, P.spp);  // :103
            if (sub2 == 0) {
                lum_s[3 * slot] = acc.x;
                lum_s[3 * slot + 1] = acc.y;
                lum_s[3 * slot + 2] = acc.z;
            }
        } else {
            const uint32_t t2 = opaque_tid(), lane = t2 & 63u, sub2 = t2 % L, slot = t2 / L;
            const int base = (int)(lane - sub2);
            f3 c[L];
#pragma unroll
            for (int k = 0; k < L; ++k)                          // samples r*L + k
                c[k] = f3{__shfl(s.acc.x, base + k), __shfl(s.acc.y, base + k),
                          __shfl(s.acc.z, base + k)};
            if (sub2 == 0) {
                f3 acc{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
#pragma unroll
                for (int k = 0; k < L; ++k)                      // in sample order
                    if (r * L + (uint32_t)k < P.spp) acc = acc + c[k];  // :103
                lum_s[3 * slot] = acc.x;
                lum_s[3 * slot + 1] = acc.y;
                lum_s[3 * slot + 2] = acc.z;
            }
        }
#ifdef RT_STATS
        if (!SPH && GEO != kGeoTriBvh) {  // 24-31: the BVH any-hit walks' there
            RT_STAT(24, clock64() - t_round);
            RT_STAT(25, 1);
        }
#endif
    }
    // the pixel of the epilogue, recomputed from an opaque copy of threadIdx.x
    // in every kernel: otherwise the prologue's pixel offsets are kept (and
    // spilled) across the whole sample loop
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    if (L > 1) {
        if (t % L != 0) return;
        const uint32_t slot = t / L;
        lum = f3{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
    }
    if constexpr (kDeadSkip) {
        // x + (+0) once is x + (+0) spp times: only x == -0 changes, on the first
        if (dead && P.spp != 0u) lum = lum + f3{0.0f, 0.0f, 0.0f};
    }
    uint32_t x, j;
    pixel_of(t, x, j);
    // finish_pixel, spelled out: the call compiles to another branch order in
    // the L = 1 kernels
    const size_t o = (size_t)j * (size_t)P.W + x;
    if (P.sum) P.sum[o] = make_float4(lum.x, lum.y, lum.z, (float)P.samples_total);
    if (P.out) {
        const float fs = (float)P.samples_total;                 // :106
        const float r = lum.x / fs, g = lum.y / fs, bl = lum.z / fs;
        store_pixel(P, o, r, g, bl);
    }
}

#include "rt_free.hpp"

// waves per SIMD of the sorted kernel: the pair layout keeps 8; the BVH walks
// hold more state (RTPT A/B: sorted_waves)
#ifndef RT_SORTED_BVH_WAVES
#define RT_SORTED_BVH_WAVES 4
#endif
template <int B, int GEO, bool SPH, bool SMALL>
__global__ __launch_bounds__(kBlockThreads, GEO == kGeoPairLds ? kMinWavesPerEu : RT_SORTED_BVH_WAVES)
void path_trace_sorted_kernel(
    KParams P) {
    extern __shared__ float4 lds[];
    SceneView sv;
    const SceneTables T = tables_of(P);
    RT_LDS_GUARD(16 * (size_t)(kSortF4 + staged_f4(GEO, T.nT, T.nP, T.nC).rec));
    float4* scene = lds + kSortF4;  // sort buffers first: compile-time offsets
    stage_records<GEO, kBlockThreads>(scene, T);
    bind_scene<GEO, SPH>(sv, T, scene);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t x = blockIdx.x * kTile + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t j = blockIdx.y * kTile + (wave >> 1) * 8u + (lane >> 3);
    const bool valid = x < (uint32_t)P.W && j < P.row_count;  // every thread stays (barriers)
    const uint32_t y = P.row_start + j * P.row_step;
    const size_t o = (size_t)j * (size_t)P.W + x;
    const uint32_t seed = valid ? P.seeds[(size_t)y * (size_t)P.W + x] : 0u;  // raytrace.metal:37
    float* sum = reinterpret_cast<float*>(lds + kSortLum);
    {
        float4 prev = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // luminance = 0 (:32)
        if (valid && P.accumulate) prev = P.sum[o];
        sum[tid] = prev.x;
        sum[kBlockThreads + tid] = prev.y;
        sum[2 * kBlockThreads + tid] = prev.z;
    }
    __syncthreads();
    const float fx = (float)x, fy = (float)y, fW = (float)P.W, fH = (float)P.H;
    for (uint32_t n = 0; n < P.spp; ++n) {                       // :34
        PathState s;
        s.i = seed + (P.sample_base + n);
        s.acc = f3{0.0f, 0.0f, 0.0f};
        s.thr = f3{1.0f, 1.0f, 1.0f};
        s.o = ld_f3(P.cam_pos);
        s.d = f3{0.0f, 0.0f, 0.0f};
        if (valid) {
            const float jx = halton_dim<0, SMALL>(s.i), jy = halton_dim<1, SMALL>(s.i);
            s.d = camera_dir(P, ld_f3(P.cam_u), ld_f3(P.cam_v), ld_f3(P.cam_w), fW, fH, fx, fy, jx, jy);
        }
        uint32_t owner = tid;
        bool alive = valid;
        SortedChain<0, B, GEO, SPH, SMALL>::run(P, sv, lds, s, owner, alive);
        __syncthreads();  // sample n's hand-offs land before sample n+1's
    }
    if (!valid) return;
    finish_pixel(P, o, f3{sum[tid], sum[kBlockThreads + tid], sum[2 * kBlockThreads + tid]});
}

// rt_math_selfcheck: the shipped sqrt_cr / rcp_cr (rt_math.h) against the
// IEEE sqrtf / division on every float bit pattern b in [lo, lo + n): bad[0]
// counts sqrt mismatches (NaN results compare as NaN), bad[1] reciprocal ones.
__global__ void math_check_kernel(uint32_t lo, uint32_t n, unsigned long long* bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float x = __uint_as_float(lo + i);
        float y = x;
        asm volatile("" : "+v"(y));  // an opaque copy: the references stay the IEEE expansions
        const float s = sqrt_cr(x), sr = sqrtf(y);
        const float r = rcp_cr(x), rr = 1.0f / y;
        const bool sbad = !(__float_as_uint(s) == __float_as_uint(sr) || (s != s && sr != sr));
        const bool rbad = !(__float_as_uint(r) == __float_as_uint(rr) || (r != r && rr != rr));
        if (sbad) atomicAdd(&bad[0], 1ull);
        if (rbad) atomicAdd(&bad[1], 1ull);
    }
}

__global__ void fill_seeds_kernel(uint32_t* seeds, uint64_t key, uint64_t n) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = key + p + 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z = z ^ (z >> 31);
        seeds[p] = (uint32_t)(z & 0xFFFFFu);
    }
}

// The Halton low-digit tables of a context (KParams::halton_tab): one workgroup
// runs the fill that every workgroup of the box-cluster kernel used to run.
__global__ __launch_bounds__(kBlockThreads) void halton_tables_kernel(float* tab) {
    fill_halton_tables(tab, threadIdx.x, kBlockThreads);
}

// Placement of the gathered row tiles (rt_render_gather / rt_place_tiles): one
// thread per U-byte unit of the frame, consecutive threads along a row, so the
// reads (a tile row) and the writes (a frame row) are both coalesced.  A
// kernel on the caller's stream rather than N strided hipMemcpy2DAsync: a
// device-to-device 2D copy enqueued on the null stream was measured to start
// before the kernels enqueued ahead of it had finished (it read the gather
// buffer's previous contents), and the kernel is one launch whatever N.
// Frames taller than the grid's y extent walk their rows with a grid stride.
template <typename U>
__global__ void place_tiles_kernel(const U* __restrict__ gathered, U* __restrict__ frame, uint32_t row_u,
                                   size_t tile_u, uint32_t H, uint32_t N) {
    for (uint32_t y = blockIdx.y; y < H; y += gridDim.y) {
        const uint32_t k = y % N, j = y / N;
        const U* src = gathered + k * tile_u + (size_t)j * row_u;
        U* dst = frame + (size_t)y * row_u;
        for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < row_u; u += gridDim.x * blockDim.x)
            dst[u] = src[u];
    }
}

hipError_t launch_place_tiles(const void* gathered, void* frame, size_t row_bytes, size_t tile_bytes,
                              uint32_t H, uint32_t N, hipStream_t stream) {
    if (H == 0 || N == 0 || row_bytes == 0) return hipSuccess;
    if (row_bytes % 4 || tile_bytes % 4) return hipErrorInvalidValue;
    const bool wide = row_bytes % 16 == 0 && tile_bytes % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(gathered) % 16 == 0 && reinterpret_cast<uintptr_t>(frame) % 16 == 0;
    const size_t unit = wide ? 16 : 4;
    const uint32_t row_u = (uint32_t)(row_bytes / unit);
    const dim3 grid((row_u + 255u) / 256u, H < 65535u ? H : 65535u);  // grid.y limit: rows by grid stride
    if (wide)
        hipLaunchKernelGGL(place_tiles_kernel<uint4>, grid, dim3(256), 0, stream,
                           static_cast<const uint4*>(gathered), static_cast<uint4*>(frame), row_u,
                           tile_bytes / 16, H, N);
    else
        hipLaunchKernelGGL(place_tiles_kernel<uint32_t>, grid, dim3(256), 0, stream,
                           static_cast<const uint32_t*>(gathered), static_cast<uint32_t*>(frame), row_u,
                           tile_bytes / 4, H, N);
    return hipGetLastError();
}

namespace {

// Lanes per pixel (measured on one GPU's share of the N-GPU weak-scaling frame,
// tools/bench_share.py): 4 for whole frames of ~1 M pixels and more (also +6 % on
// the whole 1080p frame: 4x4-pixel waves, more lanes in flight), 16 below that
// and for interleaved shares, never more than spp.  The LDS sphere-walk kernel
// takes 16 at every size (measured on config 4, the whole 1080p frame: 198.4 ms
// at 16 lanes, 204.8 at 4, 227.6 at 1).
inline int lanes_per_pixel(const KParams& P, int geo) {
    if (P.lanes == 1 || P.lanes == 4 || P.lanes == 16) return P.spp >= P.lanes ? (int)P.lanes : 1;
    const uint64_t px = (uint64_t)P.W * P.row_count;
    // interleaved rows (a rank's share of a multi-GPU frame) take 16 lanes at any
    // size when every lane still gets the Halton tables' 8 rounds (measured,
    // tools/lanes_probe.py: 1080p share of N = 2 20,229 vs 19,922; 4096^2 share
    // of N = 8 19,450 vs 18,824); whole frames of >= 1 M pixels keep 4 (1080p
    // 20,288 vs 20,143; 4096^2 18,505 vs 17,978)
    const bool share16 = P.row_step > 1 && P.spp >= 16u * kHaltonTabMinRounds;
    // the BVH walk kernels (spheres, and since round 6 triangles) take 16 at any
    // size: triangles 100k / 10k / 1M at 1080p x 64 spp 1,176 / 1,234 / 575
    // Msamples/s with 16 lanes vs 1,101 / 1,172 / 514 with 4
    const int want = (px >= 1000000ull && geo != kGeoSphLds && geo != kGeoTriBvh && !share16) ? 4 : 16;
    if (P.spp >= (uint32_t)want) return want;
    return P.spp >= 4 ? 4 : 1;
}

constexpr int kGeoPairSorted = kLayPairSorted;
constexpr int kGeoFreeSph = kLayFreeSph;
constexpr int kGeoFreeTri = kLayFreeTri;
constexpr int kGeoSortSph = kLaySortSph;
constexpr int kGeoSortTri = kLaySortTri;
static_assert(kGeoTriLds == kLayTriLds && kGeoPairLds == kLayPairLds && kGeoTriGlobal == kLayTriGlobal &&
                  kGeoPairSmem == kLayPairSmem && kGeoTriBvh == kLayTriBvh && kGeoPairClu == kLayPairClu &&
                  kGeoSphLds == kLaySphLds,
              "rt_trace.hpp Geo == rt_kernel.hpp KernelLayout");
static_assert(kHaltonTabLdsFloats == kHaltonTabFloats && kSortLdsF4 == kSortF4, "staged_lds_bytes terms");

// The most recent launch of this thread (launch_path_trace copies it out).
thread_local LaunchInfo g_last;

template <int B, int GEO, bool SPH, bool SMALL, int L>
void note_launch(const char* name, const KParams& P, dim3 grid, uint32_t threads, size_t lds) {
    fill_launch_info(g_last, (uint32_t)L, halton_tables_on(GEO, SMALL, P.spp, (uint32_t)L), SMALL, threads, grid, lds,
                     "rt::%s<%d, %d, %s, %s, %d>", name, B, GEO, SPH ? "true" : "false", SMALL ? "true" : "false", L);
}

// Dynamic LDS above 64 KB must be allowed per kernel (the compact sphere BVH).
inline hipError_t allow_lds(const void* kernel, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <int B, int GEO, bool SPH, bool SMALL, int L>
hipError_t launch_tl(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    KParams Q = P;
    // wave tile: 8x8 pixels at one lane per pixel; L > 1: compact (4x4, 2x2)
    // for whole frames, one row of 64/L pixels when the rows are interleaved
    // (row_step > 1), which keeps a wave's camera rays adjacent in the image
    // (N = 8 share: 10,822 -> 11,211 Msamples/s)
    const WaveGrid g = wave_grid((uint32_t)P.W, P.row_count, P.row_step, (uint32_t)L, waves_per_row(GEO), waves_per_col(GEO));
    if (L > 1) Q.wave_w = g.wave_w;
    const dim3 grid(g.grid_x, g.grid_y);
    // the box-cluster kernel reads its waves' masks from the context's table
    if (RT_CAM_CAND && GEO == kGeoPairClu && P.nP - 1u < 32u && !P.wave_masks) return hipErrorInvalidValue;
    if (GEO == kGeoSphLds) {
        const hipError_t e = allow_lds((const void*)path_trace_kernel<B, GEO, SPH, SMALL, L>, lds_bytes);
        if (e != hipSuccess) return e;
    }
    note_launch<B, GEO, SPH, SMALL, L>("path_trace_kernel", Q, grid, block_threads(GEO), lds_bytes);
    hipLaunchKernelGGL((path_trace_kernel<B, GEO, SPH, SMALL, L>), grid, dim3(block_threads(GEO)),
                       lds_bytes, stream, Q);  // staged_lds_bytes of the layout
    return hipGetLastError();
}

template <int B, int GEO, bool SPH, bool SMALL>
hipError_t launch_t(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    if (SMALL) {
        const int lpp = lanes_per_pixel(P, GEO);
        if (lpp == 16) return launch_tl<B, GEO, SPH, SMALL, 16>(P, lds_bytes, stream);
        if (lpp == 4) return launch_tl<B, GEO, SPH, SMALL, 4>(P, lds_bytes, stream);
    }
    return launch_tl<B, GEO, SPH, SMALL, 1>(P, lds_bytes, stream);
}

template <int B, int GEO, bool SPH, bool SMALL>
hipError_t launch_sorted_t(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid((P.W + kTile - 1) / kTile, (P.row_count + kTile - 1) / kTile);
    note_launch<B, GEO, SPH, SMALL, 1>("path_trace_sorted_kernel", P, grid, kBlockThreads, lds_bytes);
    hipLaunchKernelGGL((path_trace_sorted_kernel<B, GEO, SPH, SMALL>), grid, dim3(kBlockThreads),
                       lds_bytes, stream, P);  // staged_lds_bytes: path buffers + scene records
    return hipGetLastError();
}

template <int B, int GEO, bool SORTED, bool SPH, bool SMALL>
hipError_t launch_k(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    if constexpr (SORTED)
        return launch_sorted_t<B, GEO, SPH, SMALL>(P, lds_bytes, stream);
    else
        return launch_t<B, GEO, SPH, SMALL>(P, lds_bytes, stream);
}

template <int B, int GEO, bool SORTED, bool SPH>
hipError_t launch_h(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    return P.max_index < kSmallIndexMax ? launch_k<B, GEO, SORTED, SPH, true>(P, lds_bytes, stream)
                                        : launch_k<B, GEO, SORTED, SPH, false>(P, lds_bytes, stream);
}

// The free-running kernel (rt_free.hpp): one pixel per lane, 8x8-pixel waves
// (one row of 64 pixels for interleaved rows), one-wave workgroups.
template <int B, int GEO, bool SMALL>
hipError_t launch_free_t(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    KParams Q = P;
    Q.wave_w = (P.row_step > 1) ? 64u : 8u;
    const uint32_t TY = 64u / Q.wave_w;
    const dim3 grid((P.W + Q.wave_w - 1) / Q.wave_w, (P.row_count + TY - 1) / TY);
    note_launch<B, GEO, GEO == kGeoSphLds, SMALL, 1>("path_free_kernel", Q, grid, kFreeThreads, lds_bytes);
    hipLaunchKernelGGL((path_free_kernel<B, GEO, SMALL>), grid, dim3(kFreeThreads), lds_bytes, stream,
                       Q);  // staged_lds_bytes of the layout
    return hipGetLastError();
}

template <int B, int GEO>
hipError_t launch_free(const KParams& P, size_t lds_bytes, hipStream_t stream) {
    if constexpr (B < 1) {
        return hipErrorInvalidValue;
    } else {
        return P.max_index < kSmallIndexMax ? launch_free_t<B, GEO, true>(P, lds_bytes, stream)
                                            : launch_free_t<B, GEO, false>(P, lds_bytes, stream);
    }
}

// The kernel of layout `geo` (choose_kernel) at B bounces.  A free-running or
// octant-sorted layout runs the records and walks of its lockstep layout
// (ray_query_layout), so all three schedulers take their layout and sphere form
// from dispatch_layout; the Halton form is launch_h's / launch_free's, the lanes
// launch_t's.  The sorted triangle BVH is chosen for triangle-only scenes
// (choose_kernel) and has that one form.
#ifdef RT_DEV_ISA  // ISA-inspection builds only (tools/isa.sh): the render kernels of the headline layouts
constexpr bool dev_isa_skips(int geo) { return geo != kGeoPairClu && geo != kGeoSphLds && geo != kGeoTriBvh; }
#else
constexpr bool dev_isa_skips(int) { return false; }
#endif
template <int B>
hipError_t launch_b(const KParams& P, int geo, size_t lds_bytes, hipStream_t stream) {
    const bool free_run = geo == kGeoFreeSph || geo == kGeoFreeTri;
    const bool sorted = geo == kGeoPairSorted || geo == kGeoSortSph || geo == kGeoSortTri;
    return dispatch_layout(ray_query_layout(geo), P.nS, [&](auto g, auto sph) {
        constexpr int GEO = decltype(g)::value;
        constexpr bool SPH = decltype(sph)::value;
        if constexpr (dev_isa_skips(GEO)) {
            return hipErrorInvalidValue;
        } else {
            if (free_run) {
                if constexpr (GEO == kGeoSphLds || GEO == kGeoTriBvh) return launch_free<B, GEO>(P, lds_bytes, stream);
            } else if (sorted) {
                if constexpr (GEO == kGeoPairLds || GEO == kGeoSphLds || (GEO == kGeoTriBvh && !SPH))
                    return launch_h<B, GEO, true, SPH>(P, lds_bytes, stream);
            } else {
                return launch_h<B, GEO, false, SPH>(P, lds_bytes, stream);
            }
            return hipErrorInvalidValue;  // a layout without that scheduler: choose_kernel gives none
        }
    });
}

}  // namespace

size_t kernel_lds_bytes(uint32_t n_tri, uint32_t n_pairs, uint32_t n_sph, uint32_t n_nodes) {
    (void)n_sph;  // sphere BVH nodes and records stay in global memory (scalar loads)
    (void)n_nodes;
    return n_pairs ? staged_lds_bytes(kLayPairLds, n_tri, n_pairs, 0) : staged_lds_bytes(kLayTriLds, n_tri, 0, 0);
}

KernelChoice choose_kernel(const SceneTables& t, bool sph_compact, uint32_t bounces, SceneMem mem, uint32_t walk) {
    const uint32_t nP = t.nP, nS = t.nS, nC = t.nC, nTN = t.nTN;
    auto lds = [&](int lay) { return staged_lds_bytes(lay, t.nT, nP, nC); };
    const bool pairs = nP > 0 && mem != SceneMem::kLdsSingle;
    int geo = kGeoTriGlobal;
    if (mem != SceneMem::kSmem && lds(pairs ? kGeoPairLds : kGeoTriLds) <= kMaxLdsBytes)
        geo = pairs ? kGeoPairLds : kGeoTriLds;
    if (mem == SceneMem::kPairSmem && nP > 0) geo = kGeoPairSmem;
    // triangle BVH whenever rt_create built one (kTriBvhMinTriangles or no LDS fit),
    // unless another layout is forced
    if (nTN > 0 && (mem == SceneMem::kTriBvh || mem == SceneMem::kAuto)) geo = kGeoTriBvh;
    // the sphere kernel (one-wave workgroups, its BVH in L2) while its
    // per-workgroup copy of the pair records is small (rt_kernel.hpp)
    if (geo == kGeoPairLds && nS > 0 && sph_compact && mem == SceneMem::kAuto &&
        lds(kGeoSphLds) <= kSphPairLdsMaxBytes)
        geo = kGeoSphLds;
    // box clusters whenever rt_create found some; not with
    // spheres, where the sphere walks dominate and the cluster code's register
    // pressure measured 4.6 % slower than the culled pair loop (config 4)
    if (geo == kGeoPairLds && nC > 0 && nS == 0 && mem == SceneMem::kAuto && lds(kGeoPairClu) <= kMaxLdsBytes)
        geo = kGeoPairClu;
    // Opt-in only: bit-identical, 31% fewer pair tests, but 18% slower on the
    // Cornell 1080p workload (barrier + occupancy cost).
    if (geo == kGeoPairLds && mem == SceneMem::kPairSorted && lds(kGeoPairSorted) <= kMaxLdsBytes)
        geo = kGeoPairSorted;
    // the free-running kernel for BVH scenes (rt_create_options.walk_scheduler)
    if (bounces >= 1 && walk == kWalkFree) {
        if (geo == kGeoSphLds) geo = kGeoFreeSph;
        if (geo == kGeoTriBvh && nS == 0) geo = kGeoFreeTri;
    }
    // octant-sorted paths for BVH scenes (rt_create_options.walk_scheduler)
    if (walk == kWalkSorted) {
        if (geo == kGeoSphLds) geo = kGeoSortSph;
        if (geo == kGeoTriBvh && nS == 0) geo = kGeoSortTri;
    }
    return KernelChoice{geo, lds(geo)};
}

namespace {
hipError_t launch_path_trace_impl(const KParams& P, uint32_t bounces, SceneMem mem,
                                  hipStream_t stream) {
    const KernelChoice kc = choose_kernel(tables_of(P), P.sph_lds != nullptr, bounces, mem, P.walk);
    const int geo = kc.layout;
    const size_t lds_total = kc.lds_bytes;  // exactly what the layout's staging loops write
#ifdef RT_LDS_UNDERSIZE  // negative control of the RT_LDS_CHECK build: one float4 short
    const size_t lds_req = lds_total >= 16 ? lds_total - 16 : lds_total;
#else
    const size_t lds_req = lds_total;
#endif
#ifdef RT_DEV_ISA  // ISA-inspection builds only (tools/isa.sh): the render kernels at B = 3 alone
    return bounces == 3 ? launch_b<3>(P, geo, lds_req, stream) : hipErrorInvalidValue;
#else
    return dispatch_bounces(bounces, [&](auto b) { return launch_b<decltype(b)::value>(P, geo, lds_req, stream); });
#endif
}
}  // namespace

hipError_t launch_path_trace(const KParams& P, uint32_t bounces, SceneMem mem,
                             hipStream_t stream, LaunchInfo* info) {
    const hipError_t e = launch_path_trace_impl(P, bounces, mem, stream);
    if (info) *info = g_last;
    return e;
}

bool wave_mask_grid(const KParams& P, uint32_t bounces, SceneMem mem, uint32_t lanes_override, WaveGrid* g) {
    if (!RT_CAM_CAND || P.nP - 1u >= 32u) return false;
    if (choose_kernel(tables_of(P), P.sph_lds != nullptr, bounces, mem, P.walk).layout != kGeoPairClu) return false;
    KParams Q = P;
    if (lanes_override) Q.lanes = lanes_override;
    // launch_h and launch_t: lanes per pixel above 1 only with fixed-digit indices
    const int L = P.max_index < kSmallIndexMax ? lanes_per_pixel(Q, kGeoPairClu) : 1;
    *g = clu_wave_grid((uint32_t)P.W, P.row_count, P.row_step, (uint32_t)(L == 16 || L == 4 ? L : 1));
    return true;
}

// the render with per-pixel sample counts: after every kernel and launcher above
#include "rt_counts.hpp"
// path-traced radiance along the caller's own rays: after the counts kernels
#include "rt_paths.hpp"

hipError_t lds_check_result(uint32_t* end) {
    *end = 0;
#ifdef RT_LDS_CHECK
    hipError_t e = hipMemcpyFromSymbol(end, HIP_SYMBOL(g_lds_overflow), sizeof(uint32_t));
    if (e != hipSuccess) return e;
    const uint32_t zero = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lds_overflow), &zero, sizeof(zero));
#else
    return hipSuccess;
#endif
}

hipError_t read_debug_stats(unsigned long long* out, int n) {
#if defined(RT_FREE_DEBUG)
    // the free kernel's event log (rt_free.hpp), as 64-bit words
    constexpr int kWords = (int)(sizeof(g_free_dbg) / 8);
    if (n > kWords) n = kWords;
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_free_dbg), n * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    static const uint32_t zero[4] = {0, 0, 0, 0};  // the three slot counters
    return hipMemcpyToSymbol(HIP_SYMBOL(g_free_dbg), zero, sizeof(zero));
#elif defined(RT_STATS)
    if (n > 40) n = 40;
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rt_stats), n * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    const unsigned long long zero[40] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_rt_stats), zero, sizeof(zero));
#else
    (void)out;
    (void)n;
    return hipErrorNotSupported;
#endif
}

hipError_t math_selfcheck(unsigned long long bad[2]) {
    unsigned long long* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, 2 * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    if ((e = hipMemset(d, 0, 2 * sizeof(unsigned long long))) == hipSuccess) {
        // every float: 2^32 bit patterns in two halves of 2^31
        hipLaunchKernelGGL(math_check_kernel, dim3(16384), dim3(256), 0, 0, 0u, 0x80000000u, d);
        hipLaunchKernelGGL(math_check_kernel, dim3(16384), dim3(256), 0, 0, 0x80000000u, 0x80000000u, d);
        if ((e = hipGetLastError()) == hipSuccess && (e = hipDeviceSynchronize()) == hipSuccess)
            e = hipMemcpy(bad, d, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    return e;
}

hipError_t launch_fill_halton_tables(float* tab, hipStream_t stream) {
    hipLaunchKernelGGL(halton_tables_kernel, dim3(1), dim3(kBlockThreads), 0, stream, tab);
    return hipGetLastError();
}

hipError_t launch_fill_seeds(uint32_t* seeds, uint64_t key, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(fill_seeds_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, seeds,
                       key, n);
    return hipGetLastError();
}

// The mask table of one launch geometry: wave w of this
// kernel decides entry w = wy * waves_x + wx, the masks of the render wave
// whose pixels are columns wx * wave_w .. and partition rows wy * wave_h ..
// The tests are rt_beam.hpp's and rt_shaft.hpp's, in the lane layout the
// render kernel's prologue had: lane k tests pair k against the wave's beam
// and the ballot is the camera mask; lane k and lane k + 32 test target pair k
// against the shafts of triangle A and triangle B of a source pair, for EVERY
// pair of the camera mask in turn (wave-uniform loop), and the occluder mask is
// the union.  A light's triangle ends the path: it casts no shadow ray.  One
// undecidable source (a grazing or crossing plane): nothing is decided for the
// wave, the generic query runs.  The records come from global memory.
// A template, instantiated by the launcher below, last in this file: the code
// object keeps the order of the kernels before it (tools/isa_diff.sh).
template <bool MULTI>
__global__ __launch_bounds__(kBlockThreads) void wave_masks_kernel(KParams P, uint4* table, uint32_t waves_x,
                                                                   uint32_t n_waves, uint32_t kWX, uint32_t kWY) {
    const uint32_t w = wave_uniform(blockIdx.x * (kBlockThreads / 64u) + (threadIdx.x >> 6));
    if (w >= n_waves) return;  // wave-uniform
    const float* pair = reinterpret_cast<const float*>(P.pair_isect);  // 1..32 pairs (wave_mask_grid)
    const Beam beam = wave_beam(P, (w % waves_x) * kWX, (w / waves_x) * kWY, kWX, kWY);
    const uint32_t nP = P.nP, nC = P.nC;
    // the two masks, spelled out here and in path_counts_kernel: through shared routines
    // both kernels compile differently (tools/isa_diff.sh)
    const uint32_t k = threadIdx.x & 63u;
    const uint32_t kc = min(k, nP - 1u);  // lanes past the last pair re-test it (discarded)
    const bool keep = !beam_excludes_pair(beam, pair + 4u * kPairF4 * kc);
    const uint32_t cam_mask = wave_uniform((uint32_t)__builtin_amdgcn_ballot_w64(k < nP && keep));
    uint32_t shd_mask = 0u, shd_cskip = 0u;
    bool shd_avail = false;
    if constexpr (RT_SHD_CAND) {
        const uint32_t tb = k >> 5, kt = min(k & 31u, nP - 1u);
        const ShaftLight lq = shaft_light(ld_f3(P.light_center));
        bool undecided = !MULTI && (cam_mask & (cam_mask - 1u)) != 0u;
        for (uint32_t m = undecided ? 0u : cam_mask; m != 0u; m &= m - 1u) {  // wave-uniform
            const uint32_t sp = (uint32_t)__builtin_ctz(m);
            const float4 s0 = P.tri_shade[4 * (2u * sp + tb)];
            bool occ = false, bad = false;
            if (s0.w == 0.0f) {
                const ShaftSrc src = shaft_source(beam, pair + 4u * kPairF4 * sp, (int)tb, f3{s0.x, s0.y, s0.z}, lq);
                bad = !src.ok;
                occ = !shaft_excludes_pair(src, lq, pair + 4u * kPairF4 * kt);
            }
            const unsigned long long ob = __builtin_amdgcn_ballot_w64((k & 31u) < nP && occ);
            shd_mask |= wave_uniform((uint32_t)ob | (uint32_t)(ob >> 32));
            undecided = undecided || __builtin_amdgcn_ballot_w64(bad) != 0ull;
        }
        shd_avail = !undecided && nC <= 32u;
        // clusters none of whose faces is in the mask (record word 22: all its pairs)
        if (nC != 0u) {
            const uint32_t kc2 = min(k, nC - 1u);
            const uint32_t all = __float_as_uint(reinterpret_cast<const float*>(P.clusters + kCluF4 * kc2)[22]);
            shd_cskip = wave_uniform((uint32_t)__builtin_amdgcn_ballot_w64(k < nC && (all & shd_mask) == 0u));
        }
    }
    if (k == 0u) table[w] = make_uint4(cam_mask, shd_mask, shd_cskip, shd_avail ? 1u : 0u);
}

hipError_t launch_wave_masks(const KParams& P, const WaveGrid& g, uint4* table, hipStream_t stream) {
    const uint32_t n = g.waves_x * g.waves_y, per_block = kBlockThreads / 64u;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(wave_masks_kernel<RT_WAVE_MASK_MULTI != 0>, dim3((n + per_block - 1) / per_block), dim3(kBlockThreads), 0, stream, P, table,
                       g.waves_x, n, g.wave_w, g.wave_h);
    return hipGetLastError();
}

}  // namespace rt
