// rt_cluorder.hpp — one ray against one box cluster, with the candidate faces
// split by the side the ray meets them on.  One source text
// for the gfx950 kernel (rt_trace.hpp cluster_candidates_split: the closest
// queries of bounce >= 1) and for the host (tests/native/closest_order_check.cpp,
// tools/closest_rounds.cpp).  Per-lane work only: the wave ballots around it
// stay in rt_trace.hpp.
//
// The slab and face filter are those of rt_trace.hpp cluster_candidates
// (DESIGN.md §3.12), term for term.  What is new is where a candidate goes:
//   near    entry-side faces of a box the ray comes at from outside, and
//           single-face clusters: where a ray that meets the box is stopped
//   far     exit-side faces, and every candidate face of a container (the
//           room: the ray is inside it)
//   far_lo  the smallest lower end of the far candidates' face-plane
//           intervals: no accepted hit on a far candidate has t < far_lo
// A closest query tests near first and then far only where
// far_lo <= best * (1 + 2^-16): the comparison by which the filter itself drops
// an exit face for tmax = best, made again with the best the near tests found.
// Only speed depends on any of it: a kept pair gets the exact test.
#pragma once

#include "rt_math.h"

// Leaner filter paths for the cluster kinds the scene compiler marks
// (rt_kernel.hpp has the switch's description).
// RT_CLU_LEAN_ITEMS is the set of items built: 1 turned boxes, 2 containers
// left from inside, 4 the light's own cluster in shadow queries.  The kernel
// ships items 2 and 4: item 4 spilled 8 VGPRs of the box-cluster kernel (72
// VGPRs, 7 waves/SIMD) while shade() loaded the light flag of the shading
// record first; with the flag taken from the launch's light mask (DESIGN.md
// §3.21) it spills none.  Item 1 spills 12; it stays for measurements and is
// checked on the host (tests/test_lean_filter.py builds its checker with all
// three).
#ifndef RT_CLU_LEAN
#define RT_CLU_LEAN 1
#endif
#ifndef RT_CLU_LEAN_ITEMS
#define RT_CLU_LEAN_ITEMS 6
#endif

namespace rt {

constexpr float kCluEps = 1.52587890625e-05f;  // 2^-16 relative slack

// Flag bits of a cluster record (word r[3].w; rt_scene.cpp build_clusters).
// Bits 0-2: axis a is world axis a; the kinds of DESIGN.md §3.19 from bit 5.
constexpr uint32_t kCluContainer = 8u;   // all axes world axes, room inside
constexpr uint32_t kCluSingle = 16u;     // one face: a candidate whenever the padded box is hit
constexpr uint32_t kCluTurned = 32u;     // exactly one world axis, and the other two axis vectors
                                         // have a +-0 component along it
constexpr uint32_t kCluInside = 64u;     // a container whose shrunk box (r[0..2].xy) is not empty
constexpr uint32_t kCluOwnLight = 128u;  // single face, all of it light triangles in the plane
                                         // the light samples are drawn from
constexpr bool kLeanTurned = RT_CLU_LEAN != 0 && (RT_CLU_LEAN_ITEMS & 1) != 0;
constexpr bool kLeanExit = RT_CLU_LEAN != 0 && (RT_CLU_LEAN_ITEMS & 2) != 0;
constexpr bool kLeanOwnLight = RT_CLU_LEAN != 0 && (RT_CLU_LEAN_ITEMS & 4) != 0;

// min / max of the culling tests, issued directly.  fminf/fmaxf lower to
// v_min/v_max_f32 plus a v_max_f32 x,x "canonicalize" of every operand the
// compiler cannot prove canonical (loads, values through phis: the
// loop-carried best, the branch-merged slab terms) -- 8 extra VALU per box
// cluster and 2 per BVH step.  The operands here are results of arithmetic on
// finite scene data (no signalling NaNs), for which v_min/v_max_f32 return
// exactly fminf/fmaxf; and these values only decide what is culled, never a
// result.
#if defined(__HIPCC__)
#define RT_HOST_ONLY __host__ inline
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// 1/v clamped to +-1e20 (v = +-0 gives +-1e20): one v_rcp + one v_med3.
// Feeds only conservative slab tests (speed, not results, depends on it).
__device__ __forceinline__ float safe_rcp(float v) {
    return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(v), -1e20f, 1e20f);
}
#else
#define RT_HOST_ONLY inline
#endif
// The host forms of the same five (overloads of the device ones under hipcc).
// The host takes the correctly rounded quotient where the device takes the
// 1-ulp reciprocal: the filter's 2^-16 slack is what covers the difference.
RT_HOST_ONLY float vmin(float a, float b) { return fminf(a, b); }
RT_HOST_ONLY float vmax(float a, float b) { return fmaxf(a, b); }
RT_HOST_ONLY float vmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
RT_HOST_ONLY float vmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
RT_HOST_ONLY float safe_rcp(float v) { return fminf(fmaxf(1.0f / v, -1e20f), 1e20f); }

// What one ray's closest query has to test among the clustered pairs.
struct CluSplit {
    uint32_t near, far;  // pair bit masks, disjoint after clu_split_finish
    float far_lo;        // +inf: no far candidate
};

RT_HD CluSplit clu_split_init() { return CluSplit{0u, 0u, INFINITY}; }

#if RT_CLU_LEAN
// The slab terms of a box turned about world axis W (kCluTurned, DESIGN.md
// §3.19): axis W takes the ray's own reciprocal, and the other two axis vectors
// have a +-0 component W, so their products with o and d are formed from the
// two other components, in dot()'s order.  The dropped term is fma(+-0, x, m)
// or +-0 * x under an fma: it leaves m as it is up to the sign of a zero.
template <int W, class V4>
RT_HD void clu_turned_terms(const V4* r, const float hi[3], const float iv[3], const float oi[3], f3 o, f3 d,
                            float en[3], float ex[3], float ida[3]) {
    constexpr int I = W == 0 ? 1 : 0, J = W == 2 ? 1 : 2;  // the kept components, I < J
    const float oc[3] = {o.x, o.y, o.z}, dc[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const V4 A = r[a];
        float t0, t1;
        if (a == W) {
            ida[a] = iv[a];
            t0 = fmaf(A.w, iv[a], -oi[a]);
            t1 = fmaf(hi[a], iv[a], -oi[a]);
        } else {
            const float ac[3] = {A.x, A.y, A.z};
            const float oa = fmaf(ac[J], oc[J], ac[I] * oc[I]), da = fmaf(ac[J], dc[J], ac[I] * dc[I]);
            ida[a] = safe_rcp(da);
            t0 = (A.w - oa) * ida[a];
            t1 = (hi[a] - oa) * ida[a];
        }
        en[a] = vmin(t0, t1);
        ex[a] = vmax(t0, t1);
    }
}
#endif

// Slab test of a multi-face cluster record r (kCluF4 vectors with .x .y .z .w):
// entry and exit parameter per box axis and the slackened overlap [tlo, thi]
// of the padded box with (tmin, tmax).  iv / oi: 1/d and o/d per world axis
// (used for the axes that are world axes, flags bit a).
template <class V4>
RT_HD void clu_slab(const V4* r, uint32_t flags, const float iv[3], const float oi[3], f3 o, f3 d, float tmin,
                    float tmax, float en[3], float ex[3], float ida[3], float* tlo, float* thi) {
    const V4 H = r[3];
    const float hi[3] = {H.x, H.y, H.z};
#if RT_CLU_LEAN
    if (kLeanTurned && (flags & kCluTurned)) {  // the same for every ray: one branch for the kind
        if (flags & 2u) clu_turned_terms<1>(r, hi, iv, oi, o, d, en, ex, ida);
        else if (flags & 1u) clu_turned_terms<0>(r, hi, iv, oi, o, d, en, ex, ida);
        else clu_turned_terms<2>(r, hi, iv, oi, o, d, en, ex, ida);
    } else
#endif
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const V4 A = r[a];
            float t0, t1;
            if (flags & (1u << a)) {  // the same for every ray
                ida[a] = iv[a];
                t0 = fmaf(A.w, iv[a], -oi[a]);
                t1 = fmaf(hi[a], iv[a], -oi[a]);
            } else {
                const float oa = dot(f3{A.x, A.y, A.z}, o), da = dot(f3{A.x, A.y, A.z}, d);
                ida[a] = safe_rcp(da);
                t0 = (A.w - oa) * ida[a];
                t1 = (hi[a] - oa) * ida[a];
            }
            en[a] = vmin(t0, t1);
            ex[a] = vmax(t0, t1);
        }
    }
    const float tlo0 = vmax3(en[0], en[1], vmax(en[2], tmin));
    const float thi0 = vmin3(ex[0], ex[1], vmin(ex[2], tmax));
    *tlo = fmaf(-kCluEps, fabsf(tlo0), tlo0);  // kCluEps*|x| is exact: the same values
    *thi = fmaf(kCluEps, fabsf(thi0), thi0);
}

// The candidate faces of that cluster, split.  A ray with d_a >= 0 enters
// through the low face of axis a (slot 2a) and leaves through the high one
// (2a + 1); the face plane lies wf * |1/d_a| inside the padded slab, +- the
// tolerance.  A container's entry-side candidates (a ray that starts on a
// wall) go to far with far_lo = -inf: they are never culled.
// SLACK = false forms far_lo at the padded plane itself, without the filter's
// interval: the wrong bound that tests/test_closest_order.py must catch.
template <bool SLACK = true, class V4>
RT_HD void clu_faces_split(const V4* r, uint32_t flags, const float en[3], const float ex[3], const float ida[3],
                           float tlo, float thi, CluSplit* s) {
    const V4 M0 = r[4], M1 = r[5], W = r[6];
    const uint32_t m[6] = {f2u(M0.x), f2u(M0.y), f2u(M0.z), f2u(M0.w), f2u(M1.x), f2u(M1.y)};
    const float wf[3] = {W.x, W.y, W.z};
    const bool hit = tlo <= thi;
    const bool container = (flags & 8u) != 0u;  // the same for every ray
    uint32_t cn = 0, cf = 0;
    float lo = s->far_lo;
    bool en_far = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool neg = ida[a] < 0.0f;
        const uint32_t m_en = neg ? m[2 * a + 1] : m[2 * a];
        const uint32_t m_ex = neg ? m[2 * a] : m[2 * a + 1];
        const float wa = wf[a] * fabsf(ida[a]);
        const bool c_en = hit && en[a] + fmaf(fabsf(en[a]), kCluEps, wa) >= tlo;
        const float xl = ex[a] - fmaf(fabsf(ex[a]), kCluEps, wa);
        const bool c_ex = hit && xl <= thi;
        if (container) {
            cf |= c_en ? m_en : 0u;
            en_far = en_far || c_en;
        } else {
            cn |= c_en ? m_en : 0u;
        }
        cf |= c_ex ? m_ex : 0u;
        lo = c_ex ? vmin(lo, SLACK ? xl : ex[a]) : lo;
    }
    s->near |= cn;
    s->far |= cf;
    s->far_lo = en_far ? -INFINITY : lo;
}

#if RT_CLU_LEAN
// Does the ray start strictly inside the shrunk box of a container record
// (r[0..2].xy: every face plane + tol_seg, rt_scene.cpp)?  No face the ray
// moves away from can then accept a hit with t > tmin > 0.
template <class V4>
RT_HD bool clu_origin_inside(const V4* r, f3 o) {
    const V4 X = r[0], Y = r[1], Z = r[2];
    return o.x > X.x && o.x < X.y && o.y > Y.x && o.y < Y.y && o.z > Z.x && o.z < Z.y;
}

// The candidate faces of a container (kCluInside) for a ray that starts inside
// its shrunk box: the exit side alone.  The box is hit, the entry terms are not
// formed, and the exit parameter of axis a is that of the plane the ray moves
// towards -- max(t0, t1) of clu_slab, bit for bit: fma(x, iv, -oi) is monotone
// in x, and lo < hi.  far and far_lo are those clu_faces_split gives for the
// exit faces; no entry-side candidate makes far_lo -inf.
template <bool SLACK = true, class V4>
RT_HD void clu_container_exit(const V4* r, const float iv[3], const float oi[3], float tmax, CluSplit* s) {
    const V4 H = r[3], M0 = r[4], M1 = r[5], W = r[6];
    const float lo3[3] = {r[0].w, r[1].w, r[2].w}, hi[3] = {H.x, H.y, H.z}, wf[3] = {W.x, W.y, W.z};
    const uint32_t m[6] = {f2u(M0.x), f2u(M0.y), f2u(M0.z), f2u(M0.w), f2u(M1.x), f2u(M1.y)};
    bool neg[3];
    float ex[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        neg[a] = iv[a] < 0.0f;
        ex[a] = fmaf(neg[a] ? lo3[a] : hi[a], iv[a], -oi[a]);
    }
    const float thi0 = vmin3(ex[0], ex[1], vmin(ex[2], tmax));
    const float thi = fmaf(kCluEps, fabsf(thi0), thi0);
    uint32_t cf = 0;
    float lo = s->far_lo;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float wa = wf[a] * fabsf(iv[a]);
        const float xl = ex[a] - fmaf(fabsf(ex[a]), kCluEps, wa);
        const bool c_ex = xl <= thi;
        cf |= c_ex ? (neg[a] ? m[2 * a] : m[2 * a + 1]) : 0u;
        lo = c_ex ? vmin(lo, SLACK ? xl : ex[a]) : lo;
    }
    s->far |= cf;
    s->far_lo = lo;
}
#endif

// A single-face cluster (the light, a lone rectangle): its face is a near
// candidate whenever the padded box is hit (a superset of its face test).
template <class V4>
RT_HD void clu_single_split(const V4* r, uint32_t flags, const float iv[3], const float oi[3], f3 o, f3 d,
                            float tmin, float tmax, CluSplit* s) {
    const V4 A0 = r[0], A1 = r[1], A2 = r[2], H = r[3];
    const V4 A[3] = {A0, A1, A2};
    const float hi[3] = {H.x, H.y, H.z};
    float tlo0 = tmin, thi0 = tmax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float t0, t1;
        if (flags & (1u << a)) {  // the same for every ray
            t0 = fmaf(A[a].w, iv[a], -oi[a]);
            t1 = fmaf(hi[a], iv[a], -oi[a]);
        } else {
            const float oa = dot(f3{A[a].x, A[a].y, A[a].z}, o);
            const float ida = safe_rcp(dot(f3{A[a].x, A[a].y, A[a].z}, d));
            t0 = (A[a].w - oa) * ida;
            t1 = (hi[a] - oa) * ida;
        }
        tlo0 = vmax(tlo0, vmin(t0, t1));
        thi0 = vmin(thi0, vmax(t0, t1));
    }
    const float tlo = fmaf(-kCluEps, fabsf(tlo0), tlo0), thi = fmaf(kCluEps, fabsf(thi0), thi0);
    s->near |= (tlo <= thi) ? f2u(r[5].z) : 0u;
}

// After the last cluster: a pair in both masks counts as near only, and a ray
// with nothing near (the common one, which only sees the room's wall) takes
// its far candidates first.
RT_HD void clu_split_finish(CluSplit* s) {
    const uint32_t far = s->far & ~s->near;
    const bool promote = s->near == 0u;
    s->near = promote ? far : s->near;
    s->far = promote ? 0u : far;
}

// After the near tests: can a far candidate still hold a hit that wins against
// best?  The filter's own test of an exit face against thi <= best * (1 + 2^-16).
RT_HD bool clu_far_needed(float far_lo, float best) { return far_lo <= fmaf(kCluEps, fabsf(best), best); }

}  // namespace rt
