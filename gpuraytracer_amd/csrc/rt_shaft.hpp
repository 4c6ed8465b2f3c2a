// rt_shaft.hpp — which pair records the bounce-0 shadow rays of a pixel
// rectangle can hit.  One source text for the gfx950 kernel
// (rt_kernel.hip: the per-wave occluder mask of the bounce-0 shadow query) and
// for the host (rt_api_host.cpp rt_debug_shadow_candidates, the CPU tests).
//
// The bounce-0 shadow segments of a wave start at the camera rays' hit points,
// lifted by the shading normal, and end inside the light patch.  The hit
// points on one triangle lie in the footprint of the wave's beam (rt_beam.hpp)
// on that triangle's plane, a convex quadrilateral, so every segment lies in
// the shaft hull(footprint + N*1e-3, light patch), cut short of the light by
// the 1e-3 that shade() takes off tmax.  A target pair is left out only when
// an axis separates that shaft from each of its two triangles by more than
// the inflation (the target's padding and the rounding of the hit point; the
// source side uses the triangle's plane only, so its padding does not enter):
//   a  the target triangle's own normal;
//   b  a world axis: the shaft's extent against the record's padded AABB;
//   c  cross(edge of the target triangle, source centre -> light corner);
//   d  (no axis) a triangle in the light's own plane, by the cut of tmax.
// Any axis is conservative: both sets are projected with the axis as it was
// rounded.  Every comparison is written so that a NaN, an overflow or a
// degenerate case keeps the pair.  Only speed depends on the outcome.
#pragma once

#include "rt_beam.hpp"

namespace rt {

// Which families are compiled in (bit 0: a, bit 1: b, bit 2: c, bit 3: d).
// Every subset is conservative.  The switch exists for the family table of
// profiles/r8/ab_results.md: rt_api.cpp built with -DRT_SHAFT_FAM=n and
// tools/shadow_mask_stats.py run against that library (RTPT_LIB).
#ifndef RT_SHAFT_FAM
#define RT_SHAFT_FAM 15
#endif

constexpr float kShaftEps = 3.814697265625e-06f;  // 2^-18 relative slack
constexpr float kShaftBig = 1e15f;                // products of two such magnitudes stay finite

// The light patch: q of shade() (rt_kernel.hip) at ux, uy = +-1, in both of
// its forms; they may differ in the sign of a zero only.
struct ShaftLight {
    f3 q[4];     // (-,-) (+,-) (+,+) (-,+)
    float qmax;  // largest |q|
    bool ok;
};

RT_HD ShaftLight shaft_light(f3 c) {
    ShaftLight L;
    L.ok = true;
    L.qmax = 0.0f;
    for (int i = 0; i < 4; ++i) {
        const float ux = (i == 1 || i == 2) ? 1.0f : -1.0f, uy = i >= 2 ? 1.0f : -1.0f;
        const f3 a{c.x + 0.25f * ux, c.y, c.z + 0.25f * uy};                                // light_plain
        const f3 b = (c + f3{0.25f, 0.0f, 0.0f} * ux) + f3{0.0f, 0.0f, 0.25f} * uy;       // literal
        L.q[i] = a;
        const float l = sqrtf(dot(a, a));
        L.ok = L.ok && a.x == b.x && a.y == b.y && a.z == b.z && l < kShaftBig;
        L.qmax = fmaxf(L.qmax, l);
    }
    return L;
}

// The padding a pair record's AABB carries (as beam_excludes_pair recovers
// it) and the record's corners.
RT_HD float shaft_pair_pad(const float* q, f3 w[4]) {
    const f3 v0{q[0], q[1], q[2]}, S{q[3], q[4], q[5]}, eA{q[6], q[7], q[8]}, eB{q[12], q[13], q[14]};
    const f3 lo{q[20], q[21], q[22]}, hi{q[23], q[24], q[25]};
    w[0] = v0;
    w[1] = v0 + S;
    w[2] = v0 + eA;
    w[3] = v0 + eB;
    f3 mn = w[0], mx = w[0];
    for (int j = 1; j < 4; ++j) {
        mn = f3{fminf(mn.x, w[j].x), fminf(mn.y, w[j].y), fminf(mn.z, w[j].z)};
        mx = f3{fmaxf(mx.x, w[j].x), fmaxf(mx.y, w[j].y), fmaxf(mx.z, w[j].z)};
    }
    return fmaxf(fmaxf(fmaxf(mn.x - lo.x, mn.y - lo.y), mn.z - lo.z),
                 fmaxf(fmaxf(hi.x - mx.x, hi.y - mx.y), hi.z - mx.z));
}

// The source set of one triangle of a pair the wave's camera rays can hit.
struct ShaftSrc {
    f3 p[4];     // the beam's footprint on the triangle's plane + N*1e-3
    f3 pc;       // their mean
    float rho;   // every shadow segment point lies within rho of the shaft
    float smax;  // ... at a parameter s <= smax < 1 of its segment p -> q
    float xmax;  // largest |p|, |q|
    float dmax;  // no segment is longer
    bool ok;     // false: nothing is decided for the wave
};

// rec: the source pair's record; tb: 0 its triangle A, 1 its triangle B;
// N: the shading normal of that triangle (tri_shade).
RT_HD ShaftSrc shaft_source(const Beam& B, const float* rec, int tb, f3 N, const ShaftLight& L) {
    ShaftSrc S;
    const f3 v0{rec[0], rec[1], rec[2]};
    const f3 n = tb ? f3{rec[15], rec[16], rec[17]} : f3{rec[9], rec[10], rec[11]};
    const float nl = sqrtf(dot(n, n));
    const float num = dot(n, v0 - B.apex);
    const float al = sqrtf(dot(B.apex, B.apex)), vl = sqrtf(dot(v0, v0));
    bool ok = B.ok && L.ok && nl > 0.0f && nl < kShaftBig && al < kShaftBig && vl < kShaftBig;
    const float den0 = dot(n, B.b[0]);
    float cmin = 1e30f, pmax = 0.0f;
    f3 sum{0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; ++i) {
        const float den = dot(n, B.b[i]);
        const float t = num / den;
        // one sign, clear of zero; the plane is crossed in front of the camera
        ok = ok && fabsf(den) > kBeamEps * (nl * B.bl[i]) && (den > 0.0f) == (den0 > 0.0f) && t > 0.0f && t < kShaftBig;
        S.p[i] = (B.apex + B.b[i] * t) + N * 1e-3f;
        sum = sum + S.p[i];
        cmin = fminf(cmin, fabsf(den) / (nl * B.bl[i]));
        const float pl = sqrtf(dot(S.p[i], S.p[i]));
        ok = ok && pl < kShaftBig;
        pmax = fmaxf(pmax, pl);
    }
    S.pc = sum * 0.25f;
    // the longest segment: |q - p| <= |q - p0| + |p - p0|
    float dq = 0.0f, dp = 0.0f;
    for (int j = 0; j < 4; ++j) {
        const f3 a = L.q[j] - S.p[0], b = S.p[j] - S.p[0];
        dq = fmaxf(dq, sqrtf(dot(a, a)));
        dp = fmaxf(dp, sqrtf(dot(b, b)));
    }
    const float dmax = (dq + dp) * 1.001f;
    S.dmax = dmax;
    S.smax = 1.0f - 1e-3f / dmax;
    ok = ok && dmax > 2e-3f && S.smax > 0.0f && S.smax < 1.0f;
    S.xmax = fmaxf(pmax, L.qmax);
    // rounding of the hit point (o + d*t) + N*1e-3 and of p[] above: a few
    // 2^-24 of the scale across the plane, over the cosine along the ray
    const float scale = (al + vl) + 2.0f * (pmax + L.qmax);
    S.rho = kShaftEps * (scale / cmin);
    ok = ok && S.rho >= 0.0f && S.rho < 1e30f;
    S.ok = ok;
    return S;
}

// Extremes of x -> dot(n, x) over the four source points (pl, ph) and the
// four light corners (ql, qh).
RT_HD void shaft_extents(const ShaftSrc& S, const ShaftLight& L, f3 n, float* pl, float* ph, float* ql,
                         float* qh) {
    *pl = *ph = dot(n, S.p[0]);
    *ql = *qh = dot(n, L.q[0]);
    for (int i = 1; i < 4; ++i) {
        const float a = dot(n, S.p[i]), b = dot(n, L.q[i]);
        *pl = fminf(*pl, a);
        *ph = fmaxf(*ph, a);
        *ql = fminf(*ql, b);
        *qh = fmaxf(*qh, b);
    }
}

// Range of x -> dot(n, x) over the shaft's segments p + s*(q - p), s in [0, smax].
RT_HD void shaft_range(const ShaftSrc& S, const ShaftLight& L, f3 n, float* lo, float* hi) {
    float pl, ph, ql, qh;
    shaft_extents(S, L, n, &pl, &ph, &ql, &qh);
    *lo = fminf(pl, pl + S.smax * (ql - pl));
    *hi = fmaxf(ph, ph + S.smax * (qh - ph));
}

// True when the axis n separates the shaft from the triangle (a, b, c) by
// more than m (a distance) and the rounding of the projections.
RT_HD bool shaft_axis_separates(const ShaftSrc& S, const ShaftLight& L, f3 n, f3 a, f3 b, f3 c, float m,
                                float wmax) {
    const float nl = sqrtf(dot(n, n));
    if (!(nl > 1e-30f && nl < kShaftBig)) return false;
    float lo, hi;
    shaft_range(S, L, n, &lo, &hi);
    const float ta = dot(n, a), tb = dot(n, b), tc = dot(n, c);
    const float tlo = fminf(fminf(ta, tb), tc), thi = fmaxf(fmaxf(ta, tb), tc);
    const float gap = (m + kShaftEps * (S.xmax + wmax)) * nl;
    return lo - thi > gap || tlo - hi > gap;
}

// d: a triangle in whose plane the light patch lies (the light's own pair).
// Every segment ends on that plane, so the exact crossing is at t = dist and
// only tmax = dist - 1e-3 keeps it out: with the patch within eta of the plane
// through the record's v0 and the rounding of t below kShaftEps * scale, both
// over the cosine between segment and normal, the computed t stays above tmax
// when that cosine is bounded away from zero over the whole shaft.
RT_HD bool shaft_ends_on_plane(const ShaftSrc& S, const ShaftLight& L, f3 n, f3 v0, float wmax) {
    const float nl = sqrtf(dot(n, n));
    if (!(nl > 1e-30f && nl < kShaftBig)) return false;
    float pl, ph, ql, qh;
    shaft_extents(S, L, n, &pl, &ph, &ql, &qh);
    const float t0 = dot(n, v0);
    const float eta = fmaxf(fabsf(qh - t0), fabsf(ql - t0)) / nl;
    const float gap = fmaxf(ql - ph, pl - qh) - (S.rho + kShaftEps * S.xmax) * nl;
    const float cosmin = gap / (nl * (S.dmax + S.rho));
    // t > tmax = fl(dist - 1e-3) needs (eta + rounding)/cos + 2^-23 * dist < 1e-3:
    // half of the 1e-3 for the first term, what the second leaves of the other half
    const float tround = 1.1920929e-07f * S.dmax;
    return tround < 0.5e-3f && eta + kShaftEps * (3.0f * S.xmax + wmax) < (0.5e-3f - tround) * cosmin;
}

// ma: the margin along the triangle's own normal n (the record's, the one
// pair_t divides by): across its plane an accepted t is off only by its
// rounding, not by the padding.  m: the margin along any other axis.
RT_HD bool shaft_misses_triangle(const ShaftSrc& S, const ShaftLight& L, f3 n, f3 a, f3 b, f3 c, float ma,
                                 float m, float wmax) {
    if ((RT_SHAFT_FAM & 1) && shaft_axis_separates(S, L, n, a, b, c, ma, wmax)) return true;
    if ((RT_SHAFT_FAM & 8) && shaft_ends_on_plane(S, L, n, a, wmax)) return true;
    if (RT_SHAFT_FAM & 4) {
        const f3 e[3] = {b - a, c - b, a - c};
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 4; ++j)
                if (shaft_axis_separates(S, L, cross(e[k], L.q[j] - S.pc), a, b, c, m, wmax)) return true;
    }
    return false;
}

// True when no bounce-0 shadow segment that starts on the source triangle S
// can have an accepted hit on the pair record q (28 floats, PairIsect).
RT_HD bool shaft_excludes_pair(const ShaftSrc& S, const ShaftLight& L, const float* q) {
    if (!S.ok) return false;
    f3 w[4];
    const float pad = shaft_pair_pad(q, w);
    if (!(pad >= 0.0f && pad < 1e30f)) return false;
    float wmax = 0.0f;
    for (int j = 0; j < 4; ++j) wmax = fmaxf(wmax, sqrtf(dot(w[j], w[j])));
    if (!(wmax < kShaftBig)) return false;
    if (RT_SHAFT_FAM & 2) {
        // b: every accepted hit point lies in the record's padded AABB
        const float lo[3] = {q[20], q[21], q[22]}, hi[3] = {q[23], q[24], q[25]};
        const float gap = S.rho + kShaftEps * (S.xmax + wmax);
        for (int a = 0; a < 3; ++a) {
            float slo, shi;
            shaft_range(S, L, f3{a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f}, &slo, &shi);
            if (slo - hi[a] > gap || lo[a] - shi > gap) return true;
        }
    }
    // an accepted hit point lies within 2*pad of its triangle (DESIGN.md
    // §3.16), and within the rounding of t of its plane
    const float m = S.rho + 2.0f * pad;
    const float ma = S.rho + kShaftEps * (3.0f * S.xmax + wmax);
    const f3 nA{q[9], q[10], q[11]}, nB{q[15], q[16], q[17]};
    return shaft_misses_triangle(S, L, nA, w[0], w[1], w[2], ma, m, wmax) &&
           shaft_misses_triangle(S, L, nB, w[0], w[1], w[3], ma, m, wmax);
}

}  // namespace rt
