// rt_beam.hpp — which pair records the camera rays of a pixel rectangle can hit
// (DESIGN.md §3.16).  One source text for the gfx950 kernel (rt_kernel.hip: the
// per-wave candidate mask of the bounce-0 closest query) and for the host
// (rt_api_host.cpp rt_debug_camera_candidates, the CPU tests).
//
// Every camera ray of the rectangle starts at the camera position and its
// un-normalised direction (cu*sh + cv*th) - cw is affine in (sh, th), so the
// rays fill a four-sided pyramid (the beam) with its apex at the camera.  sh and
// th are monotone float functions of x + jx and y + jy (correctly rounded
// +, /, *), so the kernel's own expressions at the rectangle's ends bound them.
// A pair is left out only when a plane through the apex separates the beam
// from the pair's two triangles, inflated by the padding of the record's AABB
// (an accepted hit point lies within that padding of its quad):
//   A  one of the beam's four side planes has all four padded corners outside;
//   B  for each triangle, a plane through the apex and one of its edges has
//      the triangle on one side and the four beam corner directions on the
//      other, by more than the angle the padding subtends at the nearest point
//      of the padded AABB.
// Every comparison is written so that a NaN, an overflow or a degenerate case
// keeps the pair.  Only speed depends on the outcome: a kept pair is tested
// with the exact test (rt_trace.hpp pair_test_rank).
#pragma once

#include "rt_math.h"

namespace rt {

constexpr float kBeamEps = 1.52587890625e-05f;  // 2^-16 relative slack (as cluster_candidates)

// generateCameraRay's image-plane coordinates (rt_kernel.hip, sampling.metal:125-157)
RT_HD float beam_sh(float fx, float jx, float fW, float halfW) { return (((fx + jx) / fW) * 2.0f - 1.0f) * halfW; }
RT_HD float beam_th(float fy, float jy, float fH, float halfH) { return (-(((fy + jy) / fH) * 2.0f - 1.0f)) * halfH; }

struct Beam {
    f3 apex;
    f3 fwd;       // -cw: the view axis
    f3 b[4];      // corner directions (sh0,th0) (sh1,th0) (sh1,th1) (sh0,th1), as the kernel forms them
    float bl[4];  // their lengths
    f3 n[4];      // inward normals of the side planes sh >= sh0, sh <= sh1, th >= th0, th <= th1
    float nl[4];  // their lengths
    bool ok;      // false: nothing can be decided (every pair stays)
};

// The beam of the pixels [x0, x1] x [y0, y1] (closed, pixel coordinates as the
// kernel's floats) with jitters in [0, 1].
RT_HD Beam make_beam(f3 pos, f3 cu, f3 cv, f3 cw, float halfW, float halfH, float fW, float fH, float x0,
                     float x1, float y0, float y1) {
    Beam B;
    B.apex = pos;
    B.fwd = -cw;
    const float sa = beam_sh(x0, 0.0f, fW, halfW), sb = beam_sh(x1, 1.0f, fW, halfW);
    const float ta = beam_th(y0, 0.0f, fH, halfH), tb = beam_th(y1, 1.0f, fH, halfH);
    const float sh0 = fminf(sa, sb), sh1 = fmaxf(sa, sb), th0 = fminf(ta, tb), th1 = fmaxf(ta, tb);
    B.b[0] = (cu * sh0 + cv * th0) - cw;
    B.b[1] = (cu * sh1 + cv * th0) - cw;
    B.b[2] = (cu * sh1 + cv * th1) - cw;
    B.b[3] = (cu * sh0 + cv * th1) - cw;
    // the side plane sh = s holds the directions cu*s + cv*th - cw of every th:
    // it is spanned by cv and cu*s - cw (two vectors far from parallel, so the
    // cross product is well conditioned, unlike that of two beam corners);
    // x = g*(cu*s - cw) + b*cv + e*cu lies on the side of cu by the sign of e
    B.n[0] = cross(cv, cu * sh0 - cw);
    B.n[1] = cross(cv, cu * sh1 - cw);
    B.n[2] = cross(cu, cv * th0 - cw);
    B.n[3] = cross(cu, cv * th1 - cw);
    const float o0 = dot(B.n[0], cu), o1 = dot(B.n[1], cu), o2 = dot(B.n[2], cv), o3 = dot(B.n[3], cv);
    if (o0 < 0.0f) B.n[0] = -B.n[0];  // inside: toward +cu
    if (o1 > 0.0f) B.n[1] = -B.n[1];  // inside: toward -cu
    if (o2 < 0.0f) B.n[2] = -B.n[2];
    if (o3 > 0.0f) B.n[3] = -B.n[3];
    bool ok = o0 != 0.0f && o1 != 0.0f && o2 != 0.0f && o3 != 0.0f && sh0 <= sh1 && th0 <= th1;
    for (int i = 0; i < 4; ++i) {
        B.bl[i] = sqrtf(dot(B.b[i], B.b[i]));
        B.nl[i] = sqrtf(dot(B.n[i], B.n[i]));
        // finite and non-zero; the corner directions point forward
        ok = ok && B.bl[i] > 0.0f && B.bl[i] < 1e30f && B.nl[i] > 0.0f && B.nl[i] < 1e30f &&
             dot(B.b[i], B.fwd) > 0.0f;
    }
    B.ok = ok;
    return B;
}

// Test B for one edge (p, q) of a triangle whose third corner is r (all
// relative to the apex): true when the plane through the apex, p and q has
// the triangle on one side and the beam beyond it by more than rho (the sine
// of the angle the padding subtends) plus the slack.
RT_HD bool beam_edge_separates(const Beam& B, f3 p, f3 q, f3 r, float lp, float lq, float lr, float rho) {
    f3 n = cross(p, q);
    const float nl = sqrtf(dot(n, n));
    const float s = dot(n, r);
    // the rounding of cross(p, q) tilts the plane by ~2^-22 |p||q| / |n|
    const float slack = kBeamEps + 9.5367431640625e-07f * ((lp * lq) / nl);
    if (!(fabsf(s) > slack * (nl * lr))) return false;  // the triangle's plane passes (almost) through the apex
    if (s > 0.0f) n = -n;                                // the triangle lies in n.x <= 0
    const float lim = (rho + slack) * nl;
    bool sep = true;
    for (int j = 0; j < 4; ++j) sep = sep && dot(n, B.b[j]) > lim * B.bl[j];
    return sep;
}

// True when no camera ray of the beam can have an accepted hit on the pair
// record q (28 floats, rt_scene.hpp PairIsect).
RT_HD bool beam_excludes_pair(const Beam& B, const float* q) {
    if (!B.ok) return false;
    const f3 v0{q[0], q[1], q[2]}, S{q[3], q[4], q[5]}, eA{q[6], q[7], q[8]}, eB{q[12], q[13], q[14]};
    const f3 lo{q[20], q[21], q[22]}, hi{q[23], q[24], q[25]};
    const f3 w[4] = {v0, v0 + S, v0 + eA, v0 + eB};  // the pair's corners (the shared edge is w0-w1)
    // the padding the AABB carries: its faces against the corners' extent; an
    // accepted hit point lies within it of the quad along every axis, so within
    // 2 x pad (> sqrt(3) x pad, and the rounding of the corners) in distance
    f3 mn = w[0], mx = w[0];
    for (int j = 1; j < 4; ++j) {
        mn = f3{fminf(mn.x, w[j].x), fminf(mn.y, w[j].y), fminf(mn.z, w[j].z)};
        mx = f3{fmaxf(mx.x, w[j].x), fmaxf(mx.y, w[j].y), fmaxf(mx.z, w[j].z)};
    }
    const float pad = fmaxf(fmaxf(fmaxf(mn.x - lo.x, mn.y - lo.y), mn.z - lo.z),
                            fmaxf(fmaxf(hi.x - mx.x, hi.y - mx.y), hi.z - mx.z));
    if (!(pad >= 0.0f && pad < 1e30f)) return false;
    const float R = 2.0f * pad;
    f3 c[4];
    float cl[4];
    const float fl = sqrtf(dot(B.fwd, B.fwd));
    for (int j = 0; j < 4; ++j) {
        c[j] = w[j] - B.apex;
        cl[j] = sqrtf(dot(c[j], c[j]));
        // a corner at or behind the plane through the camera across the view axis: keep
        if (!(dot(B.fwd, c[j]) > (R + kBeamEps * cl[j]) * fl)) return false;
    }
    // A: a side plane of the beam with the padded quad outside
    for (int i = 0; i < 4; ++i) {
        bool out = true;
        for (int j = 0; j < 4; ++j) out = out && dot(B.n[i], c[j]) < -((R + kBeamEps * cl[j]) * B.nl[i]);
        if (out) return true;
    }
    // B: per triangle, a plane through the apex and an edge.  Every accepted
    // hit point lies in the padded AABB, at least dmin from the apex.
    const f3 a = B.apex;
    const f3 g{fmaxf(fmaxf(lo.x - a.x, a.x - hi.x), 0.0f), fmaxf(fmaxf(lo.y - a.y, a.y - hi.y), 0.0f),
               fmaxf(fmaxf(lo.z - a.z, a.z - hi.z), 0.0f)};
    const float dmin = sqrtf(dot(g, g));
    if (!(dmin > R)) return false;
    const float rho = R / (dmin * (1.0f - kBeamEps));
    const bool ta = beam_edge_separates(B, c[0], c[1], c[2], cl[0], cl[1], cl[2], rho) ||
                    beam_edge_separates(B, c[1], c[2], c[0], cl[1], cl[2], cl[0], rho) ||
                    beam_edge_separates(B, c[2], c[0], c[1], cl[2], cl[0], cl[1], rho);
    if (!ta) return false;
    return beam_edge_separates(B, c[0], c[1], c[3], cl[0], cl[1], cl[3], rho) ||
           beam_edge_separates(B, c[1], c[3], c[0], cl[1], cl[3], cl[0], rho) ||
           beam_edge_separates(B, c[3], c[0], c[1], cl[3], cl[0], cl[1], rho);
}

}  // namespace rt
