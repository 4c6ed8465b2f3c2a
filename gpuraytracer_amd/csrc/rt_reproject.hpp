// rt_reproject.hpp — the per-pixel arithmetic of temporal reprojection
// (include/rtpt.h rt_reproject), written once for the device
// kernel (rt_reproject.hip) and the host function (rt_reproject_host.cpp
// rt_reproject_host), so the two cannot drift apart.  fp32 under the
// arithmetic contract of rt_math.h: no contraction except the fmaf written
// down, IEEE division and sqrtf, dot in the contract's fma form.
//
// The function is total: any bytes in any buffer give a defined result.  The
// one place where data reaches an address is reproject_pixel's conversion of
// (fx, fy) to the tap corner, after the gates that bound it, and every tap is
// tested against the frame in integers before it is read.
#pragma once

#include <stddef.h>
#include <string.h>

#include "rt_math.h"

namespace rt {

constexpr uint32_t kReprojectTile = 16;          // pixels on a side of a workgroup's tile
constexpr uint32_t kReprojectHistoryMax = 65536;  // max_history at most

// The constants of one camera (rt_scene.hpp CamConst without the frame).
struct ReprojectCam {
    f3 pos, u, v, w;
    float halfW, halfH;
};

// Whole frames of W * H pixels; plane 1 is unused when PLANES == 1.
struct ReprojectArgs {
    const float* color[2];      // rgba32F: this frame's renders
    const float* history[2];    // rgba32F: (rgb mean, history length) of the previous frame
    float* out[2];              // rgba32F; out[k] may be color[k]
    const void* hit;            // (t, id) per pixel, 8 B: this frame's centre rays
    const float* normal_depth;  // (N.xyz, t)
    const void* prev_hit;       // the previous frame's two buffers
    const float* prev_normal_depth;
    ReprojectCam cam, prev;
    int32_t W, H;
    float max_history;          // (float)max_history, exact
    float normal_cos_min, plane_rel, weight_min;
};

struct ReprojectTexel {
    float x, y, z, w;
};
struct ReprojectHit {
    float t;
    int32_t id;
};

// One 16-B / 8-B access per texel on the device (the buffers are device
// allocations); the host makes no assumption about the caller's alignment.
RT_HD ReprojectTexel reproject_ld4(const float* p, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 v = reinterpret_cast<const float4*>(p)[i];
    return ReprojectTexel{v.x, v.y, v.z, v.w};
#else
    ReprojectTexel v;
    memcpy(&v, p + 4 * i, sizeof(v));
    return v;
#endif
}
RT_HD void reproject_st4(float* p, size_t i, float x, float y, float z, float w) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<float4*>(p)[i] = make_float4(x, y, z, w);
#else
    const ReprojectTexel v{x, y, z, w};
    memcpy(p + 4 * i, &v, sizeof(v));
#endif
}
RT_HD ReprojectHit reproject_ldhit(const void* p, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint2 v = static_cast<const uint2*>(p)[i];
    return ReprojectHit{__uint_as_float(v.x), (int32_t)v.y};
#else
    ReprojectHit v;
    memcpy(&v, static_cast<const char*>(p) + 8 * i, sizeof(v));
    return v;
#endif
}

// generateCameraRay through the centre of pixel (fx, fy): the operations of
// camera_dir (rt_pixel.hpp) at jitter (0.5, 0.5), the ray of RT_AOV_CENTER.
RT_HD f3 reproject_camera_dir(const ReprojectCam& C, float fW, float fH, float fx, float fy) {
    const float sx = ((fx + 0.5f) / fW) * 2.0f - 1.0f;
    const float ty = -(((fy + 0.5f) / fH) * 2.0f - 1.0f);
    const float sh = sx * C.halfW, th = ty * C.halfH;
    return normalize_ieee((C.u * sh + C.v * th) - C.w);
}

// Pixel (x, y) of the frame, 0 <= x < W, 0 <= y < H: steps 1-6 of §3.31.
template <int PLANES>
RT_HD void reproject_pixel(const ReprojectArgs& A, int32_t x, int32_t y) {
    const size_t W = (size_t)A.W;
    const size_t p = (size_t)y * W + (size_t)x;
    ReprojectTexel cur[PLANES];
#pragma unroll
    for (int k = 0; k < PLANES; ++k) cur[k] = reproject_ld4(A.color[k], p);
    const ReprojectHit hit = reproject_ldhit(A.hit, p);

    bool reuse = false;
    float sw = 0.0f, l[PLANES];
    f3 c[PLANES];
#pragma unroll
    for (int k = 0; k < PLANES; ++k) {
        l[k] = 0.0f;
        c[k] = f3{0.0f, 0.0f, 0.0f};
    }
    if (hit.id >= 0) {  // step 1
        const float fW = (float)A.W, fH = (float)A.H;
        const ReprojectTexel nz = reproject_ld4(A.normal_depth, p);
        const f3 N{nz.x, nz.y, nz.z};
        // step 2: the point shade() forms
        const f3 d = reproject_camera_dir(A.cam, fW, fH, (float)x, (float)y);
        const f3 X = A.cam.pos + d * hit.t;
        // step 3: its projection into the previous camera
        const f3 q = X - A.prev.pos;
        const float zc = -dot(q, A.prev.w);
        const float a = dot(q, A.prev.u) / zc, b = dot(q, A.prev.v) / zc;
        const float fx = (((a / A.prev.halfW) + 1.0f) * 0.5f) * fW - 0.5f;
        const float fy = ((1.0f - (b / A.prev.halfH)) * 0.5f) * fH - 0.5f;
        const float r = sqrtf(dot(q, q));
        // step 4: the gates, each false for a NaN
        const float nd = dot(N, d), nq = dot(N, q);
        const bool side = (nd < 0.0f && nq < 0.0f) || (nd >= 0.0f && nq >= 0.0f);
        const bool inside = fx >= -1.0f && fx < fW && fy >= -1.0f && fy < fH;
        if (side && zc > 0.0f && inside) {
            // step 5: -1 <= floor(f) <= f < 2^31, the conversions are defined
            const float flx = floorf(fx), fly = floorf(fy);
            const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;
            const float wx = fx - flx, wy = fy - fly;
            const float lim = A.plane_rel * r;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float bw = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
                    const int32_t xt = x0 + i, yt = y0 + j;  // at most 2^31 - 1: floor(f) < 2^31 - 1 for W < 2^31
                    if ((uint32_t)xt >= (uint32_t)A.W || (uint32_t)yt >= (uint32_t)A.H) continue;
                    const size_t pt = (size_t)yt * W + (size_t)xt;
                    const ReprojectHit ht = reproject_ldhit(A.prev_hit, pt);
                    if (ht.id != hit.id) continue;
                    const ReprojectTexel nt = reproject_ld4(A.prev_normal_depth, pt);
                    if (!(dot(N, f3{nt.x, nt.y, nt.z}) >= A.normal_cos_min)) continue;
                    const f3 dp = reproject_camera_dir(A.prev, fW, fH, (float)xt, (float)yt);
                    const f3 Xp = A.prev.pos + dp * ht.t;
                    if (!(fabsf(dot(N, Xp - X)) <= lim)) continue;
                    sw += bw;
#pragma unroll
                    for (int k = 0; k < PLANES; ++k) {
                        const ReprojectTexel h = reproject_ld4(A.history[k], pt);
                        c[k] = f3{fmaf(bw, h.x, c[k].x), fmaf(bw, h.y, c[k].y), fmaf(bw, h.z, c[k].z)};
                        l[k] = fmaf(bw, h.w, l[k]);
                    }
                }
            }
            reuse = sw >= A.weight_min;
        }
    }
    // step 6
    const float rw = reuse ? 1.0f / sw : 0.0f;
#pragma unroll
    for (int k = 0; k < PLANES; ++k) {
        if (!reuse) {
            reproject_st4(A.out[k], p, cur[k].x, cur[k].y, cur[k].z, 1.0f);
            continue;
        }
        const f3 h = c[k] * rw;
        const float m1 = l[k] * rw + 1.0f;
        const float n = m1 < A.max_history ? m1 : A.max_history;  // a NaN length: max_history
        const float al = 1.0f / n;
        reproject_st4(A.out[k], p, fmaf(al, cur[k].x - h.x, h.x), fmaf(al, cur[k].y - h.y, h.y),
                      fmaf(al, cur[k].z - h.z, h.z), n);
    }
}

}  // namespace rt
