// rt_raydomain.h — the exactness domain of the batched ray queries
// (DESIGN.md §3.20), written once for the gfx950 query kernel (rt_rays.hip)
// and for the host (rt_api_host.cpp rt_debug_ray_domain).
//
// Every culling structure is padded by 4e-5 * extent, where extent is the
// larger of the scene's extent and the camera's distance from the origin
// (rt_scene.cpp compile_scene).  The proofs that an accepted hit lies inside
// the padded boxes cover rays of that scale; a ray outside it takes the
// id-ordered loop over the global records, which assumes nothing.
#pragma once

#include "rt_math.h"

namespace rt {

constexpr float kRayDirLen2Min = 0.25f;  // |d| in [1/2, 2]
constexpr float kRayDirLen2Max = 4.0f;
constexpr float kRayTmaxMax = 1000.0f;   // max_distance (sampling.metal:155)

struct RayDomain {
    float origin_max;  // max |origin component|: the extent the culling margin was taken from
    float dir_len2_min, dir_len2_max, tmax_max;
};

RT_HD RayDomain ray_domain(float extent) {
    return RayDomain{extent, kRayDirLen2Min, kRayDirLen2Max, kRayTmaxMax};
}

// True only for rays the accelerated layouts are proven for.  Every comparison
// is false for a NaN operand, so a NaN in any of the eight slots is out of the
// domain; an infinite origin fails its bound, an infinite direction the length
// bound, and tmax = +inf the last one.
RT_HD bool ray_in_domain(const RayDomain& D, f3 o, f3 d, float tmin, float tmax) {
    const bool o_ok = fabsf(o.x) <= D.origin_max && fabsf(o.y) <= D.origin_max && fabsf(o.z) <= D.origin_max;
    const float l2 = dot(d, d);
    const bool d_ok = l2 >= D.dir_len2_min && l2 <= D.dir_len2_max;
    const bool t_ok = tmin >= 0.0f && tmin < tmax && tmax <= D.tmax_max;
    return o_ok && d_ok && t_ok;
}

}  // namespace rt
