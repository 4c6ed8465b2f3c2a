// rt_camera.cpp — the camera constants of generateCameraRay
// (sampling.metal:125-157), validated and computed once per camera on the
// host: the camera part of the scene compile (rt_scene.cpp compile_scene), and
// what rt_reproject makes of the previous frame's camera.  Host code only:
// halfW comes from the host libm tanf, everything else from the contract ops
// of rt_math.h.
#include "rt_scene.hpp"

namespace rt {

namespace {
f3 from_abi3(const rt_float3& v) { return f3{v.x, v.y, v.z}; }
bool finite3(const rt_float3& v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
}  // namespace

bool compile_camera(const CameraGPU& cam, CamConst* out, const char** err) {
    if (cam.resolution.x <= 0 || cam.resolution.y <= 0) {
        *err = "camera resolution must be positive";
        return false;
    }
    if (cam.resolution.x / cam.resolution.y == 0) {
        // aspectRatio = float(res.x / res.y) (sampling.metal:132) would be 0 and
        // halfHeight infinite: every ray NaN.  Reject instead of rendering NaNs.
        *err = "camera resolution.x < resolution.y gives aspectRatio 0 (integer division)";
        return false;
    }
    if (!finite3(cam.position) || !finite3(cam.direction) || !finite3(cam.up)) {
        *err = "camera vectors must be finite";
        return false;
    }
    CamConst& c = *out;
    c.W = cam.resolution.x;
    c.H = cam.resolution.y;
    const float aspect = (float)(cam.resolution.x / cam.resolution.y);  // :132
    c.halfW = tanf(cam.horizontalFov / 2.0f);                            // :133
    c.halfH = c.halfW / aspect;                                          // :134
    const f3 w = -normalize(from_abi3(cam.direction));                   // :137
    const f3 u = normalize(cross(from_abi3(cam.up), w));                 // :138
    const f3 v = normalize(cross(w, u));                                 // :139
    // The same rule as for the portrait frame: a camera whose derived constants
    // are not all finite makes every camera ray NaN.  Reject instead of rendering NaNs.
    if (!isfinite(c.halfW) || !isfinite(c.halfH)) {
        *err = "camera horizontalFov: tan(horizontalFov / 2) is not finite";
        return false;
    }
    const auto unit = [](const f3& a) { return dot(a, a) > 0.5f && isfinite(dot(a, a)); };  // false for NaN
    if (!unit(w)) {
        *err = "camera direction: normalize(direction) is not a unit vector (zero length, or its square overflows)";
        return false;
    }
    // cross(up, w) of an up along an oblique direction is rounding noise of w, which
    // normalizes to some finite roll: the inputs' own cross product tells (in double
    // a product of two floats is exact and cannot underflow)
    const double ux = cam.up.x, uy = cam.up.y, uz = cam.up.z;
    const double dx = cam.direction.x, dy = cam.direction.y, dz = cam.direction.z;
    const bool parallel = uy * dz == uz * dy && uz * dx == ux * dz && ux * dy == uy * dx;
    if (!unit(u) || !unit(v) || parallel) {
        *err = "camera up: cross(up, -direction) does not normalize (up is zero, or parallel to direction)";
        return false;
    }
    const f3 p = from_abi3(cam.position);
    c.pos[0] = p.x; c.pos[1] = p.y; c.pos[2] = p.z;
    c.u[0] = u.x; c.u[1] = u.y; c.u[2] = u.z;
    c.v[0] = v.x; c.v[1] = v.y; c.v[2] = v.z;
    c.w[0] = w.x; c.w[1] = w.y; c.w[2] = w.z;
    return true;
}

}  // namespace rt
