// rt_reproject_host.cpp — the device-free part of temporal reprojection
// (include/rtpt.h): the defaults, the argument checks that rt_reproject and
// rt_reproject_host share, and rt_reproject_host itself, the per-pixel
// function of rt_reproject.hpp over the frame on the calling thread.  Apart
// from rtapi::fail (the error slot) it needs rt_camera.cpp only, so a
// stand-alone sanitizer program can link it (tools/reproject_host_check.cpp).
#include <string.h>

#include "rt_api_internal.hpp"

namespace rtapi {

std::string reproject_check(const rt_reproject_params* p, const rt_reproject_buffers* b, uint32_t flags_ok,
                            uint32_t* planes) {
    static_assert(sizeof(rt_reproject_params) == 32 && sizeof(rt_reproject_buffers) == 80 &&
                      offsetof(rt_reproject_buffers, hit) == 32 && offsetof(rt_reproject_buffers, out) == 64,
                  "rt_reproject_params / rt_reproject_buffers layout");
    if (!p) return "params is null";
    if (!b) return "buffers is null";
    const void* need[7] = {b->color[0], b->history[0], b->hit, b->normal_depth, b->prev_hit, b->prev_normal_depth,
                           b->out[0]};
    static const char* const names[7] = {"color[0]", "history[0]", "hit", "normal_depth", "prev_hit",
                                         "prev_normal_depth", "out[0]"};
    for (int k = 0; k < 7; ++k)
        if (!need[k]) return std::string(names[k]) + " is null";
    const int second = (b->color[1] ? 1 : 0) + (b->history[1] ? 1 : 0) + (b->out[1] ? 1 : 0);
    if (second != 0 && second != 3) return "color[1], history[1] and out[1] must be all null or all non-null";
    if (p->max_history < 1 || p->max_history > rt::kReprojectHistoryMax) return "max_history must be in [1, 65536]";
    if (!(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f)) return "normal_cos_min must be in [-1, 1]";
    if (!(p->plane_rel >= 0.0f)) return "plane_rel must be >= 0";
    if (!(p->weight_min > 0.0f && p->weight_min <= 1.0f)) return "weight_min must be in (0, 1]";
    if (p->flags & ~flags_ok) return "unknown flag bits";
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return "reserved must be 0";
    *planes = second ? 2u : 1u;
    return std::string();
}

namespace {
rt::ReprojectCam reproject_cam(const rt::CamConst& c) {
    return rt::ReprojectCam{rt::f3{c.pos[0], c.pos[1], c.pos[2]}, rt::f3{c.u[0], c.u[1], c.u[2]},
                            rt::f3{c.v[0], c.v[1], c.v[2]}, rt::f3{c.w[0], c.w[1], c.w[2]}, c.halfW, c.halfH};
}
}  // namespace

bool reproject_args(const rt_reproject_params* p, const rt_reproject_buffers* b, const rt::CamConst& cam,
                    const CameraGPU* prev, rt::ReprojectArgs* A, std::string* why) {
    rt::CamConst pc = cam;
    if (prev) {
        const char* err = nullptr;
        if (!rt::compile_camera(*prev, &pc, &err)) {
            *why = std::string("prev_camera: ") + err;
            return false;
        }
        if (pc.W != cam.W || pc.H != cam.H) {
            *why = "prev_camera: resolution differs from the current camera's";
            return false;
        }
    }
    memset(A, 0, sizeof(*A));
    for (int k = 0; k < 2; ++k) {
        A->color[k] = b->color[k];
        A->history[k] = b->history[k];
        A->out[k] = b->out[k];
    }
    A->hit = b->hit;
    A->normal_depth = b->normal_depth;
    A->prev_hit = b->prev_hit;
    A->prev_normal_depth = b->prev_normal_depth;
    A->cam = reproject_cam(cam);
    A->prev = reproject_cam(pc);
    A->W = cam.W;
    A->H = cam.H;
    A->max_history = (float)p->max_history;
    A->normal_cos_min = p->normal_cos_min;
    A->plane_rel = p->plane_rel;
    A->weight_min = p->weight_min;
    return true;
}

}  // namespace rtapi

using namespace rtapi;

void rt_reproject_params_default(rt_reproject_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_history = 32;
    p->normal_cos_min = 0.9f;
    p->plane_rel = 0x1p-7f;
    p->weight_min = 0.0625f;
}

int rt_reproject_host(const CameraGPU* camera, const CameraGPU* prev_camera, const rt_reproject_params* p,
                      const rt_reproject_buffers* b) {
    uint32_t planes = 0;
    const std::string bad = reproject_check(p, b, 0u, &planes);
    if (!bad.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_reproject_host: " + bad);
    if (!camera) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_reproject_host: camera is null");
    rt::CamConst cam;
    const char* err = nullptr;
    if (!rt::compile_camera(*camera, &cam, &err))
        return fail(nullptr, RT_ERR_INVALID_ARG, std::string("rt_reproject_host: camera: ") + err);
    rt::ReprojectArgs A;
    std::string why;
    if (!reproject_args(p, b, cam, prev_camera, &A, &why))
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_reproject_host: " + why);
    for (int32_t y = 0; y < A.H; ++y)
        for (int32_t x = 0; x < A.W; ++x) {
            if (planes == 2)
                rt::reproject_pixel<2>(A, x, y);
            else
                rt::reproject_pixel<1>(A, x, y);
        }
    return RT_OK;
}
