// rt_api_internal.hpp — what the two halves of the C-ABI share: rt_api.cpp
// (every entry point that takes or makes an rt_ctx) and rt_api_host.cpp (the
// entry points that need neither a context nor a stream).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/rtpt.h"
#include "rt_kernel.hpp"
#include "rt_plan.hpp"
#include "rt_reproject.hpp"
#include "rt_scene.hpp"

namespace rtapi {

// RT_TRI_BVH_DEFAULT resolves to this build: the GPU binned SAH builds the host
// build's tree (same rules, same render rate) in a tenth of the time or less --
// the measured build times and rates are in DESIGN.md §5 and profiles/
constexpr uint32_t kDefaultTriBuild = RT_TRI_BVH_GPU_SAH;

// The message goes to the context, or without one to the calling thread's
// create-error slot (rt_last_error(NULL)); rt_api.cpp holds both.
int fail(rt_ctx* ctx, int status, const std::string& msg);

inline int hip_fail(rt_ctx* ctx, int status, const char* what, hipError_t e) {
    return fail(ctx, status, std::string(what) + ": " + hipGetErrorString(e));
}

// rt_create_options (include/rtpt.h) -> the context's choices and the host
// builds' options.  False (with *why) for a value outside its range.
struct Resolved {
    uint32_t lanes = 0, tri_build = RT_TRI_BVH_HOST_SAH, walk = RT_WALK_AUTO, walk_leaf_den = 0;
    rt::SceneMem mem = rt::SceneMem::kAuto;
    uint32_t tri_leaf_max = rt::kTriLeafMax;
    double tri_leaf_cost = 1.0;
    rt::BuildOptions build;
};
bool resolve_options(const rt_create_options* o, Resolved* r, const char** why);

// A scene description that compile_desc may read (n_square_lights is the
// business of the entry points that create or update a context).
inline bool desc_ok(const rt_scene_desc* d) { return d && d->camera && d->square_lights; }

inline bool compile_desc(const rt_scene_desc* d, const rt::BuildOptions& build, rt::CompiledScene* s,
                         const char** err) {
    return rt::compile_scene(*d->camera, d->materials, d->vertices, d->n_triangles, d->square_lights[0], d->spheres,
                             d->n_spheres, s, err, build);
}

// The counts of a compiled scene's tables (rt_kernel.hpp SceneTables), which
// every layout choice is made from; the pointers stay null.
// nTN: triangle-BVH nodes per layout (0: none).
inline rt::SceneTables scene_counts(const rt::CompiledScene& s, uint32_t nTN) {
    rt::SceneTables t{};
    t.nT = (uint32_t)s.tri_isect.size();
    t.nP = (uint32_t)s.pair_isect.size();
    t.nS = (uint32_t)s.sph_isect.size();
    t.nN = s.sph_layout_nodes;
    t.nTN = nTN;
    t.nC = (uint32_t)(s.clusters.size() / (4 * rt::kCluF4));
    t.pair_free = s.pair_free_mask;
    return t;
}

// rt_create's rule: a triangle BVH above kTriBvhMinTriangles or when the
// records do not fit the LDS layouts, or when the layout is forced.
inline bool needs_tri_bvh(const rt::SceneTables& t, rt::SceneMem mem) {
    const size_t lds_pairs = rt::kernel_lds_bytes(t.nT, t.nP, 0, 0);
    const size_t lds_single = rt::kernel_lds_bytes(t.nT, 0, 0, 0);
    return t.nT > 0 && (mem == rt::SceneMem::kTriBvh ||
                        (mem == rt::SceneMem::kAuto &&
                         (t.nT > rt::kTriBvhMinTriangles || std::min(lds_pairs, lds_single) > rt::kMaxLdsBytes)));
}

// The SAH builds clamp rt_create_options.tri_leaf_max to 1..128.
inline uint32_t tri_leaf_clamp(uint32_t leaf_max) { return std::min(128u, std::max(1u, leaf_max)); }

inline size_t pixel_bytes(uint32_t flags) { return (flags & RT_OUT_RGBA8) ? 4u : (flags & RT_OUT_FP16) ? 8u : 16u; }

// Row layout of the gather (rt_tile_layout): rank k of N owns the frame rows
// y = k + j*N, j < rows; every rank sends a tile padded to rows_max rows, so
// the gathered buffer holds N tiles of tile_bytes back to back.  A rank past
// the last row (N > H) owns no row and sends its padded tile all the same.
struct TileLayout {
    uint32_t rows, rows_max;
    size_t row_bytes, tile_bytes;
};

inline TileLayout tile_layout(uint32_t W, uint32_t H, uint32_t N, uint32_t rank, uint32_t flags) {
    TileLayout L;
    L.rows = rank < H ? (H - 1u - rank) / N + 1u : 0u;
    L.rows_max = (H + N - 1u) / N;
    L.row_bytes = (size_t)W * pixel_bytes(flags);
    L.tile_bytes = (size_t)L.rows_max * L.row_bytes;
    return L;
}

// The pixel rectangles of the waves of g over the rows row_start + j * row_step
// (rt_debug_wave_rects, rt_debug_wave_masks): wave w = wy * waves_x + wx covers
// columns wx * wave_w .. + wave_w - 1 and partition rows wy * wave_h .. +
// wave_h - 1, which is what wave_masks_kernel builds its beam from.
inline void wave_rects(const rt::WaveGrid& g, uint32_t row_start, uint32_t row_step, rt_wave_mask* out,
                       uint32_t capacity) {
    const uint32_t n = g.waves_x * g.waves_y;
    for (uint32_t w = 0; w < n && w < capacity; ++w) {
        const uint32_t wx0 = (w % g.waves_x) * g.wave_w, wj0 = (w / g.waves_x) * g.wave_h;
        out[w].x0 = (int32_t)wx0;
        out[w].x1 = (int32_t)(wx0 + g.wave_w - 1u);
        out[w].y0 = (int32_t)(row_start + wj0 * row_step);
        out[w].y1 = (int32_t)(row_start + (wj0 + g.wave_h - 1u) * row_step);
    }
}

// Resolves the defaults of a row partition (0: step 1, every row from
// row_start on) and validates it against a frame of H rows.
inline bool resolve_rows(uint32_t H, uint32_t row_start, uint32_t row_step, uint32_t row_count, uint32_t* start,
                         uint32_t* step, uint32_t* count) {
    *start = row_start;
    *step = row_step ? row_step : 1u;
    if (*start >= H) return false;
    const uint32_t avail = (H - 1u - *start) / *step + 1u;
    *count = row_count ? row_count : avail;
    return *count <= avail;
}

// rt_plan_params (rt_plan_samples and rt_plan_samples_host): null when every
// field is in its range, else what is wrong.  `flags_ok`: the flag bits the
// entry point accepts.
inline const char* plan_params_error(const rt_plan_params* p, uint32_t flags_ok) {
    static_assert(sizeof(rt_plan_params) == 40 && sizeof(rt_plan_stats) == 32 && sizeof(rt::PlanStats) == 32,
                  "rt_plan_params / rt_plan_stats layout");
    if (!p) return "params is null";
    if (p->flags & ~flags_ok) return "unknown flag bits";
    if (p->reserved[0] || p->reserved[1]) return "reserved must be 0";
    if (p->count_max > rt::kPlanCountMax) return "count_max must be <= 2^24";
    if (p->count_min > p->count_max) return "count_min must be <= count_max";
    if (p->budget >= rt::kPlanBudgetEnd) return "budget must be < 2^38";
    if (p->radius > rt::kPlanRadiusMax) return "radius must be in [0, 2]";
    if ((p->flags & RT_PLAN_RELATIVE) && !(p->luminance_floor > 0.0f))
        return "luminance_floor must be > 0 with RT_PLAN_RELATIVE";
    return nullptr;
}

// rt_reproject, rt_reproject_async and rt_reproject_host (rt_reproject_host.cpp):
// the checks they share.  reproject_check: empty when params and buffers are
// fine (*planes: 1 or 2), else what is wrong, naming the field; `flags_ok`: the
// flag bits the entry point accepts.  reproject_args: the kernel's arguments
// from checked params and buffers (every pointer as given) and the two
// cameras; `prev` null means the camera did not move.  False with *why for a
// prev that compile_camera rejects or of another resolution.
std::string reproject_check(const rt_reproject_params* p, const rt_reproject_buffers* b, uint32_t flags_ok,
                            uint32_t* planes);
bool reproject_args(const rt_reproject_params* p, const rt_reproject_buffers* b, const rt::CamConst& cam,
                    const CameraGPU* prev, rt::ReprojectArgs* A, std::string* why);

// halton(i, d) of the SwiftPM kernel (Sources/gpuRaytracer/shaders.metal:32-47),
// the same loop as RTrace/sampling.metal:107-122.
float halton_host(uint32_t i, uint32_t d);

}  // namespace rtapi
