// rt_api_host.cpp — the entry points of the C-ABI (include/rtpt.h) that need
// neither a context nor a stream: the status and version strings, everything
// that works on a scene description (rt_scene_describe*, the rt_debug_*
// restatements of the kernels' host-side tables), the host tile layout and
// placement, the scene generators and the math checks with their host
// evaluators.  The context API is rt_api.cpp.
#include <string.h>

#include <thread>
#include <vector>

#include "rt_api_internal.hpp"
#include "rt_beam.hpp"
#include "rt_halton.hpp"
#include "rt_mathcheck.hpp"
#include "rt_shaft.hpp"

namespace rtapi {

bool resolve_options(const rt_create_options* o, Resolved* r, const char** why) {
    *r = Resolved();
    if (!o) return true;
    for (uint32_t v : o->reserved)
        if (v != 0) { *why = "rt_create_options.reserved must be zero"; return false; }
    switch (o->scene_layout) {
        case RT_LAYOUT_AUTO: r->mem = rt::SceneMem::kAuto; break;
        case RT_LAYOUT_PAIRS: r->mem = rt::SceneMem::kPairLds; break;
        case RT_LAYOUT_SINGLE: r->mem = rt::SceneMem::kLdsSingle; break;
        case RT_LAYOUT_GLOBAL: r->mem = rt::SceneMem::kSmem; break;
        case RT_LAYOUT_PAIRS_SMEM: r->mem = rt::SceneMem::kPairSmem; break;
        case RT_LAYOUT_SORTED: r->mem = rt::SceneMem::kPairSorted; break;
        case RT_LAYOUT_BVH: r->mem = rt::SceneMem::kTriBvh; break;
        default: *why = "rt_create_options.scene_layout out of range"; return false;
    }
    if (o->lanes_per_pixel != 0 && o->lanes_per_pixel != 1 && o->lanes_per_pixel != 4 &&
        o->lanes_per_pixel != 16) {
        *why = "rt_create_options.lanes_per_pixel must be 0, 1, 4 or 16";
        return false;
    }
    r->lanes = o->lanes_per_pixel;
    switch (o->tri_bvh_build) {
        case RT_TRI_BVH_DEFAULT: r->tri_build = kDefaultTriBuild; break;
        case RT_TRI_BVH_HOST_SAH: case RT_TRI_BVH_GPU_LBVH: case RT_TRI_BVH_GPU_SAH:
            r->tri_build = o->tri_bvh_build; break;
        default: *why = "rt_create_options.tri_bvh_build out of range"; return false;
    }
    if (o->tri_leaf_max > 128) { *why = "rt_create_options.tri_leaf_max must be <= 128"; return false; }
    if (o->tri_leaf_max) r->tri_leaf_max = o->tri_leaf_max;
    if (!(o->tri_leaf_cost >= 0.0f) || o->tri_leaf_cost > 1e6f) {
        *why = "rt_create_options.tri_leaf_cost must be in [0, 1e6]";
        return false;
    }
    if (o->tri_leaf_cost > 0.0f) r->tri_leaf_cost = o->tri_leaf_cost;
    if (o->sphere_leaf_max > 255) { *why = "rt_create_options.sphere_leaf_max must be <= 255"; return false; }
    if (o->sphere_leaf_max) r->build.sphere_leaf_max = o->sphere_leaf_max;
    if (o->sphere_median > 1) { *why = "rt_create_options.sphere_median must be 0 or 1"; return false; }
    r->build.sphere_sah = o->sphere_median == 0;
    if (o->walk_scheduler > RT_WALK_SORTED) { *why = "rt_create_options.walk_scheduler out of range"; return false; }
    r->walk = o->walk_scheduler;
    if (o->walk_leaf_den > 64) { *why = "rt_create_options.walk_leaf_den must be <= 64"; return false; }
    r->walk_leaf_den = o->walk_leaf_den;
    return true;
}

float halton_host(uint32_t i, uint32_t d) {
    static const uint32_t primes[24] = RT_PRIMES_INIT;
    const uint32_t b = primes[d];
    float f = 1.0f;
    const float invB = 1.0f / (float)b;
    float r = 0.0f;
    while (i > 0) {
        f = f * invB;
        r = r + f * (float)(i % b);
        i = i / b;
    }
    return r;
}

}  // namespace rtapi

using namespace rtapi;

namespace {

bool tile_args_ok(int32_t W, int32_t H, int32_t N) { return W > 0 && H > 0 && N > 0; }

// The host SAH tree of a compiled scene, as rt_debug_tri_bvh dumps a context's:
// every array the caller gave room for.
struct HostTree {
    std::vector<uint32_t> nodes, perm;
    std::vector<rt::TriIsect> sorted;
};

void dump_host_tree(const HostTree& t, rt_tri_bvh_dump* dump) {
    const size_t nT = t.perm.size();
    dump->nodes_per_layout = (uint32_t)(t.nodes.size() / (4 * rt::kTriCompactLayouts));
    if (dump->nodes) memcpy(dump->nodes, t.nodes.data(), t.nodes.size() * sizeof(uint32_t));
    if (dump->sorted) memcpy(dump->sorted, t.sorted.data(), nT * sizeof(rt::TriIsect));
    if (dump->perm) memcpy(dump->perm, t.perm.data(), nT * sizeof(uint32_t));
}

// The beam of the pixel rectangle [x0, x1] x [y0, y1] with the kernel's own
// floats: (float) of the unsigned pixel coordinates, W and H.
rt::Beam desc_beam(const rt::CamConst& c, int32_t x0, int32_t x1, int32_t y0, int32_t y1) {
    return rt::make_beam(rt::f3{c.pos[0], c.pos[1], c.pos[2]}, rt::f3{c.u[0], c.u[1], c.u[2]},
                         rt::f3{c.v[0], c.v[1], c.v[2]}, rt::f3{c.w[0], c.w[1], c.w[2]}, c.halfW, c.halfH, (float)c.W,
                         (float)c.H, (float)(uint32_t)x0, (float)(uint32_t)x1, (float)(uint32_t)y0,
                         (float)(uint32_t)y1);
}

void fill_scene_arrays(const rt::Scene& s, CameraGPU* camera, MaterialGPU* materials, rt_float3* vertices,
                       SquareLightGPU* light, uint32_t* n_triangles) {
    *camera = rt::convert_camera(s.camera);
    for (size_t k = 0; k < s.triangles.size(); ++k) {
        materials[k] = rt::convert_material(s.triangles[k].material);
        for (int v = 0; v < 3; ++v) vertices[3 * k + v] = rt::to_abi(s.triangles[k].vertices[v]);
    }
    *light = rt::convert_square_light(s.light);
    *n_triangles = (uint32_t)s.triangles.size();
}

// rt_debug_math_*: the x86 compile of rt::math_eval (rt_mathcheck.hpp); the
// host's only Halton form is the reference loop.
inline __attribute__((always_inline)) uint32_t math_eval_host(uint32_t fn, uint32_t D, uint32_t b) {
    switch (fn) {
        case RT_MATH_SIN: return rt::math_eval<RT_MATH_SIN>(b);
        case RT_MATH_COS: return rt::math_eval<RT_MATH_COS>(b);
        case RT_MATH_LOG: return rt::math_eval<RT_MATH_LOG>(b);
        case RT_MATH_EXP: return rt::math_eval<RT_MATH_EXP>(b);
        case RT_MATH_POW_GAMMA: return rt::math_eval<RT_MATH_POW_GAMMA>(b);
        case RT_MATH_SQRT: return rt::math_eval<RT_MATH_SQRT>(b);
        case RT_MATH_RCP: return rt::math_eval<RT_MATH_RCP>(b);
        case RT_MATH_F2H: return rt::math_eval<RT_MATH_F2H>(b);
        case RT_MATH_H2F: return rt::math_eval<RT_MATH_H2F>(b);
        case RT_MATH_TONEMAP: return rt::math_eval<RT_MATH_TONEMAP>(b);
        case RT_MATH_MIS_UNIT: return rt::math_eval<RT_MATH_MIS_UNIT>(b);
        default: return rt::canon_f32(halton_host(b, D));
    }
}

// Host side of rt_debug_math_sums: thread t of T takes the pieces t, t + T, ...
// of the inputs (2^12 inputs a piece, so a single large chunk is shared as
// well; a piece may span several small chunks) and adds its partial sums with
// one atomic add per piece and chunk: sums mod 2^64, any order.
inline __attribute__((always_inline)) void math_sum_pieces_body(uint32_t fn, uint32_t D, uint32_t first,
                                                                uint64_t count, uint32_t chunk_log2, uint32_t t,
                                                                uint32_t T, uint64_t* sums) {
    constexpr uint64_t kPiece = 1ull << 12;
    const uint64_t pieces = (count + kPiece - 1) / kPiece;
    for (uint64_t p = t; p < pieces; p += T) {
        const uint64_t lo = p * kPiece, hi = std::min(count, lo + kPiece);
        for (uint64_t j = lo; j < hi;) {
            const uint64_t c = j >> chunk_log2, end = std::min(hi, (c + 1) << chunk_log2);
            uint64_t s0 = 0, s1 = 0;
            for (; j < end; ++j) {
                const uint64_t o = math_eval_host(fn, D, first + (uint32_t)j);
                s0 += o;
                s1 += o * (2 * (j - (c << chunk_log2)) + 1);
            }
            __atomic_fetch_add(&sums[2 * c], s0, __ATOMIC_RELAXED);
            __atomic_fetch_add(&sums[2 * c + 1], s1, __ATOMIC_RELAXED);
        }
    }
}
void math_sum_pieces(uint32_t fn, uint32_t D, uint32_t first, uint64_t count, uint32_t chunk_log2, uint32_t t,
                     uint32_t T, uint64_t* sums) {
    math_sum_pieces_body(fn, D, first, count, chunk_log2, t, T, sums);
}
__attribute__((target("fma"))) void math_sum_pieces_fma(uint32_t fn, uint32_t D, uint32_t first, uint64_t count,
                                                        uint32_t chunk_log2, uint32_t t, uint32_t T,
                                                        uint64_t* sums) {
    math_sum_pieces_body(fn, D, first, count, chunk_log2, t, T, sums);
}

// fn word -> (function, dimension); the checks shared by both entry points.
// max_index: the largest input of the call (an index for the Halton forms).
const char* math_fn_args(uint32_t fn_word, uint32_t where, uint64_t max_index, uint32_t* fn, uint32_t* D) {
    *fn = fn_word & 0xFFu;
    *D = (fn_word >> 8) & 0x1Fu;
    if (where != RT_MATH_HOST && where != RT_MATH_DEVICE) return "where is neither RT_MATH_HOST nor RT_MATH_DEVICE";
    if (*fn >= rt::kMathFnCount || (fn_word >> 13)) return "fn is not an rt_math_fn";
    const bool halton = *fn >= RT_MATH_HALTON_LOOP;
    if (!halton && *D) return "fn carries a dimension but is no Halton form";
    if (*D >= 24) return "Halton dimension >= 24";
    if (halton && *fn != RT_MATH_HALTON_LOOP) {
        if (where == RT_MATH_HOST) return "the host has only the reference loop (RT_MATH_HALTON_LOOP)";
        if (*fn == RT_MATH_HALTON_TAB && !rt::math_dim_has_table(*D)) return "no low-digit table for this dimension";
        if (max_index >= rt::math_small_index_max()) return "RT_MATH_HALTON_SMALL / _TAB index >= 3^13";
    }
    return nullptr;
}

int math_device_ready() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(nullptr, RT_ERR_NO_DEVICE, "no HIP device");
    return RT_OK;
}

}  // namespace

extern "C" {

void rt_create_options_default(rt_create_options* opt) {
    if (opt) memset(opt, 0, sizeof(*opt));
}

int rt_abi_version(void) { return RTPT_ABI_VERSION; }

const char* rt_status_string(int s) {
    switch (s) {
        case RT_OK: return "RT_OK";
        case RT_ERR_INVALID_ARG: return "RT_ERR_INVALID_ARG";
        case RT_ERR_NO_DEVICE: return "RT_ERR_NO_DEVICE";
        case RT_ERR_OUT_OF_MEMORY: return "RT_ERR_OUT_OF_MEMORY";
        case RT_ERR_LAUNCH: return "RT_ERR_LAUNCH";
        case RT_ERR_STATE: return "RT_ERR_STATE";
        case RT_ERR_COMM: return "RT_ERR_COMM";
        default: return "RT_ERR_UNKNOWN";
    }
}

void rt_plan_params_default(rt_plan_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->count_max = rt::kPlanCountMax;
    p->luminance_floor = 0.01f;
    p->radius = 1;
}

// The planner of rt_adaptive.hip in plain C++: the same
// per-pixel functions (rt_plan.hpp), the maximum and the sums in any order.
int rt_plan_samples_host(int32_t width, const rt_plan_params* p, const float* first, const float* all,
                         uint32_t* counts, rt_plan_stats* stats) {
    if (const char* why = rtapi::plan_params_error(p, RT_PLAN_RELATIVE))
        return rtapi::fail(nullptr, RT_ERR_INVALID_ARG, std::string("rt_plan_samples_host: ") + why);
    if (!first || !all || !counts)
        return rtapi::fail(nullptr, RT_ERR_INVALID_ARG, "rt_plan_samples_host: first, all or counts is null");
    if (width < 1 || p->rows < 1 || p->rows > 0x7FFFFFFFu)
        return rtapi::fail(nullptr, RT_ERR_INVALID_ARG, "rt_plan_samples_host: width and params->rows must be >= 1");
    const int W = width, H = (int)p->rows, R = (int)p->radius;
    const size_t n = (size_t)W * (size_t)H;
    const bool relative = (p->flags & RT_PLAN_RELATIVE) != 0;
    std::vector<uint32_t> q(n);
    for (size_t k = 0; k < n; ++k) {
        const float* f = first + 4 * k;
        const float* a = all + 4 * k;
        q[k] = rt::plan_weight(f[0], f[1], f[2], a[0], a[1], a[2], relative, p->luminance_floor);
    }
    uint64_t Q = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint32_t m = 0;
            for (int j = std::max(0, y - R); j <= std::min(H - 1, y + R); ++j)
                for (int i = std::max(0, x - R); i <= std::min(W - 1, x + R); ++i)
                    m = std::max(m, q[(size_t)j * (size_t)W + (size_t)i]);
            counts[(size_t)y * (size_t)W + (size_t)x] = m;
            Q += m;
        }
    rt_plan_stats s{};
    s.weight_sum = Q;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t share = rt::plan_share(p->budget, counts[k], Q, p->count_min);
        const bool capped = share > (uint64_t)p->count_max;
        const uint32_t c = capped ? p->count_max : (uint32_t)share;
        counts[k] = c;
        s.samples += c;
        s.at_cap += capped ? 1u : 0u;
        s.count_max_seen = std::max(s.count_max_seen, c);
    }
    if (stats) *stats = s;
    return RT_OK;
}

void rt_denoise_params_default(rt_denoise_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->iterations = 5;
    p->normal_power_log2 = 7;
    p->sigma_luminance = 4.0f;
    p->sigma_depth = 1.0f;
    p->depth_floor = 0.01f;
}

void rt_path_params_default(rt_path_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->spp = 1;
    p->bounces = 3;
}

int rt_scene_describe(const rt_scene_desc* d, rt_scene_info* info) {
    return rt_scene_describe_ex(d, nullptr, info);
}

int rt_scene_describe_ex(const rt_scene_desc* d, const rt_create_options* opt, rt_scene_info* info) {
    if (!desc_ok(d) || !info) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    Resolved ro;
    const char* why = nullptr;
    if (!resolve_options(opt, &ro, &why)) return fail(nullptr, RT_ERR_INVALID_ARG, why);
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, ro.build, &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    rt::SceneTables t = scene_counts(s, 0);
    info->n_triangles = t.nT;
    info->n_triangle_pairs = t.nP;
    info->n_box_clusters = t.nC;
    info->pair_free_mask = t.pair_free;
    info->n_spheres = t.nS;
    info->n_sphere_nodes = t.nN;
    const size_t lds = rt::kernel_lds_bytes(t.nT, t.nP, t.nS, t.nN);
    const bool bvh = needs_tri_bvh(t, ro.mem);
    info->n_triangle_bvh_nodes = t.nTN = bvh ? 2 * t.nT - 1 : 0u;
    // the launcher takes the sphere kernel only for the pair layout (every
    // triangle paired) and no triangle BVH, with its pair copy within 6 KB
    info->sphere_kernel_lds_bytes = (rt::sphere_compact_usable(s) && t.nP > 0 && !bvh &&
                                     ro.mem == rt::SceneMem::kAuto && lds <= rt::kSphPairLdsMaxBytes)
                                        ? (uint32_t)lds
                                        : 0u;
    // box clusters are staged after the pairs in triangle-only scenes
    const size_t lds_clu =
        lds + (t.nS ? 0u : 16 * rt::staged_f4<size_t>(rt::kLayPairClu, t.nT, t.nP, t.nC).clu);
    info->lds_bytes = (!bvh && lds <= rt::kMaxLdsBytes)
                          ? (uint32_t)(lds_clu <= rt::kMaxLdsBytes ? lds_clu : lds)
                          : 0u;
    // the launcher's own choice (rt::choose_kernel), for a render of >= 1 bounce
    const rt::KernelChoice kc = rt::choose_kernel(t, rt::sphere_compact_usable(s), 3, ro.mem, ro.walk);
    info->kernel_layout = (uint32_t)kc.layout;
    info->kernel_lds_bytes = (uint32_t)kc.lds_bytes;
    return RT_OK;
}

int rt_debug_ray_domain(const rt_scene_desc* d, rt_ray_domain_info* info) {
    if (!desc_ok(d) || !info) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, rt::BuildOptions(), &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    const rt::RayDomain D = rt::ray_domain(s.extent);
    info->origin_max = D.origin_max;
    info->dir_len2_min = D.dir_len2_min;
    info->dir_len2_max = D.dir_len2_max;
    info->tmax_max = D.tmax_max;
    return RT_OK;
}

int rt_debug_camera_candidates(const rt_scene_desc* d, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                               uint8_t* may_hit) {
    if (!desc_ok(d) || !may_hit || x1 < x0 || y1 < y0 || x0 < 0 || y0 < 0)
        return fail(nullptr, RT_ERR_INVALID_ARG, "null argument or empty rectangle");
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, rt::BuildOptions(), &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    memset(may_hit, 1, d->n_triangles);
    const rt::Beam beam = desc_beam(s.cam, x0, x1, y0, y1);
    for (size_t k = 0; k < s.pair_isect.size(); ++k)
        if (rt::beam_excludes_pair(beam, s.pair_isect[k].q)) may_hit[2 * k] = may_hit[2 * k + 1] = 0;
    return RT_OK;
}

int rt_debug_shadow_candidates(const rt_scene_desc* d, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                               uint8_t* may_occlude, int32_t* available) {
    if (!desc_ok(d) || !may_occlude || !available || x1 < x0 || y1 < y0 || x0 < 0 || y0 < 0)
        return fail(nullptr, RT_ERR_INVALID_ARG, "null argument or empty rectangle");
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, rt::BuildOptions(), &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    memset(may_occlude, 1, d->n_triangles);
    *available = 0;
    const size_t nP = s.pair_isect.size();
    if (nP == 0) return RT_OK;
    const rt::Beam beam = desc_beam(s.cam, x0, x1, y0, y1);
    const rt::ShaftLight L = rt::shaft_light(rt::f3{s.light.center[0], s.light.center[1], s.light.center[2]});
    // the kernel's prologue: the union over the source triangles of the
    // wave's camera mask; a light's triangle ends the path (no shadow ray)
    std::vector<uint8_t> keep(nP, 0);
    bool ok = true;
    for (size_t k = 0; k < nP; ++k) {
        if (rt::beam_excludes_pair(beam, s.pair_isect[k].q)) continue;
        for (int tb = 0; tb < 2; ++tb) {
            const float* sh = s.tri_shade[2 * k + tb].s;
            if (sh[3] != 0.0f) continue;
            const rt::ShaftSrc S = rt::shaft_source(beam, s.pair_isect[k].q, tb, rt::f3{sh[0], sh[1], sh[2]}, L);
            ok = ok && S.ok;
            for (size_t j = 0; j < nP; ++j)
                if (!rt::shaft_excludes_pair(S, L, s.pair_isect[j].q)) keep[j] = 1;
        }
    }
    if (!ok) return RT_OK;
    *available = 1;
    for (size_t j = 0; j < nP; ++j) may_occlude[2 * j] = may_occlude[2 * j + 1] = keep[j];
    return RT_OK;
}

int rt_debug_wave_rects(int32_t width, int32_t height, uint32_t row_start, uint32_t row_step, uint32_t row_count,
                        uint32_t lanes, rt_wave_mask* masks, uint32_t capacity, uint32_t* waves_x, uint32_t* waves_y) {
    static_assert(sizeof(rt_wave_mask) == 32, "rt_wave_mask layout");
    if (width < 1 || height < 1 || !waves_x || !waves_y || (!masks && capacity))
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_wave_rects: empty frame or null argument");
    if (lanes != 1 && lanes != 4 && lanes != 16)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_wave_rects: lanes_per_pixel must be 1, 4 or 16");
    uint32_t start, step, count;
    if (!resolve_rows((uint32_t)height, row_start, row_step, row_count, &start, &step, &count))
        return fail(nullptr, RT_ERR_INVALID_ARG, "row partition outside the frame");
    const rt::WaveGrid g = rt::clu_wave_grid((uint32_t)width, count, step, lanes);
    *waves_x = g.waves_x;
    *waves_y = g.waves_y;
    wave_rects(g, start, step, masks, capacity);
    return RT_OK;
}

int rt_debug_cluster_kinds(const rt_scene_desc* d, uint32_t* flags, uint32_t capacity, uint32_t* n_clusters) {
    if (!desc_ok(d) || !n_clusters || (!flags && capacity)) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, rt::BuildOptions(), &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    const size_t rec = 4 * rt::kCluF4, nC = s.clusters.size() / rec;
    *n_clusters = (uint32_t)nC;
    for (size_t c = 0; c < nC && c < capacity; ++c) memcpy(&flags[c], &s.clusters[c * rec + 15], 4);
    return RT_OK;
}

int rt_debug_light_mask(const rt_scene_desc* d, uint64_t* mask, float* records, uint32_t capacity_triangles) {
    if (!desc_ok(d) || !mask || (!records && capacity_triangles))
        return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, rt::BuildOptions(), &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    *mask = rt::light_mask(s);
    for (size_t k = 0; k < s.tri_shade.size() && k < capacity_triangles; ++k)
        memcpy(records + 16 * k, s.tri_shade[k].s, sizeof(s.tri_shade[k].s));
    return RT_OK;
}

int rt_debug_halton_table(float* table, uint32_t capacity, uint32_t* n_floats, uint32_t* offsets, uint32_t* sizes) {
    static_assert(rt::kHaltonTabFloats == rt::kHaltonTabLdsFloats, "rt_kernel.hpp's size of the tables");
    if (!n_floats || (!table && capacity)) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    *n_floats = rt::kHaltonTabFloats;
    for (int D = 0; D < 24; ++D) {
        if (offsets) offsets[D] = rt::tab_offset(D);
        if (sizes) sizes[D] = rt::tab_size(D);
    }
    if (!table) return RT_OK;
    if (capacity < rt::kHaltonTabFloats)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_halton_table: capacity below the table's size");
    rt::fill_halton_tables(table, 0u, 1u);  // the kernels' fill as one thread of one
    return RT_OK;
}

int rt_debug_tri_bvh_host(const rt_scene_desc* d, const rt_create_options* opt, rt_tri_bvh_dump* dump) {
    if (!desc_ok(d) || !dump) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    Resolved ro;
    const char* why = nullptr;
    if (!resolve_options(opt, &ro, &why)) return fail(nullptr, RT_ERR_INVALID_ARG, why);
    rt::CompiledScene s;
    const char* err = nullptr;
    if (!compile_desc(d, ro.build, &s, &err)) return fail(nullptr, RT_ERR_INVALID_ARG, err);
    const size_t nT = s.tri_isect.size();
    dump->n_triangles = (uint32_t)nT;
    dump->nodes_per_layout = 0;
    dump->leaf_max = tri_leaf_clamp(ro.tri_leaf_max);
    dump->margin = s.margin;
    if (nT == 0) return fail(nullptr, RT_ERR_INVALID_ARG, "the scene has no triangles");
    if (dump->isect) memcpy(dump->isect, s.tri_isect.data(), nT * sizeof(rt::TriIsect));
    if (!dump->nodes && !dump->sorted && !dump->perm) return RT_OK;  // sizes only: no build
    HostTree t;
    if (!rt::build_tri_sah(s.tri_isect, s.margin, &t.nodes, &t.sorted, &t.perm, ro.tri_leaf_max, ro.tri_leaf_cost))
        return fail(nullptr, RT_ERR_INVALID_ARG, "triangle BVH build: too many triangles (2^24)");
    dump_host_tree(t, dump);
    return RT_OK;
}

int rt_debug_tri_bvh_refit_host(const rt_scene_desc* from, const rt_create_options* opt, const rt_scene_desc* to,
                                rt_tri_bvh_dump* dump) {
    if (!desc_ok(from) || !desc_ok(to) || !dump) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (from->n_triangles != to->n_triangles)
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_tri_bvh_refit_host: n_triangles of the two scenes differ");
    Resolved ro;
    const char* why = nullptr;
    if (!resolve_options(opt, &ro, &why)) return fail(nullptr, RT_ERR_INVALID_ARG, why);
    rt::CompiledScene a, b;
    const char* err = nullptr;
    if (!compile_desc(from, ro.build, &a, &err) || !compile_desc(to, ro.build, &b, &err))
        return fail(nullptr, RT_ERR_INVALID_ARG, err);
    const size_t nT = a.tri_isect.size();
    if (nT == 0) return fail(nullptr, RT_ERR_INVALID_ARG, "the scene has no triangles");
    if (b.tri_isect.size() != nT) return fail(nullptr, RT_ERR_INVALID_ARG, "n_triangles of the compiled scenes differ");
    HostTree t;
    if (!rt::build_tri_sah(a.tri_isect, a.margin, &t.nodes, &t.sorted, &t.perm, ro.tri_leaf_max, ro.tri_leaf_cost))
        return fail(nullptr, RT_ERR_INVALID_ARG, "triangle BVH build: too many triangles (2^24)");
    if (!rt::refit_tri_bvh_host(b.tri_isect, b.margin, &t.nodes, t.perm, &t.sorted))
        return fail(nullptr, RT_ERR_STATE, "triangle BVH refit: the tree is outside the format");
    dump->n_triangles = (uint32_t)nT;
    dump->leaf_max = tri_leaf_clamp(ro.tri_leaf_max);
    dump->margin = b.margin;
    dump_host_tree(t, dump);
    if (dump->isect) memcpy(dump->isect, b.tri_isect.data(), nT * sizeof(rt::TriIsect));
    return RT_OK;
}

int rt_tile_layout(int32_t width, int32_t height, int32_t world, int32_t rank, uint32_t flags,
                   rt_tile_layout_info* out) {
    if (!out || !tile_args_ok(width, height, world) || rank < 0 || rank >= world)
        return RT_ERR_INVALID_ARG;
    const TileLayout L = tile_layout((uint32_t)width, (uint32_t)height, (uint32_t)world, (uint32_t)rank, flags);
    out->rows = L.rows;
    out->rows_max = L.rows_max;
    out->row_bytes = L.row_bytes;
    out->tile_bytes = L.tile_bytes;
    return RT_OK;
}

int rt_place_tiles_host(const void* gathered, int32_t width, int32_t height, int32_t world, uint32_t flags,
                        void* frame) {
    if (!gathered || !frame || !tile_args_ok(width, height, world)) return RT_ERR_INVALID_ARG;
    const uint32_t W = (uint32_t)width, H = (uint32_t)height, N = (uint32_t)world;
    for (uint32_t k = 0; k < N && k < H; ++k) {
        const TileLayout L = tile_layout(W, H, N, k, flags);
        for (uint32_t j = 0; j < L.rows; ++j)
            memcpy(static_cast<char*>(frame) + (size_t)(k + j * N) * L.row_bytes,
                   static_cast<const char*>(gathered) + k * L.tile_bytes + j * L.row_bytes, L.row_bytes);
    }
    return RT_OK;
}

int rt_math_selfcheck(uint64_t* mismatches) {
    if (!mismatches) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (const int st = math_device_ready()) return st;
    unsigned long long bad[2] = {0, 0};
    const hipError_t e = rt::math_selfcheck(bad);
    if (e != hipSuccess) return hip_fail(nullptr, RT_ERR_LAUNCH, "math_selfcheck", e);
    mismatches[0] = bad[0];
    mismatches[1] = bad[1];
    return RT_OK;
}

int rt_debug_math_values(uint32_t fn_word, uint32_t where, const uint32_t* in_bits, uint64_t n, uint32_t* out_bits) {
    if (n == 0) return RT_OK;
    if (!in_bits || !out_bits) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (n > RT_MATH_VALUES_MAX) return fail(nullptr, RT_ERR_INVALID_ARG, "n > RT_MATH_VALUES_MAX");
    uint32_t fn, D, top = 0;
    if ((fn_word & 0xFFu) >= RT_MATH_HALTON_SMALL)  // the forms with an index bound
        for (uint64_t j = 0; j < n; ++j) top = std::max(top, in_bits[j]);
    if (const char* why = math_fn_args(fn_word, where, top, &fn, &D)) return fail(nullptr, RT_ERR_INVALID_ARG, why);
    if (where == RT_MATH_HOST) {
        for (uint64_t j = 0; j < n; ++j) out_bits[j] = math_eval_host(fn, D, in_bits[j]);
        return RT_OK;
    }
    if (const int st = math_device_ready()) return st;
    const hipError_t e = rt::math_values_device(fn, D, in_bits, (uint32_t)n, out_bits);
    if (e != hipSuccess) return hip_fail(nullptr, RT_ERR_LAUNCH, "math_values", e);
    return RT_OK;
}

int rt_debug_math_sums(uint32_t fn_word, uint32_t where, uint32_t first_bits, uint64_t count, uint32_t chunk_log2,
                       uint32_t host_threads, uint64_t* sums) {
    if (count == 0) return RT_OK;
    if (!sums) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (chunk_log2 < rt::kMathChunkLog2Min || chunk_log2 > rt::kMathChunkLog2Max)
        return fail(nullptr, RT_ERR_INVALID_ARG, "chunk_log2 outside 6..31");
    if ((uint64_t)first_bits + count > (1ull << 32))
        return fail(nullptr, RT_ERR_INVALID_ARG, "first_bits + count > 2^32");
    uint32_t fn, D;
    if (const char* why = math_fn_args(fn_word, where, (uint64_t)first_bits + count - 1, &fn, &D))
        return fail(nullptr, RT_ERR_INVALID_ARG, why);
    const uint64_t chunk = 1ull << chunk_log2, chunks = (count + chunk - 1) >> chunk_log2;
    if (where == RT_MATH_DEVICE) {
        if (const int st = math_device_ready()) return st;
        const hipError_t e = rt::math_sums_device(fn, D, first_bits, count, chunk_log2, sums);
        if (e != hipSuccess) return hip_fail(nullptr, RT_ERR_LAUNCH, "math_sums", e);
        return RT_OK;
    }
    if (host_threads < 1 || host_threads > 256) return fail(nullptr, RT_ERR_INVALID_ARG, "host_threads outside 1..256");
    for (uint64_t c = 0; c < 2 * chunks; ++c) sums[c] = 0;
    // fmaf is the same function with or without the FMA instructions; with
    // them it is an instruction instead of a library call
    const bool fma = __builtin_cpu_supports("fma");
    auto work = [&](uint32_t t) {
        (fma ? math_sum_pieces_fma : math_sum_pieces)(fn, D, first_bits, count, chunk_log2, t, host_threads, sums);
    };
    std::vector<std::thread> pool;
    bool started = true;
    try {
        pool.reserve(host_threads);
        for (uint32_t t = 1; t < host_threads; ++t) pool.emplace_back(work, t);
    } catch (...) {  // no exception crosses the C boundary
        started = false;
    }
    if (started) work(0);
    for (auto& th : pool) th.join();
    if (!started) return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "could not start host_threads threads");
    return RT_OK;
}

void rt_seed_splitmix(uint64_t key, uint32_t* seeds, size_t n) {
    if (!seeds) return;
    for (size_t p = 0; p < n; ++p) seeds[p] = rt::seed_splitmix(key, p);
}

int rt_scene_cornell_box(int32_t width, int32_t height, CameraGPU* camera, MaterialGPU* materials,
                         rt_float3* vertices, SquareLightGPU* light, uint32_t* n_triangles) {
    if (!camera || !materials || !vertices || !light || !n_triangles || width <= 0 || height <= 0)
        return RT_ERR_INVALID_ARG;
    fill_scene_arrays(rt::init_cornell_box(width, height), camera, materials, vertices, light, n_triangles);
    return RT_OK;
}

int rt_scene_cornell_box_mis(int32_t width, int32_t height, CameraGPU* camera, MaterialGPU* materials,
                             rt_float3* vertices, SquareLightGPU* light, uint32_t* n_triangles) {
    if (!camera || !materials || !vertices || !light || !n_triangles || width <= 0 || height <= 0)
        return RT_ERR_INVALID_ARG;
    fill_scene_arrays(rt::init_cornell_box_mis(width, height), camera, materials, vertices, light, n_triangles);
    return RT_OK;
}

int rt_scene_random_spheres(int32_t width, int32_t height, uint32_t n_spheres, uint64_t seed,
                            CameraGPU* camera, MaterialGPU* materials, rt_float3* vertices,
                            SquareLightGPU* light, uint32_t* n_triangles, SphereGPU* spheres) {
    if (!camera || !materials || !vertices || !light || !n_triangles || width <= 0 ||
        height <= 0 || (n_spheres && !spheres))
        return RT_ERR_INVALID_ARG;
    const rt::Scene s = rt::init_random_spheres(width, height, n_spheres, seed);
    fill_scene_arrays(s, camera, materials, vertices, light, n_triangles);
    for (uint32_t k = 0; k < n_spheres; ++k) spheres[k] = rt::convert_sphere(s.spheres[k]);
    return RT_OK;
}

}  // extern "C"
