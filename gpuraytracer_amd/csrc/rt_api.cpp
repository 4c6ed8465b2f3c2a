// rt_api.cpp — the context API of librtpt.so (include/rtpt.h): every entry
// point that takes or makes an rt_ctx.  (The entry points that need neither a
// context nor a stream are rt_api_host.cpp.)
//
// Replaces the Metal host boundary of the reference:
//   Renderer.init()  (RTrace/renderer.swift:29-115)  -> rt_create / rt_set_seeds
//   Renderer.draw()  (RTrace/renderer.swift:117-146) -> rt_render
// Inputs are copied at create time (makeBuffer(bytes:) semantics), the context
// owns every device buffer, and every failure is returned as an rt_status with
// a message (the reference fatalError()s / force-unwraps instead).
#include <rccl/rccl.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <new>
#include <vector>

#include "rt_api_internal.hpp"

using namespace rtapi;

namespace {

// A device allocation and its size: THE owner of device memory on the host
// side (no hipMalloc / hipFree outside it).  Freed with the buffer's device
// current: rt_ctx's members go inside a DeviceGuard (rt_destroy).
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // Grows, never shrinks: room for `bytes` at least.  A buffer that has to
    // grow is freed first; after a failure it is null.
    hipError_t reserve(size_t bytes) { return bytes_ >= bytes ? hipSuccess : allocate(bytes); }
    // Exactly `bytes` (0: null), allocated again only when the size differs.
    hipError_t resize_exact(size_t bytes) { return bytes_ == bytes ? hipSuccess : allocate(bytes); }
    // Takes over an allocation made elsewhere (rt::refit_tri_bvh's table).
    void adopt(void* p, size_t bytes) {
        reset();
        p_ = p;
        bytes_ = bytes;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    hipError_t allocate(size_t bytes) {
        reset();
        if (bytes == 0) return hipSuccess;
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else bytes_ = bytes;
        return e;
    }
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// An owned stream or event: `h` is filled by its hipXxxCreate.
template <typename H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// The record arrays of a compiled scene on the device (rt_ctx::d_scene).
enum SceneArray {
    kTriIsect, kTriShade, kPairIsect, kClusters, kSphLds, kSphLdsId,
    kSphBox,  // the leaf-box layout of the sphere BVH (rt_scene.hpp sph_box)
    kSphIsect, kSphShade, kSphNodes, kSphPerm, kMisShade, kSceneArrays
};

// Everything the per-wave masks of a launch depend on (rt_ctx::d_wave_masks):
// the camera, the light centre, the scene's tables (the epoch counts their
// updates), the frame, the row partition and the wave geometry.  Compared
// with memcmp: zero it before filling.
struct MaskKey {
    float cam[14];  // pos, u, v, w, halfW, halfH
    float light_center[3];
    int32_t W, H;
    uint32_t row_start, row_step, row_count;
    uint32_t L, wave_w, wave_h;
    uint64_t scene_epoch;
};

// A stream that has a render in flight (or finished) that reads the mask
// table, and the event recorded after its last such render.
struct MaskReader {
    hipStream_t stream;
    hipEvent_t done;
};

}  // namespace

// Teardown is the destructor and the members' own, in this order (all with
// `device` current: whoever deletes a context holds a DeviceGuard round the
// delete): wait for a pending gather, destroy the communicator, free every
// buffer, destroy the events, destroy the stream.  Members are destroyed in
// reverse order of declaration, hence stream and events first.
struct rt_ctx {
    int device = 0;
    Stream stream;
    Event ev0, ev1;      // round the last launch (rt_last_kernel_ms)
    Event ev_u0, ev_u1;  // round the refit's kernels (made by the first rt_update_scene)
    Event ev_tiles;      // end of the last gather's reads of d_tile / d_gather
    rt::CompiledScene scene;
    DevBuf d_scene[kSceneArrays];    // the record arrays, sized exactly (upload_scene)
    DevBuf d_tri_nodes;              // triangle BVH: 8 compact layouts (build_tri_sah / rt_lbvh.hip)
    uint32_t tri_build = kDefaultTriBuild;  // rt_create_options.tri_bvh_build (resolved)
    DevBuf d_tri_sorted, d_tri_perm;
    DevBuf d_refit;                  // rt_refit.hip: parents and counters of the built tree (first refit)
    uint32_t tri_bvh_nodes = 0;      // per layout
    rt::SceneTables tab{};           // what every kernel traces through: borrows the buffers above (finish_scene)
    bool sph_compact = false;        // rt_scene.hpp sphere_compact_usable: the sphere kernel's tables exist
    uint64_t light_mask = 0;         // rt_scene.hpp light_mask: the box-cluster kernel's light flags
    DevBuf d_halton_tab;             // the Halton low-digit tables (rt_halton.hpp), filled once by rt_create_ex
    // The per-wave candidate masks of ONE launch geometry (rt_kernel.hpp WaveMask):
    // filled by the first render launch of that geometry, reused while mask_key matches.
    DevBuf d_wave_masks;
    MaskKey mask_key{};              // what the table was filled for (valid: d_wave_masks holds it)
    bool mask_valid = false;
    uint64_t scene_epoch = 0;        // counts rt_update_scene: the tables the masks were computed from
    uint64_t mask_fills = 0;         // launches of the fill kernel (rt_debug_wave_masks reports it)
    Event ev_mask_fill;              // end of the last fill
    std::vector<MaskReader> mask_readers;  // the streams whose renders may still read the table
    uint32_t tri_bvh_build_used = 0; // rt_tri_bvh_build of the built tree (0: none)
    uint32_t tri_leaf_max = 1;       // triangles per leaf at most in the built tree (rt_debug_tri_bvh)
    float tri_bvh_build_ms = 0.0f;   // wall time of the triangle-BVH build
    size_t tri_bvh_temp_bytes = 0;   // peak temporaries of the GPU SAH build
    float scene_compile_ms = 0.0f;   // host scene compile (rt_scene.cpp compile_scene)
    DevBuf d_mis_tab;              // Halton table of the MIS integrator
    uint32_t mis_tab_S = 0;        // samples per strategy it was built for
    DevBuf d_mis_part;             // per-ray MIS results of a split launch (rt_mis.hip)
    DevBuf d_out, d_out8;          // staging for host outputs (d_out8: the MIS integrator's RGBA8)
    DevBuf d_rays, d_hits;         // staging for host rays and hits (rt_trace_rays)
    DevBuf d_ray_seeds, d_radiance;  // staging for host ray seeds and radiance (rt_trace_paths)
    DevBuf d_aov[3];               // staging for host feature buffers (rt_render_aov)
    DevBuf d_den[6];               // rt_denoise: the (D, V) ping-pong, then staging for the four host inputs
    DevBuf d_rep[8];               // rt_reproject: staging for the eight host inputs (the outputs: the staged colours)
    DevBuf d_counts, d_totals;     // staging for host counts and totals (rt_render_counts, rt_plan_samples)
    DevBuf d_plan_in[2];           // staging for the planner's two host images
    DevBuf d_plan;                 // the planner's accumulators (rt::PlanStats)
    DevBuf d_seeds;
    bool seeds_ready = false;
    uint32_t seed_max = 0xFFFFFFFFu;  // max seed value (bounds the Halton index)
    DevBuf d_sum;
    bool sum_valid = false;
    uint32_t sum_row_start = 0, sum_row_step = 0, sum_row_count = 0;
    uint32_t sum_first = 0, sum_samples = 0;  // the sum holds samples [first, first + samples)
    // rt_render_counts wrote the sum: pixel p holds the samples [first, first + its entry's .w), and
    // sum_samples is an upper bound of those counts (it grows by the cap spp with each call)
    bool sum_counts = false;
    bool timed = false;
    rt::LaunchInfo launch{};  // what the last launch that reports one launched (rt_last_launch)
    bool launched = false;
    ncclComm_t comm = nullptr;  // rt_comm_init: row-tile gather over RCCL
    int rank = 0, world = 1;
    DevBuf d_tile;              // this rank's rows before the gather
    DevBuf d_gather;            // rank 0: world x rows_max x W pixels
    bool tiles_pending = false;
    uint32_t lanes = 0;  // rt_create_options.lanes_per_pixel (0 = auto)
    rt::SceneMem scene_mem = rt::SceneMem::kAuto;  // rt_create_options.scene_layout
    uint32_t walk = 0;   // rt_create_options.walk_scheduler
    uint32_t walk_leaf_den = 0;  // rt_create_options.walk_leaf_den
    // what a later build needs of rt_create_options (rt_update_scene)
    uint32_t tri_leaf_opt = rt::kTriLeafMax;
    double tri_leaf_cost = 1.0;
    rt::BuildOptions build_opt;
    std::string broken;              // non-empty: an update failed halfway (every render / query: RT_ERR_STATE)
    bool updated = false;
    rt_update_stats update{};        // the last successful rt_update_scene
    std::string err;

    ~rt_ctx() {
        if (tiles_pending) (void)hipEventSynchronize(ev_tiles);  // a gather may still read d_tile
        if (comm) (void)ncclCommDestroy(comm);                   // before d_tile and d_gather go
        for (const MaskReader& r : mask_readers) (void)hipEventDestroy(r.done);
    }
};

namespace {
thread_local std::string g_create_err = "no error";
}

int rtapi::fail(rt_ctx* ctx, int status, const std::string& msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_err = msg;
    return status;
}

namespace {

int nccl_fail(rt_ctx* ctx, const char* what, ncclResult_t r) {
    return fail(ctx, RT_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(r));
}

// Makes ctx->device current for the duration of an API call, restores after.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Room for `bytes` in a buffer that only grows (the staging buffers, the sums).
int reserve(rt_ctx* c, DevBuf& b, size_t bytes, const char* what) {
    const hipError_t e = b.reserve(bytes);
    return e == hipSuccess ? RT_OK : hip_fail(c, RT_ERR_OUT_OF_MEMORY, what, e);
}

// A host result comes down from its staging buffer on the launch's stream.
int copy_down(rt_ctx* c, void* host, const void* dev, size_t bytes, hipStream_t stream, const char* what) {
    const hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? RT_OK : hip_fail(c, RT_ERR_LAUNCH, what, e);
}

// The end of a call: a synchronous one waits for `stream`, and a failure there
// is `status` with the caller's text; a launch that staged records in LDS then
// reports what an RT_LDS_CHECK build found (rt_kernel.hip).
int finish(rt_ctx* c, hipStream_t stream, bool sync, const char* what, bool staged = false,
           int status = RT_ERR_LAUNCH) {
    if (!sync) return RT_OK;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(c, status, what, e);
    uint32_t short_end = 0;
    if (staged && rt::lds_check_result(&short_end) == hipSuccess && short_end)
        return fail(c, RT_ERR_LAUNCH, "LDS overflow: staged records end at byte " + std::to_string(short_end) +
                                          ", past the dispatch's dynamic LDS");
    return RT_OK;
}

// Host data into an empty buffer of its size, waited for.
hipError_t upload(DevBuf& b, const void* src, size_t bytes, hipStream_t s) {
    hipError_t e = b.resize_exact(bytes);
    if (e != hipSuccess || bytes == 0) return e;
    if ((e = hipMemcpyAsync(b.as<void>(), src, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// ev0, the launch, ev1 on `stream` (rt_last_kernel_ms).  `info` is the
// context's LaunchInfo for a launcher that fills one (rt_last_launch), null
// for one that does not: rt_last_launch then keeps the launch before.
template <typename F>
int timed_launch(rt_ctx* c, hipStream_t stream, const char* what, rt::LaunchInfo* info, F launch) {
    (void)hipEventRecord(c->ev0, stream);
    const hipError_t e = launch(info);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, (std::string(what) + " launch").c_str(), e);
    if (info) c->launched = true;
    (void)hipEventRecord(c->ev1, stream);
    c->timed = true;
    return RT_OK;
}

// KParams, MisParams and AovParams name their camera members alike.
template <typename P>
void set_camera(P* K, const rt::CamConst& cam) {
    memcpy(K->cam_pos, cam.pos, sizeof(K->cam_pos));
    memcpy(K->cam_u, cam.u, sizeof(K->cam_u));
    memcpy(K->cam_v, cam.v, sizeof(K->cam_v));
    memcpy(K->cam_w, cam.w, sizeof(K->cam_w));
    K->halfW = cam.halfW;
    K->halfH = cam.halfH;
    K->W = cam.W;
    K->H = cam.H;
}

// The largest Halton index seed + sample of a launch (0xFFFFFFFF: it wraps).
uint32_t halton_max_index(const rt_ctx* c, uint32_t sample_base, uint32_t spp) {
    const uint64_t imax = (uint64_t)c->seed_max + sample_base + (spp ? spp - 1u : 0u);
    return imax > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)imax;
}

int check_out_format(rt_ctx* c, uint32_t flags) {
    if ((flags & RT_OUT_FP16) && (flags & RT_OUT_RGBA8))
        return fail(c, RT_ERR_INVALID_ARG, "RT_OUT_FP16 and RT_OUT_RGBA8 are exclusive");
    return RT_OK;
}

// KParams carries the tables as flat members (rt_kernel.hpp).
void set_tables(rt::KParams* K, const rt::SceneTables& t) {
    K->tri_isect = t.tri_isect;
    K->pair_isect = t.pair_isect;
    K->clusters = t.clusters;
    K->sph_isect = t.sph_isect;
    K->sph_nodes = t.sph_nodes;
    K->sph_perm = t.sph_perm;
    K->sph_box = t.sph_box;
    K->tri_nodes = t.tri_nodes;
    K->tri_sorted = t.tri_sorted;
    K->tri_perm = t.tri_perm;
    K->nT = t.nT;
    K->nP = t.nP;
    K->nS = t.nS;
    K->nN = t.nN;
    K->nTN = t.nTN;
    K->nC = t.nC;
    K->pair_free = t.pair_free;
}

// What every path kernel (render, counts, path query) takes from the context's
// scene: a zeroed KParams with the tables, the shading records and the light.
void set_scene(rt::KParams* K, const rt_ctx* c) {
    memset(K, 0, sizeof(*K));
    set_tables(K, c->tab);
    K->tri_shade = c->d_scene[kTriShade].as<float4>();
    K->light_mask = c->light_mask;
    K->halton_tab = c->d_halton_tab.as<float>();
    // both compact tables or neither: the launcher takes the sphere kernel when
    // sph_lds is set, and that kernel's walks read sph_box (finish_scene)
    K->sph_lds = c->sph_compact ? c->d_scene[kSphLds].as<uint32_t>() : nullptr;
    K->sph_lds_id = c->d_scene[kSphLdsId].as<uint16_t>();
    K->sph_shade = c->d_scene[kSphShade].as<float4>();
    K->nE = c->scene.sph_lds_entries;
    memcpy(K->light_center, c->scene.light.center, sizeof(K->light_center));
    {  // rt_kernel.hip shade(): the sample point's zero terms drop out exactly unless -0 is involved
        uint32_t by, bz;
        memcpy(&by, &K->light_center[1], 4);
        memcpy(&bz, &K->light_center[2], 4);
        K->light_plain = (by != 0x80000000u && bz != 0x80000000u) ? 1u : 0u;
    }
    memcpy(K->light_color, c->scene.light.color, sizeof(K->light_color));
}

// The record arrays of c->scene on the device, for rt_create_ex (nothing
// allocated yet) and rt_update_scene alike: an array is allocated again only
// when its size changes (an empty array is a null pointer, as the kernels'
// arguments expect), the copies are enqueued and waited for once.
hipError_t upload_scene(rt_ctx* c) {
    const rt::CompiledScene& s = c->scene;
    hipError_t e = hipSuccess;
    auto put = [&](SceneArray k, const auto& v) {
        const size_t bytes = v.size() * sizeof(v[0]);
        DevBuf& b = c->d_scene[k];
        if (e == hipSuccess) e = b.resize_exact(bytes);
        if (e == hipSuccess && bytes)
            e = hipMemcpyAsync(b.as<void>(), v.data(), bytes, hipMemcpyHostToDevice, c->stream);
    };
    put(kTriIsect, s.tri_isect);
    put(kTriShade, s.tri_shade);
    put(kPairIsect, s.pair_isect);
    put(kClusters, s.clusters);
    put(kSphLds, s.sph_lds);
    put(kSphLdsId, s.sph_lds_id);
    put(kSphBox, s.sph_box);
    put(kSphIsect, s.sph_isect);
    put(kSphShade, s.sph_shade);
    put(kSphNodes, s.sph_nodes);
    put(kSphPerm, s.sph_perm);
    put(kMisShade, s.mis_shade);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

bool needs_tri_bvh(const rt_ctx* c) { return rtapi::needs_tri_bvh(scene_counts(c->scene, 0), c->scene_mem); }

void free_tri_bvh(rt_ctx* c) {
    c->d_tri_nodes.reset();
    c->d_tri_sorted.reset();
    c->d_tri_perm.reset();
    c->d_refit.reset();  // the parents of the tree that goes
    c->tri_bvh_nodes = 0;
    c->tri_bvh_build_used = 0;
    c->tri_bvh_temp_bytes = 0;
}

// The triangle BVH of c->scene from the uploaded triangle records, with the
// context's builder and options (replaces setupAccelerationStructures,
// computeShader.swift:45-97); a tree the context holds is freed first.
int build_tri_bvh(rt_ctx* c, std::string* msg) {
    using clk = std::chrono::steady_clock;
    free_tri_bvh(c);
    const rt::CompiledScene& s = c->scene;
    const uint32_t nT = (uint32_t)s.tri_isect.size();
    const size_t nn = 2 * (size_t)nT - 1;
    const auto t_build = clk::now();
    hipError_t e;
    if (c->tri_build == RT_TRI_BVH_GPU_SAH || c->tri_build == RT_TRI_BVH_GPU_LBVH) {
        if ((e = c->d_tri_nodes.reserve(rt::kTriCompactLayouts * nn * sizeof(uint4))) != hipSuccess ||
            (e = c->d_tri_sorted.reserve(3 * (size_t)nT * sizeof(float4))) != hipSuccess ||
            (e = c->d_tri_perm.reserve((size_t)nT * sizeof(uint32_t))) != hipSuccess) {
            *msg = std::string("hipMalloc(triangle BVH): ") + hipGetErrorString(e);
            return RT_ERR_OUT_OF_MEMORY;
        }
    }
    const float4* d_tri = c->d_scene[kTriIsect].as<float4>();
    uint4* d_nodes = c->d_tri_nodes.as<uint4>();
    float4* d_sorted = c->d_tri_sorted.as<float4>();
    uint32_t* d_perm = c->d_tri_perm.as<uint32_t>();
    if (c->tri_build == RT_TRI_BVH_GPU_SAH) {  // GPU binned SAH (rt_gsah.hip)
        uint32_t total = 0;
        size_t temp = 0;
        if ((e = rt::build_tri_gsah(d_tri, nT, s.margin, c->tri_leaf_opt, c->tri_leaf_cost, d_nodes, d_sorted, d_perm,
                                    &total, &temp, c->stream)) != hipSuccess) {
            *msg = std::string("triangle BVH build: ") + hipGetErrorString(e);
            return (e == hipErrorInvalidValue) ? RT_ERR_INVALID_ARG
                   : (e == hipErrorOutOfMemory) ? RT_ERR_OUT_OF_MEMORY : RT_ERR_LAUNCH;
        }
        c->tri_bvh_nodes = total;
        c->tri_bvh_temp_bytes = temp;
    } else if (c->tri_build == RT_TRI_BVH_GPU_LBVH) {  // GPU Morton build (rt_lbvh.hip)
        if ((e = rt::build_tri_lbvh(d_tri, nT, s.tri_lo, s.tri_hi, s.margin, d_nodes, d_sorted, d_perm, c->stream)) !=
            hipSuccess) {
            *msg = std::string("triangle BVH build: ") + hipGetErrorString(e);
            return (e == hipErrorInvalidValue) ? RT_ERR_INVALID_ARG : RT_ERR_LAUNCH;
        }
        c->tri_bvh_nodes = (uint32_t)nn;
    } else {  // host binned SAH (rt_scene.cpp build_tri_sah), uploaded
        std::vector<uint32_t> nodes, perm;
        std::vector<rt::TriIsect> sorted;
        if (!rt::build_tri_sah(s.tri_isect, s.margin, &nodes, &sorted, &perm, c->tri_leaf_opt, c->tri_leaf_cost)) {
            *msg = "triangle BVH build: too many triangles (2^24)";
            return RT_ERR_INVALID_ARG;
        }
        if ((e = upload(c->d_tri_nodes, nodes.data(), nodes.size() * sizeof(uint32_t), c->stream)) != hipSuccess ||
            (e = upload(c->d_tri_sorted, sorted.data(), sorted.size() * sizeof(rt::TriIsect), c->stream)) != hipSuccess ||
            (e = upload(c->d_tri_perm, perm.data(), perm.size() * sizeof(uint32_t), c->stream)) != hipSuccess) {
            *msg = std::string("triangle BVH upload: ") + hipGetErrorString(e);
            return RT_ERR_OUT_OF_MEMORY;
        }
        c->tri_bvh_nodes = (uint32_t)(nodes.size() / (4 * rt::kTriCompactLayouts));
    }
    // the LBVH leaves hold one triangle
    c->tri_leaf_max = c->tri_build == RT_TRI_BVH_GPU_LBVH ? 1u : tri_leaf_clamp(c->tri_leaf_opt);
    c->tri_bvh_build_used = c->tri_build;
    c->tri_bvh_build_ms = std::chrono::duration<float, std::milli>(clk::now() - t_build).count();
    return RT_OK;
}

// The tail of rt_create_ex and of rt_update_scene: everything a launch takes
// from the context that is derived from the compiled scene and its device
// arrays.  (The ray domain is rt::ray_domain(c->scene.extent) at every query.)
// THE scene tables (rt_kernel.hpp SceneTables) are the counts of the compiled
// scene and the context's device arrays, borrowed.
void finish_scene(rt_ctx* c) {
    c->sph_compact = rt::sphere_compact_usable(c->scene);
    c->light_mask = rt::light_mask(c->scene);
    rt::SceneTables& t = c->tab = scene_counts(c->scene, c->tri_bvh_nodes);
    t.tri_isect = c->d_scene[kTriIsect].as<float4>();
    t.pair_isect = c->d_scene[kPairIsect].as<float4>();
    t.clusters = c->d_scene[kClusters].as<float4>();
    t.sph_isect = c->d_scene[kSphIsect].as<float4>();
    t.sph_nodes = c->d_scene[kSphNodes].as<float4>();
    t.sph_perm = c->d_scene[kSphPerm].as<uint32_t>();
    // the leaf-box BVH with the compact entries or not at all (sphere_compact_usable)
    t.sph_box = c->sph_compact ? c->d_scene[kSphBox].as<uint4>() : nullptr;
    t.tri_nodes = c->d_tri_nodes.as<uint4>();
    t.tri_sorted = c->d_tri_sorted.as<float4>();
    t.tri_perm = c->d_tri_perm.as<uint32_t>();
}

// Resolves row partition defaults and validates it against the frame height.
bool resolve_rows(const rt_ctx* c, uint32_t row_start, uint32_t row_step, uint32_t row_count, uint32_t* start,
                  uint32_t* step, uint32_t* count) {
    return rtapi::resolve_rows((uint32_t)c->scene.cam.H, row_start, row_step, row_count, start, step, count);
}

// What a render launch takes from its parameters and the context's options:
// the camera, the samples, the resolved row partition and the launch choices.
void set_launch(rt::KParams* K, const rt_ctx* c, const rt_render_params* p, uint32_t start, uint32_t step,
                uint32_t count) {
    set_camera(K, c->scene.cam);
    K->spp = p->spp;
    K->sample_base = p->sample_base;
    K->row_start = start;
    K->row_step = step;
    K->row_count = count;
    K->lanes = c->lanes;
    K->walk = c->walk;
    K->walk_leaf_den = c->walk_leaf_den;
}

// The per-wave masks of the launch (K, g) in the context's table, K->wave_masks
// set to it.  The table is reused while its key matches;
// otherwise the fill is enqueued on `stream`, after every render that may still
// read the old table on any stream.  A launch on another stream than the fill's
// waits for the fill.
int ensure_wave_masks(rt_ctx* c, rt::KParams* K, const rt::WaveGrid& g, hipStream_t stream) {
    MaskKey key;
    memset(&key, 0, sizeof(key));
    memcpy(key.cam, K->cam_pos, sizeof(K->cam_pos));
    memcpy(key.cam + 3, K->cam_u, sizeof(K->cam_u));
    memcpy(key.cam + 6, K->cam_v, sizeof(K->cam_v));
    memcpy(key.cam + 9, K->cam_w, sizeof(K->cam_w));
    key.cam[12] = K->halfW;
    key.cam[13] = K->halfH;
    memcpy(key.light_center, K->light_center, sizeof(key.light_center));
    key.W = K->W;
    key.H = K->H;
    key.row_start = K->row_start;
    key.row_step = K->row_step;
    key.row_count = K->row_count;
    key.L = g.L;
    key.wave_w = g.wave_w;
    key.wave_h = g.wave_h;
    key.scene_epoch = c->scene_epoch;
    hipError_t e;
    if (!c->ev_mask_fill.h && (e = hipEventCreateWithFlags(&c->ev_mask_fill.h, hipEventDisableTiming)) != hipSuccess)
        return hip_fail(c, RT_ERR_OUT_OF_MEMORY, "hipEventCreate(mask fill)", e);
    const size_t bytes = (size_t)g.waves_x * g.waves_y * sizeof(rt::WaveMask);
    if (!c->mask_valid || memcmp(&key, &c->mask_key, sizeof(key)) != 0 || c->d_wave_masks.bytes() < bytes) {
        c->mask_valid = false;
        for (const MaskReader& r : c->mask_readers)
            if ((e = hipStreamWaitEvent(stream, r.done, 0)) != hipSuccess)
                return hip_fail(c, RT_ERR_LAUNCH, "hipStreamWaitEvent(mask table readers)", e);
        // and the last fill, which waited for the readers before it: the readers start over
        if ((e = hipStreamWaitEvent(stream, c->ev_mask_fill, 0)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "hipStreamWaitEvent(mask table fill)", e);
        for (const MaskReader& r : c->mask_readers) (void)hipEventDestroy(r.done);
        c->mask_readers.clear();
        int st;  // a table that has to grow is freed first, which waits for the device
        if ((st = reserve(c, c->d_wave_masks, bytes, "hipMalloc(wave masks)")) != RT_OK) return st;
        if ((e = rt::launch_wave_masks(*K, g, c->d_wave_masks.as<uint4>(), stream)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "wave_masks launch", e);
        if ((e = hipEventRecord(c->ev_mask_fill, stream)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "hipEventRecord(mask fill)", e);
        c->mask_key = key;
        c->mask_valid = true;
        ++c->mask_fills;
    } else if ((e = hipStreamWaitEvent(stream, c->ev_mask_fill, 0)) != hipSuccess) {
        return hip_fail(c, RT_ERR_LAUNCH, "hipStreamWaitEvent(mask table fill)", e);
    }
    K->wave_masks = c->d_wave_masks.as<uint4>();
    return RT_OK;
}

// After a render on `stream` that reads the mask table: the event a later
// refill on any stream waits for.
int note_mask_reader(rt_ctx* c, hipStream_t stream) {
    MaskReader* r = nullptr;
    for (MaskReader& q : c->mask_readers)
        if (q.stream == stream) r = &q;
    hipError_t e;
    if (!r) {
        hipEvent_t ev = nullptr;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess)
            return hip_fail(c, RT_ERR_OUT_OF_MEMORY, "hipEventCreate(mask reader)", e);
        c->mask_readers.push_back(MaskReader{stream, ev});
        r = &c->mask_readers.back();
    }
    if ((e = hipEventRecord(r->done, stream)) != hipSuccess)
        return hip_fail(c, RT_ERR_LAUNCH, "hipEventRecord(mask reader)", e);
    return RT_OK;
}

// What rt_render_counts adds to a render: one count per pixel in, the totals out.
struct CountsArgs {
    const uint32_t* counts;
    uint32_t* totals;  // or null
};

// rt_render / rt_render_async (ca == null) and rt_render_counts /
// rt_render_counts_async: one launch of a path kernel over the context's tables.
int render_impl(rt_ctx* c, const rt_render_params* p, void* out, bool out_is_device,
                hipStream_t stream, bool sync, const CountsArgs* ca = nullptr) {
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is null");
    if (ca && !ca->counts) return fail(c, RT_ERR_INVALID_ARG, "rt_render_counts: counts is null");
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (p->bounces > RT_MAX_BOUNCES)
        return fail(c, RT_ERR_INVALID_ARG,
                    "bounces > 4: Halton dimensions would leave primes[24] (sampling.metal:97)");
    if (!c->seeds_ready) return fail(c, RT_ERR_STATE, "seeds not set (rt_set_seeds/rt_fill_seeds)");
    uint32_t start, step, count;
    if (!resolve_rows(c, p->row_start, p->row_step, p->row_count, &start, &step, &count))
        return fail(c, RT_ERR_INVALID_ARG, "row partition outside the frame");
    const bool want_out = !(p->flags & RT_OUT_NONE);
    const bool keep_sum = (p->flags & RT_KEEP_SUM) != 0;
    const bool sums = keep_sum || p->accumulate;
    if (want_out && !out) return fail(c, RT_ERR_INVALID_ARG, "out is null");
    if (p->accumulate) {
        const bool rows_same = c->sum_valid && c->sum_row_start == start && c->sum_row_step == step &&
                               c->sum_row_count == count;
        if (ca) {  // every pixel continues its own sequence, which started at sample_base
            if (!rows_same || c->sum_first != p->sample_base)
                return fail(c, RT_ERR_STATE,
                            "rt_render_counts: accumulate: context sum does not start at sample_base for these rows "
                            "(render with RT_KEEP_SUM first)");
        } else {
            if (rows_same && c->sum_counts)
                return fail(c, RT_ERR_STATE,
                            "accumulate: context sum holds per-pixel sample counts (rt_render_counts): "
                            "continue it with rt_render_counts");
            if (!rows_same || (uint64_t)c->sum_first + c->sum_samples != (uint64_t)p->sample_base)
                return fail(c, RT_ERR_STATE,
                            "accumulate: context sum does not end at sample_base for these rows "
                            "(render with RT_KEEP_SUM first)");
        }
    }
    // a counts render: the upper bound of the totals (spp is the cap)
    const uint64_t total = (uint64_t)(p->accumulate ? c->sum_samples : 0u) + p->spp;
    if (ca) {
        if (total > (1ull << 24))
            return fail(c, RT_ERR_INVALID_ARG,
                        "rt_render_counts: the bound of the per-pixel totals (the caps spp of the calls into this "
                        "sum) must stay <= 2^24");
    } else if (total == 0 || total > 0xFFFFFFFFull) {
        return fail(c, RT_ERR_INVALID_ARG, "samples in the sum must be in [1, 2^32)");
    }

    const size_t pixels = (size_t)count * (size_t)c->scene.cam.W;
    int st;
    if ((st = check_out_format(c, p->flags)) != RT_OK) return st;
    const size_t out_bytes = pixels * pixel_bytes(p->flags);
    if (sums) {
        if (c->d_sum.bytes() < pixels * sizeof(float4)) c->sum_valid = false;  // it goes, even if no new one comes
        if ((st = reserve(c, c->d_sum, pixels * sizeof(float4), "hipMalloc(sum)")) != RT_OK) return st;
    }
    void* kout = want_out ? out : nullptr;
    if (want_out && !out_is_device) {
        if ((st = reserve(c, c->d_out, out_bytes, "hipMalloc(out staging)")) != RT_OK) return st;
        kout = c->d_out.as<void>();
    }
    const uint32_t* kcounts = ca ? ca->counts : nullptr;
    uint32_t* ktotals = ca ? ca->totals : nullptr;
    if (ca && !out_is_device) {  // host counts and totals through the context's staging buffers
        if ((st = reserve(c, c->d_counts, pixels * sizeof(uint32_t), "hipMalloc(counts staging)")) != RT_OK) return st;
        const hipError_t e = hipMemcpyAsync(c->d_counts.as<void>(), ca->counts, pixels * sizeof(uint32_t),
                                            hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(counts)", e);
        kcounts = c->d_counts.as<uint32_t>();
        if (ca->totals) {
            if ((st = reserve(c, c->d_totals, pixels * sizeof(uint32_t), "hipMalloc(totals staging)")) != RT_OK)
                return st;
            ktotals = c->d_totals.as<uint32_t>();
        }
    }

    rt::KParams K;
    set_scene(&K, c);
    K.seeds = c->d_seeds.as<uint32_t>();
    K.sum = sums ? c->d_sum.as<float4>() : nullptr;
    K.out = kout;
    set_launch(&K, c, p, start, step, count);
    K.accumulate = p->accumulate ? 1u : 0u;
    K.samples_total = (uint32_t)total;
    K.flags = ((p->flags & RT_OUT_FP16) ? rt::kOutFp16 : 0u) | ((p->flags & RT_OUT_RGBA8) ? rt::kOutRgba8 : 0u);
    // a counts render: pixel p's last index is sample_base + total_p - 1, and total_p <= total
    K.max_index = halton_max_index(c, p->sample_base, ca ? (uint32_t)total : p->spp);

    // the box-cluster render kernel reads its waves' masks from the context's table
    // (the counts kernel keeps its own prologue); a fill goes before ev0
    rt::WaveGrid wg{};
    const bool masks = !ca && rt::wave_mask_grid(K, p->bounces, c->scene_mem, 0, &wg);
    if (masks && (st = ensure_wave_masks(c, &K, wg, stream)) != RT_OK) return st;

    if (keep_sum && !p->accumulate) c->sum_valid = false;  // being overwritten
    if ((st = timed_launch(c, stream, ca ? "path_counts" : "path_trace", &c->launch, [&](rt::LaunchInfo* info) {
             return ca ? rt::launch_path_counts(K, kcounts, ktotals, p->bounces, c->scene_mem, stream, info)
                       : rt::launch_path_trace(K, p->bounces, c->scene_mem, stream, info);
         })) != RT_OK)
        return st;
    if (masks && (st = note_mask_reader(c, stream)) != RT_OK) return st;
    if (sums) {  // the kernel (re)wrote the running sums
        c->sum_valid = true;
        c->sum_row_start = start;
        c->sum_row_step = step;
        c->sum_row_count = count;
        if (!p->accumulate) c->sum_first = p->sample_base;
        c->sum_samples = (uint32_t)total;
        c->sum_counts = ca != nullptr;  // a uniform render never continues a counts sum
    }
    if (ca && ca->totals && !out_is_device &&
        (st = copy_down(c, ca->totals, ktotals, pixels * sizeof(uint32_t), stream, "hipMemcpyAsync(totals)")) != RT_OK)
        return st;
    if (want_out && !out_is_device &&
        (st = copy_down(c, out, kout, out_bytes, stream, "hipMemcpyAsync(out)")) != RT_OK)
        return st;
    return finish(c, stream, sync, "path_trace execution", /*staged*/ true);
}

// Rank 0's placement after the gather: tile row j of rank k -> frame row
// k + j*N (rt_kernel.hip place_tiles_kernel, one launch on `stream`).  A host
// frame is assembled in the context's staging buffer, then copied down once
// the kernel has finished.
int place_tiles_impl(rt_ctx* c, const void* gathered, uint32_t N, uint32_t flags, void* frame,
                     hipStream_t stream) {
    const uint32_t W = (uint32_t)c->scene.cam.W, H = (uint32_t)c->scene.cam.H;
    const TileLayout L = tile_layout(W, H, N, 0, flags);
    const bool dev = (flags & RT_OUT_DEVICE) != 0;
    const size_t frame_bytes = (size_t)H * L.row_bytes;
    void* dst = frame;
    int st;
    if (!dev) {
        if ((st = reserve(c, c->d_out, frame_bytes, "hipMalloc(frame staging)")) != RT_OK) return st;
        dst = c->d_out.as<void>();
    }
    hipError_t e = rt::launch_place_tiles(gathered, dst, L.row_bytes, L.tile_bytes, H, N, stream);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "place_tiles launch", e);
    if (!dev) {
        if ((e = hipStreamSynchronize(stream)) != hipSuccess ||
            (e = hipMemcpyAsync(frame, dst, frame_bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "frame copy to host", e);
    }
    return RT_OK;
}

// rt_render_gather: this rank's interleaved rows into d_tile, one ncclGather of
// the (padded, equal-sized) tiles to rank 0, then place_tiles_dev.
int render_gather_impl(rt_ctx* c, const rt_render_params* p, void* frame, hipStream_t stream) {
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is null");
    if (!c->comm) return fail(c, RT_ERR_STATE, "no communicator (rt_comm_init)");
    if (p->row_start || p->row_step > 1 || p->row_count)
        return fail(c, RT_ERR_INVALID_ARG, "rt_render_gather partitions the rows itself: "
                                           "params must name the whole frame (row_start 0, "
                                           "row_step 0 or 1, row_count 0)");
    int st;
    if ((st = check_out_format(c, p->flags)) != RT_OK) return st;
    const bool want_out = !(p->flags & RT_OUT_NONE);
    const bool dev = (p->flags & RT_OUT_DEVICE) != 0;
    if (want_out && c->rank == 0 && !frame) return fail(c, RT_ERR_INVALID_ARG, "frame is null on rank 0");
    const uint32_t H = (uint32_t)c->scene.cam.H, W = (uint32_t)c->scene.cam.W, N = (uint32_t)c->world;
    const TileLayout L = tile_layout(W, H, N, (uint32_t)c->rank, p->flags);
    hipError_t e;
    // d_tile / d_gather are reused: a previous call on another stream may still
    // be gathering from them (RT_OUT_DEVICE returns without a host sync)
    if (c->tiles_pending && (e = hipStreamWaitEvent(stream, c->ev_tiles, 0)) != hipSuccess)
        return hip_fail(c, RT_ERR_LAUNCH, "hipStreamWaitEvent(previous gather)", e);
    if (want_out && (st = reserve(c, c->d_tile, L.tile_bytes, "hipMalloc(tile)")) != RT_OK) return st;
    if (L.rows > 0) {  // a rank past the last row renders nothing but still joins the gather
        rt_render_params q = *p;
        q.row_start = (uint32_t)c->rank;
        q.row_step = N;
        q.row_count = L.rows;
        q.flags = p->flags | RT_OUT_DEVICE;
        if ((st = render_impl(c, &q, c->d_tile.as<void>(), true, stream, false)) != RT_OK) return st;
    }
    if (!want_out) return RT_OK;
    if (c->rank == 0 && (st = reserve(c, c->d_gather, L.tile_bytes * N, "hipMalloc(gather)")) != RT_OK) return st;
    ncclResult_t r = ncclGather(c->d_tile.as<void>(), c->rank == 0 ? c->d_gather.as<void>() : nullptr, L.tile_bytes,
                                ncclUint8, 0, c->comm, stream);
    if (r != ncclSuccess) return nccl_fail(c, "ncclGather", r);
    if (c->rank == 0 && (st = place_tiles_impl(c, c->d_gather.as<void>(), N, p->flags, frame, stream)) != RT_OK)
        return st;
    if ((e = hipEventRecord(c->ev_tiles, stream)) != hipSuccess)
        return hip_fail(c, RT_ERR_LAUNCH, "hipEventRecord(gather)", e);
    c->tiles_pending = true;
    return finish(c, stream, !dev, "render+gather execution", /*staged*/ false, RT_ERR_COMM);
}

// MIS sample table: the u of every strategy depends only on the sample index
// (haltonRandom(i, d), shaders.metal:556,564,584,595,617), not on the pixel.
int mis_table(rt_ctx* c, uint32_t S) {
    if (c->d_mis_tab && c->mis_tab_S == S) return RT_OK;
    std::vector<float> t((size_t)S * 12u);
    for (uint32_t i = 0; i < S; ++i) {
        float* q = &t[(size_t)i * 12u];
        q[0] = halton_host(i, 0);            // light sampling :556
        q[1] = halton_host(i, 1);
        q[2] = 0.0f;
        q[3] = 0.0f;
        q[4] = halton_host(i + S, 2);        // cosine :564
        q[5] = halton_host(i + S, 3);
        q[6] = halton_host(i, 6);            // its secondary NEE :584
        q[7] = halton_host(i, 7);
        q[8] = halton_host(i + 2 * S, 4);    // VNDF :595
        q[9] = halton_host(i + 2 * S, 5);
        q[10] = halton_host(i + S, 6);       // its secondary NEE :617
        q[11] = halton_host(i + S, 7);
    }
    c->d_mis_tab.reset();
    c->mis_tab_S = 0;
    hipError_t e = upload(c->d_mis_tab, t.data(), t.size() * sizeof(float), c->stream);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_OUT_OF_MEMORY, "MIS table upload", e);
    c->mis_tab_S = S;
    return RT_OK;
}

int render_mis_impl(rt_ctx* c, const rt_mis_params* p, float* out, uint8_t* out8) {
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "params is null");
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (!out && !out8) return fail(c, RT_ERR_INVALID_ARG, "both outputs are null");
    if (!c->scene.sph_isect.empty())
        return fail(c, RT_ERR_INVALID_ARG,
                    "the MIS integrator traces triangle scenes only (shaders.metal:459-509)");
    if (c->scene.tri_isect.empty()) return fail(c, RT_ERR_INVALID_ARG, "scene has no triangles");
    if (p->camera_rays == 0) return fail(c, RT_ERR_INVALID_ARG, "camera_rays must be >= 1");
    if (p->mis_samples < 3 || p->mis_samples / 3u > (1u << 20))
        return fail(c, RT_ERR_INVALID_ARG, "mis_samples must be in [3, 3 * 2^20]");
    uint32_t start, step, count;
    if (!resolve_rows(c, p->row_start, p->row_step, p->row_count, &start, &step, &count))
        return fail(c, RT_ERR_INVALID_ARG, "row partition outside the frame");
    const uint32_t S = p->mis_samples / 3u;  // samplesPerStrategy (:546)
    int st = mis_table(c, S);
    if (st != RT_OK) return st;
    const bool dev = (p->flags & RT_OUT_DEVICE) != 0;
    const size_t pixels = (size_t)count * (size_t)c->scene.cam.W;
    float4* kout = reinterpret_cast<float4*>(out);
    uchar4* kout8 = reinterpret_cast<uchar4*>(out8);
    if (out && !dev) {
        if ((st = reserve(c, c->d_out, pixels * 16u, "hipMalloc(out staging)")) != RT_OK) return st;
        kout = c->d_out.as<float4>();
    }
    if (out8 && !dev) {
        if ((st = reserve(c, c->d_out8, pixels * 4u, "hipMalloc(out8 staging)")) != RT_OK) return st;
        kout8 = c->d_out8.as<uchar4>();
    }

    rt::MisParams K;
    memset(&K, 0, sizeof(K));
    K.tab = c->tab;  // no spheres (checked above): its sphere members are null / 0
    K.mis_shade = c->d_scene[kMisShade].as<float4>();
    K.u_tab = c->d_mis_tab.as<float4>();
    K.out = kout;
    K.out8 = kout8;
    set_camera(&K, c->scene.cam);
    const rt::MisLightConst& ml = c->scene.mis_light;
    memcpy(K.l_center, ml.center, sizeof(K.l_center));
    memcpy(K.l_tangent, ml.tangent, sizeof(K.l_tangent));
    memcpy(K.l_bitangent, ml.bitangent, sizeof(K.l_bitangent));
    memcpy(K.l_radiance, ml.radiance, sizeof(K.l_radiance));
    K.l_width = ml.width;
    K.l_depth = ml.depth;
    K.l_area = ml.area;
    K.exposure = ml.exposure;
    K.camera_rays = p->camera_rays;
    K.S = S;
    K.row_start = start;
    K.row_step = step;
    K.row_count = count;
    const size_t pb = rt::mis_part_bytes(K.camera_rays, pixels);
    hipError_t e;
    if (c->d_mis_part.bytes() > 2 * pb) {  // a much smaller (or unsplit) frame: give the memory back
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)  // the last launch may still read it
            return hip_fail(c, RT_ERR_LAUNCH, "hipStreamSynchronize(mis)", e);
        c->d_mis_part.reset();
    }
    if (pb) {
        if ((st = reserve(c, c->d_mis_part, pb, "hipMalloc(mis records)")) != RT_OK) return st;
        K.part = c->d_mis_part.as<float4>();
    }

    // the MIS launcher reports no LaunchInfo: rt_last_launch keeps the launch before
    if ((st = timed_launch(c, c->stream, "mis", nullptr,
                           [&](rt::LaunchInfo*) { return rt::launch_mis(K, c->scene_mem, c->stream); })) != RT_OK)
        return st;
    if (out && !dev && (st = copy_down(c, out, kout, pixels * 16u, c->stream, "hipMemcpyAsync(out)")) != RT_OK)
        return st;
    if (out8 && !dev && (st = copy_down(c, out8, kout8, pixels * 4u, c->stream, "hipMemcpyAsync(out8)")) != RT_OK)
        return st;
    return finish(c, c->stream, true, "mis execution");
}

// rt_trace_rays / rt_trace_rays_async: one launch of the query kernel
// (rt_rays.hip) over the context's tables.  Host pointers go through the
// context's staging buffers on its own stream.
int trace_rays_impl(rt_ctx* c, const rt_ray* rays, uint64_t n, uint32_t flags, rt_ray_hit* hits, bool dev,
                    hipStream_t stream, bool sync) {
    static_assert(sizeof(rt_ray) == 32 && sizeof(rt_ray_hit) == 8, "rt_ray / rt_ray_hit layout");
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (flags & ~(uint32_t)(RT_OUT_DEVICE | RT_RAYS_ANY | RT_RAYS_EXACT))
        return fail(c, RT_ERR_INVALID_ARG, "rt_trace_rays: unknown flag bits");
    if (n > 0x80000000ull) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_rays: n > 2^31");
    if (n == 0) return RT_OK;
    if (!rays || !hits) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_rays: rays or hits is null");
    hipError_t e;
    int st;
    const size_t ray_bytes = (size_t)n * sizeof(rt_ray), hit_bytes = (size_t)n * sizeof(rt_ray_hit);
    const void* krays = rays;
    void* khits = hits;
    if (!dev) {
        if ((st = reserve(c, c->d_rays, ray_bytes, "hipMalloc(ray staging)")) != RT_OK ||
            (st = reserve(c, c->d_hits, hit_bytes, "hipMalloc(hit staging)")) != RT_OK)
            return st;
        krays = c->d_rays.as<void>();
        khits = c->d_hits.as<void>();
        if ((e = hipMemcpyAsync(c->d_rays.as<void>(), rays, ray_bytes, hipMemcpyHostToDevice, stream)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(rays)", e);
    }
    rt::RayQueryParams K;
    memset(&K, 0, sizeof(K));
    K.tab = c->tab;
    K.sph_compact = c->sph_compact ? 1u : 0u;
    K.rays = reinterpret_cast<const float4*>(krays);
    K.hits = reinterpret_cast<uint2*>(khits);
    K.n = (uint32_t)n;
    K.flags = flags & (RT_RAYS_ANY | RT_RAYS_EXACT);
    K.dom = rt::ray_domain(c->scene.extent);
    if ((st = timed_launch(c, stream, "ray_query", &c->launch, [&](rt::LaunchInfo* info) {
             return rt::launch_ray_query(K, c->scene_mem, stream, info);
         })) != RT_OK)
        return st;
    if (!dev && (st = copy_down(c, hits, khits, hit_bytes, stream, "hipMemcpyAsync(hits)")) != RT_OK) return st;
    return finish(c, stream, sync, "ray_query execution");
}

// rt_trace_paths / rt_trace_paths_async: one launch of the path-query kernel
// (rt_paths.hpp) over the context's tables and shading records.  Host pointers
// go through the context's staging buffers on its own stream.
int trace_paths_impl(rt_ctx* c, const rt_path_params* p, const rt_ray* rays, const uint32_t* seeds, uint64_t n,
                     float* radiance, rt_ray_hit* first_hits, bool dev, hipStream_t stream, bool sync) {
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (n > 0x80000000ull) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: n > 2^31");
    if (n == 0) return RT_OK;
    if (!p || !rays || !radiance) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: params, rays or radiance is null");
    if (p->spp < 1 || p->spp > (1u << 24)) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: spp must be in 1 .. 2^24");
    if (p->bounces > RT_MAX_BOUNCES)
        return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: bounces > 4: Halton dimensions would leave primes[24]");
    if (p->lanes_per_ray != 0 && p->lanes_per_ray != 1 && p->lanes_per_ray != 16)
        return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: lanes_per_ray must be 0, 1 or 16");
    if ((1ull << 20) + p->sample_base + p->spp > (1ull << 32))
        return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: 2^20 + sample_base + spp passes 2^32 (the Halton index wraps)");
    if (p->flags & ~(uint32_t)RT_OUT_DEVICE) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: unknown flags bits");
    if (p->reserved != 0) return fail(c, RT_ERR_INVALID_ARG, "rt_trace_paths: reserved must be 0");
    hipError_t e;
    int st;
    const size_t ray_bytes = (size_t)n * sizeof(rt_ray), hit_bytes = (size_t)n * sizeof(rt_ray_hit);
    const size_t seed_bytes = (size_t)n * sizeof(uint32_t), rad_bytes = (size_t)n * 4 * sizeof(float);
    rt::PathQueryArgs A{};
    A.rays = reinterpret_cast<const float4*>(rays);
    A.seeds = seeds;
    A.radiance = reinterpret_cast<float4*>(radiance);
    A.hits = reinterpret_cast<uint2*>(first_hits);
    if (!dev) {
        if ((st = reserve(c, c->d_rays, ray_bytes, "hipMalloc(ray staging)")) != RT_OK ||
            (st = reserve(c, c->d_radiance, rad_bytes, "hipMalloc(radiance staging)")) != RT_OK)
            return st;
        A.rays = c->d_rays.as<float4>();
        A.radiance = c->d_radiance.as<float4>();
        if ((e = hipMemcpyAsync(c->d_rays.as<void>(), rays, ray_bytes, hipMemcpyHostToDevice, stream)) != hipSuccess)
            return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(rays)", e);
        if (seeds) {
            if ((st = reserve(c, c->d_ray_seeds, seed_bytes, "hipMalloc(ray seed staging)")) != RT_OK) return st;
            A.seeds = c->d_ray_seeds.as<uint32_t>();
            if ((e = hipMemcpyAsync(c->d_ray_seeds.as<void>(), seeds, seed_bytes, hipMemcpyHostToDevice, stream)) !=
                hipSuccess)
                return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(ray seeds)", e);
        }
        if (first_hits) {
            if ((st = reserve(c, c->d_hits, hit_bytes, "hipMalloc(hit staging)")) != RT_OK) return st;
            A.hits = c->d_hits.as<uint2>();
        }
    }
    A.n = (uint32_t)n;
    A.seed_key = p->seed_key;
    A.dom = rt::ray_domain(c->scene.extent);
    rt::KParams K;
    set_scene(&K, c);
    K.spp = p->spp;
    K.sample_base = p->sample_base;
    K.lanes = p->lanes_per_ray;
    // every seed is masked to 20 bits: the bound needs no look at device memory
    K.max_index = 0xFFFFFu + p->sample_base + (p->spp - 1u);
    if ((st = timed_launch(c, stream, "path_query", &c->launch, [&](rt::LaunchInfo* info) {
             return rt::launch_path_query(K, A, p->bounces, c->scene_mem, stream, info);
         })) != RT_OK)
        return st;
    if (!dev) {
        if ((st = copy_down(c, radiance, A.radiance, rad_bytes, stream, "hipMemcpyAsync(radiance)")) != RT_OK) return st;
        if (first_hits &&
            (st = copy_down(c, first_hits, A.hits, hit_bytes, stream, "hipMemcpyAsync(first hits)")) != RT_OK)
            return st;
    }
    return finish(c, stream, sync, "path_query execution", /*staged*/ true);
}

// rt_render_aov / rt_render_aov_async: one launch of the feature-buffer kernel
// (rt_aov.hip) over the context's tables and shading records.  Host buffers go
// through the context's staging buffers on its own stream.
int render_aov_impl(rt_ctx* c, const rt_aov_params* p, const rt_aov_buffers* b, bool dev, hipStream_t stream,
                    bool sync) {
    static_assert(sizeof(rt_aov_params) == 24 && sizeof(rt_aov_buffers) == 24, "rt_aov_params / rt_aov_buffers layout");
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: params is null");
    if (!b) return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: buffers is null");
    if (!b->albedo && !b->normal_depth && !b->first_hit)
        return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: all three buffers are null");
    if (p->flags & ~(uint32_t)(RT_OUT_DEVICE | RT_AOV_CENTER))
        return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: unknown flag bits");
    if (p->spp == 0 || p->spp > (1u << 24))
        return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: spp must be in [1, 2^24] (the coverage sum stays exact)");
    const bool center = (p->flags & RT_AOV_CENTER) != 0;
    if (center && p->spp != 1) return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: RT_AOV_CENTER needs spp == 1");
    uint32_t start, step, count;
    if (!resolve_rows(c, p->row_start, p->row_step, p->row_count, &start, &step, &count))
        return fail(c, RT_ERR_INVALID_ARG, "rt_render_aov: row partition outside the frame");
    if (!center && !c->seeds_ready)
        return fail(c, RT_ERR_STATE, "rt_render_aov: seeds not set (rt_set_seeds/rt_fill_seeds)");

    const size_t pixels = (size_t)count * (size_t)c->scene.cam.W;
    void* host[3] = {b->albedo, b->normal_depth, b->first_hit};
    const size_t bytes[3] = {pixels * sizeof(float4), pixels * sizeof(float4), pixels * sizeof(rt_ray_hit)};
    void* kbuf[3] = {host[0], host[1], host[2]};
    int st;
    if (!dev) {
        for (int k = 0; k < 3; ++k) {
            if (!host[k]) continue;
            if ((st = reserve(c, c->d_aov[k], bytes[k], "hipMalloc(aov staging)")) != RT_OK) return st;
            kbuf[k] = c->d_aov[k].as<void>();
        }
    }
    rt::AovParams K;
    memset(&K, 0, sizeof(K));
    K.tab = c->tab;
    K.sph_compact = c->sph_compact ? 1u : 0u;
    K.tri_shade = c->d_scene[kTriShade].as<float4>();
    K.sph_shade = c->d_scene[kSphShade].as<float4>();
    K.seeds = center ? nullptr : c->d_seeds.as<uint32_t>();
    K.albedo = static_cast<float4*>(kbuf[0]);
    K.normal_depth = static_cast<float4*>(kbuf[1]);
    K.first_hit = static_cast<uint2*>(kbuf[2]);
    set_camera(&K, c->scene.cam);
    K.spp = p->spp;
    K.sample_base = center ? 0u : p->sample_base;
    K.row_start = start;
    K.row_step = step;
    K.row_count = count;
    K.flags = center ? rt::kAovCenter : 0u;
    if (!center) K.max_index = halton_max_index(c, p->sample_base, p->spp);
    if ((st = timed_launch(c, stream, "aov", &c->launch, [&](rt::LaunchInfo* info) {
             return rt::launch_aov(K, c->scene_mem, stream, info);
         })) != RT_OK)
        return st;
    if (!dev) {
        for (int k = 0; k < 3; ++k)
            if (host[k] && (st = copy_down(c, host[k], kbuf[k], bytes[k], stream, "hipMemcpyAsync(aov)")) != RT_OK)
                return st;
    }
    return finish(c, stream, sync, "aov execution");
}

// rt_denoise / rt_denoise_async: prepare, variance pre-filter and the a-trous
// passes (rt_denoise.hip) on whole frames.  Host buffers go through the
// context's staging buffers on its own stream; the staged output is the staged
// color_a (the filter may write over it).
int denoise_impl(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_buffers* b, bool dev, hipStream_t stream,
                 bool sync) {
    static_assert(sizeof(rt_denoise_params) == 32 && sizeof(rt_denoise_buffers) == 40 &&
                      offsetof(rt_denoise_buffers, out) == 32,
                  "rt_denoise_params / rt_denoise_buffers layout");
    if (!p) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: params is null");
    if (!b) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: buffers is null");
    const void* in[4] = {b->color_a, b->color_b, b->albedo, b->normal_depth};
    static const char* const names[4] = {"color_a", "color_b", "albedo", "normal_depth"};
    for (int k = 0; k < 4; ++k)
        if (!in[k]) return fail(c, RT_ERR_INVALID_ARG, std::string("rt_denoise: ") + names[k] + " is null");
    if (!b->out) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: out is null");
    if (p->iterations < 1 || p->iterations > 6)
        return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: iterations must be in [1, 6]");
    if (p->normal_power_log2 > 10) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: normal_power_log2 must be <= 10");
    if (!(p->sigma_luminance >= 0.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: sigma_luminance must be >= 0");
    if (!(p->sigma_depth >= 0.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: sigma_depth must be >= 0");
    if (!(p->depth_floor > 0.0f)) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: depth_floor must be > 0");
    if (p->flags & ~(uint32_t)RT_OUT_DEVICE) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: unknown flag bits");
    if (p->reserved[0] || p->reserved[1]) return fail(c, RT_ERR_INVALID_ARG, "rt_denoise: reserved must be 0");

    const size_t bytes = (size_t)c->scene.cam.W * (size_t)c->scene.cam.H * sizeof(float4);
    int st;
    for (int k = 0; k < (dev ? 2 : 6); ++k)
        if ((st = reserve(c, c->d_den[k], bytes, "hipMalloc(denoise scratch)")) != RT_OK) return st;
    hipError_t e;
    const void* kin[4] = {in[0], in[1], in[2], in[3]};
    void* kout = b->out;
    if (!dev) {
        for (int k = 0; k < 4; ++k) {
            void* staged = c->d_den[2 + k].as<void>();
            if ((e = hipMemcpyAsync(staged, in[k], bytes, hipMemcpyHostToDevice, stream)) != hipSuccess)
                return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(denoise inputs)", e);
            kin[k] = staged;
        }
        kout = c->d_den[2].as<void>();  // the staged color_a
    }
    rt::DenoiseParams K{};
    K.color_a = static_cast<const float4*>(kin[0]);
    K.color_b = static_cast<const float4*>(kin[1]);
    K.albedo = static_cast<const float4*>(kin[2]);
    K.normal_depth = static_cast<const float4*>(kin[3]);
    K.out = static_cast<float4*>(kout);
    K.scratch[0] = c->d_den[0].as<float4>();
    K.scratch[1] = c->d_den[1].as<float4>();
    K.W = c->scene.cam.W;
    K.H = c->scene.cam.H;
    K.iterations = p->iterations;
    K.normal_power_log2 = p->normal_power_log2;
    K.sigma_luminance = p->sigma_luminance;
    K.sigma_depth = p->sigma_depth;
    K.depth_floor = p->depth_floor;
    if ((st = timed_launch(c, stream, "denoise", &c->launch,
                           [&](rt::LaunchInfo* info) { return rt::launch_denoise(K, stream, info); })) != RT_OK)
        return st;
    if (!dev && (st = copy_down(c, b->out, kout, bytes, stream, "hipMemcpyAsync(denoise out)")) != RT_OK) return st;
    return finish(c, stream, sync, "denoise execution");
}

// rt_reproject / rt_reproject_async: one launch of reproject_kernel
// (rt_reproject.hip) on whole frames, the context's camera against
// `prev_camera`.  Host buffers go through the context's staging buffers on its
// own stream; the staged outputs are the staged colours (out[k] may be color[k]).
int reproject_impl(rt_ctx* c, const rt_reproject_params* p, const CameraGPU* prev_camera,
                   const rt_reproject_buffers* b, bool dev, hipStream_t stream, bool sync) {
    uint32_t planes = 0;
    const std::string bad = reproject_check(p, b, RT_OUT_DEVICE, &planes);
    if (!bad.empty()) return fail(c, RT_ERR_INVALID_ARG, "rt_reproject: " + bad);
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    rt::ReprojectArgs A;
    std::string why;
    if (!reproject_args(p, b, c->scene.cam, prev_camera, &A, &why))
        return fail(c, RT_ERR_INVALID_ARG, "rt_reproject: " + why);
    const size_t px = (size_t)A.W * (size_t)A.H, bytes = px * sizeof(float4), hit_bytes = px * sizeof(uint2);
    int st;
    if (!dev) {
        // color[0], color[1], history[0], history[1], normal_depth, prev_normal_depth, hit, prev_hit
        const void* in[8] = {b->color[0], b->color[1], b->history[0], b->history[1],
                             b->normal_depth, b->prev_normal_depth, b->hit, b->prev_hit};
        void* staged[8] = {};
        for (int k = 0; k < 8; ++k) {
            if (!in[k]) continue;  // plane 1 of a one-plane call
            const size_t n = k < 6 ? bytes : hit_bytes;
            if ((st = reserve(c, c->d_rep[k], n, "hipMalloc(reproject staging)")) != RT_OK) return st;
            staged[k] = c->d_rep[k].as<void>();
            const hipError_t e = hipMemcpyAsync(staged[k], in[k], n, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(reproject inputs)", e);
        }
        for (int k = 0; k < 2; ++k) {
            A.color[k] = static_cast<const float*>(staged[k]);
            A.history[k] = static_cast<const float*>(staged[2 + k]);
            A.out[k] = static_cast<float*>(staged[k]);
        }
        A.normal_depth = static_cast<const float*>(staged[4]);
        A.prev_normal_depth = static_cast<const float*>(staged[5]);
        A.hit = staged[6];
        A.prev_hit = staged[7];
    }
    if ((st = timed_launch(c, stream, "reproject", &c->launch, [&](rt::LaunchInfo* info) {
             return rt::launch_reproject(A, planes, stream, info);
         })) != RT_OK)
        return st;
    if (!dev)
        for (uint32_t k = 0; k < planes; ++k)
            if ((st = copy_down(c, b->out[k], A.out[k], bytes, stream, "hipMemcpyAsync(reproject out)")) != RT_OK)
                return st;
    return finish(c, stream, sync, "reproject execution");
}

// rt_plan_samples / rt_plan_samples_async: the planner's two kernels
// (rt_adaptive.hip) on a tile of `rows` rows of the camera's width.  Host
// images and counts go through the context's staging buffers on its own
// stream; the statistics come from the context's accumulators.  `stats` is
// host memory in the synchronous call, device memory in the asynchronous one.
int plan_impl(rt_ctx* c, const rt_plan_params* p, const float* first, const float* all, uint32_t* counts,
              rt_plan_stats* stats, bool dev, hipStream_t stream, bool sync) {
    if (const char* why = plan_params_error(p, RT_OUT_DEVICE | RT_PLAN_RELATIVE))
        return fail(c, RT_ERR_INVALID_ARG, std::string("rt_plan_samples: ") + why);
    if (!first || !all || !counts) return fail(c, RT_ERR_INVALID_ARG, "rt_plan_samples: first, all or counts is null");
    const uint32_t H = (uint32_t)c->scene.cam.H, rows = p->rows ? p->rows : H;
    if (rows > H) return fail(c, RT_ERR_INVALID_ARG, "rt_plan_samples: rows exceeds the camera's height");
    const size_t pixels = (size_t)rows * (size_t)c->scene.cam.W;
    const size_t img_bytes = pixels * sizeof(float4), cnt_bytes = pixels * sizeof(uint32_t);
    int st;
    hipError_t e;
    if ((st = reserve(c, c->d_plan, sizeof(rt::PlanStats), "hipMalloc(plan accumulators)")) != RT_OK) return st;
    const void* kin[2] = {first, all};
    uint32_t* kcounts = counts;
    if (!dev) {
        for (int k = 0; k < 2; ++k) {
            if ((st = reserve(c, c->d_plan_in[k], img_bytes, "hipMalloc(plan staging)")) != RT_OK) return st;
            if ((e = hipMemcpyAsync(c->d_plan_in[k].as<void>(), kin[k], img_bytes, hipMemcpyHostToDevice, stream)) !=
                hipSuccess)
                return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(plan inputs)", e);
            kin[k] = c->d_plan_in[k].as<void>();
        }
        if ((st = reserve(c, c->d_counts, cnt_bytes, "hipMalloc(counts staging)")) != RT_OK) return st;
        kcounts = c->d_counts.as<uint32_t>();
    }
    rt::PlanParams K{};
    K.first = static_cast<const float4*>(kin[0]);
    K.all = static_cast<const float4*>(kin[1]);
    K.counts = kcounts;
    K.acc = c->d_plan.as<rt::PlanStats>();
    K.budget = p->budget;
    K.count_min = p->count_min;
    K.count_max = p->count_max;
    K.luminance_floor = p->luminance_floor;
    K.radius = p->radius;
    K.W = c->scene.cam.W;
    K.rows = (int32_t)rows;
    K.flags = p->flags & RT_PLAN_RELATIVE;
    if ((st = timed_launch(c, stream, "plan", &c->launch,
                           [&](rt::LaunchInfo* info) { return rt::launch_plan(K, stream, info); })) != RT_OK)
        return st;
    if (!dev && (st = copy_down(c, counts, kcounts, cnt_bytes, stream, "hipMemcpyAsync(counts)")) != RT_OK) return st;
    if (stats) {  // synchronous: host memory; asynchronous: device memory
        e = hipMemcpyAsync(stats, K.acc, sizeof(rt_plan_stats), sync ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           stream);
        if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "hipMemcpyAsync(plan stats)", e);
    }
    return finish(c, stream, sync, "plan execution");
}

}  // namespace

extern "C" {

const char* rt_last_error(const rt_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_create_err.c_str();
}

int rt_create(const rt_scene_desc* d, rt_ctx** out_ctx) { return rt_create_ex(d, nullptr, out_ctx); }

int rt_create_ex(const rt_scene_desc* d, const rt_create_options* opt, rt_ctx** out_ctx) {
    if (!out_ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "out_ctx is null");
    *out_ctx = nullptr;
    if (!d) return fail(nullptr, RT_ERR_INVALID_ARG, "scene desc is null");
    if (!d->camera) return fail(nullptr, RT_ERR_INVALID_ARG, "camera is null");
    if (!d->square_lights || d->n_square_lights < 1)
        return fail(nullptr, RT_ERR_INVALID_ARG, "square_lights[0] is required (raytrace.metal:22)");
    Resolved ro;
    const char* why = nullptr;
    if (!resolve_options(opt, &ro, &why)) return fail(nullptr, RT_ERR_INVALID_ARG, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE,
                    std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0"));
    if (d->device < 0 || d->device >= count)
        return fail(nullptr, RT_ERR_NO_DEVICE, "device ordinal out of range");

    rt_ctx* c = new (std::nothrow) rt_ctx();
    if (!c) return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "host allocation");
    c->device = d->device;
    c->lanes = ro.lanes;
    c->tri_build = ro.tri_build;
    c->scene_mem = ro.mem;
    c->walk = ro.walk;
    c->walk_leaf_den = ro.walk_leaf_den;
    c->tri_leaf_opt = ro.tri_leaf_max;
    c->tri_leaf_cost = ro.tri_leaf_cost;
    c->build_opt = ro.build;
    DeviceGuard g(c->device);  // also round every `delete c` below: a partly built context frees what it has
    const char* err = nullptr;
    using clk = std::chrono::steady_clock;
    const auto t_compile = clk::now();
    if (!compile_desc(d, ro.build, &c->scene, &err)) {
        delete c;
        return fail(nullptr, RT_ERR_INVALID_ARG, err);
    }
    c->scene_compile_ms = std::chrono::duration<float, std::milli>(clk::now() - t_compile).count();
    int status = RT_OK;
    std::string msg;
    do {
        if ((e = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking)) != hipSuccess) {
            status = RT_ERR_NO_DEVICE; msg = std::string("hipStreamCreate: ") + hipGetErrorString(e); break;
        }
        if ((e = hipEventCreate(&c->ev0.h)) != hipSuccess || (e = hipEventCreate(&c->ev1.h)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&c->ev_tiles.h, hipEventDisableTiming)) != hipSuccess) {
            status = RT_ERR_NO_DEVICE; msg = std::string("hipEventCreate: ") + hipGetErrorString(e); break;
        }
        if ((e = upload_scene(c)) != hipSuccess) {
            status = RT_ERR_OUT_OF_MEMORY; msg = std::string("scene upload: ") + hipGetErrorString(e); break;
        }
        if (needs_tri_bvh(c) && (status = build_tri_bvh(c, &msg)) != RT_OK) break;
        const size_t npx = (size_t)c->scene.cam.W * (size_t)c->scene.cam.H;
        if ((e = c->d_seeds.reserve(npx * sizeof(uint32_t))) != hipSuccess) {
            status = RT_ERR_OUT_OF_MEMORY; msg = std::string("hipMalloc(seeds): ") + hipGetErrorString(e); break;
        }
        // the Halton low-digit tables: the same for every scene, made once per
        // context and copied into LDS by the box-cluster kernel's workgroups
        if ((e = c->d_halton_tab.resize_exact(sizeof(float) * rt::kHaltonTabLdsFloats)) != hipSuccess) {
            status = RT_ERR_OUT_OF_MEMORY; msg = std::string("hipMalloc(halton tables): ") + hipGetErrorString(e); break;
        }
        if ((e = rt::launch_fill_halton_tables(c->d_halton_tab.as<float>(), c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
            status = RT_ERR_LAUNCH; msg = std::string("halton tables: ") + hipGetErrorString(e); break;
        }
    } while (0);
    if (status != RT_OK) {
        delete c;
        return fail(nullptr, status, msg);
    }
    finish_scene(c);
    *out_ctx = c;
    return RT_OK;
}

int rt_destroy(rt_ctx* c) {
    if (!c) return RT_OK;
    DeviceGuard g(c->device);  // ~rt_ctx and the members' destructors run inside it
    delete c;
    return RT_OK;
}

int rt_update_scene(rt_ctx* c, const rt_scene_desc* d, uint32_t flags) {
    static_assert(sizeof(rt_update_stats) == 32, "rt_update_stats layout");
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    if (!d) return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: scene is null");
    if (!d->camera) return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: camera is null");
    if (!d->square_lights || d->n_square_lights < 1)
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: square_lights[0] is required");
    if (flags & ~(uint32_t)RT_UPDATE_REBUILD) return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: unknown bits in flags");
    if (d->n_triangles != c->scene.tri_isect.size())
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: n_triangles differs from the context's (" +
                                               std::to_string(c->scene.tri_isect.size()) + ")");
    if (d->n_spheres != c->scene.sph_shade.size())
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: n_spheres differs from the context's (" +
                                               std::to_string(c->scene.sph_shade.size()) + ")");
    if (d->camera->resolution.x != c->scene.cam.W || d->camera->resolution.y != c->scene.cam.H)
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: camera resolution differs from the context's");
    if (d->device != c->device) return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: device differs from the context's");
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); };
    const auto t_all = clk::now();
    rt::CompiledScene next;
    const char* err = nullptr;
    if (!compile_desc(d, c->build_opt, &next, &err))
        return fail(c, RT_ERR_INVALID_ARG, std::string("rt_update_scene: ") + err);
    if (next.tri_isect.size() != c->scene.tri_isect.size() || next.sph_shade.size() != c->scene.sph_shade.size())
        return fail(c, RT_ERR_INVALID_ARG, "rt_update_scene: the compiled scene changed its primitive counts");
    rt_update_stats st{};
    st.compile_ms = ms_since(t_all);

    // From here on the device arrays change: a failure leaves the context marked.
    DeviceGuard g(c->device);
    auto broken = [&](int status, const std::string& what) {
        c->broken = "the context holds a half-updated scene (" + what + "): rt_update_scene must succeed first";
        return fail(c, status, "rt_update_scene: " + what);
    };
    hipError_t e;
    if (c->tiles_pending) (void)hipEventSynchronize(c->ev_tiles);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return broken(RT_ERR_LAUNCH, std::string("stream: ") + hipGetErrorString(e));
    if (!c->ev_u0.h && ((e = hipEventCreate(&c->ev_u0.h)) != hipSuccess || (e = hipEventCreate(&c->ev_u1.h)) != hipSuccess))
        return broken(RT_ERR_OUT_OF_MEMORY, std::string("hipEventCreate: ") + hipGetErrorString(e));
    c->broken = "rt_update_scene in progress";
    c->sum_valid = false;
    c->scene = std::move(next);
    ++c->scene_epoch;  // the per-wave masks of the old tables no longer hold (ensure_wave_masks)
    const auto t_up = clk::now();
    if ((e = upload_scene(c)) != hipSuccess) return broken(RT_ERR_OUT_OF_MEMORY, std::string("scene upload: ") + hipGetErrorString(e));
    st.upload_ms = ms_since(t_up);

    const bool need = needs_tri_bvh(c), have = c->tri_bvh_build_used && c->d_tri_nodes;
    const auto t_bvh = clk::now();
    if (need && have && !(flags & RT_UPDATE_REBUILD)) {  // refit (rt_refit.hip)
        uint32_t* table = c->d_refit.as<uint32_t>();  // null: the first refit of this tree allocates it
        bool table_made = false;
        e = rt::refit_tri_bvh(c->d_scene[kTriIsect].as<float4>(), (uint32_t)c->scene.tri_isect.size(), c->scene.margin,
                              c->d_tri_nodes.as<uint4>(), c->tri_bvh_nodes, c->d_tri_sorted.as<float4>(),
                              c->d_tri_perm.as<uint32_t>(), &table, &table_made, c->ev_u0, c->ev_u1, c->stream);
        if (table_made) c->d_refit.adopt(table, rt::tri_refit_table_bytes(c->tri_bvh_nodes));  // whatever e says
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the one wait of the update's device work
        if (e != hipSuccess)
            return broken(e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_LAUNCH,
                          std::string("triangle BVH refit: ") + hipGetErrorString(e));
        uint32_t bad = 0;
        if (table_made && ((e = rt::refit_format_errors(table, c->tri_bvh_nodes, &bad)) != hipSuccess || bad))
            return broken(RT_ERR_LAUNCH, "triangle BVH refit: the tree is outside the format of its builders");
        if ((e = hipEventElapsedTime(&st.tri_bvh_ms, c->ev_u0, c->ev_u1)) != hipSuccess)
            return broken(RT_ERR_LAUNCH, std::string("hipEventElapsedTime: ") + hipGetErrorString(e));
        st.tri_bvh = 1;
    } else if (need) {  // as rt_create: the context's builder
        std::string msg;
        const int status = build_tri_bvh(c, &msg);
        if (status != RT_OK) return broken(status == RT_ERR_INVALID_ARG ? RT_ERR_LAUNCH : status, msg);
        st.tri_bvh_ms = ms_since(t_bvh);
        st.tri_bvh = 2;
        c->scene_compile_ms = st.compile_ms;
    } else {
        free_tri_bvh(c);
    }
    finish_scene(c);
    c->broken.clear();
    st.updates = c->update.updates + 1;
    st.total_ms = ms_since(t_all);
    c->update = st;
    c->updated = true;
    return RT_OK;
}

int rt_update_info(const rt_ctx* c, rt_update_stats* info) {
    if (!c || !info) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (!c->updated)
        return fail(const_cast<rt_ctx*>(c), RT_ERR_STATE, "rt_update_info: no successful rt_update_scene on this context yet");
    *info = c->update;
    return RT_OK;
}

int rt_set_seeds(rt_ctx* c, const uint32_t* seeds, int32_t width, int32_t height) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    if (!seeds) return fail(c, RT_ERR_INVALID_ARG, "seeds is null");
    if (width != c->scene.cam.W || height != c->scene.cam.H)
        return fail(c, RT_ERR_INVALID_ARG, "seed texture size must equal the camera resolution");
    DeviceGuard g(c->device);
    const size_t bytes = (size_t)width * (size_t)height * sizeof(uint32_t);
    hipError_t e = hipMemcpyAsync(c->d_seeds.as<void>(), seeds, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "seed upload", e);
    uint32_t mx = 0;
    for (size_t k = 0, n = (size_t)width * (size_t)height; k < n; ++k) mx = seeds[k] > mx ? seeds[k] : mx;
    c->seed_max = mx;
    c->seeds_ready = true;
    return RT_OK;
}

int rt_fill_seeds(rt_ctx* c, uint64_t key) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    const uint64_t n = (uint64_t)c->scene.cam.W * (uint64_t)c->scene.cam.H;
    hipError_t e = rt::launch_fill_seeds(c->d_seeds.as<uint32_t>(), key, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "fill_seeds", e);
    c->seed_max = 0xFFFFFu;  // splitmix64(.) mod 2^20
    c->seeds_ready = true;
    return RT_OK;
}

int rt_render(rt_ctx* c, const rt_render_params* p, void* out) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    const bool dev = p && (p->flags & RT_OUT_DEVICE);
    return render_impl(c, p, out, dev, c->stream, true);
}

int rt_render_async(rt_ctx* c, const rt_render_params* p, void* out_device, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return render_impl(c, p, out_device, true, (hipStream_t)hip_stream, false);
}

int rt_render_mis(rt_ctx* ctx, const rt_mis_params* params, float* out_rgba32f, uint8_t* out_rgba8) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(ctx->device);
    return render_mis_impl(ctx, params, out_rgba32f, out_rgba8);
}

int rt_trace_rays(rt_ctx* c, const rt_ray* rays, uint64_t n, uint32_t flags, rt_ray_hit* hits) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return trace_rays_impl(c, rays, n, flags, hits, (flags & RT_OUT_DEVICE) != 0, c->stream, true);
}

int rt_trace_rays_async(rt_ctx* c, const rt_ray* rays_dev, uint64_t n, uint32_t flags, rt_ray_hit* hits_dev,
                        void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return trace_rays_impl(c, rays_dev, n, flags, hits_dev, true, (hipStream_t)hip_stream, false);
}

int rt_trace_paths(rt_ctx* c, const rt_path_params* p, const rt_ray* rays, const uint32_t* seeds, uint64_t n,
                   float* radiance, rt_ray_hit* first_hits) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return trace_paths_impl(c, p, rays, seeds, n, radiance, first_hits, p && (p->flags & RT_OUT_DEVICE), c->stream,
                            true);
}

int rt_trace_paths_async(rt_ctx* c, const rt_path_params* p, const rt_ray* rays_dev, const uint32_t* seeds_dev,
                         uint64_t n, float* radiance_dev, rt_ray_hit* first_hits_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return trace_paths_impl(c, p, rays_dev, seeds_dev, n, radiance_dev, first_hits_dev, true, (hipStream_t)hip_stream,
                            false);
}

int rt_render_aov(rt_ctx* c, const rt_aov_params* p, const rt_aov_buffers* b) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return render_aov_impl(c, p, b, p && (p->flags & RT_OUT_DEVICE), c->stream, true);
}

int rt_render_aov_async(rt_ctx* c, const rt_aov_params* p, const rt_aov_buffers* b_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return render_aov_impl(c, p, b_dev, true, (hipStream_t)hip_stream, false);
}

int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_buffers* b) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return denoise_impl(c, p, b, p && (p->flags & RT_OUT_DEVICE), c->stream, true);
}

int rt_denoise_async(rt_ctx* c, const rt_denoise_params* p, const rt_denoise_buffers* b_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return denoise_impl(c, p, b_dev, true, (hipStream_t)hip_stream, false);
}

int rt_reproject(rt_ctx* c, const rt_reproject_params* p, const CameraGPU* prev_camera,
                 const rt_reproject_buffers* b) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return reproject_impl(c, p, prev_camera, b, p && (p->flags & RT_OUT_DEVICE), c->stream, true);
}

int rt_reproject_async(rt_ctx* c, const rt_reproject_params* p, const CameraGPU* prev_camera,
                       const rt_reproject_buffers* b_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return reproject_impl(c, p, prev_camera, b_dev, true, (hipStream_t)hip_stream, false);
}

int rt_render_counts(rt_ctx* c, const rt_render_params* p, const uint32_t* counts, void* out, uint32_t* totals) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    const CountsArgs ca{counts, totals};
    return render_impl(c, p, out, p && (p->flags & RT_OUT_DEVICE), c->stream, true, &ca);
}

int rt_render_counts_async(rt_ctx* c, const rt_render_params* p, const uint32_t* counts_dev, void* out_dev,
                           uint32_t* totals_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    const CountsArgs ca{counts_dev, totals_dev};
    return render_impl(c, p, out_dev, true, (hipStream_t)hip_stream, false, &ca);
}

int rt_plan_samples(rt_ctx* c, const rt_plan_params* p, const float* first, const float* all, uint32_t* counts,
                    rt_plan_stats* stats) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return plan_impl(c, p, first, all, counts, stats, p && (p->flags & RT_OUT_DEVICE), c->stream, true);
}

int rt_plan_samples_async(rt_ctx* c, const rt_plan_params* p, const float* first_dev, const float* all_dev,
                          uint32_t* counts_dev, rt_plan_stats* stats_dev, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    return plan_impl(c, p, first_dev, all_dev, counts_dev, stats_dev, true, (hipStream_t)hip_stream, false);
}

int rt_last_kernel_ms(rt_ctx* c, float* ms) {
    if (!c || !ms) return fail(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->timed) return fail(c, RT_ERR_STATE, "no render or ray query yet");
    DeviceGuard g(c->device);
    hipError_t e = hipEventSynchronize(c->ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, c->ev0, c->ev1);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "hipEventElapsedTime", e);
    return RT_OK;
}

int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]) {
    if (!id) return fail(nullptr, RT_ERR_INVALID_ARG, "id is null");
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return nccl_fail(nullptr, "ncclGetUniqueId", r);
    memcpy(id, &u, sizeof(u));
    return RT_OK;
}

int rt_comm_init(rt_ctx* c, int32_t rank, int32_t world, const uint8_t id[RT_COMM_ID_BYTES]) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    if (!id) return fail(c, RT_ERR_INVALID_ARG, "id is null");
    if (world < 1 || rank < 0 || rank >= world)
        return fail(c, RT_ERR_INVALID_ARG, "need 0 <= rank < world");
    if (c->comm) return fail(c, RT_ERR_STATE, "context already has a communicator");
    DeviceGuard g(c->device);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, world, u, rank);
    if (r != ncclSuccess) return nccl_fail(c, "ncclCommInitRank", r);
    c->comm = comm;
    c->rank = rank;
    c->world = world;
    return RT_OK;
}

int rt_render_gather(rt_ctx* c, const rt_render_params* p, void* frame, void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    DeviceGuard g(c->device);
    // NULL is the HIP null stream (rt_render_async's convention): a caller on
    // the default stream (torch's current stream is handle 0) gets its work
    // ordered after everything it enqueued there
    hipStream_t s = (hipStream_t)hip_stream;
    return render_gather_impl(c, p, frame, s);
}

int rt_comm_info(const rt_ctx* c, int32_t* count, int32_t* rank) {
    if (!c || !count || !rank) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    rt_ctx* m = const_cast<rt_ctx*>(c);  // the error message slot only
    if (!c->comm) return fail(m, RT_ERR_STATE, "rt_comm_info: no communicator (rt_comm_init first)");
    int n = 0, r = 0;
    ncclResult_t res = ncclCommCount(c->comm, &n);
    if (res != ncclSuccess) return nccl_fail(m, "ncclCommCount", res);
    res = ncclCommUserRank(c->comm, &r);
    if (res != ncclSuccess) return nccl_fail(m, "ncclCommUserRank", res);
    *count = n;
    *rank = r;
    return RT_OK;
}

int rt_place_tiles(rt_ctx* c, const void* gathered_device, int32_t world, uint32_t flags, void* frame,
                   void* hip_stream) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    if (!gathered_device || !frame || world < 1) return fail(c, RT_ERR_INVALID_ARG, "null buffer or world < 1");
    if (const int st = check_out_format(c, flags)) return st;
    DeviceGuard g(c->device);
    // NULL is the HIP null stream (rt_render_async's convention): a caller on
    // the default stream (torch's current stream is handle 0) gets its work
    // ordered after everything it enqueued there
    hipStream_t s = (hipStream_t)hip_stream;
    return place_tiles_impl(c, gathered_device, (uint32_t)world, flags, frame, s);
}

int rt_build_info(const rt_ctx* c, rt_build_stats* info) {
    if (!c || !info) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    memset(info, 0, sizeof(*info));
    info->tri_bvh_build = c->tri_bvh_build_used;
    info->tri_bvh_nodes = c->tri_bvh_nodes;
    info->tri_bvh_build_ms = c->tri_bvh_build_ms;
    info->scene_compile_ms = c->scene_compile_ms;
    info->tri_bvh_temp_kib = (uint32_t)((c->tri_bvh_temp_bytes + 1023) / 1024);
    return RT_OK;
}

int rt_debug_tri_bvh(const rt_ctx* c, rt_tri_bvh_dump* dump) {
    if (!c || !dump) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (!c->broken.empty()) return fail(const_cast<rt_ctx*>(c), RT_ERR_STATE, c->broken);
    if (!c->tri_bvh_build_used || !c->d_tri_nodes) return RT_ERR_STATE;
    const size_t nT = c->scene.tri_isect.size(), nn = c->tri_bvh_nodes;
    dump->n_triangles = (uint32_t)nT;
    dump->nodes_per_layout = (uint32_t)nn;
    dump->leaf_max = c->tri_leaf_max;
    dump->margin = c->scene.margin;
    DeviceGuard g(c->device);
    const struct { void* dst; const DevBuf& src; size_t bytes; } copies[4] = {
        {dump->nodes, c->d_tri_nodes, rt::kTriCompactLayouts * nn * sizeof(uint4)},
        {dump->sorted, c->d_tri_sorted, nT * sizeof(rt::TriIsect)},
        {dump->perm, c->d_tri_perm, nT * sizeof(uint32_t)},
        {dump->isect, c->d_scene[kTriIsect], nT * sizeof(rt::TriIsect)}};
    for (const auto& cp : copies) {
        if (!cp.dst) continue;
        const hipError_t e = hipMemcpy(cp.dst, cp.src.as<void>(), cp.bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return RT_ERR_LAUNCH;
    }
    return RT_OK;
}

int rt_debug_halton_table_device(const rt_ctx* c, float* table, uint32_t capacity) {
    if (!c || !table) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (capacity < rt::kHaltonTabLdsFloats)
        return fail(const_cast<rt_ctx*>(c), RT_ERR_INVALID_ARG, "rt_debug_halton_table_device: capacity below the table's size");
    if (!c->d_halton_tab) return RT_ERR_STATE;
    DeviceGuard g(c->device);
    const hipError_t e =
        hipMemcpy(table, c->d_halton_tab.as<void>(), sizeof(float) * rt::kHaltonTabLdsFloats, hipMemcpyDeviceToHost);
    return e == hipSuccess ? RT_OK : RT_ERR_LAUNCH;
}

int rt_debug_wave_masks(rt_ctx* c, const rt_render_params* p, uint32_t lanes, rt_wave_mask* masks, uint32_t capacity,
                        uint32_t* waves_x, uint32_t* waves_y, uint64_t* fills) {
    static_assert(sizeof(rt_wave_mask) == 32 && sizeof(rt::WaveMask) == 16, "rt_wave_mask / WaveMask layout");
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "ctx is null");
    if (!p || !waves_x || !waves_y || (!masks && capacity))
        return fail(c, RT_ERR_INVALID_ARG, "rt_debug_wave_masks: null argument");
    if (lanes != 0 && lanes != 1 && lanes != 4 && lanes != 16)
        return fail(c, RT_ERR_INVALID_ARG, "rt_debug_wave_masks: lanes_per_pixel must be 0, 1, 4 or 16");
    if (!c->broken.empty()) return fail(c, RT_ERR_STATE, c->broken);
    if (p->bounces > RT_MAX_BOUNCES) return fail(c, RT_ERR_INVALID_ARG, "bounces > 4");
    uint32_t start, step, count;
    if (!resolve_rows(c, p->row_start, p->row_step, p->row_count, &start, &step, &count))
        return fail(c, RT_ERR_INVALID_ARG, "row partition outside the frame");
    DeviceGuard g(c->device);
    rt::KParams K;
    set_scene(&K, c);
    set_launch(&K, c, p, start, step, count);
    K.max_index = halton_max_index(c, p->sample_base, p->spp);
    *waves_x = *waves_y = 0;
    if (fills) *fills = c->mask_fills;
    rt::WaveGrid wg{};
    if (!rt::wave_mask_grid(K, p->bounces, c->scene_mem, lanes, &wg)) return RT_OK;
    int st;
    if ((st = ensure_wave_masks(c, &K, wg, c->stream)) != RT_OK) return st;
    if (fills) *fills = c->mask_fills;
    const uint32_t n = wg.waves_x * wg.waves_y;
    std::vector<rt::WaveMask> host(n);
    hipError_t e = hipMemcpyAsync(host.data(), c->d_wave_masks.as<void>(), (size_t)n * sizeof(rt::WaveMask),
                                  hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "rt_debug_wave_masks: read-back", e);
    *waves_x = wg.waves_x;
    *waves_y = wg.waves_y;
    wave_rects(wg, start, step, masks, capacity);
    for (uint32_t w = 0; w < n && w < capacity; ++w) {
        masks[w].cam_mask = host[w].cam_mask;
        masks[w].shd_mask = host[w].shd_mask;
        masks[w].shd_cskip = host[w].shd_cskip;
        masks[w].shd_available = host[w].shd_avail;
    }
    return RT_OK;
}

int rt_last_launch(const rt_ctx* c, rt_launch_info* info) {
    if (!c || !info) return fail(nullptr, RT_ERR_INVALID_ARG, "null argument");
    if (!c->launched) return RT_ERR_STATE;
    memset(info, 0, sizeof(*info));
    static_assert(sizeof(info->kernel) == sizeof(c->launch.kernel), "kernel name buffer");
    memcpy(info->kernel, c->launch.kernel, sizeof(info->kernel));
    info->kernel[sizeof(info->kernel) - 1] = 0;
    info->lanes_per_pixel = c->launch.lanes;
    info->halton_tables = c->launch.tables;
    info->small_index = c->launch.small;
    info->block_threads = c->launch.threads;
    info->grid_x = c->launch.grid_x;
    info->grid_y = c->launch.grid_y;
    info->lds_bytes = c->launch.lds;
    return RT_OK;
}

int rt_debug_stats(rt_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n <= 0) return fail(c, RT_ERR_INVALID_ARG, "null argument");
    DeviceGuard g(c->device);
    hipError_t e = rt::read_debug_stats(reinterpret_cast<unsigned long long*>(out), n);
    if (e == hipErrorNotSupported) return fail(c, RT_ERR_STATE, "not an RT_STATS build");
    if (e != hipSuccess) return hip_fail(c, RT_ERR_LAUNCH, "read stats", e);
    return RT_OK;
}

#ifndef RT_SRC_SHA
#define RT_SRC_SHA "unknown"
#endif
const char* rt_build_sha(void) { return RT_SRC_SHA; }

}  // extern "C"
