// rt_kernel.hpp — launch interface of the gfx950 path-tracing kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "rt_math.h"
#include "rt_raydomain.h"

namespace rt {

constexpr uint32_t kBlockThreads = 256;  // 4 waves; each wave = 8x8 pixel tile
constexpr uint32_t kTile = 16;           // workgroup = 16x16 pixels
constexpr size_t kMaxLdsBytes = 64 * 1024;
constexpr uint32_t kOutFp16 = 0x2u;
constexpr uint32_t kOutRgba8 = 0x10u;  // fused image.swift:35-65 epilogue, uchar4 store
constexpr uint32_t kPairF4 = 7;  // float4 per pair record: 5 geometry + 2 padded AABB
// The sphere kernel (kGeoSphLds): one-wave workgroups that stage only the
// pair records in LDS and walk the compact sphere BVH (8 octant layouts) from
// global memory (L2-resident).  A workgroup keeps its wave slots until its
// slowest wave ends and sphere walks make wave times differ a lot (config 4:
// 1024 threads 186.1 ms, 512 177.9, 256 162.1, 128 160.5, 64 158.4).  Every
// workgroup stages its own copy of the pair records, so the kernel is taken
// only while they are small (kSphPairLdsMaxBytes; config 4: 672 B): above it
// the pair kernel with the 32-B-node sphere walks serves the scene.  Measured
// on Cornell + 1000 spheres + extra quads, 1080p x 64 spp (tools/bench_mixed.py,
// one-wave vs pair kernel): 37 pairs 47.9 vs 66.7 ms, 48 pairs 59.5 vs 69.4,
// 58 pairs 71.8 vs 71.7, 68 pairs 84.8 vs 73.0: the crossover is ~6.5 KB.
constexpr uint32_t kSphBlockThreads = 64;
constexpr size_t kSphPairLdsMaxBytes = 6 * 1024;
constexpr uint32_t kCluF4 = 7;   // float4 per box cluster (rt_scene.hpp CompiledScene::clusters)
// The box-cluster kernel's bounce-0 closest query tests only the pairs its
// wave's camera rays can hit: one candidate mask per wave, computed in the
// kernel prologue (rt_beam.hpp); 0: cluster_query as for
// every other ray
#ifndef RT_CAM_CAND
#define RT_CAM_CAND 1
#endif
// Its bounce-0 shadow query tests only the pairs that can occlude a segment
// from the wave's camera-ray hit points to the light patch: one occluder mask
// per wave from the same prologue (rt_shaft.hpp; needs
// RT_CAM_CAND); 0: cluster_query as for every other shadow ray
#ifndef RT_SHD_CAND
#define RT_SHD_CAND 1
#endif
// An occluder mask of at most this many pairs is tested directly, pair by pair
// on every lit lane, without the cluster filter (needs
// RT_SHD_CAND); 0: every non-empty mask goes through the filter.  Measured at
// 1, 2 and 3 (profiles/r19/ab_results.md): 3 covers 99.8 % of the decided
// non-empty masks of the 1080p Cornell frame and ran fastest
#ifndef RT_SHD_SHORT
#define RT_SHD_SHORT 3
#endif
// A wave whose camera mask is empty skips the sample loop: its pixels' sums
// get +0 once (needs RT_CAM_CAND); 0: the loop runs
#ifndef RT_DEAD_SKIP
#define RT_DEAD_SKIP 1
#endif
// Its closest queries of bounce >= 1 test each lane's entry-side candidates
// first and the exit-side ones only where they can still win against the hit
// found (rt_cluorder.hpp); 0: one candidate mask per lane in
// bit order
#ifndef RT_CLU_ORDER
#define RT_CLU_ORDER 1
#endif
// The cluster filter takes a leaner wave-uniform path for the kinds the scene
// compiler marks in the record's flag word (rt_cluorder.hpp kCluTurned,
// kCluInside, kCluOwnLight): a box turned about one world
// axis forms its two oblique products from two components, a container every
// lane starts inside gives its exit side alone, and a shade() shadow query
// passes over the light's own cluster; 0: the one filter for every cluster
#ifndef RT_CLU_LEAN
#define RT_CLU_LEAN 1
#endif
// Layouts of the triangle BVH (rt_scene.cpp build_tri_sah / rt_lbvh.hip,
// rt_trace.hpp tri_cbvh_*): one per direction octant, 16 B per node.
constexpr uint32_t kTriCompactLayouts = 8;
// Above this many triangles rt_create builds the triangle BVH (measured crossover
// of the LDS brute-force layouts and the BVH walks on random triangles: ~300).
constexpr uint32_t kTriBvhMinTriangles = 384;

// The scene's device tables and counts, the same for every kernel of a
// context: what the kernels build their SceneView from (rt_trace.hpp
// tables_of, stage_records, bind_scene).
struct SceneTables {
    const float4* tri_isect;   // 3 float4 per triangle (TriIsect)
    const float4* pair_isect;  // kPairF4 float4 per shared-edge triangle pair (PairIsect), or null
    const float4* clusters;    // box clusters, kCluF4 float4 each, or null
    const float4* sph_isect;   // 1 float4 per sphere, BVH leaf order (SphIsect)
    const float4* sph_nodes;   // 2 float4 per sphere-BVH node (BvhNode)
    const uint32_t* sph_perm;  // BVH leaf order -> sphere id
    const uint4* sph_box;      // the same BVH with leaf boxes: 8 layouts x nN entries, or null
    const uint4* tri_nodes;    // triangle BVH: 8 compact layouts x nTN nodes, or null
    const float4* tri_sorted;  // 3 float4 per triangle, BVH leaf order
    const uint32_t* tri_perm;  // BVH leaf order -> triangle id
    uint32_t nT, nP, nS, nN;   // triangles, triangle pairs (0: no pair layout), spheres, sphere-BVH nodes
    uint32_t nTN;              // triangle-BVH nodes per layout (0: no triangle BVH)
    uint32_t nC;               // box clusters (0: none)
    uint32_t pair_free;        // pairs in no cluster (bit mask)
};
// Kernel arguments (passed by value -> kernarg segment / SGPRs).  The scene
// tables stay flat members here (tables_of, rt_trace.hpp, gathers them): with
// them moved into one SceneTables member the spills and loop bodies of the
// path kernels changed (profiles/r13/isa.md), unlike MisParams and
// RayQueryParams, which embed the block.
struct KParams {
    const float4* tri_isect;  // 3 float4 per triangle (TriIsect)
    const float4* pair_isect; // kPairF4 float4 per shared-edge triangle pair (PairIsect) or null
    const float4* tri_shade;  // 4 float4 per triangle (TriShade)
    const float4* sph_isect;  // 1 float4 per sphere, BVH leaf order (SphIsect)
    const float4* sph_nodes;  // 2 float4 per sphere-BVH node (BvhNode)
    const uint32_t* sph_perm; // BVH leaf order -> sphere id
    const float4* sph_shade;  // 3 float4 per sphere, by id (SphShade)
    const uint32_t* sph_lds;  // compact sphere BVH (8 layouts x nE x 16 B), or null
    const uint16_t* sph_lds_id;  // sphere id per compact entry
    const uint4* sph_box;     // the same BVH with leaf boxes: 8 layouts x nN entries, or null
    const uint4* tri_nodes;   // triangle BVH: 8 compact layouts x nTN nodes, or null
    const float4* tri_sorted; // 3 float4 per triangle, BVH leaf order
    const uint32_t* tri_perm; // BVH leaf order -> triangle id
    const uint32_t* seeds;    // W*H, full frame
    float4* sum;              // running sums (tile layout) or null
    void* out;                // rgba32F / rgba16F tile or null
    uint32_t nT, nP, nS, nN;  // triangles, triangle pairs (0: no pair layout), spheres, BVH nodes
    uint32_t nE;              // entries per layout of the compact sphere BVH
    uint32_t nTN;             // triangle-BVH nodes per layout (0: no triangle BVH)
    float cam_pos[3], cam_u[3], cam_v[3], cam_w[3];
    float halfW, halfH;
    int32_t W, H;
    float light_center[3], light_color[3];
    uint32_t spp, sample_base;
    uint32_t row_start, row_step, row_count;
    uint32_t accumulate;      // read P.sum before adding
    uint32_t samples_total;   // S of `luminance /= samples`
    uint32_t flags;
    uint32_t max_index;       // max Halton index seed+n of this launch (0xFFFFFFFF: unknown/wraps)
    uint32_t lanes;           // lanes per pixel: 0 = auto, else 1, 4 or 16 (rt_create_options)
    uint32_t walk;            // rt_walk_scheduler: 0 auto, 1 lockstep, 2 free-running lanes, 3 sorted
    uint32_t wave_w;          // pixels per wave row (set by the launcher)
    uint32_t walk_leaf_den;   // free-running walks: leaf-round threshold, 0 = default
    uint32_t light_plain;     // light_center.y, .z are not -0 (shade(): q without its zero terms)
    const float4* clusters;   // box clusters, kCluF4 float4 each, or null
    uint32_t nC;              // clusters (0: none)
    uint32_t pair_free;       // pairs in no cluster (bit mask)
    uint64_t light_mask;      // box-cluster kernel: bit id set when triangle id is a light, i.e. its
                              // TriShade s0.w != 0 (ids < 64; rt_scene.hpp light_mask)
    const float* halton_tab;  // box-cluster kernel: the context's Halton low-digit tables, kHaltonTabLdsFloats
                              // floats (launch_fill_halton_tables), copied into LDS when halton_tables_on
    const uint4* wave_masks;  // box-cluster render kernel, 1..32 pairs: one WaveMask per wave of this launch's
                              // geometry in wave row-major order (launch_wave_masks)
};

// ---- per-wave candidate masks (rt_kernel.hip wave_masks_kernel)
// What the box-cluster render kernel knows about one wave before its first
// sample, 16 B that the wave reads with one scalar load: the pairs its camera
// rays can hit (rt_beam.hpp), the pairs that can occlude its bounce-0 shadow
// rays (rt_shaft.hpp), the box clusters none of whose faces is among those, and
// whether the occluder mask is decided.
struct WaveMask {
    uint32_t cam_mask, shd_mask, shd_cskip, shd_avail;
};
static_assert(sizeof(WaveMask) == sizeof(uint4), "one dwordx4 load per wave");
// The occluder mask of a wave with SEVERAL camera pairs is the union over all of
// them; 0: decided only for one camera pair, as the render kernel's own
// prologue did before the table (the A/B switch of profiles/r22/ab_results.md)
#ifndef RT_WAVE_MASK_MULTI
#define RT_WAVE_MASK_MULTI 1
#endif
// THE wave geometry of a lockstep launch at L lanes per pixel over W columns and
// row_count rows of the row partition: a wave is wave_w x wave_h pixels (8x8 at
// L = 1; L > 1: 4x4 / 2x2 for whole frames, one row of 64/L pixels when the rows
// are interleaved), a workgroup WR x WC waves, and the grid rounds up to whole
// workgroups: waves_x x waves_y waves, some of them past the frame's edge.
// Wave (wx, wy) covers columns wx * wave_w .. + wave_w - 1 and partition rows
// wy * wave_h .. + wave_h - 1.  launch_tl and the mask table share this one
// definition.
struct WaveGrid {
    uint32_t L, wave_w, wave_h, grid_x, grid_y, waves_x, waves_y;
};
constexpr WaveGrid wave_grid(uint32_t W, uint32_t row_count, uint32_t row_step, uint32_t L, uint32_t WR,
                             uint32_t WC) {
    const uint32_t ww = L == 1 ? 8u : (row_step > 1 ? 64u / L : (L == 4 ? 4u : 2u));
    const uint32_t wh = (64u / L) / ww;
    const uint32_t gx = (W + WR * ww - 1) / (WR * ww), gy = (row_count + WC * wh - 1) / (WC * wh);
    return WaveGrid{L, ww, wh, gx, gy, gx * WR, gy * WC};
}
// The box-cluster kernel's workgroup: 2 x 2 waves (rt_kernel.hip block_threads).
constexpr WaveGrid clu_wave_grid(uint32_t W, uint32_t row_count, uint32_t row_step, uint32_t L) {
    return wave_grid(W, row_count, row_step, L, 2u, 2u);
}

size_t kernel_lds_bytes(uint32_t n_tri, uint32_t n_pairs, uint32_t n_sph, uint32_t n_nodes);

// Kernel layouts the launcher chooses between (0-7 = rt_trace.hpp enum Geo).
enum KernelLayout : int {
    kLayTriLds = 0,      // single-triangle records in LDS
    kLayPairLds = 1,     // shared-edge pair records in LDS
    kLayTriGlobal = 2,   // single-triangle records from global memory
    kLayPairSorted = 3,  // pair records + per-bounce octant sort of the paths
    kLayPairSmem = 4,    // pair records by scalar loads
    kLayTriBvh = 5,      // triangle BVH from global memory
    kLayPairClu = 6,     // pair records + box clusters + Halton tables in LDS (Cornell)
    kLaySphLds = 7,      // pair records in LDS, compact sphere BVH in L2 (config 4)
    kLayFreeSph = 8,     // free-running lanes, sphere scene (rt_free.hpp)
    kLayFreeTri = 9,     // free-running lanes, triangle BVH
    kLaySortSph = 10,    // octant-sorted paths, sphere scene
    kLaySortTri = 11,    // octant-sorted paths, triangle BVH
};
// THE LDS order of every layout: the float4 count of the
// records a workgroup of layout `lay` stages (pair records, or triangle records
// for kLayTriLds; 0: the records stay in global memory) and of the box clusters
// right after them (kLayPairClu).  What a kernel adds of its own -- Halton
// tables, MIS shading records and stash -- follows; the sorted kernels' path
// buffers come first.  Every LDS size below and every kernel's offsets
// (rt_trace.hpp stage_records, bind_scene) are these two terms.
// N: uint32_t in the kernels (LDS offsets), size_t where the host decides
// whether a scene fits at all.
template <typename N>
struct StagedF4 {
    N rec, clu;
};
template <typename N = uint32_t>
__host__ __device__ __forceinline__ constexpr StagedF4<N> staged_f4(int lay, N nT, N nP, N nC) {
    return StagedF4<N>{lay == kLayTriLds ? 3u * nT
                       : (lay == kLayPairLds || lay == kLayPairClu || lay == kLaySphLds || lay == kLayFreeSph ||
                          lay == kLayPairSorted || lay == kLaySortSph)
                           ? kPairF4 * nP
                           : N(0),  // TriGlobal, PairSmem, TriBvh, FreeTri, SortTri
                       lay == kLayPairClu ? kCluF4 * nC : N(0)};
}
// LDS of the Halton low-digit tables (rt_halton.hpp kHaltonTabFloats) and of
// the sorted kernel's path buffers (rt_kernel.hip kSortF4), static-asserted
// against their definitions.
constexpr uint32_t kHaltonTabLdsFloats = 4679;
constexpr uint32_t kSortLdsF4 = 1097;
// THE dynamic LDS of a workgroup of layout `lay`: the bytes its staging writes
// (staged_f4, then the Halton tables; the sorted kernels' path buffers first).
// The launcher requests exactly this and the kernels place their staged arrays
// by the same terms; an -DRT_LDS_CHECK build also checks it against the
// dispatch's LDS allocation.
__host__ __device__ constexpr size_t staged_lds_bytes(int lay, uint32_t nT, uint32_t nP, uint32_t nC) {
    const StagedF4<size_t> n = staged_f4<size_t>(lay, nT, nP, nC);
    return 16 * (n.rec + n.clu) + (lay == kLayPairClu ? (size_t)4 * kHaltonTabLdsFloats : (size_t)0) +
           ((lay == kLayPairSorted || lay == kLaySortSph || lay == kLaySortTri) ? (size_t)16 * kSortLdsF4 : (size_t)0);
}
constexpr uint32_t kHaltonTabMinRounds = 8;  // samples per lane below which no tables
// Whether a launch fills the LDS low-digit Halton tables: box-cluster kernel,
// fixed-digit indices, and every lane tracing enough samples to amortise the
// fill (~700 VALU per thread): config 1 (1 spp) runs without them.  The kernels
// (render and AOV) and the launchers' rt_last_launch reports share this one
// definition.
__host__ __device__ constexpr bool halton_tables_on(int geo, bool small, uint32_t spp, uint32_t L) {
    return geo == kLayPairClu && small && (spp + L - 1) / L >= kHaltonTabMinRounds;
}
// The kernel layout a launch takes and its dynamic LDS (launch_path_trace and
// rt_scene_describe_ex both ask this one function).  t: the scene's counts (its
// pointers are not read), sph_compact: every table of the compact
// sphere kernel exists (rt_scene.hpp sphere_compact_usable; the launcher reads
// it from P.sph_lds, which rt_api.cpp sets by that predicate).
struct KernelChoice {
    int layout;
    size_t lds_bytes;
};
// What launch_path_trace launched (rt_last_launch, include/rtpt.h).
struct LaunchInfo {
    char kernel[96];
    uint32_t lanes, tables, small, threads, grid_x, grid_y, lds;
};
// THE way a launcher fills one: the kernel's name as rt_last_launch returns it
// (printf-style, last), then the fields in the order of the record.
__attribute__((format(printf, 8, 9))) inline void fill_launch_info(LaunchInfo& I, uint32_t lanes, bool tables,
                                                                   bool small, uint32_t threads, dim3 grid, size_t lds,
                                                                   const char* name_fmt, ...) {
    va_list ap;
    va_start(ap, name_fmt);
    vsnprintf(I.kernel, sizeof(I.kernel), name_fmt, ap);
    va_end(ap);
    I.lanes = lanes;
    I.tables = tables ? 1u : 0u;
    I.small = small ? 1u : 0u;
    I.threads = threads;
    I.grid_x = grid.x;
    I.grid_y = grid.y;
    I.lds = (uint32_t)lds;
}
// Where the workgroup reads the intersection records from.
// rt_walk_scheduler (include/rtpt.h)
constexpr uint32_t kWalkAuto = 0, kWalkLockstep = 1, kWalkFree = 2, kWalkSorted = 3;
enum class SceneMem { kAuto = 0, kLdsSingle = 1, kSmem = 2, kPairSorted = 3, kPairSmem = 4, kTriBvh = 5, kPairLds = 6 };
hipError_t launch_path_trace(const KParams& P, uint32_t bounces, SceneMem mem, hipStream_t stream,
                             LaunchInfo* info);
KernelChoice choose_kernel(const SceneTables& t, bool sph_compact, uint32_t bounces, SceneMem mem, uint32_t walk);
// Whether launch_path_trace(P, bounces, mem) reads P.wave_masks (the box-cluster
// kernel on a scene of 1..32 pairs), and then *g: the wave geometry it launches
// with, lanes_override = 0, or with that many lanes per pixel instead of P.lanes.
// The masks depend on P's camera, light centre, tables, W, H, row partition and
// on *g, on nothing else of P.
bool wave_mask_grid(const KParams& P, uint32_t bounces, SceneMem mem, uint32_t lanes_override, WaveGrid* g);
// Fills table[wy * g.waves_x + wx] for every wave of g: one launch of
// wave_masks_kernel on `stream`.
hipError_t launch_wave_masks(const KParams& P, const WaveGrid& g, uint4* table, hipStream_t stream);
// The render with one sample count per pixel (rt_counts.hpp; include/rtpt.h
// rt_render_counts): pixel p draws min(counts[p], P.spp) samples after the
// P.sum[p].w samples its sum holds (P.accumulate), `totals` (or null) receives
// the new total.  counts / totals: row_count * W words of device memory in the
// layout of P.out.  P.samples_total and P.lanes are not read; P.max_index
// bounds seed + sample_base + every total.  The layout is ray_query_layout of
// the context's.
hipError_t launch_path_counts(const KParams& P, const uint32_t* counts, uint32_t* totals, uint32_t bounces,
                              SceneMem mem, hipStream_t stream, LaunchInfo* info);
hipError_t read_debug_stats(unsigned long long* out, int n);  // RT_STATS builds only
// -DRT_LDS_CHECK builds: the largest staging end a kernel found past its
// dispatch's dynamic LDS since the last call (0: none; always 0 otherwise).
hipError_t lds_check_result(uint32_t* end);
// Arguments of the MIS integrator kernel (rt_mis.hip; Sources/gpuRaytracer/
// shaders.metal:635-707).
struct MisParams {
    SceneTables tab;           // triangle scenes only: the sphere members are null / 0
    const float4* mis_shade;   // 3 float4 per triangle (MisShade)
    const float4* u_tab;       // 3 float4 per MIS sample index i < S (Halton table)
    float4* out;               // (sum over camera rays, camera_rays) per pixel, or null
    uchar4* out8;              // writeToPixelBuffer RGBA8, or null
    float cam_pos[3], cam_u[3], cam_v[3], cam_w[3];
    float halfW, halfH;
    int32_t W, H;
    float l_center[3], l_tangent[3], l_bitangent[3], l_radiance[3];
    float l_width, l_depth, l_area, exposure;
    uint32_t camera_rays, S;   // S = misSamples / 3 (samples per strategy)
    uint32_t row_start, row_step, row_count;
    float4* part;              // split launches: one float4 per record and pixel, or null (rt_mis.hip SPLIT)
};
// ---- batched ray queries (rt_rays.hip; include/rtpt.h rt_trace_rays) --------
constexpr uint32_t kRaysAny = 0x100u;    // RT_RAYS_ANY
constexpr uint32_t kRaysExact = 0x200u;  // RT_RAYS_EXACT
// A workgroup of kBlockThreads lanes stages its layout's records once and
// traces kRayChunk consecutive rays, 64 consecutive rays per wave and pass
// (RT_RAYS_CHUNK of include/rtpt.h).
constexpr uint32_t kRayChunk = 2048;
// The layout a query takes for the layout choose_kernel gives the context: the
// free and sorted schedulers are render schedulers, a query runs their scenes
// through the lockstep walks; the path-sorting pair kernel has no query form.
constexpr int ray_query_layout(int lay) {
    return (lay == kLayFreeSph || lay == kLaySortSph)   ? (int)kLaySphLds
           : (lay == kLayFreeTri || lay == kLaySortTri) ? (int)kLayTriBvh
           : lay == kLayPairSorted                      ? (int)kLayPairLds
                                                        : lay;
}
// ---- the launchers' dispatch ------------------------------
// A run-time bounce count as a compile-time one: f(integral_constant<int, B>)
// for bounces = B in 0..4, hipErrorInvalidValue for every other count.
template <typename F>
hipError_t dispatch_bounces(uint32_t bounces, F&& f) {
    switch (bounces) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
}
// THE rule of layout and sphere form, for every launcher of a lockstep layout
// (`lay` after ray_query_layout where the context's may be a free or sorted
// one): f(integral_constant<int, GEO>, bool_constant<SPH>).  choose_kernel gives
// the box-cluster layout to triangle-only scenes and the sphere layout to sphere
// scenes only, so these two have one form; every other layout has both, picked
// by the scene's sphere count nS.  Not a lockstep layout: hipErrorInvalidValue.
template <typename F>
hipError_t dispatch_layout(int lay, uint32_t nS, F&& f) {
    auto by_spheres = [&](auto geo) { return nS > 0 ? f(geo, std::true_type{}) : f(geo, std::false_type{}); };
    switch (lay) {
        case kLayTriLds: return by_spheres(std::integral_constant<int, kLayTriLds>{});
        case kLayPairLds: return by_spheres(std::integral_constant<int, kLayPairLds>{});
        case kLayTriGlobal: return by_spheres(std::integral_constant<int, kLayTriGlobal>{});
        case kLayPairSmem: return by_spheres(std::integral_constant<int, kLayPairSmem>{});
        case kLayTriBvh: return by_spheres(std::integral_constant<int, kLayTriBvh>{});
        case kLayPairClu: return f(std::integral_constant<int, kLayPairClu>{}, std::false_type{});
        case kLaySphLds: return f(std::integral_constant<int, kLaySphLds>{}, std::true_type{});
        default: return hipErrorInvalidValue;
    }
}
// THE dynamic LDS of a query workgroup of layout `lay` (after ray_query_layout):
// staged_f4 and nothing else (no Halton tables).  The kernel places its arrays
// by these terms and the launcher requests exactly this.
__host__ __device__ constexpr size_t ray_query_lds_bytes(int lay, uint32_t nT, uint32_t nP, uint32_t nC) {
    const StagedF4<size_t> n = staged_f4<size_t>(lay, nT, nP, nC);
    return 16 * (n.rec + n.clu);
}
struct RayQueryParams {
    SceneTables tab;
    uint32_t sph_compact;      // every table of the sphere kernel exists (as P.sph_lds != null for a render)
    const float4* rays;        // 2 float4 per ray: (origin, tmin) (dir, tmax), device memory
    uint2* hits;               // (t bits, id) per ray, device memory
    uint32_t n;                // rays, <= 2^31
    uint32_t flags;            // kRaysAny | kRaysExact
    RayDomain dom;             // rt_raydomain.h
};
hipError_t launch_ray_query(const RayQueryParams& P, SceneMem mem, hipStream_t stream, LaunchInfo* info);

// ---- path queries (rt_paths.hpp; include/rtpt.h rt_trace_paths) -------------
// What rt_trace_paths adds to KParams (extra kernel arguments of
// path_query_kernel; KParams is not regrouped, see above).  Of P the kernel
// reads the tables, the shading records, the light, halton_tab, spp,
// sample_base; the launcher also max_index (the host's bound 0xFFFFF +
// sample_base + spp - 1 of every index) and lanes (0 = auto, 1 or 16 lanes per
// ray).  No camera, no seeds of the context, no sums.
struct PathQueryArgs {
    const float4* rays;        // 2 float4 per ray: (origin, tmin) (dir, tmax), device memory
    const uint32_t* seeds;     // one per ray (the low 20 bits are used), or null: splitmix64(seed_key + r)
    float4* radiance;          // (sum / spp, 1) per ray; (0, 0, 0, 0) for a ray outside the domain
    uint2* hits;               // (t bits, id) of the first segment per ray, or null
    uint32_t n;                // rays, 1 .. 2^31
    uint64_t seed_key;
    RayDomain dom;             // rt_raydomain.h
};
// Automatic lanes per ray (fixed-digit indices only; one lane otherwise): 16
// from 16 samples per ray on, from 8 on for at most 65,536 rays and from 4 on
// for at most 4,096 rays, where one lane per ray leaves most of the device
// idle.  Every cell of the table measured over spp and ray count on three
// scenes agrees (tools/bench_paths.py, profiles/r21/paths.md).
constexpr bool path_auto_lanes16(uint32_t spp, uint32_t n) {
    return spp >= 16u || (spp >= 8u && n <= 65536u) || (spp >= 4u && n <= 4096u);
}
// halton_tables_on for the path-query kernel, always inlined.  The largest
// instantiations of the render kernels call halton_tables_on out of line, and
// that copy is specialised for its callers: one more device caller changes it
// and them (tools/isa_diff.sh).
__host__ __device__ __forceinline__ constexpr bool path_query_tables_on(int geo, bool small, uint32_t spp, uint32_t L) {
    return geo == kLayPairClu && small && (spp + L - 1) / L >= kHaltonTabMinRounds;
}
static_assert(path_query_tables_on(kLayPairClu, true, 128, 16) == halton_tables_on(kLayPairClu, true, 128, 16) &&
                  path_query_tables_on(kLayPairClu, true, 127, 16) == halton_tables_on(kLayPairClu, true, 127, 16) &&
                  path_query_tables_on(kLayPairClu, false, 128, 1) == halton_tables_on(kLayPairClu, false, 128, 1) &&
                  path_query_tables_on(kLayPairLds, true, 128, 1) == halton_tables_on(kLayPairLds, true, 128, 1) &&
                  path_query_tables_on(kLayPairClu, true, 8, 1) == halton_tables_on(kLayPairClu, true, 8, 1) &&
                  path_query_tables_on(kLayPairClu, true, 7, 1) == halton_tables_on(kLayPairClu, true, 7, 1),
              "one rule for the Halton tables");
// THE dynamic LDS of a path-query workgroup of layout `lay` (after
// ray_query_layout): staged_f4, then the Halton tables when the launch copies
// them (halton_tables_on).  The kernel places its arrays by these terms and the
// launcher requests exactly this.
__host__ __device__ constexpr size_t path_query_lds_bytes(int lay, uint32_t nT, uint32_t nP, uint32_t nC, bool tables) {
    return ray_query_lds_bytes(lay, nT, nP, nC) + (tables ? (size_t)4 * kHaltonTabLdsFloats : (size_t)0);
}
hipError_t launch_path_query(const KParams& P, const PathQueryArgs& A, uint32_t bounces, SceneMem mem,
                             hipStream_t stream, LaunchInfo* info);

// ---- first-hit feature buffers (rt_aov.hip; include/rtpt.h rt_render_aov) ---
constexpr uint32_t kAovCenter = 0x400u;  // RT_AOV_CENTER
// The AOV kernel draws Halton dimensions 0 and 1 only; dimension 0 is a bit
// reversal, so the one low-digit table it stages is dimension 1's (3^6 floats,
// the first of rt_halton.hpp's tables; static-asserted in rt_aov.hip).
constexpr uint32_t kAovTabLdsFloats = 729;
// THE dynamic LDS of an AOV workgroup of layout `lay` (after ray_query_layout):
// staged_f4, then the Halton table when the launch fills it (halton_tables_on
// at one lane per pixel).  The kernel places its arrays by these terms and the
// launcher requests exactly this.
__host__ __device__ constexpr size_t aov_lds_bytes(int lay, uint32_t nT, uint32_t nP, uint32_t nC, bool tables) {
    return ray_query_lds_bytes(lay, nT, nP, nC) + (tables ? (size_t)4 * kAovTabLdsFloats : (size_t)0);
}
struct AovParams {
    SceneTables tab;
    uint32_t sph_compact;      // every table of the sphere kernel exists (as for a query)
    const float4* tri_shade;   // 4 float4 per triangle (TriShade)
    const float4* sph_shade;   // 3 float4 per sphere, by id (SphShade)
    const uint32_t* seeds;     // W*H, full frame; not read with kAovCenter
    float4* albedo;            // (sum diffuse, sum hits) / spp per pixel, or null
    float4* normal_depth;      // (sum N, sum t) / spp per pixel, or null
    uint2* first_hit;          // (t bits, id) of sample sample_base per pixel, or null
    float cam_pos[3], cam_u[3], cam_v[3], cam_w[3];
    float halfW, halfH;
    int32_t W, H;
    uint32_t spp, sample_base;
    uint32_t row_start, row_step, row_count;
    uint32_t flags;            // kAovCenter
    uint32_t max_index;        // max Halton index seed+n of this launch (0xFFFFFFFF: unknown/wraps)
};
hipError_t launch_aov(const AovParams& P, SceneMem mem, hipStream_t stream, LaunchInfo* info);

// ---- a-trous denoiser (rt_denoise.hip; include/rtpt.h rt_denoise) -----------
// Pixels on a side of a workgroup's tile; a wave is four rows of it.
constexpr uint32_t kDenoiseTile = 16;
// The largest a-trous step whose footprint a workgroup stages in LDS (0: none);
// larger steps read global memory.  Measured: profiles/r16/denoise.md.
#ifndef RT_DENOISE_LDS_MAX_STEP
#define RT_DENOISE_LDS_MAX_STEP 4
#endif
static_assert(RT_DENOISE_LDS_MAX_STEP <= 8, "a step-16 footprint (80 x 80 texels of 32 B) is past the CU's 160 KiB of LDS");
// THE dynamic LDS of an iteration workgroup at `step`: (D, V) and (N, Z) of the
// tile and its halo of 2 * step pixels, 32 B per texel, or nothing.
__host__ __device__ constexpr size_t denoise_lds_bytes(uint32_t step) {
    return step <= RT_DENOISE_LDS_MAX_STEP ? (size_t)32 * (kDenoiseTile + 4 * step) * (kDenoiseTile + 4 * step)
                                           : (size_t)0;
}
struct DenoiseParams {
    const float4* color_a;       // W*H each, device memory
    const float4* color_b;
    const float4* albedo;
    const float4* normal_depth;
    float4* out;                 // may be color_a or color_b
    float4* scratch[2];          // W*H each: the (D, V) ping-pong
    int32_t W, H;
    uint32_t iterations;         // 1..6
    uint32_t normal_power_log2;  // 0..10
    float sigma_luminance, sigma_depth, depth_floor;
};
// prepare, variance pre-filter, `iterations` a-trous launches; *info: the last.
hipError_t launch_denoise(const DenoiseParams& P, hipStream_t stream, LaunchInfo* info);

// ---- temporal reprojection (rt_reproject.hip; include/rtpt.h rt_reproject) --
// One launch of reproject_kernel<planes> (planes 1 or 2) over whole frames; the
// arguments and the per-pixel arithmetic are rt_reproject.hpp's.
struct ReprojectArgs;
hipError_t launch_reproject(const ReprojectArgs& A, uint32_t planes, hipStream_t stream, LaunchInfo* info);

// ---- sample planner (rt_adaptive.hip; include/rtpt.h rt_plan_samples) -------
constexpr uint32_t kPlanTile = 16;  // pixels on a side of a workgroup's tile
// rt_plan_stats, and the planner's accumulators on the device
struct PlanStats {
    unsigned long long weight_sum, samples;
    uint32_t count_max_seen, at_cap;
    uint32_t reserved[2];
};
struct PlanParams {
    const float4* first;   // rows * W pixels each, device memory
    const float4* all;
    uint32_t* counts;      // rows * W words: the dilated weights, then the counts
    PlanStats* acc;        // zeroed by the launcher, complete when the stream has run the launches
    unsigned long long budget;
    uint32_t count_min, count_max;
    float luminance_floor;
    uint32_t radius;       // 0..2
    int32_t W, rows;
    uint32_t flags;        // kPlanRelative (rt_plan.hpp)
};
// the memset of P.acc, plan_weights_kernel, plan_counts_kernel; *info: the last
hipError_t launch_plan(const PlanParams& P, hipStream_t stream, LaunchInfo* info);

hipError_t launch_mis(const MisParams& P, SceneMem mem, hipStream_t stream);
size_t mis_lds_bytes(uint32_t n_tri, uint32_t n_pairs);
size_t mis_part_bytes(uint32_t camera_rays, size_t pixels);  // 0: no split launch

// GPU build of the triangle BVH (rt_lbvh.hip).  d_nodes: 8 * (2n-1) uint4,
// d_sorted: 3n float4, d_perm: n.  Synchronises the stream.
hipError_t build_tri_lbvh(const float4* d_tri, uint32_t n, const float lo[3], const float hi[3],
                          float margin, uint4* d_nodes, float4* d_sorted, uint32_t* d_perm,
                          hipStream_t s);

// GPU binned-SAH build of the triangle BVH (rt_gsah.hip): the host build's
// rules (32 bins, SAH leaf rule) level by level on the device, written in the
// same compact layout.  d_nodes: 8 * (2n-1) uint4 at most, d_sorted: 3n
// float4, d_perm: n; *total_nodes = nodes per layout, *temp_bytes = the peak
// of the build's temporary device memory.  Synchronises the stream.
hipError_t build_tri_gsah(const float4* d_tri, uint32_t n, float margin, uint32_t leaf_max, double trav_cost,
                          uint4* d_nodes, float4* d_sorted, uint32_t* d_perm, uint32_t* total_nodes,
                          size_t* temp_bytes, hipStream_t s);
// Deterministic exclusive scan of n uint32 (rt_gsah.hip); tile_sums holds
// ceil(n / 1024) words.
hipError_t scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tile_sums, hipStream_t s);

// Refit of a built triangle BVH onto new id-order records (rt_refit.hip,
// DESIGN.md §3.25): d_sorted[k] = d_tri[d_perm[k]] and new fp16 boxes in every
// entry of the 8 layouts of `total` entries; the fourth word of every entry
// and d_perm are only read.  *d_table: the per-tree table of parents and
// arrival counters (tri_refit_table_bytes), allocated and filled when null
// (*table_made; the caller frees it with the tree, and reads
// refit_format_errors once the stream is idle: entries outside the format, 0
// for any builder's tree).  ev0 / ev1 are recorded round the refit's own
// memset and kernels.  Enqueues only: no synchronisation.
size_t tri_refit_table_bytes(uint32_t total);
hipError_t refit_tri_bvh(const float4* d_tri, uint32_t n, float margin, uint4* d_nodes, uint32_t total,
                         float4* d_sorted, const uint32_t* d_perm, uint32_t** d_table, bool* table_made,
                         hipEvent_t ev0, hipEvent_t ev1, hipStream_t s);
hipError_t refit_format_errors(const uint32_t* d_table, uint32_t total, uint32_t* bad);

hipError_t launch_fill_seeds(uint32_t* seeds, uint64_t key, uint64_t n, hipStream_t stream);
// The Halton low-digit tables (rt_halton.hpp fill_halton_tables) into `tab`,
// kHaltonTabLdsFloats floats of device memory: once per context (rt_create_ex).
hipError_t launch_fill_halton_tables(float* tab, hipStream_t stream);
// The shipped short sqrt / reciprocal (rt_math.h sqrt_cr, rcp_cr) against IEEE
// sqrtf and 1/x over every float on the current device: mismatch counts.
hipError_t math_selfcheck(unsigned long long bad[2]);

// Rank 0's placement after the gather (rt_place_tiles): frame row y comes from
// tile y mod N, tile row y / N; `gathered` holds N tiles of tile_bytes back to
// back.  One kernel on `stream` (device -> device), row_bytes and tile_bytes
// multiples of 4.
hipError_t launch_place_tiles(const void* gathered, void* frame, size_t row_bytes, size_t tile_bytes,
                              uint32_t H, uint32_t N, hipStream_t stream);

}  // namespace rt
