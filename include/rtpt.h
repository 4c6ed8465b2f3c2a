/*
 * rtpt.h — C-ABI of the MI355X path-tracing hot path (librtpt.so).
 *
 * Drop-in boundary for the reference's Metal dispatch of `kernel pathTrace`
 * (`RTrace/raytrace.metal:11-111`).  The reference host (`RTrace/renderer.swift`)
 * builds the scene arrays, copies them into MTLBuffers/textures in
 * `Renderer.init()` (`renderer.swift:29-115`), then `Renderer.draw()`
 * (`renderer.swift:117-146`) binds them to the argument table and dispatches a
 * W×H grid.  Here the same arrays (same `shaderTypes.h` layout, see
 * rt_types.h) cross a plain C boundary instead:
 *
 *   Renderer.init()   -> rt_create()     + rt_set_seeds() / rt_fill_seeds()
 *   Renderer.draw()   -> rt_render()     (synchronous, like waitUntilCompleted)
 *   deinit (ARC)      -> rt_destroy()
 *
 * No torch / HIP types appear in any signature; the optional stream is an
 * opaque pointer (a hipStream_t).  All calls return an rt_status; the message
 * of the last failure on a context is in rt_last_error().
 *
 * Semantics of the rendered value per pixel are SURVEY.md Appendix A with the
 * arithmetic contract of DESIGN.md §3 (identical on the CPU oracle).
 */
#ifndef RTPT_H
#define RTPT_H

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTPT_ABI_VERSION 11

/* Maximum bounce count: Halton dimensions 2+5b..5+5b must stay inside the
 * 24-entry `primes[]` table (`RTrace/sampling.metal:97-104`); b <= 3. */
#define RT_MAX_BOUNCES 4

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bad partition        */
    RT_ERR_NO_DEVICE = 2,     /* no HIP device / bad ordinal                  */
    RT_ERR_OUT_OF_MEMORY = 3, /* hipMalloc failed                             */
    RT_ERR_LAUNCH = 4,        /* kernel launch or execution error             */
    RT_ERR_STATE = 5,         /* e.g. render before seeds, accumulate mismatch */
    RT_ERR_COMM = 6           /* collective (gather) failure                  */
} rt_status;

typedef struct rt_ctx rt_ctx;

/* Scene input: the Metal argument table of pathTrace (raytrace.metal:11-19),
 * minus the acceleration structure (geometry is the arrays themselves).
 * All arrays are COPIED by rt_create; the caller keeps ownership
 * (renderer.swift:61-72 copies with makeBuffer(bytes:) as well). */
typedef struct rt_scene_desc {
    const CameraGPU* camera;             /* buffer(0): cameras[0] is used           */
    const MaterialGPU* materials;        /* buffer(1): one per triangle             */
    const SquareLightGPU* square_lights; /* buffer(2): squareLights[0] is used      */
    uint32_t n_square_lights;            /* >= 1                                    */
    const rt_float3* vertices;           /* buffer(3): 3 per triangle, 16-B stride  */
    uint32_t n_triangles;                /* triangle primitive ids 0..n_triangles-1 */
    const SphereGPU* spheres;            /* optional sphere primitives (config 4),  */
    uint32_t n_spheres;                  /*   primitive ids follow the triangles    */
    int32_t device;                      /* HIP device ordinal                      */
} rt_scene_desc;

/* Output flags */
#define RT_OUT_DEVICE 0x1u  /* `out` is a device pointer (else host memory)          */
#define RT_OUT_FP16   0x2u  /* store rgba16F (the reference texture format,
                               renderer.swift:74-82) instead of rgba32F             */
#define RT_OUT_NONE   0x4u  /* no image output (use with RT_KEEP_SUM)                 */
#define RT_KEEP_SUM   0x8u  /* also write the running per-pixel sum into the context,
                               so that a following call may set accumulate=1
                               (progressive rendering)               */
#define RT_OUT_RGBA8  0x10u /* store the reference's 8-bit image instead (4 B/px):
                               the epilogue of RTrace/image.swift:35-65 fused into
                               the kernel's store -- rgba16F round trip
                               (renderer.swift:74-82), x2 exposure, Reinhard,
                               pow(v, 1/2.2), clamp, truncating UInt8, alpha 255.
                               Exclusive with RT_OUT_FP16.                         */

typedef struct rt_render_params {
    uint32_t spp;          /* samples this call (reference: 400, raytrace.metal:24) */
    uint32_t bounces;      /* 0..RT_MAX_BOUNCES (reference: 3, raytrace.metal:25)   */
    uint32_t sample_base;  /* global index n of the first sample (Halton i=seed+n) */
    uint32_t row_start;    /* rows rendered: y = row_start + j*row_step,           */
    uint32_t row_step;     /*   j = 0..row_count-1 (multi-GPU interleaved tiles)    */
    uint32_t row_count;    /*   0 => all rows                                      */
    uint32_t accumulate;   /* 1: continue the context's running per-pixel sum,
                              which must then hold the samples [first,
                              sample_base) of the same rows, written by previous
                              calls with RT_KEEP_SUM (the first of them started
                              at sample index `first`); the image is the sum
                              divided by the samples it holds                      */
    uint32_t flags;        /* RT_OUT_* */
} rt_render_params;

/* Renderer.init(): validate and copy the scene to the device, precompute the
 * per-primitive records (edges, normals, shading frames).  Default options. */
int rt_create(const rt_scene_desc* scene, rt_ctx** out_ctx);

/* ---- creation options ----------------------------------------------------
 * Speed-only choices of one context: which record layout / kernel serves the
 * scene, how the acceleration structures are built, lanes per pixel.  None of
 * them changes a rendered value (every layout and build is bit-exact against
 * the oracle).  They are per context and the library reads no environment
 * variable: a caller (Swift, C, Python) sets them here or gets the defaults,
 * which are the measured-best choices.  Zero-initialised fields mean
 * "default", so `rt_create_options o = {0};` is valid. */
typedef enum rt_scene_layout {
    RT_LAYOUT_AUTO = 0,        /* measured best for the scene (box clusters, sphere
                                  kernel, triangle BVH above 384 triangles)        */
    RT_LAYOUT_PAIRS = 1,       /* shared-edge pair records in LDS, no box clusters   */
    RT_LAYOUT_SINGLE = 2,      /* one record per triangle in LDS                     */
    RT_LAYOUT_GLOBAL = 3,      /* one record per triangle, read from global memory   */
    RT_LAYOUT_PAIRS_SMEM = 4,  /* pair records by scalar loads, no LDS               */
    RT_LAYOUT_SORTED = 5,      /* pair records + octant sort of the paths per bounce */
    RT_LAYOUT_BVH = 6          /* triangle BVH at any triangle count                 */
} rt_scene_layout;

typedef enum rt_tri_bvh_build {
    RT_TRI_BVH_DEFAULT = 0,    /* = RT_TRI_BVH_GPU_SAH                               */
    RT_TRI_BVH_HOST_SAH = 1,   /* host binned SAH (32 bins), uploaded                */
    RT_TRI_BVH_GPU_LBVH = 2,   /* GPU Morton LBVH (Karras hierarchy + refit)         */
    RT_TRI_BVH_GPU_SAH = 3     /* GPU binned SAH, the host build's rules             */
} rt_tri_bvh_build;

typedef enum rt_walk_scheduler {
    RT_WALK_AUTO = 0,          /* measured best per scene                            */
    RT_WALK_LOCKSTEP = 1,      /* a wave's lanes run each bounce's queries together  */
    RT_WALK_FREE = 2,          /* every lane runs its own path state; lanes whose
                                  walk ended park until half the wave has, then
                                  shade and start their next query together        */
    RT_WALK_SORTED = 3         /* between bounces the paths of a workgroup are
                                  counting-sorted by direction octant (ballots),
                                  finished paths dropped: a wave walks one BVH
                                  layout                                           */
} rt_walk_scheduler;

typedef struct rt_create_options {
    uint32_t scene_layout;     /* rt_scene_layout                                    */
    uint32_t lanes_per_pixel;  /* 0 = auto, else 1, 4 or 16                          */
    uint32_t tri_bvh_build;    /* rt_tri_bvh_build                                   */
    uint32_t tri_leaf_max;     /* triangles per BVH leaf at most, 0 = 1; 1..128      */
    float tri_leaf_cost;       /* SAH leaf rule: box step cost in triangle tests,
                                  0 = 1.0                                            */
    uint32_t sphere_leaf_max;  /* spheres per BVH leaf at most, 0 = 1; 1..255        */
    uint32_t sphere_median;    /* 1: median splits instead of the exact SAH sweep    */
    uint32_t walk_scheduler;   /* rt_walk_scheduler (BVH scenes)                     */
    uint32_t walk_leaf_den;    /* RT_WALK_FREE: parked leaves are tested once they
                                  are >= 1/den of the walking lanes, 0 = default;
                                  1..64 (1: only when every walker is parked, so
                                  leaves stay parked into the service phase)       */
    uint32_t reserved[7];      /* must be 0                                          */
} rt_create_options;

/* The defaults (all zero). */
void rt_create_options_default(rt_create_options* opt);

/* rt_create with options (NULL = defaults).  RT_ERR_INVALID_ARG for a value
 * outside its range. */
int rt_create_ex(const rt_scene_desc* scene, const rt_create_options* opt, rt_ctx** out_ctx);

/* Seed texture (renderer.swift:84-110): W*H uint32 row-major, values are the
 * per-pixel Halton offsets (reference range [0, 2^20)).  W,H must equal the
 * camera resolution. */
int rt_set_seeds(rt_ctx* ctx, const uint32_t* seeds, int32_t width, int32_t height);

/* Deterministic replacement for the unseeded arc4random() seeds
 * (renderer.swift:99-101): seed[p] = splitmix64(key + p) mod 2^20, generated on
 * the device.  rt_seed_splitmix() below is the host form of the same function. */
int rt_fill_seeds(rt_ctx* ctx, uint64_t key);

/* Renderer.draw(): render and block until done (commit+waitUntilCompleted).
 * out: row_count*W pixels, rgba32F (16 B), rgba16F (8 B) or RGBA8 (4 B) by
 * flags; value (sum/S, 1) where S = samples in the sum. */
int rt_render(rt_ctx* ctx, const rt_render_params* params, void* out);

/* Asynchronous variant: enqueue on `hip_stream` (a hipStream_t, may be NULL
 * for the null stream); `out` must be a device pointer.  No host sync. */
int rt_render_async(rt_ctx* ctx, const rt_render_params* params, void* out_device,
                    void* hip_stream);

/* Device time of the most recent render or ray-query kernel (hipEvents on its stream), ms.
 * Synchronizes on that event. */
int rt_last_kernel_ms(rt_ctx* ctx, float* ms);

int rt_destroy(rt_ctx* ctx);

/* ---- multi-GPU: row-interleaved tiles + one RCCL gather ----
 * north_star: "the image is row-tile-partitioned across the 8 GPUs of one node
 * with a single RCCL gather of tiles over xGMI at the end of each spp batch".
 * One process (or thread) per GPU, one context per GPU.  Rank k of N renders
 * the rows y = k, k+N, k+2N, ... with the global y (so the frame is
 * bit-identical to a single-GPU render) and the tiles are gathered to rank 0
 * by one ncclGather over xGMI, then placed at their rows by one kernel on rank
 * 0 (rt_place_tiles).  The reference's draw (renderer.swift:117-146) has no multi-GPU
 * path; this extends it. */
#define RT_COMM_ID_BYTES 128   /* ncclUniqueId */

/* Rank 0 makes the communicator id and hands it to every rank out of band
 * (MPI, a TCP store, a file).  RT_ERR_COMM on failure. */
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);

/* Join the N-rank communicator (collective: every rank calls it with the same
 * id).  RT_ERR_INVALID_ARG for a bad rank/world, RT_ERR_COMM for RCCL errors,
 * RT_ERR_STATE if the context already has a communicator. */
int rt_comm_init(rt_ctx* ctx, int32_t rank, int32_t world, const uint8_t id[RT_COMM_ID_BYTES]);

/* Renderer.draw() across the communicator (collective): render this rank's
 * rows with params (which name the whole frame: row_start 0, row_step 0 or 1,
 * row_count 0; the partition is y = rank (mod world)), then gather every tile into `frame` on rank 0 --
 * H*W pixels in the format of params->flags (rgba32F / rgba16F / RGBA8), host
 * memory (the call then blocks) or device memory with RT_OUT_DEVICE (enqueued
 * on `hip_stream`, a hipStream_t; NULL is the HIP null stream, as for
 * rt_render_async; no host sync).  `frame` is
 * ignored on other ranks.  With RT_OUT_NONE (progressive batches into the
 * running sums) nothing is gathered.  RT_ERR_STATE without rt_comm_init,
 * RT_ERR_COMM when the gather fails. */
int rt_render_gather(rt_ctx* ctx, const rt_render_params* params, void* frame, void* hip_stream);

/* The communicator as RCCL sees it (ncclCommCount / ncclCommUserRank): lets a
 * caller prove that N ranks joined.  RT_ERR_STATE without rt_comm_init. */
int rt_comm_info(const rt_ctx* ctx, int32_t* count, int32_t* rank);

/* Row layout of rt_render_gather (host-only, no device): rank `rank` of
 * `world` owns rows y = rank + j*world, j < rows; every rank sends a tile
 * padded to rows_max rows (tile_bytes = rows_max * row_bytes, the ncclGather
 * count), so rank 0 receives world tiles back to back.  rows is 0 for a rank
 * past the last row (world > height).  Pixel bytes by flags (16 / 8 / 4). */
typedef struct rt_tile_layout_info {
    uint32_t rows;
    uint32_t rows_max;
    uint64_t row_bytes;
    uint64_t tile_bytes;
} rt_tile_layout_info;
int rt_tile_layout(int32_t width, int32_t height, int32_t world, int32_t rank, uint32_t flags,
                   rt_tile_layout_info* out);

/* Rank 0's placement step of rt_render_gather on its own: `gathered_device`
 * holds `world` tiles of rt_tile_layout's tile_bytes back to back (device
 * memory); tile row j of rank k lands at frame row k + j*world.  `frame` is
 * H*W pixels in the format of flags, device memory with RT_OUT_DEVICE
 * (enqueued on hip_stream; NULL is the HIP null stream) or host memory (the
 * call blocks).  The same code rt_render_gather runs after its ncclGather. */
int rt_place_tiles(rt_ctx* ctx, const void* gathered_device, int32_t world, uint32_t flags,
                   void* frame, void* hip_stream);

/* The same placement on host memory (no device). */
int rt_place_tiles_host(const void* gathered, int32_t width, int32_t height, int32_t world,
                        uint32_t flags, void* frame);

/* Which kernel instantiation the most recent rt_render/rt_render_async,
 * rt_trace_rays/rt_trace_rays_async, rt_trace_paths/rt_trace_paths_async,
 * rt_render_aov/rt_render_aov_async or
 * rt_denoise/rt_denoise_async (its last pass) launched, with its launch shape:
 * lets a caller (bench, tests) state which configuration it timed or checked.  `kernel` is the demangled name rocprofv3
 * reports, e.g. "rt::path_trace_kernel<3, 6, false, true, 4>". */
typedef struct rt_launch_info {
    char kernel[96];
    uint32_t lanes_per_pixel;   /* 1, 4 or 16 lanes trace one pixel's samples     */
    uint32_t halton_tables;     /* 1: LDS low-digit Halton tables filled (§3.3)   */
    uint32_t small_index;       /* 1: fixed-digit Halton (max index < 3^13)       */
    uint32_t block_threads;
    uint32_t grid_x, grid_y;
    uint32_t lds_bytes;         /* dynamic LDS per workgroup                      */
} rt_launch_info;
int rt_last_launch(const rt_ctx* ctx, rt_launch_info* info);

/* ---- batched ray queries -------------------------------------------------
 * The exact ray queries of the render kernels (DESIGN.md §3.5, §3.6, §3.9,
 * §3.10, §3.24) for the caller's own rays, through the record layout and the
 * acceleration structures of the context: picking, visibility and ambient
 * occlusion between arbitrary points, line of sight, probing a scene.
 *
 * Closest hit: id = the lowest-id primitive among those with the smallest
 * accepted t, tmin < t < tmax strictly; triangles are 0..n_triangles-1, sphere
 * k of the caller's array is n_triangles + k; t is that primitive's t.  A miss
 * gives id = -1 and t = the ray's tmax, bit for bit.
 * RT_RAYS_ANY: id = 1 if any primitive accepts the ray, else 0; t = +0.
 *
 * The call is total: any 32 bytes are a ray (NaN, infinity, a zero direction,
 * tmin >= tmax), and the answer for every ray is what the id-ordered scan with
 * strict '<' over the primitive tests of DESIGN.md §3.5 / §3.6 gives.  Rays
 * inside the exactness domain (rt_debug_ray_domain) take the
 * context's accelerated layout, every other ray takes that scan itself.  The
 * one known limit of the accelerated layouts: a ray that lies in the plane of
 * a triangle to rounding (|dot(n, dir)| <= 2^-20 |n| |dir|, n no world axis)
 * may be accepted by that triangle on rounding residues, anywhere along the
 * ray; the accelerated answer is then the scan's without that hit.
 * RT_RAYS_EXACT answers such rays like the scan. */
typedef struct rt_ray {
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} rt_ray; /* 32 B */

typedef struct rt_ray_hit {
    float t;
    int32_t id;
} rt_ray_hit; /* 8 B */

#define RT_RAYS_ANY   0x100u /* any-hit (accept_any_intersection) instead of closest hit */
#define RT_RAYS_EXACT 0x200u /* every ray takes the id-ordered loop (no acceleration)    */
#define RT_RAYS_CHUNK 2048   /* consecutive rays one workgroup traces                    */

/* Trace n rays and block until done.  flags: RT_RAYS_ANY, RT_RAYS_EXACT, and
 * RT_OUT_DEVICE when BOTH pointers are device memory (otherwise both are host
 * memory and the context's staging buffers carry them).  n == 0 is RT_OK
 * without a launch; n > 2^31, an unknown flag bit, or a null pointer with
 * n > 0 is RT_ERR_INVALID_ARG.  No seeds are needed.  rt_last_launch then
 * names the instantiation, e.g. "rt::ray_query_kernel<6, false, false>"
 * (layout, spheres, any-hit) with its grid, block size and dynamic LDS, and
 * rt_last_kernel_ms gives the query kernel's device time. */
int rt_trace_rays(rt_ctx* ctx, const rt_ray* rays, uint64_t n, uint32_t flags, rt_ray_hit* hits);

/* Asynchronous variant: both pointers are device memory, the query is enqueued
 * on `hip_stream` (a hipStream_t, NULL = the null stream).  No host sync. */
int rt_trace_rays_async(rt_ctx* ctx, const rt_ray* rays_dev, uint64_t n, uint32_t flags,
                        rt_ray_hit* hits_dev, void* hip_stream);

/* ---- first-hit feature buffers ----------------------------------------------
 * What each pixel sees: for sample index n in
 * [sample_base, sample_base + spp) the camera ray of rt_render's sample n of
 * that pixel (seed + n, Halton dimensions 0 and 1, generateCameraRay) and its
 * closest hit (t, id) exactly as bounce 0 of the render finds it.  Per sample
 * a hit gives a = material.diffuse.xyz of primitive id (a light: its diffuse,
 * not its emissive), N = the triangle's unflipped unit normal
 * normalize(cross(e1, e2)) or the sphere's normalize(hit point - centre),
 * t, and h = 1; a miss gives zero for all four.  The sums run in fp32 in
 * ascending n from +0 and are divided by (float)spp:
 *   albedo        4 floats per pixel: (sum a.r, sum a.g, sum a.b, sum h) / spp;
 *                 the fourth is the coverage
 *   normal_depth  4 floats per pixel: (sum N.x, sum N.y, sum N.z, sum t) / spp;
 *                 depth / coverage is the mean t over the hits
 *   first_hit     (t, id) of sample n = sample_base; a miss is (1000.0f, -1),
 *                 the render's tmax bit for bit, as rt_trace_rays reports it
 * RT_AOV_CENTER: one ray through every pixel centre (jitter 0.5, 0.5), the
 * picking / id-buffer form: spp must be 1, sample_base is ignored and no seeds
 * are needed.
 *
 * These entry points were added without a change of RTPT_ABI_VERSION (nothing
 * else changed): a caller that may meet an older library detects the feature
 * by the presence of the symbol rt_render_aov (dlsym). */
#define RT_AOV_CENTER 0x400u

typedef struct rt_aov_params {
    uint32_t spp;         /* 1 .. 2^24 (the coverage sum stays exact)            */
    uint32_t sample_base;
    uint32_t row_start;   /* rows as in rt_render_params                         */
    uint32_t row_step;
    uint32_t row_count;
    uint32_t flags;       /* RT_OUT_DEVICE, RT_AOV_CENTER                        */
} rt_aov_params; /* 24 B */

typedef struct rt_aov_buffers {
    float* albedo;          /* row_count * W * 4 floats, or NULL                 */
    float* normal_depth;    /* row_count * W * 4 floats, or NULL                 */
    rt_ray_hit* first_hit;  /* row_count * W entries, or NULL                    */
} rt_aov_buffers; /* 24 B */

/* Render the feature buffers and block until done.  Any subset of the three
 * buffers may be NULL, but not all.  With RT_OUT_DEVICE every non-NULL buffer
 * is device memory, otherwise host memory (the context's staging buffers carry
 * them).  RT_ERR_INVALID_ARG: a NULL context, params or buffers, all three
 * buffers NULL, spp == 0 or spp > 2^24, RT_AOV_CENTER with spp != 1, an
 * unknown flag bit, a bad row partition.  RT_ERR_STATE: a jittered call before
 * seeds are set.  rt_last_launch then names the instantiation, e.g.
 * "rt::aov_kernel<6, false, true>" (layout, spheres, fixed-digit Halton) at
 * one lane per pixel, and rt_last_kernel_ms gives its device time.  The
 * context's lanes_per_pixel and walk_scheduler options are ignored. */
int rt_render_aov(rt_ctx* ctx, const rt_aov_params* params, const rt_aov_buffers* buffers);

/* Asynchronous variant: every non-NULL buffer is device memory, the kernel is
 * enqueued on `hip_stream` (a hipStream_t, NULL = the null stream).  No host
 * sync. */
int rt_render_aov_async(rt_ctx* ctx, const rt_aov_params* params, const rt_aov_buffers* buffers_dev,
                        void* hip_stream);

/* ---- denoiser for low-spp renders ------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
 * albedo-demodulated colour.  Its edge-stopping weights come from the feature
 * buffers of rt_render_aov (normal, depth; Schied et al. 2017); its luminance
 * weight is scaled by a per-pixel variance estimated from two renders of half
 * the samples each (dual buffers, Rousselle et al. 2012): render spp/2 samples
 * at sample_base into color_a, spp/2 at sample_base + spp/2 into color_b, and
 * rt_render_aov of all spp samples at sample_base into albedo / normal_depth.
 * The result estimates the mean of the two halves.  The arithmetic is fixed
 * operation by operation: the output is a function of the
 * buffers and the parameters alone, bit for bit.  Inputs must be finite; for
 * other inputs the result is unspecified, but no address depends on data.
 *
 * All five frames are whole frames of the context's camera resolution (H*W
 * pixels of 4 floats, no row partition: a filter needs its neighbours).  No
 * seeds are needed.  The context owns the filter's scratch (32 B per pixel),
 * grown on first use and freed by rt_destroy; calls on one context must be
 * ordered (one stream, or the caller's events between streams).
 *
 * These entry points were added without a change of RTPT_ABI_VERSION (nothing
 * else changed): a caller that may meet an older library detects the feature
 * by the presence of the symbol rt_denoise (dlsym). */
typedef struct rt_denoise_params {
    uint32_t iterations;         /* 1..6: a-trous steps 1, 2, 4, ... 2^(iterations-1) pixels  */
    uint32_t normal_power_log2;  /* 0..10: normal weight = max(0, dot)^(2^k)                  */
    float sigma_luminance;       /* >= 0: larger = smoother across luminance differences      */
    float sigma_depth;           /* >= 0: tolerance along the local depth slope               */
    float depth_floor;           /* > 0, scene units: depth difference that always passes     */
    uint32_t flags;              /* RT_OUT_DEVICE                                             */
    uint32_t reserved[2];        /* must be 0                                                 */
} rt_denoise_params; /* 32 B */

typedef struct rt_denoise_buffers {
    const float* color_a;        /* H*W rgba32F: rt_render of the first half of the samples   */
    const float* color_b;        /* H*W rgba32F: rt_render of the second half                 */
    const float* albedo;         /* H*W*4: rt_render_aov albedo (rgb, coverage), all samples  */
    const float* normal_depth;   /* H*W*4: rt_render_aov normal_depth                         */
    float* out;                  /* H*W rgba32F; may alias color_a or color_b                 */
} rt_denoise_buffers; /* 40 B */

/* iterations 5, normal_power_log2 7, sigma_luminance 4.0f, sigma_depth 1.0f,
 * depth_floor 0.01f, flags 0, reserved {0, 0}. */
void rt_denoise_params_default(rt_denoise_params* params);

/* Denoise and block until done.  The five buffers are host memory (the
 * context's staging buffers carry them), or all device memory with
 * RT_OUT_DEVICE.  out.a is color_a's alpha; a pixel without coverage gets the
 * mean of the halves.  RT_ERR_INVALID_ARG, with an rt_last_error message that
 * names the field: a NULL context, params, buffers or any of the five
 * pointers, iterations outside 1..6, normal_power_log2 > 10, a negative or NaN
 * sigma, depth_floor not > 0 (NaN included), an unknown flag bit, nonzero
 * reserved.  rt_last_launch then names the last iteration's kernel, e.g.
 * "rt::denoise_atrous_kernel<false>" (whether the workgroup staged its
 * footprint in LDS) with its grid, block and LDS bytes, and rt_last_kernel_ms
 * gives the device time from the first to the last launch of the call. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_buffers* buffers);

/* Asynchronous variant: all five buffers are device memory, the kernels are
 * enqueued on `hip_stream` (a hipStream_t, NULL = the null stream).  No host
 * sync. */
int rt_denoise_async(rt_ctx* ctx, const rt_denoise_params* params, const rt_denoise_buffers* buffers_dev,
                     void* hip_stream);

/* ---- temporal accumulation under a moving camera -----------------------------
 * rt_reproject carries the accumulated colour of the previous frame over to
 * this frame's pixels (Schied et al. 2017, the temporal half): the world point
 * a pixel's centre ray hit is projected into the previous camera, the previous
 * outputs are gathered there bilinearly from the taps that show the same
 * primitive with a like normal near the pixel's tangent plane, and this
 * frame's colour is blended in with weight 1 / n, n the gathered history
 * length + 1 capped at max_history.  out.rgb is the new mean and out.a = n; a
 * pixel without usable history (a miss, a point behind or outside the previous
 * frame, the other side of a surface, too little tap weight) gives
 * (color.rgb, 1).  So the outputs of one call are the histories of the next,
 * and the first frame's rt_render output (a = 1) is a valid history.  Two
 * colour planes (the two half renders rt_denoise wants) share one set of tap
 * tests.  The arithmetic is fixed operation by operation:
 * the output is a function of the buffers, the two cameras and the parameters
 * alone, bit for bit, and it is defined for any bytes in any buffer: no read
 * leaves the frame.  When every history alpha is >= 1, reuse shows as
 * out.a > 1.
 *
 * Per frame: rt_render the colour plane(s), rt_render_aov with RT_AOV_CENTER
 * into first_hit and normal_depth, and keep both and the camera for the next
 * frame.  The current camera is the context's (after rt_update_scene: the new
 * pose); prev_camera is a host pointer, NULL when the camera did not move, and
 * must have the context's resolution.  Geometry that moved between the frames
 * is not compensated: only the tap tests reject its history.
 *
 * All frames are whole frames of the camera resolution (no row partition: a
 * filter needs its neighbours).  No seeds are needed.  The context owns the
 * staging of host buffers, grown on first use and freed by rt_destroy; calls
 * on one context must be ordered.
 *
 * These entry points were added without a change of RTPT_ABI_VERSION (nothing
 * else changed): a caller that may meet an older library detects the feature
 * by the presence of the symbol rt_reproject (dlsym). */
typedef struct rt_reproject_params {
    uint32_t max_history;     /* 1 .. 65536: cap of the history length n (blend weight >= 1/max_history) */
    float    normal_cos_min;  /* -1 .. 1: a tap needs dot(N, N_tap) >= this                               */
    float    plane_rel;       /* >= 0: a tap's world point may lie plane_rel * r off the pixel's tangent
                                 plane, r = distance of the point from the previous camera                */
    float    weight_min;      /* (0, 1]: least sum of valid bilinear weights for reuse                    */
    uint32_t flags;           /* RT_OUT_DEVICE                                                            */
    uint32_t reserved[3];     /* must be 0                                                                */
} rt_reproject_params; /* 32 B */

typedef struct rt_reproject_buffers {
    const float*      color[2];          /* H*W rgba32F: this frame's renders; [1] may be NULL (one plane)  */
    const float*      history[2];        /* H*W rgba32F: previous out[k] (rgb mean, a = history length);
                                            the first frame's rt_render output (a = 1) is a valid history   */
    const rt_ray_hit* hit;               /* this frame, rt_render_aov with RT_AOV_CENTER: first_hit         */
    const float*      normal_depth;      /* this frame, the same call: normal_depth                         */
    const rt_ray_hit* prev_hit;          /* the previous frame's two buffers                                */
    const float*      prev_normal_depth;
    float*            out[2];            /* H*W rgba32F; out[k] may be color[k]; must not overlap a history */
} rt_reproject_buffers; /* 80 B */

/* max_history 32, normal_cos_min 0.9f, plane_rel 0x1p-7f, weight_min 0.0625f,
 * flags 0, reserved {0, 0, 0}. */
void rt_reproject_params_default(rt_reproject_params* params);

/* Reproject and block until done.  The buffers are host memory (the context's
 * staging buffers carry them), or all device memory with RT_OUT_DEVICE.
 * color[1], history[1] and out[1] are all NULL (one plane) or all non-NULL.
 * RT_ERR_INVALID_ARG, with an rt_last_error message that names the field: a
 * NULL context, params, buffers or required pointer, a mixed plane 1, a
 * parameter outside its range (NaN included), an unknown flag bit, nonzero
 * reserved, a prev_camera that rt_create would reject or of another
 * resolution.  RT_ERR_STATE: a context left broken by a failed
 * rt_update_scene.  rt_last_launch then names "rt::reproject_kernel<1>" or
 * "<2>" (the planes) with its grid, block and LDS bytes, and rt_last_kernel_ms
 * gives the device time. */
int rt_reproject(rt_ctx* ctx, const rt_reproject_params* params, const CameraGPU* prev_camera,
                 const rt_reproject_buffers* buffers);

/* Asynchronous variant: every buffer is device memory (prev_camera stays a
 * host pointer, read before the call returns), the kernel is enqueued on
 * `hip_stream` (a hipStream_t, NULL = the null stream).  No host sync. */
int rt_reproject_async(rt_ctx* ctx, const rt_reproject_params* params, const CameraGPU* prev_camera,
                       const rt_reproject_buffers* buffers_dev, void* hip_stream);

/* The same function on the host: no device, no context; `camera` is the
 * current camera (required), every buffer is host memory and no flag is
 * accepted.  Bit for bit what rt_reproject computes (one per-pixel function
 * compiled for both).  Errors go to rt_last_error(NULL). */
int rt_reproject_host(const CameraGPU* camera, const CameraGPU* prev_camera, const rt_reproject_params* params,
                      const rt_reproject_buffers* buffers);

/* ---- adaptive sampling: per-pixel sample counts and a sample planner --------
 * rt_render_counts is rt_render with one sample count per pixel; rt_plan_samples
 * makes such counts from a pilot render.  These entry points
 * were added without a change of RTPT_ABI_VERSION (nothing else changed): a
 * caller that may meet an older library detects the feature by the presence of
 * the symbol rt_render_counts (dlsym).
 *
 * rt_render_counts: `counts` and `totals` (optional) hold row_count * W words
 * in the layout of `out` (tile row j, column x): host memory (the context's
 * staging buffers carry them), or all device memory with RT_OUT_DEVICE.
 * params->spp is a cap: pixel p draws c_p = min(counts[p], spp) samples.
 *   accumulate = 0: pixel p renders the samples [sample_base, sample_base + c_p);
 *                   its total is c_p.
 *   accumulate = 1: the context's running sum must hold, for these rows, a
 *                   sequence that started at sample_base (RT_ERR_STATE
 *                   otherwise).  Pixel p already holds k_p samples (the fourth
 *                   word of its sum entry), renders
 *                   [sample_base + k_p, sample_base + k_p + c_p), and its total
 *                   is k_p + c_p.
 * The pixel is (sum / (float)total, 1) in the format the flags ask for, colour
 * +0 where the total is 0; with RT_KEEP_SUM its sum entry becomes
 * (sum, (float)total); `totals` receives the total.  So pixel p equals the same
 * pixel of rt_render with spp = total_p from sample_base, bit for bit, whatever
 * its neighbours' counts, and uniform counts reproduce rt_render.
 *
 * The context keeps an upper bound of the totals, which grows by spp with each
 * accumulating call and must stay <= 2^24 (RT_ERR_INVALID_ARG above: the sum's
 * count stays an exact float).  After a counts call the sum holds per-pixel
 * counts: rt_render with accumulate = 1 then returns RT_ERR_STATE; a counts call
 * may continue a uniform sum; a non-accumulating RT_KEEP_SUM render starts a
 * uniform sum again; rt_update_scene drops the sum.  RT_OUT_NONE, the
 * RT_OUT_FP16 / RT_OUT_RGBA8 exclusivity, the row partition and the seeds
 * behave as for rt_render.  An all-zero map is RT_OK.
 *
 * The kernel is rt::path_counts_kernel<B, layout, spheres, small, L>
 * (rt_last_launch): L = 16 lanes per pixel for fixed-digit Halton indices, one
 * lane per pixel otherwise; rt_create_options.lanes_per_pixel is ignored, and
 * a context of RT_WALK_FREE, RT_WALK_SORTED or RT_LAYOUT_SORTED renders counts
 * through its lockstep form. */
int rt_render_counts(rt_ctx* ctx, const rt_render_params* params, const uint32_t* counts, void* out,
                     uint32_t* totals);

/* Asynchronous variant: counts, out and totals are device memory, the kernel is
 * enqueued on `hip_stream` (a hipStream_t, NULL = the null stream).  No host
 * sync. */
int rt_render_counts_async(rt_ctx* ctx, const rt_render_params* params, const uint32_t* counts_dev, void* out_dev,
                           uint32_t* totals_dev, void* hip_stream);

/* rt_plan_samples: sample counts from a pilot render.  `first` is the rgba32F
 * image of the pilot's first h samples, `all` the image of all 2h: the outputs
 * of the two calls that build the running sum (h samples with RT_KEEP_SUM, then
 * h more with accumulate = 1), so no sample is rendered twice.  Both are
 * rows * W pixels; the neighbourhood is taken within that tile (the rows of an
 * interleaved share are treated as adjacent).  Per pixel, in fp32 under the
 * contract of DESIGN.md §3 up to q and in integers from there:
 *   el = |lum(all) - lum(first)|            lum: the denoiser's (§3.23)
 *   r  = el, or el / (lum(all) + luminance_floor) with RT_PLAN_RELATIVE
 *   r  = (r >= 0) ? r : 0                   NaN gives 0
 *   q  = 1 + (uint32)min(r * 65536.0f, 16777216.0f)
 *   m  = max of q over the in-tile (2 radius + 1)^2 neighbourhood
 *   Q  = sum of m over the tile (64 bit)
 *   counts = min(count_max, count_min + (budget * m) / Q)    in 64-bit integers
 * Samples lost to the cap are not redistributed:
 * sum(counts) <= pixels * count_min + budget.  Any 32 bytes per pixel give a
 * defined answer and no address depends on data; the device, the host function
 * and tests/adaptive_ref.py agree bit for bit. */
#define RT_PLAN_RELATIVE 0x800u
typedef struct rt_plan_params {
    uint64_t budget;         /* samples to hand out over the tile beyond count_min each, < 2^38 */
    uint32_t count_min, count_max;   /* count_min <= count_max <= 2^24                          */
    float luminance_floor;   /* RT_PLAN_RELATIVE: > 0                                           */
    uint32_t radius;         /* 0..2: dilation                                                  */
    uint32_t rows;           /* rows of the tile, 0 = the camera's H                            */
    uint32_t flags;          /* RT_OUT_DEVICE, RT_PLAN_RELATIVE                                 */
    uint32_t reserved[2];    /* must be 0                                                       */
} rt_plan_params; /* 40 B */

typedef struct rt_plan_stats {
    uint64_t weight_sum;     /* Q                                                               */
    uint64_t samples;        /* sum of counts                                                   */
    uint32_t count_max_seen; /* the largest count                                               */
    uint32_t at_cap;         /* pixels whose share was cut by count_max                         */
    uint32_t reserved[2];    /* 0                                                               */
} rt_plan_stats; /* 32 B */

/* budget 0, count_min 0, count_max 2^24, luminance_floor 0.01f, radius 1,
 * rows 0, flags 0 (absolute), reserved {0, 0}. */
void rt_plan_params_default(rt_plan_params* params);

/* Plan and block until done.  first / all / counts (and stats, optional) are
 * host memory, or first / all / counts device memory with RT_OUT_DEVICE (stats
 * stays host memory).  The tile is `rows` rows (<= H) of the camera's width.
 * The context owns the planner's scratch (its staging buffers and 32 B of
 * accumulators), grown on first use and freed by rt_destroy; calls on one
 * context must be ordered.  RT_ERR_INVALID_ARG with a message: a NULL pointer,
 * count_min > count_max, count_max > 2^24, budget >= 2^38, radius > 2, a floor
 * not > 0 with RT_PLAN_RELATIVE, rows > H, nonzero reserved, unknown flag bits. */
int rt_plan_samples(rt_ctx* ctx, const rt_plan_params* params, const float* first, const float* all,
                    uint32_t* counts, rt_plan_stats* stats);

/* Asynchronous variant: first, all, counts and stats_dev (optional) are device
 * memory; enqueued on `hip_stream`.  No host sync. */
int rt_plan_samples_async(rt_ctx* ctx, const rt_plan_params* params, const float* first_dev, const float* all_dev,
                          uint32_t* counts_dev, rt_plan_stats* stats_dev, void* hip_stream);

/* The same plan in plain C++ on the host (no device, no context): a tile of
 * params->rows (>= 1) rows of `width` pixels.  RT_OUT_DEVICE is not accepted. */
int rt_plan_samples_host(int32_t width, const rt_plan_params* params, const float* first, const float* all,
                         uint32_t* counts, rt_plan_stats* stats);

/* ---- path queries: radiance along the caller's own rays ---------------------
 * rt_trace_rays answers geometry for the caller's rays; rt_trace_paths answers
 * light: the render's path tracer started on ray r
 * instead of a camera ray.  Light probes, lightmap and vertex
 * baking, irradiance caches, reflection and off-screen lookups.  These entry
 * points were added without a change of RTPT_ABI_VERSION (nothing else
 * changed): a caller that may meet an older library detects the feature by the
 * presence of the symbol rt_trace_paths (dlsym).
 *
 * Seed: s_r = seeds[r] & 0xFFFFF (only the low 20 bits of a supplied seed are
 * used); with seeds == NULL, s_r = splitmix64(seed_key + r) mod 2^20, the value
 * rt_fill_seeds(seed_key) gives pixel r.
 * First segment: the closest hit of the ray with tmin < t < tmax strictly, ties
 * to the lowest id: what rt_trace_rays returns for that ray.  It is the same
 * for every sample.
 * Samples: for n in [sample_base, sample_base + spp), i = s_r + n, the bounce
 * loop of the render for b = 0 .. bounces-1: bounce 0's hit is the first
 * segment, bounces >= 1 query with tmin 0.001 / tmax 1000, the Halton
 * dimensions are the render's 2+5b .. 5+5b (dimensions 0 and 1, the camera
 * jitter, are not drawn).
 * Sum: in fp32 in ascending n from +0; radiance[r] = (sum / (float)spp, 1.0f).
 * So a ray that equals the camera ray of pixel p, sample n, with tmin 0.001 and
 * tmax 1000, traced with seeds[r] = seed[p], spp = 1 and sample_base = n, gives
 * that sample's radiance of rt_render bit for bit.
 *
 * A ray outside the exactness domain (rt_debug_ray_domain: any NaN or infinity,
 * a far origin, a direction length outside [1/2, 2], tmin < 0, tmin >= tmax,
 * tmax > 1000) is not traced: radiance[r] = (0, 0, 0, 0) -- alpha 0 tells it
 * from a traced miss, whose alpha is 1 -- and first_hits[r] = (tmax bit for
 * bit, -1).  The call is total: any 32 bytes are a ray, and no value from a ray
 * or a seed is used as an index.  From the first hit on the path is the
 * render's own, with the accelerated layouts' one known limit (a ray lying in
 * an oblique triangle's plane to rounding, see rt_trace_rays).
 * first_hits (optional): for every in-domain ray the answer of rt_trace_rays
 * (closest hit). */
typedef struct rt_path_params {
    uint32_t spp;            /* 1 .. 2^24                                    */
    uint32_t bounces;        /* 0 .. RT_MAX_BOUNCES                          */
    uint32_t sample_base;    /* 2^20 + sample_base + spp must not pass 2^32  */
    uint32_t lanes_per_ray;  /* 0 = auto, 1 or 16                            */
    uint64_t seed_key;       /* used when seeds == NULL                      */
    uint32_t flags;          /* RT_OUT_DEVICE                                */
    uint32_t reserved;       /* must be 0                                    */
} rt_path_params; /* 32 B */

/* spp 1, bounces 3, everything else 0. */
void rt_path_params_default(rt_path_params* params);

/* Trace n rays and block until done.  rays, seeds (optional), radiance (n * 4
 * floats) and first_hits (optional) are host memory (the context's staging
 * buffers carry them), or all device memory with RT_OUT_DEVICE.  n == 0 is
 * RT_OK without a launch.  RT_ERR_INVALID_ARG, with an rt_last_error message
 * that names the field: n > 2^31; a NULL params, rays or radiance with n > 0;
 * spp outside 1 .. 2^24; bounces > RT_MAX_BOUNCES; lanes_per_ray not 0, 1 or
 * 16; 2^20 + sample_base + spp > 2^32; an unknown flag bit; nonzero reserved.
 * RT_ERR_STATE: a context a failed rt_update_scene left broken.  No context
 * seeds are needed; rt_create_options' lanes_per_pixel and walk_scheduler are
 * ignored, and a context of RT_WALK_FREE, RT_WALK_SORTED or RT_LAYOUT_SORTED
 * runs through its lockstep form.
 * The kernel is rt::path_query_kernel<B, layout, spheres, small, L>
 * (rt_last_launch, with its grid, block, dynamic LDS and whether the Halton
 * tables were copied; lanes_per_pixel reports L).  L lanes trace one ray's
 * samples: 16 (one DPP row) needs fixed-digit Halton indices (0xFFFFF +
 * sample_base + spp - 1 < 3^13) and is taken when lanes_per_ray is 16, or
 * automatically from spp >= 16 on, from 8 on for n <= 65536 and from 4 on for
 * n <= 4096 (measured); otherwise one lane traces the ray.
 * The result does not depend on L.  rt_last_kernel_ms gives the device time. */
int rt_trace_paths(rt_ctx* ctx, const rt_path_params* params, const rt_ray* rays, const uint32_t* seeds,
                   uint64_t n, float* radiance, rt_ray_hit* first_hits);

/* Asynchronous variant: all pointers are device memory, the kernel is enqueued
 * on `hip_stream` (a hipStream_t, NULL = the null stream).  No host sync. */
int rt_trace_paths_async(rt_ctx* ctx, const rt_path_params* params, const rt_ray* rays_dev,
                         const uint32_t* seeds_dev, uint64_t n, float* radiance_dev, rt_ray_hit* first_hits_dev,
                         void* hip_stream);

/* The exactness domain of a scene (host-only, no device): a ray is in it when
 * all eight floats are finite, max |origin component| <= origin_max,
 * dir_len2_min <= dot(dir, dir) <= dir_len2_max and
 * 0 <= tmin < tmax <= tmax_max.  origin_max is the extent every culling
 * structure's padding was taken from: the largest |coordinate| of the scene
 * (at least 2.5) or of the camera position, whichever is larger (9.0 for the
 * Cornell scene).  Only speed depends on it. */
typedef struct rt_ray_domain_info {
    float origin_max, dir_len2_min, dir_len2_max, tmax_max;
} rt_ray_domain_info;
int rt_debug_ray_domain(const rt_scene_desc* scene, rt_ray_domain_info* info);

/* How rt_create built the scene: which triangle-BVH build ran (rt_tri_bvh_build,
 * 0 = no triangle BVH), its nodes per octant layout, the wall times of the
 * build (device sync / upload included) and of the host scene compile, and the
 * peak temporary device memory of the GPU SAH build (KiB; 0 for the others). */
typedef struct rt_build_stats {
    uint32_t tri_bvh_build;
    uint32_t tri_bvh_nodes;
    float tri_bvh_build_ms;
    float scene_compile_ms;
    uint32_t tri_bvh_temp_kib;
} rt_build_stats;
int rt_build_info(const rt_ctx* ctx, rt_build_stats* info);

/* Debug: the triangle BVH as the walks read it, copied to
 * host memory for a node-by-node check of a build (tests/tri_bvh_tree.py).
 * The four counts and the margin are always written; each non-NULL buffer is
 * filled, so a first call with NULL buffers gives the sizes:
 *   nodes   8 * nodes_per_layout entries of 4 uint32: layout o of octant o at
 *           entry o * nodes_per_layout; three words of fp16 near/far planes,
 *           then escape | 2^31 (an entry index over all 8 layouts) or a leaf
 *           word first | (count - 1) << 24
 *   sorted  n_triangles intersection records of 12 floats, in leaf order
 *   perm    n_triangles ids: leaf order -> triangle id
 *   isect   n_triangles intersection records of 12 floats, in id order
 * margin is the culling margin every box was padded by before it was rounded
 * outward to fp16, leaf_max the most triangles a leaf of this build may hold
 * (tri_leaf_max as resolved; 1 for the LBVH).
 *
 * These entry points were added without a change of RTPT_ABI_VERSION: a caller
 * detects them by the presence of the symbol rt_debug_tri_bvh (dlsym). */
typedef struct rt_tri_bvh_dump {
    uint32_t n_triangles;
    uint32_t nodes_per_layout;
    uint32_t leaf_max;
    float margin;
    uint32_t* nodes;
    float* sorted;
    uint32_t* perm;
    float* isect;
} rt_tri_bvh_dump; /* 48 B */

/* The tree of a context, whichever build made it (host-side copies of the
 * device arrays; no kernel runs).  RT_ERR_STATE when the context built no
 * triangle BVH. */
int rt_debug_tri_bvh(const rt_ctx* ctx, rt_tri_bvh_dump* dump);

/* The same dump from the scene compile and the host binned-SAH build alone
 * (host-only, no device): what a context created with RT_TRI_BVH_HOST_SAH and
 * these options uploads.  The tree is built at any triangle count >= 1,
 * whatever layout rt_create would choose.  nodes_per_layout is known only
 * after the build and is at most 2 * n_triangles - 1: a caller sizes `nodes`
 * for that bound to get the tree in one call. */
int rt_debug_tri_bvh_host(const rt_scene_desc* scene, const rt_create_options* opt, rt_tri_bvh_dump* dump);

/* ---- in-place scene updates ---------------------------------
 * Added without a change of RTPT_ABI_VERSION: a caller detects them by the
 * presence of the symbol rt_update_scene (dlsym). */
#define RT_UPDATE_REBUILD 0x1u   /* rebuild the triangle BVH with the context's builder instead of refitting it */

/* Replace the scene of a context.  `scene` is a whole rt_scene_desc with the
 * same n_triangles, n_spheres, camera resolution and device as the context was
 * created with; everything else may differ (camera pose, materials, light,
 * vertices, spheres).  Afterwards every call on the context returns what a
 * context newly created from `scene` with the same rt_create_options returns,
 * bit for bit; only speed may differ.  Seeds are kept.  The running sum of
 * RT_KEEP_SUM is dropped (accumulate=1 is RT_ERR_STATE until a new RT_KEEP_SUM
 * call).  Synchronous; no other call on the context may be in flight.
 *
 * The triangle BVH keeps its topology and gets new boxes from a refit on the
 * device (rt_refit.hip) when the context has a tree and the new scene still
 * needs one; otherwise, or with RT_UPDATE_REBUILD, the update does what
 * rt_create does (build one with the context's builder, or free it).  The
 * refit keeps one table per context, made on the first refit and freed by
 * rt_destroy: the parent entry and an arrival counter of every entry of the 8
 * layouts, 2 x 4 B x 8 = 64 B per node of a layout.
 *
 * Failures: RT_ERR_INVALID_ARG (a null pointer, a changed count, resolution or
 * device, an unknown flag bit, a scene the compile rejects) names the field in
 * rt_last_error and leaves the context exactly as it was.  A device failure
 * halfway (RT_ERR_OUT_OF_MEMORY, RT_ERR_LAUNCH) marks the context: every
 * render, query and tree dump on it returns RT_ERR_STATE with a message until
 * an rt_update_scene succeeds; no half-updated scene is ever read.
 * rt_set_seeds, rt_fill_seeds, rt_denoise and rt_destroy keep working. */
int rt_update_scene(rt_ctx* ctx, const rt_scene_desc* scene, uint32_t flags);

typedef struct rt_update_stats {
    uint32_t tri_bvh;      /* 0: the context has no triangle BVH, 1: refitted, 2: rebuilt */
    uint32_t updates;      /* successful updates of this context so far */
    float compile_ms;      /* host scene compile (wall) */
    float upload_ms;       /* record upload (wall, sync included) */
    float tri_bvh_ms;      /* refit: device time of its kernels (hipEvents); rebuild: wall */
    float total_ms;        /* the whole call (wall) */
    uint32_t reserved[2];  /* 0 */
} rt_update_stats; /* 32 B */
/* The last successful update.  RT_ERR_STATE (with a message) before the first. */
int rt_update_info(const rt_ctx* ctx, rt_update_stats* info);

/* rt_debug_tri_bvh_host(built_from, opt), then the refit onto `updated`'s triangles
 * (same n_triangles, else RT_ERR_INVALID_ARG) with `updated`'s margin: what a context
 * created with RT_TRI_BVH_HOST_SAH from `built_from` holds after rt_update_scene(updated).
 * Host-only, no device: the refit is restated in plain C++ (rt_scene.cpp refit_tri_bvh). */
int rt_debug_tri_bvh_refit_host(const rt_scene_desc* built_from, const rt_create_options* opt,
                                const rt_scene_desc* updated, rt_tri_bvh_dump* dump);

/* Self-check of the kernels' short correctly rounded sqrt and reciprocal
 *  against the IEEE expansions on every one of the 2^32 float
 * bit patterns, on the current device: mismatches[0] sqrt, [1] reciprocal
 * (both 0 for a library whose results equal the oracle's). */
int rt_math_selfcheck(uint64_t* mismatches);

/* Debug: one scalar function of the arithmetic contract on
 * 32-bit input patterns, evaluated by the x86 compile of the shared headers
 * (RT_MATH_HOST: no device needed) or by a kernel on the current device
 * (RT_MATH_DEVICE; no context, as rt_math_selfcheck).  A test holds the two
 * sides equal over a function's whole domain (tests/test_gpu_math_fns.py).
 *
 * fn is an rt_math_fn; the Halton forms carry the dimension D < 24 in bits
 * 8-12 (RT_MATH_HALTON(form, D)) and take the sample index as input.  The
 * host has only the reference loop: host RT_MATH_HALTON_SMALL / _TAB are
 * RT_ERR_INVALID_ARG.  _TAB exists for the dimensions the kernels keep a
 * low-digit table for; _SMALL and _TAB refuse an index >= 3^13 = 1594323.
 *
 * The output is the result's 32-bit pattern; a byte (TONEMAP) or a half (F2H)
 * is zero-extended.  Every NaN result is canonicalised, a float to 0x7FC00000
 * and a half to 0x7E00: NaN signs and payloads differ between x86 and gfx950.
 *
 * Added without a change of RTPT_ABI_VERSION: detect them by the presence of
 * the symbol rt_debug_math_values (dlsym). */
typedef enum rt_math_fn {
    RT_MATH_SIN = 0,          /* first output of sincos_pt(x)                          */
    RT_MATH_COS = 1,          /* second output of sincos_pt(x)                         */
    RT_MATH_LOG = 2,          /* log_pt(x)                                             */
    RT_MATH_EXP = 3,          /* exp_pt(x)                                             */
    RT_MATH_POW_GAMMA = 4,    /* pow_pt(x, 1.0f / 2.2f)                                */
    RT_MATH_SQRT = 5,         /* sqrt_cr(x); host sqrtf(x)                             */
    RT_MATH_RCP = 6,          /* rcp_cr(x); host 1.0f / x                              */
    RT_MATH_F2H = 7,          /* float -> half bits: __float2half_rn; host to_half     */
    RT_MATH_H2F = 8,          /* half bits (low 16) -> float: __half2float; from_half  */
    RT_MATH_TONEMAP = 9,      /* tonemap_channel(half -> float): the RGBA8 epilogue
                                 after its fp16 round trip, one channel's byte         */
    RT_MATH_MIS_UNIT = 10,    /* mis_unit(mis_hash(x))                                 */
    RT_MATH_HALTON_LOOP = 11, /* halton<D>(i): the reference loop, any index           */
    RT_MATH_HALTON_SMALL = 12,/* halton_small<D>(i), device only                       */
    RT_MATH_HALTON_TAB = 13   /* halton_tab<D>(i, LDS tables), device only             */
} rt_math_fn;
#define RT_MATH_HALTON(form, D) ((uint32_t)(form) | ((uint32_t)(D) << 8))
#define RT_MATH_HOST   0u
#define RT_MATH_DEVICE 1u
#define RT_MATH_VALUES_MAX (1u << 24) /* most inputs of one rt_debug_math_values call */

/* out_bits[j] = fn(in_bits[j]) for j < n <= RT_MATH_VALUES_MAX (host arrays). */
int rt_debug_math_values(uint32_t fn, uint32_t where, const uint32_t* in_bits, uint64_t n, uint32_t* out_bits);

/* Two checksums per chunk of 2^chunk_log2 consecutive inputs first_bits + j,
 * j < count (first_bits + count <= 2^32; 6 <= chunk_log2 <= 31; the last chunk
 * may be partial).  With out = fn(input) and j' the offset in chunk c:
 *   sums[2c]     = sum of out            mod 2^64
 *   sums[2c + 1] = sum of out * (2j'+1)  mod 2^64
 * The second catches compensating errors and swapped outputs.  `sums` holds
 * 2 * ceil(count / 2^chunk_log2) values.  The host side runs on host_threads
 * (1..256) threads; the device side runs one workgroup per chunk. */
int rt_debug_math_sums(uint32_t fn, uint32_t where, uint32_t first_bits, uint64_t count, uint32_t chunk_log2,
                       uint32_t host_threads, uint64_t* sums);

/* Hash of the sources this library was built from (gpuraytracer_amd/srchash.py:
 * csrc/ + include/): a loader can refuse a stale binary. */
const char* rt_build_sha(void);

/* Diagnostic counters of a -DRT_STATS build of the kernel (reads and clears
 * up to 32 uint64 counters, slots in rt_trace.hpp; RT_ERR_STATE in normal
 * builds). */
int rt_debug_stats(rt_ctx* ctx, uint64_t* out, int n);

/* Message of the last failure on ctx (or of the last failed rt_create when
 * ctx is NULL).  Never NULL. */
const char* rt_last_error(const rt_ctx* ctx);
const char* rt_status_string(int status);
int rt_abi_version(void);

/* ---- host-side helpers (no device needed) ---------------------------- */

/* seeds[p] = splitmix64(key + p) mod 2^20 for p in [0, n). */
void rt_seed_splitmix(uint64_t key, uint32_t* seeds, size_t n);

/* initCornellBox() (RTrace/scene.swift:14-62): 36 triangles in reference
 * primitive order; camera resolution overridden to width×height.
 * Arrays: materials[36], vertices[108], one light. */
#define RT_CORNELL_TRIANGLES 36
int rt_scene_cornell_box(int32_t width, int32_t height, CameraGPU* camera,
                         MaterialGPU* materials, rt_float3* vertices,
                         SquareLightGPU* light, uint32_t* n_triangles);

/* Config-4 scene: Cornell walls + light (primIds 0-9, 34-35 -> 12 triangles)
 * plus n_spheres spheres from PCG32(seed).
 * materials[12], vertices[36], spheres[n_spheres]. */
#define RT_SPHERE_SCENE_TRIANGLES 12
int rt_scene_random_spheres(int32_t width, int32_t height, uint32_t n_spheres,
                            uint64_t seed, CameraGPU* camera, MaterialGPU* materials,
                            rt_float3* vertices, SquareLightGPU* light,
                            uint32_t* n_triangles, SphereGPU* spheres);

/* ---- MIS integrator ----------------------------------------------------
 * The SwiftPM build's kernel `drawTriangle` (Sources/gpuRaytracer/shaders.metal:
 * 635-707, bound at Sources/gpuRaytracer/computeShader.swift:99-189): per pixel
 * `camera_rays` hash-jittered camera rays; a camera ray that hits the light
 * adds light.emittedRadiance, a surface hit adds the one-bounce three-strategy
 * MIS estimate of recursiveMultiImportanceSampling (:543-625) with
 * samplesPerStrategy = mis_samples / 3.  Triangle scenes only. */
typedef struct rt_mis_params {
    uint32_t camera_rays;   /* cameraRaysPerPixel (:644), reference 6 */
    uint32_t mis_samples;   /* misSamples (:648), reference 300 */
    uint32_t row_start, row_step, row_count;  /* as rt_render_params */
    uint32_t flags;         /* RT_OUT_DEVICE: both outputs are device pointers */
} rt_mis_params;

/* out_rgba32f (optional): (sum of the camera-ray radiances, camera_rays) per
 *   pixel, row_count*W float4 -- the reference's textBuffer (:627-633,705)
 *   plus the divisor.
 * out_rgba8 (optional): the reference's pixels (:248-257,688-706): exposure
 *   1/(1.2*2^ev100), Reinhard, clamp, gamma 1/2.2, uchar(c*255), alpha 255.
 * At least one output must be non-null.  Synchronous.  When camera_rays is
 * above the kernel's lanes per pixel (2) the frame runs as one workgroup per
 * round of camera rays and an ordered per-pixel sum: the context then keeps a
 * device buffer of 16 B per camera ray and pixel (46 MB at 800x600 x 6; frames
 * that would need more than 1 GB run without the split). */
int rt_render_mis(rt_ctx* ctx, const rt_mis_params* params, float* out_rgba32f,
                  uint8_t* out_rgba8);

/* The SwiftPM scene (Sources/gpuRaytracer/main.swift:21-67, :96-173): the
 * RTrace room with a 1.5 x 1.5 light.  Arrays as rt_scene_cornell_box. */
int rt_scene_cornell_box_mis(int32_t width, int32_t height, CameraGPU* camera,
                             MaterialGPU* materials, rt_float3* vertices,
                             SquareLightGPU* light, uint32_t* n_triangles);

/* How rt_create would lay a scene out on the device (host-only, no device),
 * with default options; rt_scene_describe_ex with `opt` (NULL = defaults).
 * kernel_layout and kernel_lds_bytes follow opt->walk_scheduler (layouts 8-11
 * for FREE and SORTED on a BVH scene) and are the launcher's own choice: the
 * kernel rt_last_launch names after a render of >= 1 bounce with these options.
 * Only n_triangle_bvh_nodes is an estimate (see below).  A sphere scene whose
 * tree has a leaf of more than 128 spheres (sphere_leaf_max > 128) or a
 * non-finite node box takes layout 1, the pair kernel with the 32-B-node walk,
 * and reports sphere_kernel_lds_bytes == 0. */
typedef struct rt_scene_info {
    uint32_t n_triangles;
    uint32_t n_triangle_pairs;   /* >0: every (2k,2k+1) shares v0 and an edge -> pair records */
    uint32_t n_spheres;
    uint32_t lds_bytes;          /* intersection records staged per workgroup (0: read from global) */
    uint32_t n_sphere_nodes;     /* sphere BVH nodes per layout (32 B each, 8 layouts, global) */
    uint32_t n_triangle_bvh_nodes; /* triangle BVH nodes per layout (0: LDS layouts); 2n - 1 with
                                      one triangle per leaf (tri_leaf_max <= 1), an upper bound
                                      with larger leaves */
    uint32_t n_box_clusters;     /* pair runs on the faces of one oriented box (slab-tested first) */
    uint32_t pair_free_mask;     /* pairs in no box cluster (bit k = pair k) */
    uint32_t sphere_kernel_lds_bytes; /* dynamic LDS of the sphere kernel (its pair records; 0: sphere kernel not taken) */
    uint32_t kernel_layout;      /* the kernel layout a render (bounces >= 1) takes with these
                                    options (rt_kernel.hpp KernelLayout: 0 triangles in LDS,
                                    1 pairs, 2 global, 3 sorted pairs, 4 pairs by scalar loads,
                                    5 triangle BVH, 6 pairs + box clusters, 7 sphere kernel,
                                    8/9 free-running, 10/11 sorted BVH walks) */
    uint32_t kernel_lds_bytes;   /* that kernel's dynamic LDS per workgroup: exactly what its
                                    staging loops write (rt_last_launch reports the same) */
} rt_scene_info;
int rt_scene_describe(const rt_scene_desc* scene, rt_scene_info* info);
int rt_scene_describe_ex(const rt_scene_desc* scene, const rt_create_options* opt, rt_scene_info* info);

/* Debug (host-only, no context, no device): which triangles the camera rays of
 * the pixel rectangle [x0, x1] x [y0, y1] (closed, any jitter in [0, 1]) can
 * hit, by the test the box-cluster kernel runs once per wave for its bounce-0
 * closest query (gpuraytracer_amd/csrc/rt_beam.hpp).
 * may_hit: one byte per triangle id, 1 = the triangle's pair stays a
 * candidate.  The test runs on every scene that has pair records (every
 * (2k, 2k+1) shares v0 and an edge), whether or not a render of it takes the
 * box-cluster kernel (which needs box clusters and at most 31 pairs); a scene
 * without pair records gets all ones. */
int rt_debug_camera_candidates(const rt_scene_desc* scene, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                               uint8_t* may_hit);

/* Debug (host-only): which triangles can occlude a bounce-0 shadow ray of that
 * pixel rectangle (any jitter, any light sample), by the shaft test of
 * gpuraytracer_amd/csrc/rt_shaft.hpp: the union over every
 * triangle of every pair in the rectangle's camera mask.  may_occlude: one
 * byte per triangle id, 1 = the triangle's pair stays in the occluder mask.
 * *available = 0 when nothing is decided for the rectangle (a grazing or
 * crossing source plane, no pair records): every byte is then 1.
 * The box-cluster kernel runs the same test once per wave, but only for a
 * wave whose camera mask holds exactly one pair; for a wave with more pairs
 * it runs the generic query whatever this function reports. */
int rt_debug_shadow_candidates(const rt_scene_desc* scene, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                               uint8_t* may_occlude, int32_t* available);

/* Debug (host-only): the flag word of each box cluster the scene compiles to,
 * in the order the kernel visits them (multi-face clusters, then single-face
 * ones).  Bits 0-2: box axis a is world axis a; 8: container (world-aligned,
 * with room inside); 16: single face; and the kinds the filter has a leaner
 * path for (gpuraytracer_amd/csrc/rt_cluorder.hpp): 32 a box
 * turned about one world axis, 64 a container with a non-empty shrunk box,
 * 128 the light's own cluster.  flags: room for capacity words (may be null
 * when capacity is 0); *n_clusters: how many the scene has (at most 31). */
int rt_debug_cluster_kinds(const rt_scene_desc* scene, uint32_t* flags, uint32_t capacity, uint32_t* n_clusters);

/* Debug (host-only): the Halton low-digit tables of the box-cluster kernel
 * (gpuraytracer_amd/csrc/rt_halton.hpp), from the x86 compile
 * of the header's fill: table[offsets[D] + v], v < sizes[D], is the reference
 * loop's running sum after the tabulated digit steps of v in base primes[D];
 * sizes[D] = 0 for a dimension without a table.  offsets and sizes hold 24
 * words each (either may be null); table has room for capacity floats and may
 * be null when capacity is 0 (*n_floats alone is then reported). */
int rt_debug_halton_table(float* table, uint32_t capacity, uint32_t* n_floats, uint32_t* offsets, uint32_t* sizes);
/* Debug: the same tables as the context's device buffer holds them (filled by
 * a kernel in rt_create_ex, copied into LDS by every workgroup of a launch that
 * has the tables on); capacity >= *n_floats of rt_debug_halton_table. */
int rt_debug_halton_table_device(const rt_ctx* ctx, float* table, uint32_t capacity);

/* Debug: the per-wave candidate masks of a render launch.
 * The box-cluster render kernel (a triangle-only scene of 1..32 pairs with box
 * clusters) reads, per wave, the pairs its camera rays can hit and the pairs
 * that can occlude its bounce-0 shadow rays from a table the context fills
 * once per (scene, camera, row partition, wave geometry) and then reuses.
 * One record per wave of the launch, in wave row-major order: */
typedef struct rt_wave_mask {
    uint32_t cam_mask;      /* bit k: the camera rays can hit pair k (triangles 2k, 2k+1) */
    uint32_t shd_mask;      /* bit k: pair k can occlude a bounce-0 shadow ray */
    uint32_t shd_cskip;     /* bit c: box cluster c holds no pair of shd_mask */
    uint32_t shd_available; /* 0: shd_mask is undecided (the generic query runs) */
    int32_t x0, x1, y0, y1; /* the wave's pixel rectangle, closed, image rows y0, y0 + row_step, .., y1; it is
                               what the tests ran on and may reach past the frame (the launch rounds up to
                               whole workgroups) */
} rt_wave_mask;
/* rt_debug_wave_rects (host-only, no context, no device): the wave rectangles
 * of a lockstep launch over `width` columns and the row partition
 * (row_start, row_step, row_count; 0 resolves as for rt_render) of a frame of
 * `height` rows at lanes_per_pixel 1, 4 or 16: only x0..y1 of each record are
 * written.  *waves_x, *waves_y: the launch's waves per row and rows of waves;
 * masks has room for capacity records and may be null when capacity is 0.
 * Every pixel of the partition's rows lies in exactly one rectangle.
 * rt_debug_wave_masks: the records of the launch rt_render(ctx, params) would
 * make -- with lanes_per_pixel 1, 4 or 16 instead of the context's when it is
 * not 0 -- read back from the context's table, which is filled for that launch
 * first unless it already holds it; *fills (may be null): how often this
 * context has filled its table so far.  *waves_x = *waves_y = 0 and RT_OK when
 * that launch reads no table (another kernel layout, more than 32 pairs).
 * Synchronises the context's stream.
 * Added without a change of RTPT_ABI_VERSION: detect them by the presence of
 * the symbol rt_debug_wave_masks (dlsym). */
int rt_debug_wave_rects(int32_t width, int32_t height, uint32_t row_start, uint32_t row_step, uint32_t row_count,
                        uint32_t lanes_per_pixel, rt_wave_mask* masks, uint32_t capacity, uint32_t* waves_x,
                        uint32_t* waves_y);
int rt_debug_wave_masks(rt_ctx* ctx, const rt_render_params* params, uint32_t lanes_per_pixel, rt_wave_mask* masks,
                        uint32_t capacity, uint32_t* waves_x, uint32_t* waves_y, uint64_t* fills);

/* Debug (host-only): the light mask the box-cluster kernel tests instead of
 * loading a hit triangle's light flag: bit id of *mask is set
 * when triangle id is a light (scenes of at most 64 triangles, else 0).
 * records: room for capacity_triangles of the 64-B shading records the mask is
 * made from, 16 floats per triangle id: (N, light) (right, diffuse.r)
 * (fwd, diffuse.g) (emissive, diffuse.b) (may be null when that is 0). */
int rt_debug_light_mask(const rt_scene_desc* scene, uint64_t* mask, float* records, uint32_t capacity_triangles);

/* The reference's image epilogue (RTrace/image.swift:35-65): fp16 round trip,
 * ×2 exposure, Reinhard, gamma 1/2.2, clamp, truncating UInt8, alpha 255.
 * in: n_pixels rgba32F (host), out: n_pixels*4 bytes. */
void rt_tonemap_rgba8(const float* rgba32f, size_t n_pixels, uint8_t* rgba8);

#ifdef __cplusplus
}
#endif

#endif /* RTPT_H */
