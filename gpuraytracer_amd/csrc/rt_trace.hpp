// rt_trace.hpp — ray/primitive tests and scene queries shared by the
// pathTrace kernel (rt_kernel.hip) and the MIS kernel (rt_mis.hip).
// Device-only; every function follows the arithmetic contract of DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_cluorder.hpp"  // vmin / vmax / safe_rcp and the per-lane cluster split
#include "rt_kernel.hpp"

namespace rt {
namespace {

__device__ __forceinline__ f3 ld_f3(const float* p) { return f3{p[0], p[1], p[2]}; }

// Ray/triangle test of DESIGN.md §3.5 (stands in for Metal's intersector).
// The oracle negates (bu, bv, tn, den) when den < 0; here the same exact
// negation is an XOR with den's sign bit, |den| folds into the compare, and tn
// (with the IEEE division) is only formed for lanes inside the triangle.
__device__ __forceinline__ bool tri_test(const float4& A, const float4& Bq, const float4& C, f3 o,
                                         f3 d, float tmin, float tmax, float* t_out) {
    const f3 v0{A.x, A.y, A.z}, e1{A.w, Bq.x, Bq.y}, e2{Bq.z, Bq.w, C.x}, n{C.y, C.z, C.w};
    const f3 tv = o - v0;
    const f3 c = cross(tv, d);
    const float den = dot(n, d);
    const uint32_t sgn = __float_as_uint(den) & 0x80000000u;
    const uint32_t nsgn = sgn ^ 0x80000000u;
    const float bu = __uint_as_float(__float_as_uint(dot(e2, c)) ^ nsgn);  // -dot(e2,c), sign-normalised
    const float bv = __uint_as_float(__float_as_uint(dot(e1, c)) ^ sgn);
    const float aden = fabsf(den);
    if (aden > 0.0f && bu >= 0.0f && bv >= 0.0f && bu + bv <= aden) {
        const float tn = __uint_as_float(__float_as_uint(dot(n, tv)) ^ nsgn);  // -dot(n,tv)
        const float t = tn / aden;
        if (t > tmin && t < tmax) {
            *t_out = t;
            return true;
        }
    }
    return false;
}

// Two consecutive triangles A=(v0,..), B=(v0,..) that share v0 and one edge S
// (every quad of the reference scene, scene.swift:81-138, :212-240).  The
// per-triangle test above is evaluated for A then B with the common terms
// tv = o - v0, c = cross(tv, d) and dot(S, c) computed once: bit-identical to
// two tri_test calls, ~25% fewer VALU operations.  Record (5 x float4):
//   r0 = (v0.xyz, S.x)  r1 = (S.yz, eA.xy)  r2 = (eA.z, nA.xyz)
//   r3 = (eB.xyz, nB.x) r4 = (nB.yz, m, 0)
// m = 0 when A.e1 == S == B.e2, 0x80000000 when A.e2 == S == B.e1; eA / eB
// are the other edges.  bu+bv and the bu,bv >= 0 tests are symmetric in
// (bu, bv), so only the signs of the two terms matter.
struct PairDots {
    float denA, denB;  // dot(n, d)
    uint32_t a1, a2, b1, b2;  // sign-normalised barycentric terms (bits)
    f3 tv;
};

__device__ __forceinline__ PairDots pair_dots(const float4& r0, const float4& r1,
                                              const float4& r2, const float4& r3,
                                              const float4& r4, f3 o, f3 d) {
    PairDots q;
    const f3 v0{r0.x, r0.y, r0.z}, S{r0.w, r1.x, r1.y}, eA{r1.z, r1.w, r2.x};
    const f3 nA{r2.y, r2.z, r2.w}, eB{r3.x, r3.y, r3.z}, nB{r3.w, r4.x, r4.y};
    const uint32_t m = __float_as_uint(r4.z);
    q.tv = o - v0;
    const f3 c = cross(q.tv, d);
    const uint32_t s = __float_as_uint(dot(S, c));
    const uint32_t ea = __float_as_uint(dot(eA, c));
    const uint32_t eb = __float_as_uint(dot(eB, c));
    q.denA = dot(nA, d);
    q.denB = dot(nB, d);
    const uint32_t sA = (__float_as_uint(q.denA) & 0x80000000u) ^ m;
    const uint32_t sB = (__float_as_uint(q.denB) & 0x80000000u) ^ m;
    q.a1 = s ^ sA;
    q.a2 = ea ^ sA ^ 0x80000000u;
    q.b1 = s ^ sB ^ 0x80000000u;
    q.b2 = eb ^ sB;
    return q;
}

__device__ __forceinline__ bool bary_ok(float den, uint32_t t1, uint32_t t2) {
    const float u = __uint_as_float(t1), v = __uint_as_float(t2);
    return fabsf(den) > 0.0f && u >= 0.0f && v >= 0.0f && u + v <= fabsf(den);
}

// t of a triangle whose barycentric test passed: -dot(n, tv) / den, sign-normalised
__device__ __forceinline__ float pair_t(f3 n, f3 tv, float den) {
    const uint32_t nsgn = (__float_as_uint(den) & 0x80000000u) ^ 0x80000000u;
    const float tn = __uint_as_float(__float_as_uint(dot(n, tv)) ^ nsgn);
    return tn / fabsf(den);
}

// intersectSphere (shaders_old.metal:108-136) with the DESIGN.md §3.6 root rule.
__device__ __forceinline__ bool sph_test(const float4& S, f3 o, f3 d, float a, float tmin,
                                         float tmax, float* t_out) {
    const f3 oc = o - f3{S.x, S.y, S.z};
    const float b = 2.0f * dot(oc, d);
    const float cc = dot(oc, oc) - S.w;
    const float disc = b * b - (4.0f * a) * cc;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        const float a2 = 2.0f * a;
        float t = (-b - sq) / a2;                 // t1
        if (!(t > tmin)) t = (-b + sq) / a2;      // t2, divided only when it is the root taken
        if (t > tmin && t < tmax) {
            *t_out = t;
            return true;
        }
    }
    return false;
}

// Diagnostic counters (only in an -DRT_STATS instrumentation build, read with
// rt_debug_stats by tools/kernel_stats.py and tools/sphere_stats.py).
// Slot groups of 4 per query kind q (0: camera closest hit, 1: bounce closest
// hit, 2: shadow any-hit): [4q] pair records visited per wave, [4q+1] records
// tested, [4q+2] active lanes summed over tested records, [4q+3] division blocks.
// Box-cluster queries: [12] queries per wave, [13] candidate rounds per wave,
// [14] lanes summed over rounds, [15] lanes summed over queries; the same four
// apart for the closest queries of bounce >= 1 [32..35] and for the shadow
// queries [36..39], in the order queries, rounds, lanes over rounds, lanes over
// queries (the camera query's rounds are in [13], [14] only).
// Per-lane BVH walks (sphere_walk_box, tri_cbvh_walk), base 16 closest / 24
// any-hit: [+0] walks per wave, [+1] lanes summed over walks, [+2] walk
// steps, [+3] lanes summed over them, [+4] unused, [+5] leaf rounds, [+6]
// parked lanes summed over them.
#ifdef RT_STATS
__device__ unsigned long long g_rt_stats[40];
__device__ __forceinline__ void stat_wave(int slot, unsigned long long v) {
    const unsigned long long m = __ballot(1);
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&g_rt_stats[slot], v);
}
#define RT_STAT(slot, v) stat_wave((slot), (v))
#else
#define RT_STAT(slot, v) ((void)0)
#endif

// Where the intersection records live for one launch.
enum Geo : int {
    kGeoTriLds = 0,     // single-triangle records staged in LDS
    kGeoPairLds = 1,    // shared-edge pair records staged in LDS
    kGeoPairSmem = 4,   // shared-edge pair records read with scalar loads (no LDS)
    kGeoTriBvh = 5,     // GPU-built triangle BVH (rt_lbvh.hip), records from global
    kGeoTriGlobal = 2,  // single-triangle records read from global (big scenes)
    kGeoPairClu = 6,    // pair records in LDS + box clusters
    kGeoSphLds = 7,     // pair records in LDS + the leaf-box sphere BVH in L2 (one-wave workgroups)
};

constexpr bool geo_pairs(int g) { return g == kGeoPairLds || g == kGeoPairSmem || g == kGeoSphLds; }

// Every member starts null / 0: bind_scene sets the scene's members for the
// kernel's layout, the kernel the ones only it has.
struct SceneView {
    const float4* tri = nullptr;        // 3 float4 per triangle (single layout)
    const float4* pair = nullptr;       // kPairF4 float4 per triangle pair (pair layout)
    const float4* sph = nullptr;        // 1 float4 per sphere, BVH leaf order
    const float4* node = nullptr;       // 2 float4 per sphere-BVH node
    const uint32_t* sph_perm = nullptr; // leaf order -> sphere id (global memory)
    const uint4* tnode = nullptr;       // triangle BVH: 8 compact octant layouts of nTN nodes
    const float4* tsorted = nullptr;    // 3 float4 per triangle, BVH leaf order
    const uint32_t* tperm = nullptr;    // leaf order -> triangle id
    uint32_t nTN = 0;
    uint32_t nT = 0, nP = 0, nS = 0, nN = 0;
    const float4* clu = nullptr;        // box clusters, kCluF4 float4 each (kGeoPairClu)
    uint32_t nC = 0;
    uint32_t pair_free = 0;   // pairs in no cluster: tested by every lane
    uint32_t cam_mask = 0;    // wave-uniform: pairs the wave's camera rays can hit (rt_beam.hpp), free pairs included
    bool cam_avail = false;   // cam_mask was computed (a mask of 0 is a valid answer)
    uint32_t shd_mask = 0;    // wave-uniform: pairs that can occlude the wave's bounce-0 shadow rays (rt_shaft.hpp)
    uint32_t shd_cskip = 0;   // wave-uniform: box clusters none of whose faces is in shd_mask
    bool shd_avail = false;   // shd_mask was computed (a mask of 0: no shadow ray is occluded)
    const float* htab = nullptr;        // Halton low-digit tables in LDS (kGeoPairClu)
    const uint4* sent = nullptr;        // compact sphere BVH entries (the free-running kernel): 8 octant layouts, global
    const uint16_t* sid = nullptr;      // sphere id of each compact entry (leaves), global
    const uint4* sbox = nullptr;        // the sphere BVH with leaf boxes (kGeoSphLds): 8 layouts of nSB entries
    uint32_t nSB = 0;
    const float4* shade = nullptr;      // MIS shading records, 3 float4 per triangle (rt_mis.hip)
    float* xstash = nullptr;            // MIS: per-lane primary hit (p, din), SoA in LDS (rt_mis.hip)
};

// The scene tables of the path kernels' arguments (KParams keeps them flat).
__host__ __device__ __forceinline__ SceneTables tables_of(const KParams& P) {
    return SceneTables{P.tri_isect, P.pair_isect, P.clusters,   P.sph_isect, P.sph_nodes, P.sph_perm,
                       P.sph_box,   P.tri_nodes,  P.tri_sorted, P.tri_perm,  P.nT,        P.nP,
                       P.nS,        P.nN,         P.nTN,        P.nC,        P.pair_free};
}

constexpr bool geo_staged(int g) {
    return g == kGeoTriLds || g == kGeoPairLds || g == kGeoPairClu || g == kGeoSphLds;
}

// THE copy loop of every kernel: the workgroup's NT threads copy the layout's
// records to lds[0 ..) and the box clusters right after them (staged_f4,
// rt_kernel.hpp); nothing for the layouts whose records stay in global memory.
// No barrier: the kernel stages what only it has (Halton tables, MIS shading
// records, the sorted kernel's sums) and then synchronises once.
template <int GEO, uint32_t NT>
__device__ __forceinline__ void stage_records(float4* lds, const SceneTables& T) {
    const StagedF4<uint32_t> n = staged_f4(GEO, T.nT, T.nP, T.nC);
    const float4* src = GEO == kGeoTriLds ? T.tri_isect : T.pair_isect;
    for (uint32_t k = threadIdx.x; k < n.rec; k += NT) lds[k] = src[k];
    for (uint32_t k = threadIdx.x; k < n.clu; k += NT) lds[n.rec + k] = T.clusters[k];
}

// THE place that decides, per layout, where a kernel reads the scene from:
// tri / pair / clu in the staged records at `lds` (stage_records) or in global
// memory, and the BVH and sphere tables (always global memory, L2-resident).
template <int GEO, bool SPH>
__device__ __forceinline__ void bind_scene(SceneView& sv, const SceneTables& T, const float4* lds) {
    sv.nT = T.nT;
    sv.nP = T.nP;
    sv.nS = SPH ? T.nS : 0u;
    sv.tri = geo_staged(GEO) ? lds : T.tri_isect;
    sv.pair = geo_staged(GEO) ? lds : T.pair_isect;  // kGeoPairSmem: scalar loads from global memory
    if (GEO == kGeoPairClu) {
        sv.clu = lds + staged_f4(GEO, T.nT, T.nP, T.nC).rec;
        sv.nC = T.nC;
        sv.pair_free = T.pair_free;
    }
    sv.tnode = T.tri_nodes;
    sv.tsorted = T.tri_sorted;
    sv.tperm = T.tri_perm;
    sv.nTN = T.nTN;
    sv.node = T.sph_nodes;  // sphere BVH: scalar loads from global memory
    sv.sph = T.sph_isect;
    sv.nN = SPH ? T.nN : 0u;  // sphere walks: BVH nodes per layout
    sv.sph_perm = T.sph_perm;
    sv.sbox = T.sph_box;  // the leaf-box sphere BVH (kGeoSphLds)
    sv.nSB = T.nN;
}

// Per-ray data of the slab test.  1/d uses the 1-ulp hardware reciprocal: the
// node boxes carry the culling margin, so only speed depends on its rounding.
struct RayBox {
    f3 invd, oinv;
};

__device__ __forceinline__ RayBox ray_box(f3 o, f3 d) {
    RayBox r;
    r.invd = f3{safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z)};
    r.oinv = f3{o.x * r.invd.x, o.y * r.invd.y, o.z * r.invd.z};
    return r;
}

// Conservative ray/box overlap on (tmin, tmax): false only if no point of the
// padded box lies on the ray inside that range.
__device__ __forceinline__ bool node_hit(const float4& n0, const float4& n1, const RayBox& rb,
                                         float tmin, float tmax) {
    const float tx0 = fmaf(n0.x, rb.invd.x, -rb.oinv.x), tx1 = fmaf(n1.x, rb.invd.x, -rb.oinv.x);
    const float ty0 = fmaf(n0.y, rb.invd.y, -rb.oinv.y), ty1 = fmaf(n1.y, rb.invd.y, -rb.oinv.y);
    const float tz0 = fmaf(n0.z, rb.invd.z, -rb.oinv.z), tz1 = fmaf(n1.z, rb.invd.z, -rb.oinv.z);
    const float tnear = vmax3(vmin(tx0, tx1), vmin(ty0, ty1), vmax(vmin(tz0, tz1), tmin));
    const float tfar = vmin3(vmax(tx0, tx1), vmax(ty0, ty1), vmin(vmax(tz0, tz1), tmax));
    return tnear <= tfar;
}

// BVH layout of a ray direction: bit a set when component a is negative.
__device__ __forceinline__ uint32_t octant(f3 d) {
    return (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 31) << 1) |
           ((__float_as_uint(d.z) >> 31) << 2);
}

__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// v of lane src (wave-uniform): the query kernels of the caller's own rays run a
// copy of the wave's first in-domain ray on the lanes without one (rt_rays.hip)
__device__ __forceinline__ float lane_copy(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// Sphere-BVH walks over the 32-B nodes (the sphere scenes of the pair, single
// and global layouts; the sphere kernel walks the leaf-box BVH below).
// One stackless depth-first walk per lane through the escape-index tree of
// the ray's direction octant (near child first); a node is entered when the
// ray may hit its padded box.  Candidates are ranked by (t, sphere id) exactly
// like the oracle's id-ordered scan with strict '<', so the visiting order is
// free.
__device__ __forceinline__ void sphere_closest(const float4* __restrict__ node,
                                               const float4* __restrict__ sph,
                                               const uint32_t* __restrict__ perm, uint32_t nN,
                                               uint32_t nT, f3 o, f3 d, float tmin, float& best,
                                               int& id) {
    const float a = dot(d, d);
    const RayBox rb = ray_box(o, d);
    node += 2u * nN * octant(d);
    uint32_t idx = 0;
    while (idx < nN) {
        const float4 n0 = node[2 * idx], n1 = node[2 * idx + 1];
        uint32_t next = __float_as_uint(n0.w);
        if (node_hit(n0, n1, rb, tmin, best)) {
            const uint32_t leaf = __float_as_uint(n1.w);
            if (leaf == 0u) {
                next = idx + 1;
            } else {
                const uint32_t first = leaf & 0xFFFFFFu, end = first + (leaf >> 24);
                for (uint32_t k = first; k < end; ++k) {
                    float t;
                    if (sph_test(sph[k], o, d, a, tmin, 3.0e38f, &t) && t <= best) {
                        const int sid = (int)(nT + perm[k]);
                        if (t < best || sid < id) {
                            best = t;
                            id = sid;
                        }
                    }
                }
            }
        }
        idx = next;
    }
}

__device__ __forceinline__ bool sphere_any(const float4* __restrict__ node,
                                           const float4* __restrict__ sph, uint32_t nN, f3 o,
                                           f3 d, float tmin, float tmax) {
    const float a = dot(d, d);
    const RayBox rb = ray_box(o, d);
    node += 2u * nN * octant(d);
    uint32_t idx = 0;
    while (idx < nN) {
        const float4 n0 = node[2 * idx], n1 = node[2 * idx + 1];
        uint32_t next = __float_as_uint(n0.w);
        if (node_hit(n0, n1, rb, tmin, tmax)) {
            const uint32_t leaf = __float_as_uint(n1.w);
            if (leaf == 0u) {
                next = idx + 1;
            } else {
                const uint32_t first = leaf & 0xFFFFFFu, end = first + (leaf >> 24);
                for (uint32_t k = first; k < end; ++k) {
                    float t;
                    if (sph_test(sph[k], o, d, a, tmin, tmax, &t)) return true;
                }
            }
        }
        idx = next;
    }
    return false;
}

// Compact BVH entries (rt_scene.cpp build_sphere_lds, rt_lbvh.hip): 16 B per
// node, an fp16 box rounded outward (still conservative) and one word --
// escape | 2^31 for an inner node (the escape is an entry index over all
// layouts, so a walk's position names its layout); a sphere leaf stores the
// sphere (c, r*r) itself (a leaf's escape is the next entry).
__device__ __forceinline__ float h2f(uint32_t b16) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)b16);
}

__device__ __forceinline__ bool lds_node_hit(const uint4& e, const RayBox& rb, float tmin,
                                             float tmax) {
    const float4 n0 = make_float4(h2f(e.x & 0xFFFFu), h2f(e.x >> 16), h2f(e.y & 0xFFFFu), 0.0f);
    const float4 n1 = make_float4(h2f(e.y >> 16), h2f(e.z & 0xFFFFu), h2f(e.z >> 16), 0.0f);
    return node_hit(n0, n1, rb, tmin, tmax);
}

// Slab test of a near/far entry: in the layout of direction octant k the lo
// slots hold the planes a ray of that octant enters through.  Equal to
// lds_node_hit for such rays: fma(p, invd, -oinv) is monotone in p and
// sign(invd) orders the two planes of each axis, so the min/max pairs of
// node_hit select exactly these values.
__device__ __forceinline__ bool lds_node_hit_nf(const uint4& e, const RayBox& rb, float tmin,
                                                float tmax) {
    const float nx = fmaf(h2f(e.x & 0xFFFFu), rb.invd.x, -rb.oinv.x);
    const float ny = fmaf(h2f(e.x >> 16), rb.invd.y, -rb.oinv.y);
    const float nz = fmaf(h2f(e.y & 0xFFFFu), rb.invd.z, -rb.oinv.z);
    const float fx = fmaf(h2f(e.y >> 16), rb.invd.x, -rb.oinv.x);
    const float fy = fmaf(h2f(e.z & 0xFFFFu), rb.invd.y, -rb.oinv.y);
    const float fz = fmaf(h2f(e.z >> 16), rb.invd.z, -rb.oinv.z);
    return vmax3(nx, ny, vmax(nz, tmin)) <= vmin3(fx, fy, vmin(fz, tmax));
}

// One step of a lane's walk over near/far entries (tri_cbvh_walk;
// sphere_walk_box takes the same step) in select form: a leaf whose box is
// hit is parked in `leaf` (its word), a missed inner node is left by its
// escape index, everything else goes on to the next entry.
__device__ __forceinline__ void cbvh_step(const uint4* __restrict__ ent, uint32_t& idx, uint32_t& leaf,
                                          const RayBox& rb, float tmin, float best) {
    const uint4 e = ent[idx];
    const bool inner = (e.w & 0x80000000u) != 0u;
    const bool h = lds_node_hit_nf(e, rb, tmin, best);
    leaf = (h && !inner) ? e.w : leaf;
    idx = (h || !inner) ? idx + 1 : (e.w & 0x7FFFFFFFu);
}

// The free-running kernel (rt_free.hpp) walks the compact entries, where a
// leaf is the sphere itself, and tests the parked lanes' roots once they are
// >= 1/kSphParkDen of the walking lanes (config 4, a lockstep walk of the
// same entries: 2 157.3 ms, 4 158.4, 6 161.1; round 5: 3 149.7-149.8,
// 2 150.2-150.3, 1 207.4 -- 1/2 kept: with 1/3 the profiled HBM traffic rose
// from 69 to 110 MB)
#ifndef RT_SPH_PARK_DEN
#define RT_SPH_PARK_DEN 2
#endif
constexpr int kSphParkDen = RT_SPH_PARK_DEN;

// Per-lane walk of the sphere BVH with LEAF BOXES (rt_scene.cpp
// build_sphere_box), the walk of the sphere kernel: every entry is a near/far
// fp16 box -- a leaf's box is its padded sphere box, like any node's -- so
// every step of every lane is the same select-form box test (a lockstep walk
// of the compact entries ran the box test and the discriminant side by side
// whenever a wave held lanes at both kinds of entry, ~33 VALU a step; DESIGN.md
// §5).  After Aila & Laine's postponed leaf processing,
// in stackless form: a lane whose leaf box is hit parks the leaf; the parked
// lanes' spheres are tested with sph_test (the discriminant, then the IEEE
// roots) once they are >= 1/RT_SPH_BOX_PARK_DEN of the walkers, checked every
// RT_SPH_BOX_CHK steps (a lane that parks in between holds still).  Per lane
// the entries are visited in the same order whatever the other lanes do, and
// candidates are ranked by (t, sphere id) as in every walk:
// the brute-force answer.  ANY: id becomes >= 0 on the first accepted hit
// (and that lane stops).
// Config 4 (Msamples/s, profiles/r6/ab_results.md): the compact walk checked
// every step 3,512-3,520, every 6 steps 3,867-3,874; leaf boxes checked every
// 2 / 4 / 5 / 6 / 8 steps 3,883 / 4,018 / 4,027 / 4,042-4,044 / 4,037 with the
// roots at 1/3 (1/2 and 1/4 at every 6: 3,989 / 4,038); leaves of 2 / 3 / 4
// spheres 3,883 / 3,734 / 3,591
#ifndef RT_SPH_BOX_PARK_DEN
#define RT_SPH_BOX_PARK_DEN 3
#endif
#ifndef RT_SPH_BOX_CHK
#define RT_SPH_BOX_CHK 6
#endif
template <bool ANY>
__device__ __forceinline__ void sphere_walk_box(const uint4* __restrict__ ent, const float4* __restrict__ sph,
                                                const uint32_t* __restrict__ perm, uint32_t nN, uint32_t nT, f3 o,
                                                f3 d, float tmin, float& best, int& id) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const float a = dot(d, d);
    const RayBox rb = ray_box(o, d);
    uint32_t idx = octant(d) * nN;
    const uint32_t end = idx + nN;
    if (ANY && id >= 0) idx = end;
    uint32_t leaf = kNone;
    [[maybe_unused]] constexpr int ST = ANY ? 24 : 16;
    RT_STAT(ST, 1);
    RT_STAT(ST + 1, __popcll(__ballot(1)));
    for (;;) {
        for (;;) {
            if (__builtin_amdgcn_ballot_w64(idx < end && leaf == kNone) == 0) break;
#pragma unroll
            for (int q = 0; q < RT_SPH_BOX_CHK; ++q) {
                RT_STAT(ST + 2, 1);
                RT_STAT(ST + 3, __popcll(__builtin_amdgcn_ballot_w64(idx < end && leaf == kNone)));
                if (idx < end && leaf == kNone) {  // cbvh_step, spelled out: the call compiles to other code here
                    const uint4 e = ent[idx];
                    const bool inner = (e.w & 0x80000000u) != 0u;
                    const bool h = lds_node_hit_nf(e, rb, tmin, best);
                    leaf = (h && !inner) ? e.w : leaf;
                    idx = (h || !inner) ? idx + 1 : (e.w & 0x7FFFFFFFu);
                }
            }
            const int parked = __popcll(__builtin_amdgcn_ballot_w64(leaf != kNone));
            const int live = __popcll(__builtin_amdgcn_ballot_w64(idx < end || leaf != kNone));
            if (RT_SPH_BOX_PARK_DEN * parked >= live) break;
        }
        if (__builtin_amdgcn_ballot_w64(leaf != kNone) == 0) break;
        RT_STAT(ST + 5, 1);
        RT_STAT(ST + 6, __popcll(__builtin_amdgcn_ballot_w64(leaf != kNone)));
        if (leaf != kNone) {  // the parked leaf's spheres (shaders_old.metal:108-136)
            const uint32_t first = leaf & 0xFFFFFFu, cnt = (leaf >> 24) + 1u;
            for (uint32_t k = first; k < first + cnt; ++k) {
                float t;
                if (ANY) {
                    if (sph_test(sph[k], o, d, a, tmin, best, &t)) {
                        id = 0;
                        idx = end;
                        break;
                    }
                } else if (sph_test(sph[k], o, d, a, tmin, 3.0e38f, &t) && t <= best) {
                    const int s = (int)(nT + perm[k]);
                    if (t < best || s < id) {
                        best = t;
                        id = s;
                    }
                }
            }
            leaf = kNone;
        }
    }
}

// Triangle-BVH walks over the compact entries (rt_scene.cpp build_tri_sah or
// rt_lbvh.hip, rt_gsah.hip: 16 B per node, fp16 near/far boxes rounded
// outward, one layout per direction octant, near child first): stackless
// depth-first walks with conservative boxes and (t, id) ranking (DESIGN.md
// §3.10).  A per-lane walk is in its own octant's layout and tests near/far
// (lds_node_hit_nf); the wave-packet walks below use the lane-0 layout for
// every lane and the min/max test, which does not depend on the slot order.

// A leaf of the triangle BVH: up to 128 consecutive triangles in leaf order,
// word = first | (count - 1) << 24 (build_tri_sah makes leaves of up to
// RTPT_TRI_LEAF; the LBVH leaves hold one).  Every triangle is tested with
// the exact test and ranked by (t, id).
__device__ __forceinline__ void tri_leaf_closest(const float4* __restrict__ tri, const uint32_t* __restrict__ perm,
                                                 uint32_t w, f3 o, f3 d, float tmin, float& best, int& id) {
    const uint32_t first = w & 0xFFFFFFu, cnt = (w >> 24) + 1u;
    for (uint32_t k = first; k < first + cnt; ++k) {
        float t;
        if (tri_test(tri[3 * k], tri[3 * k + 1], tri[3 * k + 2], o, d, tmin, 3.0e38f, &t) && t <= best) {
            const int tid = (int)perm[k];
            if (t < best || tid < id) {
                best = t;
                id = tid;
            }
        }
    }
}
__device__ __forceinline__ bool tri_leaf_any(const float4* __restrict__ tri, uint32_t w, f3 o, f3 d, float tmin,
                                             float tmax) {
    const uint32_t first = w & 0xFFFFFFu, cnt = (w >> 24) + 1u;
    bool found = false;
    for (uint32_t k = first; k < first + cnt && !found; ++k) {
        float t;
        found = tri_test(tri[3 * k], tri[3 * k + 1], tri[3 * k + 2], o, d, tmin, tmax, &t);
    }
    return found;
}

// Wave-packet walks for the coherent camera rays and bounce-0 shadow rays: the
// wave walks ONE path (the layout of its first lane's octant) and enters a node
// when any lane's box test passes; the node index is wave uniform.  A lane whose
// own test failed still tests the leaf's triangle, which cannot change its result.
__device__ __forceinline__ void tri_cbvh_closest_packet(const uint4* __restrict__ cn,
                                                        const float4* __restrict__ tri,
                                                        const uint32_t* __restrict__ perm, uint32_t nN,
                                                        f3 o, f3 d, float tmin, float& best, int& id) {
    const RayBox rb = ray_box(o, d);
    uint32_t idx = wave_uniform(octant(d)) * nN;
    const uint32_t end = idx + nN;
    RT_STAT(23, 1);  // packet walks (camera and bounce-0 shadow rays)
    while (idx < end) {
        RT_STAT(31, 1);
        const uint4 e = cn[idx];
        const bool inner = (e.w & 0x80000000u) != 0u;  // wave-uniform
        const bool h = lds_node_hit(e, rb, tmin, best);
        uint32_t next = idx + 1;
        if (__builtin_amdgcn_ballot_w64(h) == 0) {
            if (inner) next = e.w & 0x7FFFFFFFu;
        } else if (!inner) {
            tri_leaf_closest(tri, perm, e.w, o, d, tmin, best, id);
        }
        idx = wave_uniform(next);
    }
}

__device__ __forceinline__ bool tri_cbvh_any_packet(const uint4* __restrict__ cn,
                                                    const float4* __restrict__ tri, uint32_t nN, f3 o,
                                                    f3 d, float tmin, float tmax) {
    const RayBox rb = ray_box(o, d);
    uint32_t idx = wave_uniform(octant(d)) * nN;
    const uint32_t end = idx + nN;
    bool found = false;
    RT_STAT(23, 1);  // packet walks (camera and bounce-0 shadow rays)
    while (idx < end) {
        RT_STAT(31, 1);
        const uint4 e = cn[idx];
        const bool inner = (e.w & 0x80000000u) != 0u;
        const bool h = !found && lds_node_hit(e, rb, tmin, tmax);
        uint32_t next = idx + 1;
        if (__builtin_amdgcn_ballot_w64(h) == 0) {
            if (inner) next = e.w & 0x7FFFFFFFu;
        } else if (!inner) {
            found = found || tri_leaf_any(tri, e.w, o, d, tmin, tmax);
            if (__builtin_amdgcn_ballot_w64(!found) == 0) break;
        }
        idx = wave_uniform(next);
    }
    return found;
}

// Per-lane compact-BVH walks with POSTPONED LEAVES (as sphere_walk_box parks
// its leaves): a lane whose box test passes at a leaf parks the leaf and
// stops; the others walk on until at least 1/kTriParkDen of the lanes
// still walking are parked, then the wave runs the triangle tests of all
// parked lanes together -- instead of every mixed step paying for the box
// test AND the three record loads and the test of a triangle.  Per lane the
// entries are visited in the same order and ranked by (t, id): the same result.
// the parked leaves are tested once they are >= 1/kTriParkDen of the live lanes
// (100k triangles: 1/4 738, 1/2 701, 3/4 570, 1/8 707 Msamples/s; round 5 with
// near/far boxes: 1/3 894-896, 1/4 887-890, 1/2 872, 1/6 865, 1/8 843; round 6
// with select-form steps checked every 4: 1/4 1,115, 1/3 1,111, 1/2 1,078)
#ifndef RT_TRI_PARK_DEN
#define RT_TRI_PARK_DEN 4
#endif
constexpr int kTriParkDen = RT_TRI_PARK_DEN;
// The step's outcome comes by selects (cbvh_step: no exec-mask branches around
// the box test); RT_TRI_CHK: steps between two checks of the parking condition
// (the two ballots, popcounts and compares of the check are a third of a
// step's instructions; a lane that parks in between holds still).  Round 6,
// 100k triangles (Msamples/s): branch form, check every step 988-990;
// selects 1,029; check every 2 steps 1,068; both: every 2 / 3 / 4 / 6 / 8
// steps 1,082-1,093 / 1,103 / 1,111 / 1,109 / 1,086 (profiles/r6/ab_results.md).
// The next sequential entry requested one step early: 888 -> 787 (4 more
// VGPRs, 20 spilled).
#ifndef RT_TRI_CHK
#define RT_TRI_CHK 4
#endif
template <bool ANY>
__device__ __forceinline__ void tri_cbvh_walk(const uint4* __restrict__ cn, const float4* __restrict__ tri,
                                              const uint32_t* __restrict__ perm, uint32_t nN, f3 o, f3 d,
                                              float tmin, float& best, int& id) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const RayBox rb = ray_box(o, d);
    uint32_t idx = octant(d) * nN;
    const uint32_t end = idx + nN;
    if (ANY && id >= 0) idx = end;
    uint32_t leaf = kNone;
    [[maybe_unused]] constexpr int ST = ANY ? 24 : 16;  // the slots of sphere_walk_box (no spheres here)
    RT_STAT(ST, 1);
    RT_STAT(ST + 1, __popcll(__ballot(1)));
    for (;;) {
        for (;;) {
            const bool adv = idx < end && leaf == kNone;
            if (__builtin_amdgcn_ballot_w64(adv) == 0) break;
            RT_STAT(ST + 2, 1);
            RT_STAT(ST + 3, __popcll(__builtin_amdgcn_ballot_w64(adv)));
            if (adv) cbvh_step(cn, idx, leaf, rb, tmin, best);
            // more steps before the next check (a parked lane holds still)
#pragma unroll
            for (int q = 1; q < RT_TRI_CHK; ++q) {
                RT_STAT(ST + 2, 1);
                RT_STAT(ST + 3, __popcll(__builtin_amdgcn_ballot_w64(idx < end && leaf == kNone)));
                if (idx < end && leaf == kNone) cbvh_step(cn, idx, leaf, rb, tmin, best);
            }
            const int parked = __popcll(__builtin_amdgcn_ballot_w64(leaf != kNone));
            const int live = __popcll(__builtin_amdgcn_ballot_w64(idx < end || leaf != kNone));
            if (kTriParkDen * parked >= live) break;
        }
        if (__builtin_amdgcn_ballot_w64(leaf != kNone) == 0) break;
        RT_STAT(ST + 5, 1);
        RT_STAT(ST + 6, __popcll(__builtin_amdgcn_ballot_w64(leaf != kNone)));
        if (leaf != kNone) {
            if (ANY) {
                if (tri_leaf_any(tri, leaf, o, d, tmin, best)) {
                    id = 0;
                    idx = end;
                }
            } else {
                tri_leaf_closest(tri, perm, leaf, o, d, tmin, best, id);
            }
            leaf = kNone;
        }
    }
}

// ---- box clusters ------------------------------------------
// Candidate pairs of one ray among the clustered pairs: bit k set when pair k
// can hold an accepted hit with t in (tmin, tmax).  Per cluster: slab test of
// the padded box along its three axes ([Tlo, Thi], widened by a relative
// slack for the approximate rcp arithmetic), then a face is a candidate when
// its plane's interval [t_plane -/+ w] meets [Tlo, Thi] — in a box that is the
// face the ray enters through and the one it leaves through (two or three more
// near an edge or corner).  Only speed depends on the rounding here.
// SEG (shadow any-hit): a container cluster (flags bit 3: all axes world axes,
// a box with volume, e.g. the room) is skipped for the whole wave when every
// lane's segment [o, o + d*tmax] lies inside the box shrunk to more than the
// normal tolerance from each face plane: the box is convex, so the segment
// stays away from every face and no face can accept a hit.  The shrunk box
// is precomputed on the host into the container's unused axis slots.
// ALLOW (the bounce-0 shadow query): clusters in the wave-uniform set cskip
// hold no pair of the wave's occluder mask and are skipped before their slab
// terms are formed, the container check with them.
// OWN (RT_CLU_LEAN; the shadow queries of shade(): tmax = dist - 1e-3 to a
// point drawn on the light): the light's own cluster (kCluOwnLight) is passed
// over, its pairs' exact test gives t >= tmax.
template <bool SEG = false, bool ALLOW = false, bool OWN = false>
__device__ __forceinline__ uint32_t cluster_candidates(const SceneView& sv, f3 o, f3 d, float tmin,
                                                       float tmax, uint32_t cskip = 0u) {
    constexpr float kEps = 1.52587890625e-05f;  // 2^-16 relative slack
    // containers the whole wave's segments stay inside (wave-uniform bit mask),
    // decided before the slab terms are live
    uint32_t skip = 0;
    if (SEG) {
        const f3 e = o + d * tmax;
        for (uint32_t c = 0; c < sv.nC; ++c) {
            if (ALLOW && ((cskip >> c) & 1u)) continue;
            const float4* r = sv.clu + kCluF4 * c;
            if (!(__float_as_uint(r[3].w) & 8u)) continue;
            // the shrunk box (rt_scene.cpp): face plane + tol_seg, with a 2^-20
            // relative slack for the rounding of o + d*tmax and of the bounds
            const float4 X = r[0], Y = r[1], Z = r[2];
            const bool inside = o.x > X.x && o.x < X.y && e.x > X.x && e.x < X.y &&
                                o.y > Y.x && o.y < Y.y && e.y > Y.x && e.y < Y.y &&
                                o.z > Z.x && o.z < Z.y && e.z > Z.x && e.z < Z.y;
            if (__builtin_amdgcn_ballot_w64(!inside) == 0) skip |= 1u << c;
        }
    }
    // per-ray terms of world-aligned box axes: t = lo * invd - o * invd
    const RayBox rb = ray_box(o, d);
    const float iv[3] = {rb.invd.x, rb.invd.y, rb.invd.z};
    const float oi[3] = {rb.oinv.x, rb.oinv.y, rb.oinv.z};
    uint32_t mask = 0;
    uint32_t c = 0;
    for (; c < sv.nC; ++c) {
        const float4* r = sv.clu + kCluF4 * c;
        if (ALLOW && ((cskip >> c) & 1u)) {
            if (__float_as_uint(r[3].w) & 16u) break;  // single-face clusters come last
            continue;
        }
        if (SEG && ((skip >> c) & 1u)) continue;
        const float4 H = r[3], W = r[6];
        const float4 M0 = r[4], M1 = r[5];
        const uint32_t flags = __float_as_uint(H.w);
        if (flags & 16u) break;  // single-face clusters come last (rt_scene.cpp)
#if RT_CLU_LEAN
        // the slab of rt_cluorder.hpp: the same terms, and the turned boxes' lean ones
        const float wf[3] = {W.x, W.y, W.z};
        float en[3], ex[3], ida[3], tlo, thi;
        clu_slab(r, flags, iv, oi, o, d, tmin, tmax, en, ex, ida, &tlo, &thi);
#else
        const float hi[3] = {H.x, H.y, H.z}, wf[3] = {W.x, W.y, W.z};
        float en[3], ex[3], ida[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float4 A = r[a];
            float t0, t1;
            if (flags & (1u << a)) {  // wave-uniform
                ida[a] = iv[a];
                t0 = fmaf(A.w, iv[a], -oi[a]);
                t1 = fmaf(hi[a], iv[a], -oi[a]);
            } else {
                const float oa = dot(f3{A.x, A.y, A.z}, o), da = dot(f3{A.x, A.y, A.z}, d);
                ida[a] = safe_rcp(da);
                t0 = (A.w - oa) * ida[a];
                t1 = (hi[a] - oa) * ida[a];
            }
            en[a] = vmin(t0, t1);
            ex[a] = vmax(t0, t1);
        }
        const float tlo0 = vmax3(en[0], en[1], vmax(en[2], tmin));
        const float thi0 = vmin3(ex[0], ex[1], vmin(ex[2], tmax));
        const float tlo = fmaf(-kEps, fabsf(tlo0), tlo0), thi = fmaf(kEps, fabsf(thi0), thi0);  // kEps*|x| is exact: the same values
#endif
        if (!__builtin_amdgcn_ballot_w64(tlo <= thi)) continue;  // no lane meets the box
        const uint32_t m[6] = {__float_as_uint(M0.x), __float_as_uint(M0.y), __float_as_uint(M0.z),
                               __float_as_uint(M0.w), __float_as_uint(M1.x), __float_as_uint(M1.y)};
        uint32_t cm = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // a ray with d_a >= 0 enters through the low face (slot 2a) and
            // leaves through the high one (2a + 1); the face plane lies
            // wf * |1/d_a| inside the padded slab, +- the tolerance
            const bool neg = ida[a] < 0.0f;
            const uint32_t m_en = neg ? m[2 * a + 1] : m[2 * a];
            const uint32_t m_ex = neg ? m[2 * a] : m[2 * a + 1];
            const float wa = wf[a] * fabsf(ida[a]);
            cm |= (en[a] + fmaf(fabsf(en[a]), kEps, wa) >= tlo) ? m_en : 0u;
            cm |= (ex[a] - fmaf(fabsf(ex[a]), kEps, wa) <= thi) ? m_ex : 0u;
        }
        mask |= (tlo <= thi) ? cm : 0u;
    }
    // single-face clusters (the light, lone rectangles): the face is a
    // candidate whenever the padded box is hit (a superset of its face test)
    for (; c < sv.nC; ++c) {
        if (ALLOW && ((cskip >> c) & 1u)) continue;
        const float4* r = sv.clu + kCluF4 * c;
        const float4 A0 = r[0], A1 = r[1], A2 = r[2], H = r[3];
        const uint32_t flags = __float_as_uint(H.w);
#if RT_CLU_LEAN
        if (OWN && kLeanOwnLight && (flags & kCluOwnLight)) break;  // wave-uniform; these come last (rt_scene.cpp)
#endif
        const float4 A[3] = {A0, A1, A2};
        const float hi[3] = {H.x, H.y, H.z};
        float tlo0 = tmin, thi0 = tmax;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float t0, t1;
            if (flags & (1u << a)) {  // wave-uniform
                t0 = fmaf(A[a].w, iv[a], -oi[a]);
                t1 = fmaf(hi[a], iv[a], -oi[a]);
            } else {
                const float oa = dot(f3{A[a].x, A[a].y, A[a].z}, o);
                const float ida = safe_rcp(dot(f3{A[a].x, A[a].y, A[a].z}, d));
                t0 = (A[a].w - oa) * ida;
                t1 = (hi[a] - oa) * ida;
            }
            tlo0 = vmax(tlo0, vmin(t0, t1));
            thi0 = vmin(thi0, vmax(t0, t1));
        }
        const float tlo = fmaf(-kEps, fabsf(tlo0), tlo0), thi = fmaf(kEps, fabsf(thi0), thi0);  // kEps*|x| is exact: the same values
        mask |= (tlo <= thi) ? __float_as_uint(r[5].z) : 0u;
    }
    return mask;
}

// The same filter (no SEG, no ALLOW) with the candidates split for an ordered
// closest query (rt_cluorder.hpp): near | far is the mask
// above; finished, i.e. disjoint and with the far set promoted where nothing
// is near.
__device__ __forceinline__ CluSplit cluster_candidates_split(const SceneView& sv, f3 o, f3 d, float tmin,
                                                             float tmax) {
    const RayBox rb = ray_box(o, d);
    const float iv[3] = {rb.invd.x, rb.invd.y, rb.invd.z};
    const float oi[3] = {rb.oinv.x, rb.oinv.y, rb.oinv.z};
    CluSplit s = clu_split_init();
    uint32_t c = 0;
    for (; c < sv.nC; ++c) {
        const float4* r = sv.clu + kCluF4 * c;
        const uint32_t flags = __float_as_uint(r[3].w);
        if (flags & 16u) break;  // single-face clusters come last (rt_scene.cpp)
#if RT_CLU_LEAN
        // a container every lane of the wave starts inside (the room, seen from
        // a surface in it): the exit side alone; one lane outside its shrunk
        // box, and the wave takes the full filter
        if (kLeanExit && (flags & kCluInside) &&
            __builtin_amdgcn_ballot_w64(!clu_origin_inside(r, o)) == 0) {
            clu_container_exit(r, iv, oi, tmax, &s);
            continue;
        }
#endif
        float en[3], ex[3], ida[3], tlo, thi;
        clu_slab(r, flags, iv, oi, o, d, tmin, tmax, en, ex, ida, &tlo, &thi);
        if (!__builtin_amdgcn_ballot_w64(tlo <= thi)) continue;  // no lane meets the box
        clu_faces_split(r, flags, en, ex, ida, tlo, thi, &s);
    }
    for (; c < sv.nC; ++c) {
        const float4* r = sv.clu + kCluF4 * c;
        clu_single_split(r, __float_as_uint(r[3].w), iv, oi, o, d, tmin, tmax, &s);
    }
    clu_split_finish(&s);
    return s;
}

// Exact pair test (the same arithmetic as the brute-force loops) with the
// hit ranked lexicographically by (t, triangle id): pairs are visited out of
// id order here, and (t, id) order is what the id-ordered scan with strict
// '<' computes.  ANY = shadow any-hit: *id becomes >= 0 on any accepted hit.
template <bool ANY>
__device__ __forceinline__ void pair_test_rank(const float4* r, uint32_t k, f3 o, f3 d, float tmin,
                                               float* best, int* id) {
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    const PairDots q = pair_dots(r0, r1, r2, r3, r4, o, d);
    const bool pa = bary_ok(q.denA, q.a1, q.a2);
    const bool pb = bary_ok(q.denB, q.b1, q.b2);
    if (pa || pb) {
        const f3 nsel = pa ? f3{r2.y, r2.z, r2.w} : f3{r3.w, r4.x, r4.y};
        const float t = pair_t(nsel, q.tv, pa ? q.denA : q.denB);
        const int ia = (int)(pa ? 2 * k : 2 * k + 1);
        if (t > tmin && (t < *best || (!ANY && t == *best && ia < *id))) {
            if (!ANY) *best = t;
            *id = ia;
        }
        if (pa && pb) {
            const float t2 = pair_t(f3{r3.w, r4.x, r4.y}, q.tv, q.denB);
            const int ib = (int)(2 * k + 1);
            if (t2 > tmin && (t2 < *best || (!ANY && t2 == *best && ib < *id))) {
                if (!ANY) *best = t2;
                *id = ib;
            }
        }
    }
}

// Closest hit / any hit over the pair records with box clusters: the
// unclustered pairs by every lane (wave-uniform records, LDS broadcast), then
// each lane's own candidate pairs (per-lane LDS reads).  For ANY, *best is
// tmax and is not changed.
// SEG: skip containers the wave's segments [o, o + d*tmax] stay inside (any
// hit, and the MIS light queries: closest hits that only matter up to tmax).
// ALLOW (the bounce-0 shadow query): only the pairs of the
// wave-uniform mask sv.shd_mask are tested, free pairs included.
// ORDER (the closest queries of bounce >= 1 in the box-cluster kernel,
// DESIGN.md §3.18): the candidates come split (rt_cluorder.hpp); the rounds run
// over each lane's near set, then over its far set where a far candidate can
// still win against the best found.  Most waves then end after one round,
// where one lane that met a box's padded slab used to hold the whole wave for
// the box's exit face and the wall behind it.  (t, id) ranking makes the
// visiting order free, and a culled pair holds no hit with t <= best.
// OWN: cluster_candidates<.., OWN> (the shadow queries of shade()).
template <bool ANY, bool SEG = ANY, bool ALLOW = false, bool ORDER = false, bool OWN = false>
__device__ __forceinline__ void cluster_query(const SceneView& sv, f3 o, f3 d, float tmin,
                                              float* best, int* id) {
    static_assert(!ORDER || (!ANY && !SEG && !ALLOW), "the ordered form is the plain closest query");
    [[maybe_unused]] constexpr int ST = ANY ? 36 : 32;  // RT_STATS: shadow / closest queries apart
    for (uint32_t free = ALLOW ? (sv.pair_free & sv.shd_mask) : sv.pair_free; free != 0u; free &= free - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(free);
        pair_test_rank<ANY>(sv.pair + kPairF4 * k, k, o, d, tmin, best, id);
    }
    uint32_t cand, far = 0u;
    [[maybe_unused]] float far_lo = 0.0f;
    if constexpr (ORDER) {
        const CluSplit s = cluster_candidates_split(sv, o, d, tmin, *best);
        cand = s.near;
        far = s.far;
        far_lo = s.far_lo;
    } else {
        cand = cluster_candidates<SEG, ALLOW, OWN>(sv, o, d, tmin, *best, ALLOW ? sv.shd_cskip : 0u);
        if (ALLOW) cand &= sv.shd_mask;
    }
    RT_STAT(12, 1);
    RT_STAT(15, __popcll(__ballot(1)));
    RT_STAT(ST, 1);
    RT_STAT(ST + 3, __popcll(__ballot(1)));
    while (cand != 0u && !(ANY && *id >= 0)) {
        RT_STAT(13, 1);
        RT_STAT(14, __popcll(__ballot(1)));
        RT_STAT(ST + 1, 1);
        RT_STAT(ST + 2, __popcll(__ballot(1)));
        const uint32_t k = (uint32_t)__builtin_ctz(cand);
        cand &= cand - 1u;
        pair_test_rank<ANY>(sv.pair + kPairF4 * k, k, o, d, tmin, best, id);
    }
    if constexpr (ORDER) {
        far = clu_far_needed(far_lo, *best) ? far : 0u;
        while (far != 0u) {
            RT_STAT(13, 1);
            RT_STAT(14, __popcll(__ballot(1)));
            RT_STAT(ST + 1, 1);
            RT_STAT(ST + 2, __popcll(__ballot(1)));
            const uint32_t k = (uint32_t)__builtin_ctz(far);
            far &= far - 1u;
            pair_test_rank<false>(sv.pair + kPairF4 * k, k, o, d, tmin, best, id);
        }
    }
}

// closest hit, accept_any_intersection(false) (raytrace.metal:48-49).
// Primitives are tested in id order; a strictly smaller t wins (ties keep the
// lower id), exactly as the oracle.
// With CULL (used for coherent camera rays) a pair is skipped when no lane's
// box around its current candidate segment [o, o + d*best] touches the pair's
// padded AABB: any hit that could still win has t < best and lies inside it.
template <int GEO, bool SPH, bool CULL, int QT = 0>
__device__ __forceinline__ int closest_hit(const SceneView& sv, f3& o, f3& d, float tmin,
                                           float* t_io) {
    float best = *t_io;
    int id = -1;
    if (GEO == kGeoPairClu) {
        if (RT_CAM_CAND && CULL && sv.cam_avail) {
            // camera rays: the wave's candidate pairs, the same for every lane
            // and sample (scalar k: same-address LDS reads); (t, id) ranking
            // makes the visiting order free
            for (uint32_t m = sv.cam_mask; m != 0u; m &= m - 1u) {
                const uint32_t k = (uint32_t)__builtin_ctz(m);
                RT_STAT(13, 1);
                RT_STAT(14, __popcll(__ballot(1)));
                pair_test_rank<false>(sv.pair + kPairF4 * k, k, o, d, tmin, &best, &id);
            }
        } else {
            cluster_query<false, false, false, RT_CLU_ORDER != 0>(sv, o, d, tmin, &best, &id);
        }
    } else if (geo_pairs(GEO)) {
        f3 seg_lo, seg_hi;
        if (CULL) {
            const f3 e = o + d * best;
            seg_lo = f3{fminf(o.x, e.x), fminf(o.y, e.y), fminf(o.z, e.z)};
            seg_hi = f3{fmaxf(o.x, e.x), fmaxf(o.y, e.y), fmaxf(o.z, e.z)};
        }
        for (uint32_t k = 0; k < sv.nP; ++k) {
            const float4* r = sv.pair + kPairF4 * k;
            RT_STAT(4 * QT, 1);
            if (CULL) {
                const float4 b0 = r[5], b1 = r[6];
                const bool overlap = seg_lo.x <= b0.w && seg_hi.x >= b0.x && seg_lo.y <= b1.x &&
                                     seg_hi.y >= b0.y && seg_lo.z <= b1.y && seg_hi.z >= b0.z;
                if (!__any(overlap)) continue;
            }
            RT_STAT(4 * QT + 1, 1);
            RT_STAT(4 * QT + 2, __popcll(__ballot(1)));
            const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
            const PairDots q = pair_dots(r0, r1, r2, r3, r4, o, d);
            const bool pa = bary_ok(q.denA, q.a1, q.a2);
            const bool pb = bary_ok(q.denB, q.b1, q.b2);
            if (pa || pb) {
                RT_STAT(4 * QT + 3, 1);
                // One division for whichever of A, B the ray passes (A first);
                // a ray on the shared edge passes both and also runs B after.
                const f3 nsel = pa ? f3{r2.y, r2.z, r2.w} : f3{r3.w, r4.x, r4.y};
                const float t = pair_t(nsel, q.tv, pa ? q.denA : q.denB);
                if (t > tmin && t < best) {
                    best = t;
                    id = (int)(pa ? 2 * k : 2 * k + 1);
                }
                if (pa && pb) {
                    const float t2 = pair_t(f3{r3.w, r4.x, r4.y}, q.tv, q.denB);
                    if (t2 > tmin && t2 < best) {
                        best = t2;
                        id = (int)(2 * k + 1);
                    }
                }
                if (CULL) {
                    const f3 e = o + d * best;
                    seg_lo = f3{fminf(o.x, e.x), fminf(o.y, e.y), fminf(o.z, e.z)};
                    seg_hi = f3{fmaxf(o.x, e.x), fmaxf(o.y, e.y), fmaxf(o.z, e.z)};
                }
            }
        }
    } else if (GEO == kGeoTriBvh) {
        // camera rays: wave packets; bounce rays: per-lane walks with parked leaves
        if (CULL)
            tri_cbvh_closest_packet(sv.tnode, sv.tsorted, sv.tperm, sv.nTN, o, d, tmin,
                                    best, id);
        else
            tri_cbvh_walk<false>(sv.tnode, sv.tsorted, sv.tperm, sv.nTN, o, d, tmin,
                                 best, id);
    } else {
        for (uint32_t k = 0; k < sv.nT; ++k) {
            float t;
            if (tri_test(sv.tri[3 * k], sv.tri[3 * k + 1], sv.tri[3 * k + 2], o, d, tmin, best,
                         &t)) {
                best = t;
                id = (int)k;
            }
        }
    }
    if (SPH && GEO == kGeoSphLds)
        sphere_walk_box<false>(sv.sbox, sv.sph, sv.sph_perm, sv.nSB, sv.nT, o, d, tmin, best, id);
    else if (SPH)
        sphere_closest(sv.node, sv.sph, sv.sph_perm, sv.nN, sv.nT, o, d, tmin, best, id);
    *t_io = best;
    return id;
}

// any hit, accept_any_intersection(true) (raytrace.metal:79-85).  The boolean
// result does not depend on the order of the tests.
// seg_lo/seg_hi bound every point the ray can accept (t in (tmin, tmax)); a
// pair whose padded AABB no lane's segment box touches cannot be hit by any
// lane of the wave and is skipped as a whole.
template <int GEO, bool SPH, bool PACKET>
__device__ __forceinline__ bool any_hit(const SceneView& sv, f3& o, f3& d, float tmin, float tmax,
                                        f3 seg_lo, f3 seg_hi) {
    if (GEO == kGeoPairClu) {
        float tm = tmax;
        int id = -1;
        if (RT_SHD_CAND && RT_CAM_CAND && PACKET && sv.shd_avail) {
            // bounce-0 shadow rays: the wave's occluder mask (rt_shaft.hpp);
            // the boolean does not depend on which non-occluders are skipped
            if (sv.shd_mask == 0u) return false;
            if (RT_SHD_SHORT > 0 && __builtin_popcount(sv.shd_mask) <= RT_SHD_SHORT) {
                // a short mask (wave-uniform): its pairs tested directly on every
                // lane, scalar k and same-address LDS reads, in place of the
                // cluster filter that could only drop some of them; a lane
                // stops at its first accepted hit
                for (uint32_t m = sv.shd_mask; m != 0u && id < 0; m &= m - 1u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(m);
                    pair_test_rank<true>(sv.pair + kPairF4 * k, k, o, d, tmin, &tm, &id);
                }
                return id >= 0;
            }
            cluster_query<true, true, true>(sv, o, d, tmin, &tm, &id);
        } else {
            cluster_query<true, true, false, false, RT_CLU_LEAN != 0>(sv, o, d, tmin, &tm, &id);
        }
        if (id >= 0) return true;
    } else if (geo_pairs(GEO)) {
        for (uint32_t k = 0; k < sv.nP; ++k) {
            const float4* r = sv.pair + kPairF4 * k;
            const float4 b0 = r[5], b1 = r[6];
            const bool overlap = seg_lo.x <= b0.w && seg_hi.x >= b0.x && seg_lo.y <= b1.x &&
                                 seg_hi.y >= b0.y && seg_lo.z <= b1.y && seg_hi.z >= b0.z;
            RT_STAT(8, 1);
            if (!__any(overlap)) continue;
            RT_STAT(9, 1);
            RT_STAT(10, __popcll(__ballot(1)));
            const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
            const PairDots q = pair_dots(r0, r1, r2, r3, r4, o, d);
            const bool pa = bary_ok(q.denA, q.a1, q.a2);
            const bool pb = bary_ok(q.denB, q.b1, q.b2);
            if (pa || pb) {
                RT_STAT(11, 1);
                const f3 nsel = pa ? f3{r2.y, r2.z, r2.w} : f3{r3.w, r4.x, r4.y};
                const float t = pair_t(nsel, q.tv, pa ? q.denA : q.denB);
                if (t > tmin && t < tmax) return true;
                if (pa && pb) {
                    const float t2 = pair_t(f3{r3.w, r4.x, r4.y}, q.tv, q.denB);
                    if (t2 > tmin && t2 < tmax) return true;
                }
            }
        }
    } else if (GEO == kGeoTriBvh) {
        if (PACKET) {  // bounce-0 shadow rays: wave packets
            if (tri_cbvh_any_packet(sv.tnode, sv.tsorted, sv.nTN, o, d, tmin, tmax))
                return true;
        } else {
            float tm = tmax;
            int hid = -1;
            tri_cbvh_walk<true>(sv.tnode, sv.tsorted, sv.tperm, sv.nTN, o, d, tmin,
                                tm, hid);
            if (hid >= 0) return true;
        }
    } else {
        for (uint32_t k = 0; k < sv.nT; ++k) {
            float t;
            if (tri_test(sv.tri[3 * k], sv.tri[3 * k + 1], sv.tri[3 * k + 2], o, d, tmin, tmax,
                         &t))
                return true;
        }
    }
    if (SPH && GEO == kGeoSphLds) {
        float tm = tmax;
        int id = -1;
        sphere_walk_box<true>(sv.sbox, sv.sph, sv.sph_perm, sv.nSB, sv.nT, o, d, tmin, tm, id);
        return id >= 0;
    }
    if (SPH) return sphere_any(sv.node, sv.sph, sv.nN, o, d, tmin, tmax);
    return false;
}

// Fused queries of one bounce (pair layout, triangles only): the shadow any-hit
// of bounce b from p toward the light sample, and the closest hit of bounce
// b+1 from the same p along the new direction d2.  Both are evaluated pair by
// pair over ONE load of each record; every lane's two results are exactly
// those of any_hit and closest_hit (same tests, same order, same culling rule
// for the shadow segment), so the path's arithmetic is unchanged.
struct FusedHit {
    bool occluded;
    int id;     // closest hit of (p, d2), -1 if none
    float t;
};

__device__ __forceinline__ FusedHit fused_shadow_closest(const SceneView& sv, f3 p, f3 L,
                                                         float smax, f3 seg_lo, f3 seg_hi,
                                                         f3 d2) {
    FusedHit h{false, -1, 1000.0f};  // max_distance (sampling.metal:155)
    for (uint32_t k = 0; k < sv.nP; ++k) {
        const float4* r = sv.pair + kPairF4 * k;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
        // shadow ray: segment-box cull, then the any-hit test for lanes still open
        const float4 b0 = r[5], b1 = r[6];
        const bool overlap = !h.occluded && seg_lo.x <= b0.w && seg_hi.x >= b0.x &&
                             seg_lo.y <= b1.x && seg_hi.y >= b0.y && seg_lo.z <= b1.y &&
                             seg_hi.z >= b0.z;
        if (__any(overlap)) {
            const PairDots q = pair_dots(r0, r1, r2, r3, r4, p, L);
            const bool pa = overlap && bary_ok(q.denA, q.a1, q.a2);
            const bool pb = overlap && bary_ok(q.denB, q.b1, q.b2);
            if (pa || pb) {
                const f3 nsel = pa ? f3{r2.y, r2.z, r2.w} : f3{r3.w, r4.x, r4.y};
                const float t = pair_t(nsel, q.tv, pa ? q.denA : q.denB);
                bool hit = t > 0.0f && t < smax;
                if (pa && pb && !hit) {
                    const float t2 = pair_t(f3{r3.w, r4.x, r4.y}, q.tv, q.denB);
                    hit = t2 > 0.0f && t2 < smax;
                }
                h.occluded = h.occluded || hit;
            }
        }
        // next-bounce closest hit (no culling: bounce rays are incoherent)
        const PairDots q = pair_dots(r0, r1, r2, r3, r4, p, d2);
        const bool pa = bary_ok(q.denA, q.a1, q.a2);
        const bool pb = bary_ok(q.denB, q.b1, q.b2);
        if (pa || pb) {
            const f3 nsel = pa ? f3{r2.y, r2.z, r2.w} : f3{r3.w, r4.x, r4.y};
            const float t = pair_t(nsel, q.tv, pa ? q.denA : q.denB);
            if (t > 0.001f && t < h.t) {
                h.t = t;
                h.id = (int)(pa ? 2 * k : 2 * k + 1);
            }
            if (pa && pb) {
                const float t2 = pair_t(f3{r3.w, r4.x, r4.y}, q.tv, q.denB);
                if (t2 > 0.001f && t2 < h.t) {
                    h.t = t2;
                    h.id = (int)(2 * k + 1);
                }
            }
        }
    }
    return h;
}

}  // namespace
}  // namespace rt
