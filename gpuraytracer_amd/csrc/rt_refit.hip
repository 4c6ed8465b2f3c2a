// rt_refit.hip — refit of the triangle BVH after rt_update_scene.
//
// The topology of a built tree is kept (escape and leaf words, the leaf order
// `perm`); the records in leaf order and the fp16 boxes of every entry of the
// 8 octant layouts are made again from the new id-order records.  The box rule
// is the builders' (rt_scene.cpp build_tri_sah, rt_lbvh.hip, rt_gsah.hip): a
// leaf plane = fp32 min / max over v0, fl32(v0 + e1), fl32(v0 + e2) of its
// triangles, minus / plus the margin in fp32, rounded outward to fp16; an
// inner plane = min / max of its children's planes.  The builders pad and
// round the fp32 min of a whole subtree instead; subtracting the margin and
// rounding are monotone, so both give the same halves, and a refit onto
// unchanged records writes the build's bytes again.
//
// Nothing is assumed of the tree beyond the format (tests/tri_bvh_tree.py,
// invariants 1-7): preorder layouts, an inner entry i with the children i + 1
// and end(i + 1), end(j) = the escape of an inner j, j + 1 of a leaf.  Every
// layout is refitted by itself (blockIdx.y = octant).  The parent of every
// entry is derived once per tree into a table (refit_parents_kernel); a refit
// is then one launch: a thread per entry, a leaf's thread builds its box and
// climbs; at an inner entry the first child to arrive returns and the second
// builds the box (one agent-scope counter per entry), so no thread ever waits
// for another, and min / max make the result independent of who arrives first.
//
// Hand-off between the two children (they may run on different XCDs, whose L2s
// are not coherent): every box word is stored and loaded at agent scope
// (write-through stores, L1-bypassing loads), the storing thread drains its
// stores before it adds to the counter, and the add is an agent-scope
// acquire-release.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_kernel.hpp"

namespace rt {

namespace {

constexpr uint32_t kInnerBit = 0x80000000u;
constexpr uint32_t kThreads = 256;

// sorted[k] = tri[perm[k]] (a perm entry past n cannot come from a builder: skipped)
__global__ void refit_gather_kernel(const float4* __restrict__ tri, const uint32_t* __restrict__ perm, uint32_t n,
                                    float4* __restrict__ sorted) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = perm[k];
    if (t >= n) return;
    sorted[3 * (size_t)k] = tri[3 * (size_t)t];
    sorted[3 * (size_t)k + 1] = tri[3 * (size_t)t + 1];
    sorted[3 * (size_t)k + 2] = tri[3 * (size_t)t + 2];
}

// The second child of the inner entry i of layout `oct`: end(i + 1).
__device__ __forceinline__ uint32_t second_child(const uint32_t* L, uint32_t oct, uint32_t total, uint32_t i) {
    const uint32_t w1 = L[4 * (size_t)(i + 1) + 3];
    return (w1 & kInnerBit) ? (w1 & ~kInnerBit) - oct * total : i + 2;
}

// parent[oct * total + j] = the entry whose child j is (0xFFFFFFFF, the
// memset value, stays for the root).  *bad counts entries outside the format.
__global__ void refit_parents_kernel(const uint32_t* __restrict__ words, uint32_t total,
                                     uint32_t* __restrict__ parent, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t oct = blockIdx.y;
    if (i >= total) return;
    const uint32_t* L = words + (size_t)oct * total * 4;
    if (!(L[4 * (size_t)i + 3] & kInnerBit)) return;
    if (i + 2 >= total) {  // no room for two children
        atomicAdd(bad, 1u);
        return;
    }
    const uint32_t c2 = second_child(L, oct, total, i);
    if (c2 <= i + 1 || c2 >= total) {
        atomicAdd(bad, 1u);
        return;
    }
    parent[(size_t)oct * total + i + 1] = i;
    parent[(size_t)oct * total + c2] = i;
}

__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float half_value(uint32_t bits) { return __half2float(__ushort_as_half((unsigned short)bits)); }
// min / max of two fp16 planes by value; of -0 and +0 the min is -0, the max +0
__device__ __forceinline__ uint32_t half_min(uint32_t a, uint32_t b) {
    const float x = half_value(a), y = half_value(b);
    return x < y ? a : (y < x ? b : (a | b));
}
__device__ __forceinline__ uint32_t half_max(uint32_t a, uint32_t b) {
    const float x = half_value(a), y = half_value(b);
    return x > y ? a : (y > x ? b : (a & b));
}

// One thread per entry of one layout; the fourth word of an entry is only read.
__global__ void refit_boxes_kernel(uint32_t* words, uint32_t total, const float4* __restrict__ sorted, uint32_t n,
                                   float margin, const uint32_t* __restrict__ parent, uint32_t* counter) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t oct = blockIdx.y;
    if (i >= total) return;
    uint32_t* L = words + (size_t)oct * total * 4;
    const uint32_t w = L[4 * (size_t)i + 3];
    if (w & kInnerBit) return;
    const uint32_t first = w & 0xFFFFFFu, count = (w >> 24) + 1u;  // a leaf: 1..128 triangles
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t k = first; k < first + count && k < n; ++k) {
        const float4 A = sorted[3 * (size_t)k], Bq = sorted[3 * (size_t)k + 1], C = sorted[3 * (size_t)k + 2];
        const float v0[3] = {A.x, A.y, A.z};
        const float v1[3] = {A.x + A.w, A.y + Bq.x, A.z + Bq.y};   // v0 + e1
        const float v2[3] = {A.x + Bq.z, A.y + Bq.w, A.z + C.x};   // v0 + e2
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], fminf(v0[a], fminf(v1[a], v2[a])));
            hi[a] = fmaxf(hi[a], fmaxf(v0[a], fmaxf(v1[a], v2[a])));
        }
    }
    uint32_t h[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        h[a] = __half_as_ushort(__float2half_rd(lo[a] - margin));
        h[3 + a] = __half_as_ushort(__float2half_ru(hi[a] + margin));
    }
    // near/far: the plane a ray of octant `oct` enters through takes the lo slot
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if ((oct >> a) & 1u) {
            const uint32_t x = h[a];
            h[a] = h[3 + a];
            h[3 + a] = x;
        }
    uint32_t node = i;
    for (;;) {
        uint32_t* E = L + 4 * (size_t)node;
        st_agent(E, h[0] | (h[1] << 16));
        st_agent(E + 1, h[2] | (h[3] << 16));
        st_agent(E + 2, h[4] | (h[5] << 16));
        const uint32_t p = parent[(size_t)oct * total + node];
        if (p >= node) return;  // the root (0xFFFFFFFF); a parent always precedes its children
        // the box must have left this CU before the counter says so
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t prev = __hip_atomic_fetch_add(&counter[(size_t)oct * total + p], 1u, __ATOMIC_ACQ_REL,
                                                     __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0) return;  // the sibling subtree is not done yet: its last thread goes on
        const uint32_t c2 = second_child(L, oct, total, p);
        if (c2 >= total) return;  // outside the format (refit_parents_kernel counted it)
        const uint32_t* A = L + 4 * (size_t)(p + 1);
        const uint32_t* B = L + 4 * (size_t)c2;
        const uint32_t a0 = ld_agent(A), a1 = ld_agent(A + 1), a2 = ld_agent(A + 2);
        const uint32_t b0 = ld_agent(B), b1 = ld_agent(B + 1), b2 = ld_agent(B + 2);
        const uint32_t ha[6] = {a0 & 0xFFFFu, a0 >> 16, a1 & 0xFFFFu, a1 >> 16, a2 & 0xFFFFu, a2 >> 16};
        const uint32_t hb[6] = {b0 & 0xFFFFu, b0 >> 16, b1 & 0xFFFFu, b1 >> 16, b2 & 0xFFFFu, b2 >> 16};
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            // slot s holds a hi plane when it is a far slot of a forward axis or a near slot of a flipped one
            const bool is_hi = (s >= 3) != (((oct >> (s % 3)) & 1u) != 0);
            h[s] = is_hi ? half_max(ha[s], hb[s]) : half_min(ha[s], hb[s]);
        }
        node = p;
    }
}

}  // namespace

size_t tri_refit_table_bytes(uint32_t total) { return 2 * (size_t)kTriCompactLayouts * total * sizeof(uint32_t) + 16; }

hipError_t refit_tri_bvh(const float4* d_tri, uint32_t n, float margin, uint4* d_nodes, uint32_t total,
                         float4* d_sorted, const uint32_t* d_perm, uint32_t** d_table, bool* table_made,
                         hipEvent_t ev0, hipEvent_t ev1, hipStream_t s) {
    *table_made = false;
    if (n == 0 || total == 0) return hipSuccess;
    if (n >= (1u << 24) || total > 2 * n - 1) return hipErrorInvalidValue;
    const size_t entries = (size_t)kTriCompactLayouts * total;
    uint32_t* words = reinterpret_cast<uint32_t*>(d_nodes);
    const dim3 grid((total + kThreads - 1) / kThreads, kTriCompactLayouts);
    hipError_t e;
    // the table: counters (zeroed by every refit) at its start, then the parents, then the format-error count
    if (!*d_table) {
        if ((e = hipMalloc((void**)d_table, tri_refit_table_bytes(total)))) return e;
        *table_made = true;
        if ((e = hipMemsetAsync(*d_table + entries, 0xFF, entries * sizeof(uint32_t), s))) return e;
        if ((e = hipMemsetAsync(*d_table + 2 * entries, 0, 16, s))) return e;
        hipLaunchKernelGGL(refit_parents_kernel, grid, dim3(kThreads), 0, s, words, total, *d_table + entries,
                           *d_table + 2 * entries);
        if ((e = hipGetLastError())) return e;
    }
    uint32_t* counter = *d_table;
    const uint32_t* parent = *d_table + entries;
    if ((e = hipEventRecord(ev0, s))) return e;
    if ((e = hipMemsetAsync(counter, 0, entries * sizeof(uint32_t), s))) return e;
    hipLaunchKernelGGL(refit_gather_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, d_tri, d_perm, n,
                       d_sorted);
    if ((e = hipGetLastError())) return e;
    hipLaunchKernelGGL(refit_boxes_kernel, grid, dim3(kThreads), 0, s, words, total, d_sorted, n, margin, parent,
                       counter);
    if ((e = hipGetLastError())) return e;
    return hipEventRecord(ev1, s);
}

hipError_t refit_format_errors(const uint32_t* d_table, uint32_t total, uint32_t* bad) {
    return hipMemcpy(bad, d_table + 2 * (size_t)kTriCompactLayouts * total, sizeof(uint32_t), hipMemcpyDeviceToHost);
}

}  // namespace rt
