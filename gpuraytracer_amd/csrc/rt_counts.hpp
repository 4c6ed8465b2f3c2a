// rt_counts.hpp — the render with one sample count per pixel (include/rtpt.h
// rt_render_counts): included by rt_kernel.hip inside
// namespace rt, after every existing kernel and launcher, so that trace_path
// and the existing instantiations stay where they are.
//
// path_counts_kernel is the lockstep path_trace_kernel with these differences:
//   * pixel p draws c_p = min(counts[p], P.spp) samples, starting at sample
//     sample_base + k_p, where k_p is the count its running sum already holds
//     (the .w of its sum entry; 0 without accumulate);
//   * a wave runs max over its pixels of ceil(c_p / L) rounds; a lane whose
//     sample index is past its pixel's count traces nothing in that round (the
//     uniform kernel re-traces the last sample instead: min(n, spp - 1) has no
//     meaning at c_p = 0);
//   * the in-order sum's condition n0 + k < c_p is per pixel.  The L lanes of a
//     pixel hold the same c_p, so they enter and leave every DPP row-shift add
//     together, and a row shift only reads lanes of the same pixel (L = 16: a
//     pixel is one 16-lane DPP row): an add never reads an inactive lane;
//   * the dead-wave +0 is applied per pixel, when c_p != 0;
//   * the pixel is sum / (float)(k_p + c_p), or +0 when that total is 0.
// The per-wave camera and shadow masks depend on the wave's pixel rectangle
// only and are computed as in path_trace_kernel; halton_tables_on takes the
// cap P.spp.  Two forms: L = 16 for fixed-digit (SMALL) indices -- a wave is
// 2x2 pixels (one row of four for interleaved rows), so four pixels share a
// round count -- and L = 1 otherwise.  Layouts: the lockstep ones; a context
// of the free or sorted schedulers or the path-sorting pair layout renders
// counts through ray_query_layout's lockstep form.

namespace {

template <int L, int k>
struct row_sum_counts {
    __device__ __forceinline__ static void run(f3& acc, f3 c, uint32_t n0, uint32_t cp) {
        if (n0 + (uint32_t)k < cp)  // uniform over the pixel's L lanes (one DPP row at L = 16)
            acc = acc + f3{row_shl<k>(c.x), row_shl<k>(c.y), row_shl<k>(c.z)};
        row_sum_counts<L, k + 1>::run(acc, c, n0, cp);
    }
};
template <int L>
struct row_sum_counts<L, L> {
    __device__ __forceinline__ static void run(f3&, f3, uint32_t, uint32_t) {}
};

}  // namespace

template <int B, int GEO, bool SPH, bool SMALL, int L>
__global__ __launch_bounds__(block_threads(GEO), lockstep_min_waves(GEO, SPH))
void path_counts_kernel(KParams P, const uint32_t* __restrict__ counts, uint32_t* __restrict__ totals) {
    static_assert(L == 1 || L == 16, "the counts forms: one lane or one DPP row per pixel");
    constexpr uint32_t NT = block_threads(GEO), WR = waves_per_row(GEO), WC = waves_per_col(GEO);
    extern __shared__ float4 lds[];
    SceneView sv;
    __shared__ float sph_stash[GEO == kGeoSphLds ? 6 * kSphBlockThreads : 1];
    // the Halton tables by the cap P.spp, not a pixel's count
    RT_LDS_GUARD(staged_end(GEO, P, GEO == kGeoPairClu));
    stage_scene<GEO, SPH, NT>(sv, P, lds, sph_stash, halton_tables_on(GEO, SMALL, P.spp, L));

    const uint32_t kWX = (L == 1) ? 8u : P.wave_w, kWY = (64u / L) / kWX;
    uint32_t bx, by;
    xcd_tile(bx, by);
    auto pixel_of = [&](uint32_t t, uint32_t& x, uint32_t& j) {
        const uint32_t lane = t & 63u, wave = t >> 6, pix = lane / L;
        x = bx * (WR * kWX) + (wave % WR) * kWX + (pix % kWX);
        j = by * (WC * kWY) + (wave / WR) * kWY + (pix / kWX);
    };
    if constexpr (RT_CAM_CAND && GEO == kGeoPairClu) {
        // The per-wave camera and shadow candidate masks, as in
        // path_trace_kernel: they depend on the wave's
        // pixel rectangle, not on counts.  Before any lane leaves.
        if (sv.nP - 1u < 32u) {
            const uint32_t wave = wave_uniform(threadIdx.x >> 6);
            const uint32_t wx0 = bx * (WR * kWX) + (wave % WR) * kWX;
            const uint32_t wj0 = by * (WC * kWY) + (wave / WR) * kWY;
            const Beam beam = wave_beam(P, wx0, wj0, kWX, kWY);
            // the masks of wave_masks_kernel<false>, spelled out (tools/isa_diff.sh)
            const uint32_t k = threadIdx.x & 63u;
            const uint32_t kc = min(k, sv.nP - 1u);
            const bool keep = !beam_excludes_pair(beam, reinterpret_cast<const float*>(sv.pair + kPairF4 * kc));
            sv.cam_mask = wave_uniform((uint32_t)__builtin_amdgcn_ballot_w64(k < sv.nP && keep));
            sv.cam_avail = true;
            if constexpr (RT_SHD_CAND) {
                const uint32_t tb = k >> 5, kt = min(k & 31u, sv.nP - 1u);
                bool occ = false, bad = (sv.cam_mask & (sv.cam_mask - 1u)) != 0u;
                if (sv.cam_mask != 0u && !bad) {  // wave-uniform
                    const uint32_t sp = (uint32_t)__builtin_ctz(sv.cam_mask);
                    const float4 s0 = P.tri_shade[4 * (2u * sp + tb)];
                    if (s0.w == 0.0f) {
                        const ShaftLight lq = shaft_light(ld_f3(P.light_center));
                        const ShaftSrc src = shaft_source(beam, reinterpret_cast<const float*>(sv.pair + kPairF4 * sp),
                                                          (int)tb, f3{s0.x, s0.y, s0.z}, lq);
                        bad = !src.ok;
                        occ = !shaft_excludes_pair(src, lq, reinterpret_cast<const float*>(sv.pair + kPairF4 * kt));
                    }
                }
                const unsigned long long ob = __builtin_amdgcn_ballot_w64((k & 31u) < sv.nP && occ);
                sv.shd_mask = wave_uniform((uint32_t)ob | (uint32_t)(ob >> 32));
                sv.shd_avail = __builtin_amdgcn_ballot_w64(bad) == 0ull && sv.nC <= 32u;
                if (sv.nC != 0u) {
                    const uint32_t kc2 = min(k, sv.nC - 1u);
                    const uint32_t all = __float_as_uint(reinterpret_cast<const float*>(sv.clu + kCluF4 * kc2)[22]);
                    sv.shd_cskip = wave_uniform(
                        (uint32_t)__builtin_amdgcn_ballot_w64(k < sv.nC && (all & sv.shd_mask) == 0u));
                }
            }
        }
    }
    {
        uint32_t x, j;
        pixel_of(threadIdx.x, x, j);
        if (x >= (uint32_t)P.W || j >= P.row_count) return;  // a pixel's L lanes leave together
    }
    // seed + sample_base + k_p, and c_p, of the lane's pixel: in LDS, as the
    // seed of path_trace_kernel, so that they are not live across the walks
    __shared__ uint32_t seed_s[NT];
    __shared__ uint32_t cnt_s[NT];
    __shared__ float lum_s[L > 1 ? 3 * (NT / L) : 1];
    f3 lum{0.0f, 0.0f, 0.0f};
    {
        const uint32_t t = threadIdx.x, sub = t % L;
        uint32_t x, j;
        pixel_of(t, x, j);
        const uint32_t y = P.row_start + j * P.row_step;
        const size_t o = (size_t)j * (size_t)P.W + x;
        uint32_t kp = 0u;
        if (P.accumulate) {
            const float4 prev = P.sum[o];
            lum = f3{prev.x, prev.y, prev.z};
            kp = (uint32_t)prev.w;  // the samples the sum holds: exact, <= 2^24
        }
        seed_s[t] = P.seeds[(size_t)y * (size_t)P.W + x] + P.sample_base + kp;
        cnt_s[t] = min(counts[o], P.spp);
        const uint32_t slot = t / L;
        if (L > 1 && sub == 0) {
            lum_s[3 * slot] = lum.x;
            lum_s[3 * slot + 1] = lum.y;
            lum_s[3 * slot + 2] = lum.z;
        }
    }
    const f3 cu = ld_f3(P.cam_u), cv = ld_f3(P.cam_v), cw = ld_f3(P.cam_w);
    const float fW = (float)P.W, fH = (float)P.H;
    constexpr bool kDeadSkip = RT_CAM_CAND && RT_DEAD_SKIP && GEO == kGeoPairClu && !SPH;
    bool dead = false;
    if constexpr (kDeadSkip) dead = sv.cam_avail && sv.cam_mask == 0u;  // wave-uniform
    for (uint32_t r = 0; !dead; ++r) {
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const uint32_t sub = t % L, cp = cnt_s[t];
        // wave-uniform: the wave runs max over its pixels of ceil(c_p / L) rounds
        if (__builtin_amdgcn_ballot_w64(r * L < cp) == 0ull) break;
        const uint32_t n = r * L + sub;
        PathState s;
        s.acc = f3{0.0f, 0.0f, 0.0f};
        if (n < cp) {  // per lane: a lane past its pixel's count traces nothing
            uint32_t x, j;
            pixel_of(t, x, j);
            const float fx = (float)x, fy = (float)(P.row_start + j * P.row_step);
            s.i = seed_s[t] + n;  // seed + (sample_base + k_p + n)
            const float jx = halton_dim<0, SMALL>(s.i);
            const float jy = halton_dim<1, SMALL, GEO == kGeoPairClu>(s.i, sv.htab);
            s.d = camera_dir<GEO == kGeoTriBvh>(P, cu, cv, cw, fW, fH, fx, fy, jx, jy);
            s.o = ld_f3(P.cam_pos);
            s.thr = f3{1.0f, 1.0f, 1.0f};
            trace_path<B, GEO, SPH, SMALL>(P, sv, s);
            if (L == 1) lum = lum + s.acc;
        }
        if (L > 1) {
            // every in-frame lane is here again: the L lanes of a pixel take each
            // add of the sum together (row_sum_counts)
            uint32_t t2 = threadIdx.x;
            asm volatile("" : "+v"(t2));
            const uint32_t sub2 = t2 % L, slot = t2 / L;
            f3 acc{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
            row_sum_counts<L, 0>::run(acc, s.acc, r * L, cnt_s[t2]);
            if (sub2 == 0) {
                lum_s[3 * slot] = acc.x;
                lum_s[3 * slot + 1] = acc.y;
                lum_s[3 * slot + 2] = acc.z;
            }
        }
    }
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    if (L > 1) {
        if (t % L != 0) return;
        const uint32_t slot = t / L;
        lum = f3{lum_s[3 * slot], lum_s[3 * slot + 1], lum_s[3 * slot + 2]};
    }
    const uint32_t cp = cnt_s[t];
    if constexpr (kDeadSkip) {
        // x + (+0) once is x + (+0) c_p times; a pixel without samples adds nothing
        if (dead && cp != 0u) lum = lum + f3{0.0f, 0.0f, 0.0f};
    }
    uint32_t x, j;
    pixel_of(t, x, j);
    const size_t o = (size_t)j * (size_t)P.W + x;
    // k_p again from the sum entry this lane is about to overwrite
    const uint32_t total = cp + (P.accumulate ? (uint32_t)P.sum[o].w : 0u);
    const float fs = (float)total;
    if (P.sum) P.sum[o] = make_float4(lum.x, lum.y, lum.z, fs);
    if (totals) totals[o] = total;
    if (P.out) {
        float r = 0.0f, g = 0.0f, bl = 0.0f;  // no samples at all: +0, no 0/0
        if (total != 0u) {
            r = lum.x / fs;
            g = lum.y / fs;
            bl = lum.z / fs;
        }
        store_pixel(P, o, r, g, bl);
    }
}

namespace {

template <int B, int GEO, bool SPH, bool SMALL, int L>
hipError_t launch_counts_tl(const KParams& P, const uint32_t* counts, uint32_t* totals, size_t lds_bytes,
                            hipStream_t stream) {
    KParams Q = P;
    // the wave tiles of launch_tl: 8x8 pixels at L = 1; at L = 16 2x2 pixels,
    // one row of four when the rows are interleaved
    if (L > 1) Q.wave_w = (P.row_step > 1) ? 64u / L : 2u;
    constexpr uint32_t WR = waves_per_row(GEO), WC = waves_per_col(GEO);
    const uint32_t WX = (L == 1) ? 8u : Q.wave_w;
    const uint32_t TX = WR * WX, TY = WC * ((64u / L) / WX);
    const dim3 grid((P.W + TX - 1) / TX, (P.row_count + TY - 1) / TY);
    if (GEO == kGeoSphLds) {
        const hipError_t e = allow_lds((const void*)path_counts_kernel<B, GEO, SPH, SMALL, L>, lds_bytes);
        if (e != hipSuccess) return e;
    }
    note_launch<B, GEO, SPH, SMALL, L>("path_counts_kernel", Q, grid, block_threads(GEO), lds_bytes);
    hipLaunchKernelGGL((path_counts_kernel<B, GEO, SPH, SMALL, L>), grid, dim3(block_threads(GEO)), lds_bytes,
                       stream, Q, counts, totals);
    return hipGetLastError();
}

// L = 16 with fixed-digit indices, one lane per pixel otherwise.
template <int B, int GEO, bool SPH>
hipError_t launch_counts_h(const KParams& P, const uint32_t* counts, uint32_t* totals, size_t lds_bytes,
                           hipStream_t stream) {
    return P.max_index < kSmallIndexMax
               ? launch_counts_tl<B, GEO, SPH, true, 16>(P, counts, totals, lds_bytes, stream)
               : launch_counts_tl<B, GEO, SPH, false, 1>(P, counts, totals, lds_bytes, stream);
}

}  // namespace

hipError_t launch_path_counts(const KParams& P, const uint32_t* counts, uint32_t* totals, uint32_t bounces,
                              SceneMem mem, hipStream_t stream, LaunchInfo* info) {
    if (!counts) return hipErrorInvalidValue;
    const SceneTables T = tables_of(P);
    // the lockstep form of the context's layout, as a ray query takes it
    const int geo = ray_query_layout(choose_kernel(T, P.sph_lds != nullptr, bounces, mem, P.walk).layout);
    const size_t lds_bytes = staged_lds_bytes(geo, T.nT, T.nP, T.nC);
    const hipError_t e = dispatch_bounces(bounces, [&](auto b) {
        return dispatch_layout(geo, P.nS, [&](auto g, auto sph) {
            return launch_counts_h<decltype(b)::value, decltype(g)::value, decltype(sph)::value>(P, counts, totals,
                                                                                                lds_bytes, stream);
        });
    });
    if (info) *info = g_last;
    return e;
}
