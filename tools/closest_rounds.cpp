// CPU count of the candidate rounds of the box-cluster kernel's closest queries
// at bounces 1 and 2, for the single-mask order
// (RT_CLU_ORDER=0) and the ordered and culled one, over one compiled scene:
// waves of 4x4 pixels x 4 samples, pinhole camera rays with uniform jitter,
// cosine-weighted continuation directions -- not the kernel's Halton points, so
// the figures are statistical.  Built on the kernel's own per-lane
// classification (rt_cluorder.hpp through tests/native/closest_order_host.hpp)
// and the oracle's triangle test; run by tools/closest_round_stats.py.
//   closest_rounds <scene file> <seed> <waves>     -> one JSON line
#include <stdlib.h>

#include <algorithm>
#include <random>

#include "../tests/native/closest_order_host.hpp"

using rt::f3;

namespace {
std::mt19937 g;
float U() { return std::uniform_real_distribution<float>(0.0f, 1.0f)(g); }
f3 unit(f3 v) { return v * (1.0f / sqrtf(rt::dot(v, v))); }

struct Tally {
    double waves = 0, lanes = 0, rounds = 0, lane_rounds = 0, ge2 = 0;
    long hist[8] = {0};
    void add_wave(int live, const int* cnt_a, const int* cnt_b) {  // rounds: phase a, then phase b
        int ma = 0, mb = 0;
        for (int l = 0; l < 64; ++l) {
            ma = std::max(ma, cnt_a[l]);
            mb = std::max(mb, cnt_b[l]);
            lane_rounds += cnt_a[l] + cnt_b[l];
            ge2 += (cnt_a[l] + cnt_b[l]) >= 2;
        }
        waves += 1;
        lanes += live;
        rounds += ma + mb;
        hist[std::min(ma + mb, 7)]++;
    }
    void print(const char* name) const {
        printf("\"%s\": {\"rounds_per_wave\": %.4f, \"lanes_per_round\": %.3f, \"pair_tests_per_lane\": %.4f, "
               "\"lanes_with_2_or_more_tests\": %.4f, \"rounds_histogram\": [",
               name, rounds / waves, lane_rounds / std::max(rounds, 1.0), lane_rounds / lanes, ge2 / lanes);
        for (int i = 0; i < 8; ++i) printf("%ld%s", hist[i], i < 7 ? ", " : "]}");
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        printf("usage: closest_rounds <scene file> <seed> <waves>\n");
        return 2;
    }
    g.seed((unsigned)atoi(argv[2]));
    const int n_waves = atoi(argv[3]);
    clo::HostScene s;
    const char* err = nullptr;
    if (!clo::load_scene(argv[1], &s, &err) || s.nc == 0) {
        printf("{\"error\": \"%s\"}\n", s.nc == 0 && !err ? "no clusters" : (err ? err : "scene"));
        return 1;
    }
    const int W = s.cam.resolution.x, H = s.cam.resolution.y;
    Tally now[3], ord[3];
    double live_lanes[3] = {0};
    long mismatches = 0;
    for (int w = 0; w < n_waves; ++w) {
        const int tx = (int)(U() * (float)(W / 4)) * 4, ty = (int)(U() * (float)(H / 4)) * 4;
        f3 o[64], d[64];
        bool live[64];
        for (int l = 0; l < 64; ++l) {
            const int pix = l / 4;
            float dir[3];
            pto_camera_ray(&s.cam, std::min(tx + pix % 4, W - 1), std::min(ty + pix / 4, H - 1), U(), U(), dir);
            o[l] = f3{s.cam.position.x, s.cam.position.y, s.cam.position.z};
            d[l] = f3{dir[0], dir[1], dir[2]};
            live[l] = true;
        }
        for (int b = 0; b < 3; ++b) {
            int c_now[64] = {0}, zero[64] = {0}, c_near[64] = {0}, c_far[64] = {0}, n_live = 0;
            for (int l = 0; l < 64; ++l) {
                if (!live[l]) continue;
                ++n_live;
                float t;
                const int id = clo::brute_closest(s, o[l], d[l], &t);
                if (b > 0) {
                    float tq;
                    clo::QueryCount q0, q1;
                    const int i0 = clo::cluster_closest(s, o[l], d[l], clo::kUnordered, &tq, &q0);
                    mismatches += i0 != id || rt::f2u(tq) != rt::f2u(t);
                    const int i1 = clo::cluster_closest(s, o[l], d[l], clo::kOrdered, &tq, &q1);
                    mismatches += i1 != id || rt::f2u(tq) != rt::f2u(t);
                    c_now[l] = q0.near_tests;
                    c_near[l] = q1.near_tests;
                    c_far[l] = q1.far_tests;
                }
                if (id < 0) {
                    live[l] = false;
                    continue;
                }
                const MaterialGPU& M = s.mats[id];
                if (M.emissive.x > 0.0f || M.emissive.y > 0.0f || M.emissive.z > 0.0f) {  // the light ends a path
                    live[l] = false;
                    continue;
                }
                f3 N = unit(rt::cross(s.vtx(id, 1) - s.vtx(id, 0), s.vtx(id, 2) - s.vtx(id, 0)));
                if (rt::dot(N, d[l]) > 0.0f) N = -N;
                const f3 p = (o[l] + d[l] * t) + N * 1e-3f;
                const float u1 = U(), u2 = U();
                const float ct = sqrtf(u2), st = sqrtf(1.0f - u2), ph = 6.2831853f * u1;
                const f3 a = fabsf(N.x) > 0.9f ? f3{0.0f, 1.0f, 0.0f} : f3{1.0f, 0.0f, 0.0f};
                const f3 r = unit(rt::cross(N, a)), f = rt::cross(N, r);
                o[l] = p;
                d[l] = unit(r * (st * cosf(ph)) + N * ct + f * (st * sinf(ph)));
            }
            if (b > 0 && n_live > 0) {
                now[b].add_wave(n_live, c_now, zero);
                ord[b].add_wave(n_live, c_near, c_far);
                live_lanes[b] += n_live;
            }
        }
    }
    printf("{\"waves\": %d, \"clusters\": %zu, \"pairs\": %zu, \"mismatches_vs_brute_force\": %ld", n_waves, s.nc,
           s.cs.pair_isect.size(), mismatches);
    for (int b = 1; b < 3; ++b) {
        printf(", \"bounce%d\": {\"live_lanes_per_wave\": %.2f, ", b, live_lanes[b] / std::max(now[b].waves, 1.0));
        now[b].print("single_mask");
        printf(", ");
        ord[b].print("ordered");
        printf("}");
    }
    printf("}\n");
    return mismatches ? 1 : 0;
}
