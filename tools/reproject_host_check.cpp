// reproject_host_check.cpp — stand-alone sanitizer run of rt_reproject_host
// (`make reproject-check`): its own main, linked with the host objects of
// rt_reproject_host.cpp and rt_camera.cpp built with
// -fsanitize=address,undefined and nothing of the device side; it is not
// loaded into Python.  Every buffer is a heap allocation of exactly its size,
// so a read or write outside a frame is an AddressSanitizer report, and an
// undefined float-to-int conversion or index overflow a UBSan abort.
//
// The buffers come from the deterministic adversarial generator that
// tests/reproject_cases.py restates (same seed, same tables, same draw order):
// hit records with t in {NaN, +-inf, 1e30, -5, 0, a denormal, 3, 9} and id in
// {-1, 0, 35, 2^31 - 1, -2^31, 7}, normals of NaN, 0, 1e30 and unit
// components, histories with NaN, +-inf and negative alphas; and its
// `plausible` form (the finite entries only), which makes pixels pass the
// gates.  Frames: (1,1), (2,1), (17,16), (33,17), (70,45) and 64x48, one and
// two planes, out aliasing color, three parameter sets, the camera unmoved
// (NULL), shifted by (0.1, 0.05, 0) and turned round.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "rtpt.h"

// The library's error slot (rt_api.cpp) is not linked: this is the program's.
struct rt_ctx;
namespace rtapi {
std::string g_err;
int fail(rt_ctx*, int status, const std::string& msg) {
    g_err = msg;
    return status;
}
}  // namespace rtapi

namespace {

struct Gen {  // splitmix64; pick(n) = (next() >> 33) % n
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t pick(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
};

// fp32 bit patterns; the first `plausible` entries of each table are finite and tame
const uint32_t kT[] = {0x40400000u /*3*/, 0x41100000u /*9*/, 0x7FC00000u /*NaN*/, 0x7F800000u, 0xFF800000u,
                       0x7149F2CAu /*1e30*/, 0xC0A00000u /*-5*/, 0x00000000u, 0x00000001u /*denormal*/};
const uint32_t kId[] = {0u, 7u, 35u, 0xFFFFFFFFu /*-1*/, 0x7FFFFFFFu, 0x80000000u};
const uint32_t kN[] = {0x00000000u, 0x3F800000u, 0xBF800000u, 0x3F19999Au /*0.6*/, 0x7FC00000u, 0x7149F2CAu};
const uint32_t kRgb[] = {0x3E800000u /*0.25*/, 0x3FC00000u /*1.5*/, 0x3F000000u, 0x7FC00000u, 0x7F800000u, 0xFF800000u};
const uint32_t kAlpha[] = {0x3F800000u /*1*/, 0x40E00000u /*7*/, 0x42000000u /*32*/, 0x7FC00000u, 0x7F800000u, 0xFF800000u,
                           0xC0400000u /*-3*/, 0x00000000u, 0x7149F2CAu};
const uint32_t kPlausible[5] = {2, 3, 4, 3, 3};  // of kT, kId, kN, kRgb, kAlpha

struct Frames {
    std::vector<uint32_t> hit, nd, phit, pnd, color[2], hist[2];
};

template <size_t N>
uint32_t draw(Gen& g, const uint32_t (&tab)[N], int which, bool plausible) {
    return tab[g.pick(plausible ? kPlausible[which] : (uint32_t)N)];
}

// Per pixel, row-major, in this order: (t, id), (N.xyz, w) of this frame, the
// same of the previous frame, color[0], color[1], history[0], history[1].
Frames generate(uint64_t seed, int W, int H, bool plausible) {
    Frames F;
    Gen g{seed};
    const size_t n = (size_t)W * (size_t)H;
    for (size_t p = 0; p < n; ++p) {
        for (int prev = 0; prev < 2; ++prev) {
            std::vector<uint32_t>& h = prev ? F.phit : F.hit;
            std::vector<uint32_t>& d = prev ? F.pnd : F.nd;
            h.push_back(draw(g, kT, 0, plausible));
            h.push_back(draw(g, kId, 1, plausible));
            for (int k = 0; k < 3; ++k) d.push_back(draw(g, kN, 2, plausible));
            d.push_back(draw(g, kT, 0, plausible));
        }
        for (int b = 0; b < 4; ++b) {
            std::vector<uint32_t>& c = b < 2 ? F.color[b] : F.hist[b - 2];
            for (int k = 0; k < 3; ++k) c.push_back(draw(g, kRgb, 3, plausible));
            c.push_back(draw(g, kAlpha, 4, plausible));
        }
    }
    return F;
}

// A heap copy of exactly the buffer's size (what AddressSanitizer guards).
struct Heap {
    void* p;
    explicit Heap(const std::vector<uint32_t>& v) : p(malloc(v.size() * 4)) { memcpy(p, v.data(), v.size() * 4); }
    explicit Heap(size_t words) : p(malloc(words * 4)) { memset(p, 0xA5, words * 4); }
    Heap(const Heap&) = delete;
    ~Heap() { free(p); }
    float* f() const { return static_cast<float*>(p); }
};

CameraGPU camera(int W, int H, float ex, float ey, float ez, float dx, float dy, float dz) {
    CameraGPU c;
    memset(&c, 0, sizeof(c));
    c.position.x = ex; c.position.y = ey; c.position.z = ez;
    c.direction.x = dx; c.direction.y = dy; c.direction.z = dz;
    c.up.y = 1.0f;
    c.resolution.x = W; c.resolution.y = H;
    c.horizontalFov = 0.7853982f;
    return c;
}

int failures = 0;

// One call; returns the number of pixels of plane 0 that reused history (a > 1).
long run(const Frames& F, const CameraGPU& cur, const CameraGPU* prev, const rt_reproject_params& P, int planes,
         bool alias) {
    const size_t n = (size_t)cur.resolution.x * (size_t)cur.resolution.y;
    Heap hit(F.hit), nd(F.nd), phit(F.phit), pnd(F.pnd);
    Heap c0(F.color[0]), c1(F.color[1]), h0(F.hist[0]), h1(F.hist[1]), o0(4 * n), o1(4 * n);
    rt_reproject_buffers B;
    memset(&B, 0, sizeof(B));
    B.color[0] = c0.f();
    B.history[0] = h0.f();
    B.out[0] = alias ? c0.f() : o0.f();
    if (planes == 2) {
        B.color[1] = c1.f();
        B.history[1] = h1.f();
        B.out[1] = alias ? c1.f() : o1.f();
    }
    B.hit = static_cast<const rt_ray_hit*>(hit.p);
    B.normal_depth = nd.f();
    B.prev_hit = static_cast<const rt_ray_hit*>(phit.p);
    B.prev_normal_depth = pnd.f();
    const int st = rt_reproject_host(&cur, prev, &P, &B);
    if (st != RT_OK) {
        fprintf(stderr, "rt_reproject_host: status %d (%s)\n", st, rtapi::g_err.c_str());
        ++failures;
        return 0;
    }
    long reused = 0;
    for (size_t p = 0; p < n; ++p) reused += B.out[0][4 * p + 3] > 1.0f ? 1 : 0;
    return reused;
}

}  // namespace

int main() {
    static const int frames[6][2] = {{1, 1}, {2, 1}, {17, 16}, {33, 17}, {70, 45}, {64, 48}};
    rt_reproject_params def;
    rt_reproject_params_default(&def);
    rt_reproject_params loose = def, tight = def;
    loose.normal_cos_min = -1.0f;
    loose.plane_rel = 1e30f;
    loose.weight_min = 0x1p-20f;
    loose.max_history = 65536;
    tight.weight_min = 1.0f;
    tight.max_history = 1;
    const rt_reproject_params params[3] = {def, loose, tight};
    long calls = 0, reused_plausible = 0;
    for (const auto& fr : frames) {
        const int W = fr[0], H = fr[1];
        const CameraGPU cur = camera(W, H, 0.0f, 0.0f, 9.0f, 0.0f, 0.0f, -1.0f);
        const CameraGPU shifted = camera(W, H, 0.1f, 0.05f, 9.0f, 0.0f, 0.0f, -1.0f);
        const CameraGPU turned = camera(W, H, 0.0f, 0.0f, -9.0f, 0.3f, 0.1f, 1.0f);
        const CameraGPU* prevs[3] = {nullptr, &shifted, &turned};
        for (int plausible = 0; plausible < 2; ++plausible) {
            const Frames F = generate(0x5EED0000ull + (uint64_t)(W * 1000 + H), W, H, plausible != 0);
            for (const rt_reproject_params& P : params)
                for (const CameraGPU* prev : prevs)
                    for (int planes = 1; planes <= 2; ++planes)
                        for (int alias = 0; alias < 2; ++alias) {
                            const long r = run(F, cur, prev, P, planes, alias != 0);
                            ++calls;
                            if (plausible && &P == &params[1] && prev != &turned) reused_plausible += r;
                        }
        }
    }
    // the set must not be trivial: with the loose parameters the plausible buffers reuse history
    if (reused_plausible == 0) {
        fprintf(stderr, "no pixel reused history: the plausible set decides nothing\n");
        ++failures;
    }
    printf("reproject_host_check: %ld calls, %ld reusing pixels in the plausible loose runs, %d failures\n", calls,
           reused_plausible, failures);
    return failures ? 1 : 0;
}
