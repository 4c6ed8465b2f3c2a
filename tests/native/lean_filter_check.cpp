// CPU check of the lean cluster-filter paths (rt_cluorder.hpp kCluTurned /
// kCluInside / kCluOwnLight), linked against librtpt.so (the
// scene compiler, which sets the kind flags) and oracle/liboracle.so (the
// reference triangle test).  The program runs the kernel's own per-lane filter
// text on the host; where the kernel decides per wave by ballot (the container
// left from inside), every ray is checked both ways, so whichever the wave
// takes is covered.
//   lean_filter_check <scene file> <seed> [mode] [rays per class]
// For every ray:
//   inclusion  every pair with a triangle the exact test accepts is a candidate
//   far bound  far_lo <= t of every accepted hit on a far-only candidate
//   equality   the query over the candidates returns the brute force's (t, id)
//              (closest) or its boolean (shadow)
// mode 0: the flags the scene compiler set.  Controls that must fail:
// mode 1: kCluTurned forced on every multi-face cluster that is not world-aligned
//         (the two-component products applied to a tilted box);
// mode 2: kCluOwnLight forced on every single-face cluster (the light skip
//         applied to a quad that is not in the sampling plane).
// Prints "ok ..." with the counts the Python side asserts on and exits 0, or the
// first violation and exits 1.
// Ray classes:
//   A  closest, path-like: origins at surface hit points + N * 1e-3, cosine-
//      weighted directions, three generations deep
//   W  closest, from a point of a container's wall itself, or from a class-A
//      origin moved along a world axis onto the container's shrunk box's bound,
//      onto its padded plane or about its wall plane, +- a few ulps
//   Z  closest, from a class-A origin, directions with one or two components
//      exactly +0 or -0
//   S  shadow: from a class-A origin to a point drawn on the light as shade()
//      draws it, tmin 0, tmax = dist - 1e-3
//   T  shadow, from a class-W origin
#include <stdlib.h>

#include <random>

#include "closest_order_host.hpp"

using rt::f3;

namespace {
std::mt19937 g;
float U() { return std::uniform_real_distribution<float>(0.0f, 1.0f)(g); }

f3 unit(f3 v) { return v * (1.0f / sqrtf(rt::dot(v, v))); }

f3 tri_normal(const clo::HostScene& s, int t) {
    return unit(rt::cross(s.vtx(t, 1) - s.vtx(t, 0), s.vtx(t, 2) - s.vtx(t, 0)));
}

f3 tri_point(const clo::HostScene& s, int t, float u, float v) {
    if (u + v > 1.0f) u = 1.0f - u, v = 1.0f - v;
    return s.vtx(t, 0) + (s.vtx(t, 1) - s.vtx(t, 0)) * u + (s.vtx(t, 2) - s.vtx(t, 0)) * v;
}

f3 cosine_dir(f3 N) {
    const float u1 = U(), u2 = U();
    const float ct = sqrtf(u2), st = sqrtf(1.0f - u2), ph = 6.2831853f * u1;
    const f3 a = fabsf(N.x) > 0.9f ? f3{0.0f, 1.0f, 0.0f} : f3{1.0f, 0.0f, 0.0f};
    const f3 r = unit(rt::cross(N, a)), f = rt::cross(N, r);
    return unit(r * (st * cosf(ph)) + N * ct + f * (st * sinf(ph)));
}

float ulps(float v, int n) {
    for (int i = 0; i < abs(n); ++i) v = nextafterf(v, n > 0 ? INFINITY : -INFINITY);
    return v;
}

struct Counts {
    long rays = 0, exit_only = 0, full = 0;  // closest rays; containers taken exit-only / by the full filter
    long shadow = 0, own_skipped = 0, shadow_occluded = 0;
} n;

// cluster_candidates_split for one lane, not finished.  allow_exit: the wave's
// ballot came out "every lane inside" (this lane is, or the full filter runs).
rt::CluSplit lean_split(const clo::HostScene& s, f3 o, f3 d, float tmin, float tmax, bool allow_exit, bool count) {
    const float iv[3] = {rt::safe_rcp(d.x), rt::safe_rcp(d.y), rt::safe_rcp(d.z)};
    const float oi[3] = {o.x * iv[0], o.y * iv[1], o.z * iv[2]};
    rt::CluSplit sp = rt::clu_split_init();
    for (size_t c = 0; c < s.nc; ++c) {
        const clo::V4* r = s.clu(c);
        const uint32_t flags = s.flags(c);
        if (flags & rt::kCluSingle) {
            rt::clu_single_split(r, flags, iv, oi, o, d, tmin, tmax, &sp);
            continue;
        }
        if (rt::kLeanExit && (flags & rt::kCluInside)) {
            const bool in = allow_exit && rt::clu_origin_inside(r, o);
            if (count) (in ? n.exit_only : n.full)++;
            if (in) {
                rt::clu_container_exit(r, iv, oi, tmax, &sp);
                continue;
            }
        }
        float en[3], ex[3], ida[3], tlo, thi;
        rt::clu_slab(r, flags, iv, oi, o, d, tmin, tmax, en, ex, ida, &tlo, &thi);
        rt::clu_faces_split(r, flags, en, ex, ida, tlo, thi, &sp);
    }
    return sp;
}

// cluster_candidates<SEG, false, OWN> for one lane (without the wave's
// container skip of SEG, which only removes candidates this check would accept)
uint32_t shadow_mask(const clo::HostScene& s, f3 o, f3 d, float tmin, float tmax, bool* skipped) {
    const float iv[3] = {rt::safe_rcp(d.x), rt::safe_rcp(d.y), rt::safe_rcp(d.z)};
    const float oi[3] = {o.x * iv[0], o.y * iv[1], o.z * iv[2]};
    rt::CluSplit sp = rt::clu_split_init();
    for (size_t c = 0; c < s.nc; ++c) {
        const clo::V4* r = s.clu(c);
        const uint32_t flags = s.flags(c);
        if (flags & rt::kCluSingle) {
            if (rt::kLeanOwnLight && (flags & rt::kCluOwnLight)) {  // these come last (rt_scene.cpp)
                *skipped = true;
                break;
            }
            rt::clu_single_split(r, flags, iv, oi, o, d, tmin, tmax, &sp);
            continue;
        }
        float en[3], ex[3], ida[3], tlo, thi;
        rt::clu_slab(r, flags, iv, oi, o, d, tmin, tmax, en, ex, ida, &tlo, &thi);
        rt::clu_faces_split(r, flags, en, ex, ida, tlo, thi, &sp);
    }
    return sp.near | sp.far;
}

void say(const char* what, const char* cls, f3 o, f3 d) {
    printf("%s class %s: o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g)", what, cls, o.x, o.y, o.z, d.x, d.y, d.z);
}

bool check_closest_one(const clo::HostScene& s, f3 o, f3 d, bool allow_exit, const char* cls) {
    const rt::CluSplit raw = lean_split(s, o, d, clo::kTmin, clo::kTmax, allow_exit, allow_exit);
    const uint32_t cand = raw.near | raw.far | s.cs.pair_free_mask;
    for (uint32_t t = 0; t < s.nt; ++t) {
        float th;
        if (!clo::tri_hit(s, (int)t, o, d, clo::kTmin, clo::kTmax, &th)) continue;
        const uint32_t bit = 1u << (t / 2);
        if (!(cand & bit)) {
            say("MISSING", cls, o, d);
            printf(" triangle %u t=%.9g exit-only %d\n", t, th, (int)allow_exit);
            return false;
        }
        if ((raw.far & ~raw.near & bit) && !(raw.far_lo <= th)) {
            say("FAR_LO", cls, o, d);
            printf(" triangle %u t=%.9g far_lo=%.9g exit-only %d\n", t, th, raw.far_lo, (int)allow_exit);
            return false;
        }
    }
    // the ordered query over these candidates (rt_trace.hpp cluster_query<.., ORDER>)
    float best = clo::kTmax, tb;
    int id = -1;
    for (uint32_t free = s.cs.pair_free_mask; free; free &= free - 1u)
        clo::pair_rank(s, (uint32_t)__builtin_ctz(free), o, d, &best, &id);
    rt::CluSplit sp = lean_split(s, o, d, clo::kTmin, best, allow_exit, false);
    rt::clu_split_finish(&sp);
    for (uint32_t m = sp.near; m; m &= m - 1u) clo::pair_rank(s, (uint32_t)__builtin_ctz(m), o, d, &best, &id);
    for (uint32_t m = rt::clu_far_needed(sp.far_lo, best) ? sp.far : 0u; m; m &= m - 1u)
        clo::pair_rank(s, (uint32_t)__builtin_ctz(m), o, d, &best, &id);
    const int ib = clo::brute_closest(s, o, d, &tb);
    if (ib != id || rt::f2u(tb) != rt::f2u(best)) {
        say("MISMATCH", cls, o, d);
        printf(" brute (t=%.9g id=%d) query (t=%.9g id=%d) exit-only %d\n", tb, ib, best, id, (int)allow_exit);
        return false;
    }
    return true;
}

bool check_closest(const clo::HostScene& s, f3 o, f3 d, const char* cls) {
    if (!(rt::dot(d, d) > 0.25f)) return true;
    ++n.rays;
    return check_closest_one(s, o, d, true, cls) && check_closest_one(s, o, d, false, cls);
}

// the shadow ray of shade() (rt_kernel.hip) from p: q on the light, L, tmax
bool check_shadow(const clo::HostScene& s, f3 p, const char* cls) {
    const float ux = U() * 2.0f - 1.0f, uy = U() * 2.0f - 1.0f;
    const f3 lc{s.light.center.x, s.light.center.y, s.light.center.z};
    const bool plain = rt::f2u(lc.y) != 0x80000000u && rt::f2u(lc.z) != 0x80000000u;
    const f3 q = plain ? f3{lc.x + 0.25f * ux, lc.y, lc.z + 0.25f * uy}
                       : (lc + f3{0.25f, 0.0f, 0.0f} * ux) + f3{0.0f, 0.0f, 0.25f} * uy;
    f3 L = q - p;
    const float dist = rt::length(L);
    const float inv = 1.0f / fmaxf(dist, 1e-3f);
    L = L * inv;
    const float tmax = dist - 1e-3f;
    ++n.shadow;
    bool skipped = false;
    const uint32_t cand = shadow_mask(s, p, L, 0.0f, tmax, &skipped) | s.cs.pair_free_mask;
    n.own_skipped += skipped;
    bool brute = false, query = false;
    for (uint32_t t = 0; t < s.nt; ++t) {
        float th;
        if (!clo::tri_hit(s, (int)t, p, L, 0.0f, tmax, &th)) continue;
        brute = true;
        if (cand & (1u << (t / 2))) {
            query = true;
            continue;
        }
        say("MISSING", cls, p, L);
        printf(" triangle %u t=%.9g tmax=%.9g\n", t, th, tmax);
        return false;
    }
    n.shadow_occluded += brute;
    return brute == query;
}

// a class-A origin: a surface hit point + N * 1e-3, N against the arriving ray
bool path_origin(const clo::HostScene& s, f3* o, f3* N) {
    const int t0 = (int)(g() % s.nt);
    f3 p = tri_point(s, t0, U(), U());
    f3 nn = tri_normal(s, t0);
    if (g() & 1u) nn = -nn;
    p = p + nn * 1e-3f;
    const f3 d = cosine_dir(nn);
    float t;
    const int id = clo::brute_closest(s, p, d, &t);
    if (id < 0) return false;
    f3 n2 = tri_normal(s, id);
    if (rt::dot(n2, d) > 0.0f) n2 = -n2;
    *o = (p + d * t) + n2 * 1e-3f;
    *N = n2;
    return true;
}

// class W: onto a container's wall plane, shrunk bound or padded plane
bool wall_origin(const clo::HostScene& s, const std::vector<size_t>& containers, f3* o, f3* N) {
    if (containers.empty() || !path_origin(s, o, N)) return false;
    const clo::V4* r = s.clu(containers[g() % containers.size()]);
    const int a = (int)(g() % 3u);
    const bool high = (g() & 1u) != 0u;
    const float hi = a == 0 ? r[3].x : a == 1 ? r[3].y : r[3].z;
    const float wf = a == 0 ? r[6].x : a == 1 ? r[6].y : r[6].z;
    const unsigned kind = g() % 4u;
    if (kind == 3) {  // a point of a wall itself
        const uint32_t all = rt::f2u(r[5].z);
        int t0;
        do t0 = (int)(g() % s.nt); while (!((all >> (t0 / 2)) & 1u));
        *o = tri_point(s, t0, U(), U());
        *N = tri_normal(s, t0);
        if (g() & 1u) *N = -*N;
        return true;
    }
    float v = kind == 0   ? (high ? r[a].y : r[a].x)                               // the shrunk box's bound
              : kind == 1 ? (high ? hi : r[a].w)                                   // the padded plane
                          : 0.5f * ((high ? r[a].y + hi : r[a].x + r[a].w));       // about the wall plane
    if (kind == 2 && (g() & 1u)) v += (high ? -1.0f : 1.0f) * wf * U();
    v = ulps(v, (int)(g() % 9u) - 4);
    (a == 0 ? o->x : a == 1 ? o->y : o->z) = v;
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        printf("usage: lean_filter_check <scene file> <seed> [mode] [rays per class]\n");
        return 2;
    }
    g.seed((unsigned)atoi(argv[2]));
    const int mode = argc > 3 ? atoi(argv[3]) : 0;
    const long per_class = argc > 4 ? atol(argv[4]) : 50000;
    clo::HostScene s;
    const char* err = nullptr;
    if (!clo::load_scene(argv[1], &s, &err)) {
        printf("FAIL: %s\n", err ? err : "scene");
        return 2;
    }
    if (s.nc == 0) {
        printf("no clusters (%u triangles, %zu pairs)\n", s.nt, s.cs.pair_isect.size());
        return 0;
    }
    std::vector<size_t> containers;
    for (size_t c = 0; c < s.nc; ++c) {
        uint32_t flags = s.flags(c);
        if (mode == 1 && !(flags & rt::kCluSingle) && (flags & 7u) != 7u) flags |= rt::kCluTurned;
        if (mode == 2 && (flags & rt::kCluSingle)) flags |= rt::kCluOwnLight;
        memcpy(&s.cs.clusters[28 * c + 15], &flags, 4);
        if (flags & rt::kCluContainer) containers.push_back(c);
    }
    // A
    for (long i = 0; i < per_class;) {
        f3 o, N;
        if (!path_origin(s, &o, &N)) continue;
        for (int gen = 0; gen < 3 && i < per_class; ++gen, ++i) {
            const f3 d = cosine_dir(N);
            if (!check_closest(s, o, d, "A")) return 1;
            float t;
            const int id = clo::brute_closest(s, o, d, &t);
            if (id < 0) break;
            f3 n2 = tri_normal(s, id);
            if (rt::dot(n2, d) > 0.0f) n2 = -n2;
            o = (o + d * t) + n2 * 1e-3f;
            N = n2;
        }
    }
    const Counts a = n;
    // W
    for (long i = 0; i < per_class / 2 && !containers.empty();) {
        f3 o, N;
        if (!wall_origin(s, containers, &o, &N)) continue;
        ++i;
        if (!check_closest(s, o, cosine_dir(N), "W")) return 1;
    }
    // Z
    for (long i = 0; i < per_class / 2;) {
        f3 o, N;
        if (!path_origin(s, &o, &N)) continue;
        f3 d = cosine_dir(N);
        float* dc[3] = {&d.x, &d.y, &d.z};
        const int keep = (int)(g() % 3u);
        const unsigned zeros = 1u + g() % 2u;
        for (unsigned z = 1; z <= zeros; ++z) *dc[(keep + z) % 3] = (g() & 1u) ? 0.0f : -0.0f;
        if (!(rt::dot(d, d) > 1e-6f)) continue;
        ++i;
        if (!check_closest(s, o, unit(d), "Z")) return 1;
    }
    // S
    for (long i = 0; i < per_class * 2;) {
        f3 o, N;
        if (!path_origin(s, &o, &N)) continue;
        ++i;
        if (!check_shadow(s, o, "S")) return 1;
    }
    // T
    for (long i = 0; i < per_class / 2 && !containers.empty();) {
        f3 o, N;
        if (!wall_origin(s, containers, &o, &N)) continue;
        ++i;
        if (!check_shadow(s, o, "T")) return 1;
    }
    printf("ok closest=%ld shadow=%ld clusters=%zu A-exit-only=%ld A-full=%ld exit-only=%ld full=%ld own-skipped=%ld "
           "occluded=%ld\n",
           n.rays, n.shadow, s.nc, a.exit_only, a.full, n.exit_only, n.full, n.own_skipped, n.shadow_occluded);
    return 0;
}
