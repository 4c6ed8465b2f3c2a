// CPU check of the ordered and culled closest query of the box-cluster kernel
// (rt_cluorder.hpp, rt_trace.hpp cluster_query<.., ORDER>),
// linked against librtpt.so (the scene compiler) and oracle/liboracle.so (the
// reference triangle test): for every ray the query's (t, id) must equal, bit
// for bit, the id-ordered strict-'<' brute force over all triangles.
//   closest_order_check <scene file> <seed> [mode] [rays per class]
// mode 0: the shipped query; 1, 2: the two wrong queries of
// closest_order_host.hpp (controls that must fail).  Prints "ok ..." and exits
// 0 when every ray agrees, prints the first mismatch and exits 1 otherwise; a
// scene that compiles to no box clusters prints "no clusters" and exits 0.
// Ray classes:
//   A  path-like: origins at surface hit points + N * 1e-3, cosine-weighted
//      directions, three generations deep
//   B  origins on the faces of the boxes (on the face, and 1e-3 off it on
//      either side), directions over the whole sphere
//   C  grazing: from a class-A origin at a target that lies on a triangle's
//      edge or corner (silhouettes, room edges and corners), or that is a
//      surface point moved along a cluster axis onto that cluster's padded
//      plane or into the padding, in each case +- a few ulps
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

f3 sphere_dir() {
    for (;;) {
        const f3 v{2.0f * U() - 1.0f, 2.0f * U() - 1.0f, 2.0f * U() - 1.0f};
        const float l = rt::dot(v, v);
        if (l > 1e-4f && l <= 1.0f) return unit(v);
    }
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

long n_rays = 0, n_far_kept = 0, n_far_culled = 0;

// one ray: the query under test against the brute force
bool check(const clo::HostScene& s, f3 o, f3 d, int mode, const char* cls) {
    if (!(rt::dot(d, d) > 0.25f)) return true;  // a degenerate direction
    float tb, tq;
    const int ib = clo::brute_closest(s, o, d, &tb);
    clo::QueryCount qc;
    const int iq = clo::cluster_closest(s, o, d, mode, &tq, &qc);
    ++n_rays;
    const rt::CluSplit sp = clo::split_raw(s, o, d, clo::kTmin, clo::kTmax);
    if (sp.near && (sp.far & ~sp.near)) (qc.far_tests ? n_far_kept : n_far_culled)++;
    if (ib == iq && rt::f2u(tb) == rt::f2u(tq)) return true;
    printf("MISMATCH class %s: o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g) brute (t=%.9g id=%d) query (t=%.9g id=%d)\n",
           cls, o.x, o.y, o.z, d.x, d.y, d.z, tb, ib, tq, iq);
    return false;
}

// a class-A origin: a surface hit point + N * 1e-3, N against the arriving ray
bool path_origin(const clo::HostScene& s, f3* o, f3* N) {
    const int t0 = (int)(g() % s.nt);
    f3 p = tri_point(s, t0, U(), U());
    f3 n = tri_normal(s, t0);
    if (g() & 1u) n = -n;
    p = p + n * 1e-3f;
    const f3 d = cosine_dir(n);
    float t;
    const int id = clo::brute_closest(s, p, d, &t);
    if (id < 0) return false;
    f3 n2 = tri_normal(s, id);
    if (rt::dot(n2, d) > 0.0f) n2 = -n2;
    *o = (p + d * t) + n2 * 1e-3f;
    *N = n2;
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        printf("usage: closest_order_check <scene file> <seed> [mode] [rays per class]\n");
        return 2;
    }
    g.seed((unsigned)atoi(argv[2]));
    const int mode = argc > 3 ? atoi(argv[3]) : 0;
    const long per_class = argc > 4 ? atol(argv[4]) : 30000;
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
    std::vector<int> box_tris;  // triangles of the clusters that are no containers
    for (size_t c = 0; c < s.nc; ++c) {
        if (s.flags(c) & 8u) continue;
        const uint32_t all = rt::f2u(s.clu(c)[5].z);
        for (int k = 0; k < 32; ++k)
            if ((all >> k) & 1u) box_tris.push_back(2 * k), box_tris.push_back(2 * k + 1);
    }
    // A
    for (long i = 0; i < per_class;) {
        f3 o, N;
        if (!path_origin(s, &o, &N)) continue;
        for (int gen = 0; gen < 3 && i < per_class; ++gen, ++i) {
            const f3 d = cosine_dir(N);
            if (!check(s, o, d, mode, "A")) return 1;
            float t;
            const int id = clo::brute_closest(s, o, d, &t);
            if (id < 0) break;
            f3 n2 = tri_normal(s, id);
            if (rt::dot(n2, d) > 0.0f) n2 = -n2;
            o = (o + d * t) + n2 * 1e-3f;
            N = n2;
        }
    }
    // B
    for (long i = 0; i < per_class && !box_tris.empty(); ++i) {
        const int t0 = box_tris[g() % box_tris.size()];
        const f3 n = tri_normal(s, t0);
        const float off[3] = {0.0f, 1e-3f, -1e-3f};
        const f3 o = tri_point(s, t0, U(), U()) + n * off[g() % 3u];
        if (!check(s, o, sphere_dir(), mode, "B")) return 1;
    }
    // C
    for (long i = 0; i < per_class;) {
        f3 o, N;
        if (!path_origin(s, &o, &N)) continue;
        const int t1 = (int)(g() % s.nt);
        f3 P;
        const unsigned kind = g() % 4u;
        if (kind == 0) {  // a corner
            P = s.vtx(t1, (int)(g() % 3u));
        } else if (kind == 1) {  // a point of an edge
            const unsigned e = g() % 3u;
            const float u = U();
            P = e == 0 ? tri_point(s, t1, u, 0.0f) : e == 1 ? tri_point(s, t1, 0.0f, u) : tri_point(s, t1, u, 1.0f - u);
        } else {  // a surface point moved onto a cluster's padded plane or into its padding
            P = tri_point(s, t1, U(), U());
            const size_t c = g() % s.nc;
            const clo::V4* r = s.clu(c);
            const uint32_t flags = s.flags(c);
            const int a = (int)(g() % 3u);
            f3 ax = f3{a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f};
            if (!(flags & (1u << a)) && !(flags & 8u)) ax = f3{r[a].x, r[a].y, r[a].z};
            const float lo = r[a].w, hi = a == 0 ? r[3].x : a == 1 ? r[3].y : r[3].z;
            const float wf = a == 0 ? r[6].x : a == 1 ? r[6].y : r[6].z;
            const bool high = (g() & 1u) != 0u;
            float plane = high ? hi : lo;
            if (kind == 3) plane += (high ? -1.0f : 1.0f) * 2.0f * wf * U();  // between the padded plane and the face
            P = P + ax * (plane - rt::dot(ax, P));
        }
        float* pc[3] = {&P.x, &P.y, &P.z};
        for (int a = 0; a < 3; ++a) *pc[a] = ulps(*pc[a], (int)(g() % 9u) - 4);
        const f3 v = P - o;
        if (!(rt::dot(v, v) > 1e-8f)) continue;
        ++i;
        if (!check(s, o, unit(v), mode, "C")) return 1;
    }
    printf("ok rays=%ld clusters=%zu with-near-and-far: far tested %ld, far culled %ld\n", n_rays, s.nc,
           n_far_kept, n_far_culled);
    return 0;
}
