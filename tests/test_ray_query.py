"""CPU: the batched ray queries' ABI surface (rt_trace_rays, rt_ray, rt_ray_hit,
rt_debug_ray_domain), the exactness domain of a scene, and the ray sets of
tests/ray_sets.py on the reference alone: the floors that make the sets worth
tracing, and the numpy restatement against a loop over the C oracle's
pto_ray_triangle / pto_ray_sphere on the chosen rays of set D.

The GPU side is tests/test_gpu_ray_query.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gpuraytracer_amd as g
import oracle_lib
import ray_sets as rs
from gpuraytracer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_F3 = ctypes.c_float * 3
oracle_lib.lib.pto_ray_triangle.restype = ctypes.c_int
oracle_lib.lib.pto_ray_triangle.argtypes = [_F3, _F3, _F3, _F3, _F3, ctypes.c_float, ctypes.c_float,
                                            ctypes.POINTER(ctypes.c_float)]
oracle_lib.lib.pto_ray_sphere.restype = ctypes.c_int
oracle_lib.lib.pto_ray_sphere.argtypes = [_F3, _F3, _F3, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                          ctypes.POINTER(ctypes.c_float)]


def scenes():
    return {"cornell": g.Scene.cornell_box(64, 48),
            "spheres": g.Scene.random_spheres(64, 48, 200, seed=42),
            "tri400": g.Scene.random_triangles(64, 48, 400)}


def test_abi_version_is_11():
    assert g.lib.rt_abi_version() == 11 and g.ABI_VERSION == 11


def test_ray_struct_sizes_ctypes():
    assert ctypes.sizeof(_native.Ray) == 32 and ctypes.sizeof(_native.RayHit) == 8
    assert _native.Ray.tmin.offset == 12 and _native.Ray.dir.offset == 16 and _native.Ray.tmax.offset == 28
    assert _native.RayHit.id.offset == 4
    assert ctypes.sizeof(_native.RayDomainInfo) == 16
    assert (_native.RT_RAYS_ANY, _native.RT_RAYS_EXACT) == (0x100, 0x200)


def test_ray_struct_sizes_c99(tmp_path):
    """A C99 program sees the same layout, the flags, and the domain of the
    Cornell scene through the host-only entry point."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "rays.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "rtpt.h"
int main(void) {
    if (sizeof(rt_ray) != 32 || sizeof(rt_ray_hit) != 8) return 1;
    if (offsetof(rt_ray, tmin) != 12 || offsetof(rt_ray, dir) != 16 || offsetof(rt_ray, tmax) != 28) return 2;
    if (offsetof(rt_ray_hit, id) != 4) return 3;
    if (RT_RAYS_ANY != 0x100u || RT_RAYS_EXACT != 0x200u || RTPT_ABI_VERSION != 11) return 4;
    static CameraGPU cam; static MaterialGPU m[36]; static rt_float3 v[108]; static SquareLightGPU l;
    uint32_t n = 0;
    if (rt_scene_cornell_box(64, 48, &cam, m, v, &l, &n)) return 5;
    rt_scene_desc d = {&cam, m, &l, 1, v, n, NULL, 0, 0};
    rt_ray_domain_info dom;
    if (rt_debug_ray_domain(&d, &dom)) return 6;
    if (dom.origin_max != 9.0f || dom.dir_len2_min != 0.25f || dom.dir_len2_max != 4.0f || dom.tmax_max != 1000.0f)
        return 7;
    if (rt_debug_ray_domain(NULL, &dom) != RT_ERR_INVALID_ARG) return 8;
    if (rt_trace_rays(NULL, NULL, 1, 0, NULL) != RT_ERR_INVALID_ARG) return 9;
    if (rt_trace_rays_async(NULL, NULL, 1, 0, NULL, NULL) != RT_ERR_INVALID_ARG) return 10;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "rays"
    libdir = os.path.join(ROOT, "gpuraytracer_amd")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-lrtpt", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-500:])


def test_ray_domain_of_cornell_and_of_a_camera_at_the_origin():
    dom = g.Scene.cornell_box(64, 48).ray_domain()
    # the camera sits at z = 9: the culling margin is 4e-5 * 9
    assert dom == {"origin_max": 9.0, "dir_len2_min": 0.25, "dir_len2_max": 4.0, "tmax_max": 1000.0}
    s = g.Scene.cornell_box(64, 48)
    vv = np.frombuffer(s.vertices, f32).reshape(-1, 4)
    vv[:, :3] *= f32(3.0)  # a room of 7.5 and more: above the floor of 2.5 on the extent
    s.camera.position.x = s.camera.position.y = s.camera.position.z = 0.0
    dom = s.ray_domain()
    assert dom["origin_max"] == float(np.abs(vv[:, :3]).max()) >= 7.5
    assert (dom["dir_len2_min"], dom["dir_len2_max"], dom["tmax_max"]) == (0.25, 4.0, 1000.0)
    # spheres count with their radius
    sp = g.Scene.random_spheres(64, 48, 1, seed=1)
    sp.camera.position.x = sp.camera.position.y = sp.camera.position.z = 0.0
    sp.spheres[0].center.x, sp.spheres[0].radius = 20.0, 2.0
    assert sp.ray_domain()["origin_max"] == 22.0


def test_null_arguments_return_status():
    assert g.lib.rt_trace_rays(None, None, 0, 0, None) == 1
    assert b"null" in g.lib.rt_last_error(None)
    assert g.lib.rt_trace_rays_async(None, None, 0, 0, None, None) == 1
    assert g.lib.rt_debug_ray_domain(None, None) == 1


@pytest.fixture(scope="module")
def refs():
    """name -> (scene, numpy scene, closest reference of B, any-hit reference of C)."""
    B, C = rs.sets_bc()
    out = {}
    for name, scene in scenes().items():
        sc = rs.np_scene(scene)
        out[name] = (scene, sc, rs.reference(sc, B), rs.reference(sc, C, any_hit=True))
    return out


@pytest.mark.parametrize("name", ["cornell", "spheres", "tri400"])
def test_floors_of_sets_b_and_c(refs, name):
    scene, _, (t, ids), (_, occ) = refs[name]
    B, C = rs.sets_bc()
    assert B.shape == C.shape == (4096, 8) and B.dtype == np.float32
    hit = float((ids >= 0).mean())
    print(f"{name}: B hit {hit:.3f}, on a sphere {float((ids >= scene.n_triangles).mean()):.3f}, "
          f"distinct {len(np.unique(ids[ids >= 0]))}, C occluded {float(occ.mean()):.3f}")
    assert hit >= 0.5 and 1.0 - hit >= 0.05
    assert 0.10 <= occ.mean() <= 0.60
    if name == "spheres":
        assert (ids >= scene.n_triangles).mean() >= 0.10
    if name == "cornell":
        assert len(np.unique(ids[ids >= 0])) >= 24
    # a miss carries the ray's tmax, a hit lies strictly inside (tmin, tmax)
    assert np.all(t[ids < 0] == f32(1000.0)) and np.all((t[ids >= 0] > B[ids >= 0, 3]) & (t[ids >= 0] < f32(1000.0)))
    dom = scene.ray_domain()
    assert rs.in_domain(B, dom).all() and rs.in_domain(C, dom).all()


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_chosen_rays_of_set_d(refs, name):
    scene, sc, ref_b, _ = refs[name]
    B, _ = rs.sets_bc()
    t, ids = ref_b
    # tmax exactly at the hit: the strict bound drops it, and nothing nearer exists
    again = rs.reference(sc, rs.d_tmax_at_hit(B, t, ids))
    assert np.all(again[1] == -1) and len(again[1]) == int((ids >= 0).sum())
    # tmin exactly at the hit: that primitive is dropped too
    past = rs.reference(sc, rs.d_tmin_at_hit(B, t, ids))
    assert np.all((past[1] < 0) | (past[0] > t[ids >= 0]))
    # rays through a shared edge: both triangles of the pair accept, the even id wins
    pc = rs.d_pair_corners(scene)
    assert len(pc) == 6 * (scene.n_triangles // 2)
    got_t, got_id = rs.reference(sc, pc)
    o, d, tmin, tmax = rs._soa(pc)
    both = 0
    for k in range(len(pc)):
        p = k // 6
        one = lambda v: rs.onp.V(v.x[k:k + 1], v.y[k:k + 1], v.z[k:k + 1])  # noqa: E731
        ha, ta = rs.onp._tri_test(sc.tris[2 * p], one(o), one(d), tmin[k:k + 1], tmax[k:k + 1])
        hb, tb = rs.onp._tri_test(sc.tris[2 * p + 1], one(o), one(d), tmin[k:k + 1], tmax[k:k + 1])
        if ha[0] and hb[0] and ta[0] == tb[0] == got_t[k]:
            both += 1
            assert got_id[k] == 2 * p
    print(f"{name}: {both} of {len(pc)} corner and edge rays are accepted by both triangles of their pair")
    assert both >= 1
    D = rs.set_d(scene, B, ref_b)
    assert rs.in_domain(D, scene.ray_domain()).all()
    if name == "spheres":
        sp = rs.d_spheres(scene)
        st, sid = rs.reference(sc, sp)
        inside = sid[:16] - scene.n_triangles  # from the centre of sphere k: sphere k or a nearer one
        assert np.all(sid[:16 * 8] >= 0) and (inside == np.arange(16)).sum() >= 8
        graze = sid[16 * 8:]
        assert (graze >= 0).any() and (graze < 0).any()


def _c_closest(scene, rays):
    """The id-ordered scan as a loop over the C oracle's two primitive tests."""
    v = np.frombuffer(bytes(scene.vertices), f32).reshape(-1, 3, 4)[:, :, :3]
    tris = [tuple(_F3(*map(float, v[k, j])) for j in range(3)) for k in range(len(v))]
    sph = []
    if scene.n_spheres:
        s = np.frombuffer(bytes(scene.spheres), f32).reshape(-1, 20)
        sph = [(_F3(*map(float, row[0:3])), float(row[16])) for row in s]
    t_out, id_out = np.empty(len(rays), f32), np.empty(len(rays), np.int32)
    t = ctypes.c_float()
    tri_fn, sph_fn = oracle_lib.lib.pto_ray_triangle, oracle_lib.lib.pto_ray_sphere
    for i, r in enumerate(rays):
        o, d = _F3(*map(float, r[0:3])), _F3(*map(float, r[4:7]))
        tmin, best, hit = float(r[3]), float(r[7]), -1
        for k, (a, b, c) in enumerate(tris):
            if tri_fn(o, d, a, b, c, tmin, best, ctypes.byref(t)):
                best, hit = t.value, k
        for k, (c, rad) in enumerate(sph):
            if sph_fn(o, d, c, rad, tmin, best, ctypes.byref(t)):
                best, hit = t.value, len(tris) + k
        t_out[i], id_out[i] = (best if hit >= 0 else r[7]), hit
    return t_out, id_out


def test_numpy_and_c_oracle_agree_on_set_d(refs):
    """Set D of the Cornell scene in full, and of the sphere scene its
    sphere rays, its corner and edge rays and every 16th of the rest (212
    primitives a ray through ctypes)."""
    B, _ = rs.sets_bc()
    scene, sc, ref_b, _ = refs["cornell"]
    D = rs.set_d(scene, B, ref_b)
    want = rs.reference(sc, D)
    got = _c_closest(scene, D)
    assert rs.same(got, want), rs.first_difference(got, want)
    scene, sc, ref_b, _ = refs["spheres"]
    D = np.concatenate([rs.d_spheres(scene), rs.d_pair_corners(scene), rs.set_d(scene, B, ref_b)[::16]])
    want = rs.reference(sc, D)
    got = _c_closest(scene, D)
    assert rs.same(got, want), rs.first_difference(got, want)


def test_set_e_is_out_of_domain_where_it_says():
    scene = g.Scene.cornell_box(64, 48)
    dom = scene.ray_domain()
    B, _ = rs.sets_bc()
    E = rs.set_e(B, dom)
    ind = rs.in_domain(E, dom)
    assert len(E) == 768 and not ind[512:576].any()
    # every other wave of 64 holds both kinds
    waves = ind.reshape(-1, 64)
    mixed = [w.any() and not w.all() for k, w in enumerate(waves) if k != 8]
    assert all(mixed)
    # every kind of the generator is outside the domain
    out = rs.out_of_domain_variants(B[:42], dom["origin_max"])
    assert not rs.in_domain(out, dom).any()
    # and the reference answers every one of them
    t, ids = rs.reference(rs.np_scene(scene), E)
    assert (ids[~ind] >= 0).any() and (ids[~ind] < 0).any()


def test_a_ray_in_an_oblique_face_plane_can_hit_on_residues():
    """The premise of DESIGN.md §3.20, on the reference alone: for a ray lying
    in the plane of a face whose normal is no world axis, dot(n, d) and the
    barycentric terms are rounding residues, and the test of §3.5 accepts some
    of these rays far from the triangle -- here with the hit point more than
    1e-3 outside the triangle's bounding box, 25 times the culling margin.
    None of the sets B, C and D holds such a hit."""
    scene = g.Scene.cornell_box(64, 48)
    sc = rs.np_scene(scene)
    rays = rs.in_plane_random(scene, range(10, 34))  # the two turned boxes
    assert rs.in_domain(rays, scene.ray_domain()).all()
    residue = rs.residue_hits(sc, rays)
    t, ids = rs.reference(sc, rays)
    v = rs._tri_vertices(scene)
    k = np.flatnonzero(residue & (ids >= 10) & (ids < 34))
    p = rays[k, 0:3] + rays[k, 4:7] * t[k, None]
    lo, hi = v[ids[k]].min(1) - f32(1e-3), v[ids[k]].max(1) + f32(1e-3)
    outside = ~np.all((p >= lo) & (p <= hi), axis=1)
    print(f"{int(residue.sum())} of {len(rays)} in-plane rays have a residue hit; {int(outside.sum())} closest hits "
          f"lie outside their triangle's box")
    assert residue.sum() >= 4 and outside.sum() >= 1
    B, C = rs.sets_bc()
    D = rs.set_d(scene, B, rs.reference(sc, B))
    assert not rs.residue_hits(sc, B).any() and not rs.residue_hits(sc, C).any() and not rs.residue_hits(sc, D).any()
