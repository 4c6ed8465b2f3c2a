"""CPU: the camera poses and light positions of tests/pose_scenes.py
(DESIGN.md §4).  The reference first -- the C oracle against its numpy
restatements, bit for bit, at every pose and light, so that a GPU parity test
at a pose is worth what it is at the Cornell camera; then the pose table's own
claims (frames without NaNs that show something, one BVH octant per octant
view); then the host twins of the kernels' candidate masks
(rt_debug_camera_candidates, rt_debug_shadow_candidates) at every pose and
light: conservative everywhere, decided where the camera looks at the room
from outside, and the documented fallback -- nothing decided -- where it sits
inside.  The GPU side is tests/test_gpu_poses.py."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib
import pose_scenes as ps
import test_camera_candidates as cc
import test_shadow_candidates as shc
from gpuraytracer_amd import Scene

CASES = [(p, "ceiling") for p in ps.POSES] + [("cornell", l) for l in ps.MOVED_LIGHTS] + [("diag_roll", "low")]
IDS = [p if l == "ceiling" else f"{p}-light-{l}" for p, l in CASES]
SCENES = {"cornell": lambda w, h: Scene.cornell_box(w, h),
          "boxes0": lambda w, h: Scene.random_boxes(w, h, 4, seed=0),
          "boxes1": lambda w, h: Scene.random_boxes(w, h, 4, seed=1)}


def frame(pose, w, h, own=None):
    """(w, h), or ``own`` (default: the pose's frame) for a pose with a frame of its own."""
    return (w, h) if pose not in ps.FRAME else (own or ps.FRAME[pose])


@functools.lru_cache(maxsize=None)
def table_scene(name, pose, light):
    """The scene ``name`` at (pose, light) on the candidate tests' 70 x 45 frame."""
    return ps.view(SCENES[name](*frame(pose, cc.W, cc.H)), pose, light)


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def test_the_control_rows_are_the_cornell_scene():
    s = Scene.cornell_box(ps.W, ps.H)
    assert tuple(s.light.center) == tuple(np.float32(c) for c in ps.LIGHTS["ceiling"])
    assert ps.view(s, "cornell", "ceiling") is s
    assert (tuple(s.camera.position), tuple(s.camera.direction), tuple(s.camera.up)) == ((0, 0, 9), (0, 0, -1), (0, 1, 0))
    moved = ps.view(s, "diag_roll", "low")
    assert moved.materials is s.materials and moved.vertices is s.vertices
    assert tuple(s.camera.position) == (0, 0, 9) and tuple(s.light.center)[1] == np.float32(2.49), "copies, not edits"
    assert moved.camera.resolution.x == ps.W and moved.camera.horizontalFov == s.camera.horizontalFov
    assert sorted(ps.OUTSIDE + ps.INSIDE + ["away", "aspect3"]) == sorted(ps.POSES)


# ---- the reference first ----------------------------------------------------------

@pytest.mark.parametrize("pose,light", CASES, ids=IDS)
def test_oracle_equals_its_numpy_restatement(pose, light):
    import pt_oracle_np as P
    w, h = frame(pose, 16, 12, own=(24, 8))
    s = ps.view(Scene.cornell_box(w, h), pose, light)
    sd = oracle_lib.seeds(w, h)
    out = oracle_lib.render(s, sd, 2, 3)
    ref = P.render(P.Scene(s.camera, s.materials, s.light, s.vertices), sd, 2, 3)
    assert same_words(out, ref), np.argwhere((out != ref).any(-1))[:4].tolist()


@pytest.mark.parametrize("pose,light", [("rolled", "ceiling"), ("diag_roll", "ceiling"), ("straight_down", "ceiling"),
                                        ("cornell", "low")])
def test_mis_oracle_equals_its_numpy_restatement(pose, light):
    import pt_oracle_mis_np as M
    s = ps.view(Scene.cornell_box_mis(8, 6), pose, light)
    out, out8 = oracle_lib.render_mis(s, 2, 9)
    with np.errstate(all="ignore"):  # the restatement computes both sides of its selects
        ref, ref8 = M.render_mis(M.Scene(s.camera, s.materials, s.light, s.vertices), 2, 9)
    assert same_words(out, ref) and np.array_equal(out8, ref8)
    assert np.isfinite(out).all() and out[..., :3].any()


# ---- the pose table -----------------------------------------------------------------

@pytest.mark.parametrize("pose,light", CASES, ids=IDS)
def test_every_view_shows_something(pose, light):
    """The oracle frame (Cornell scene, 70 x 45, 2 spp, 3 bounces) is NaN-free,
    at least a tenth of its pixels are lit and the pixel centres see at least
    three primitives; ``away`` is exactly the frame of rays that hit nothing."""
    s = table_scene("cornell", pose, light)
    out = oracle_lib.render(s, oracle_lib.seeds(s.width, s.height), 2, 3)
    ids = oracle_lib.primary_ids(s)
    assert np.isfinite(out).all()
    lit_share = float(out[..., :3].any(-1).mean())
    print(f"{pose} light {light}: lit {lit_share:.2f}, {len(np.unique(ids))} primary ids")
    if pose == "away":
        miss = np.zeros_like(out)
        miss[..., 3] = 1.0
        assert same_words(out, miss) and (ids == -1).all()
        return
    assert lit_share >= 0.10 and len(np.unique(ids[ids >= 0])) >= 3, (lit_share, np.unique(ids))


def test_octant_views_cover_the_eight_octants():
    """octK's centre ray (pto_camera_ray) lies in BVH octant K -- bit a set where
    component a is negative, rt_trace.hpp octant() -- and no component is zero."""
    d = (ctypes.c_float * 3)()
    seen = []
    for k in range(8):
        s = ps.view(Scene.cornell_box(ps.W, ps.H), f"oct{k}")
        cc.L.pto_camera_ray(ctypes.addressof(s.camera), ps.W // 2, ps.H // 2, 0.0, 0.0, d)
        assert all(c != 0.0 for c in d), list(d)
        seen.append(sum(1 << a for a in range(3) if d[a] < 0))
    assert seen == list(range(8)), seen
    s = Scene.cornell_box(ps.W, ps.H)
    cc.L.pto_camera_ray(ctypes.addressof(s.camera), ps.W // 2, ps.H // 2, 0.0, 0.0, d)
    assert list(d) == [0.0, 0.0, -1.0], "the Cornell centre ray lies on two octant borders"


# ---- the sphere test far from its spheres ---------------------------------------------

def scan_slack(pose, spp=3):
    """Over the camera rays of ``spp`` samples a pixel (64 x 48) that the numpy
    restatement's id-ordered scan lets hit a sphere: the largest p - r, p the
    distance of the sphere's centre from the ray's line in float64, and the
    largest (p^2 - r^2) / (eps D^2), D = |o - c|, eps = 2^-24 (0 without a hit
    beside its sphere)."""
    import aov_ref
    s = ps.view(Scene.random_spheres(ps.W, ps.H, 200), pose)
    sc = aov_ref.np_scene(s)
    sd = oracle_lib.seeds(ps.W, ps.H)
    yy, xx = np.meshgrid(np.arange(ps.H), np.arange(ps.W), indexing="ij")
    sph = np.frombuffer(s.spheres, np.float32).reshape(-1, 20).astype(np.float64)
    centre, radius = sph[:, 0:3], np.abs(sph[:, 16])
    beside = ratio = 0.0
    for n in range(spp):
        i = (sd.ravel().astype(np.uint64) + np.uint64(n)).astype(np.uint32)
        o, d = aov_ref.camera_rays(sc, xx.ravel(), yy.ravel(), aov_ref.onp.halton(i, 0), aov_ref.onp.halton(i, 1))
        with np.errstate(all="ignore"):
            ids, _ = aov_ref.onp._closest(sc, o, d, aov_ref.TMIN, aov_ref.TMAX)
        k = ids[ids >= s.n_triangles] - s.n_triangles
        if not len(k):
            continue
        hit = ids >= s.n_triangles
        O = np.stack([np.broadcast_to(c, ids.shape) for c in (o.x, o.y, o.z)], -1).astype(np.float64)[hit]
        Dv = np.stack([d.x, d.y, d.z], -1).astype(np.float64)[hit]
        oc = O - centre[k]
        along = (oc * Dv).sum(-1) / (Dv * Dv).sum(-1)
        p2 = ((oc - along[:, None] * Dv) ** 2).sum(-1)
        beside = max(beside, float((np.sqrt(p2) - radius[k]).max()))
        ratio = max(ratio, float(((p2 - radius[k] ** 2) / (2.0 ** -24 * (oc * oc).sum(-1))).max()))
    return beside, ratio


def test_far_camera_sphere_hits_stay_inside_the_padding_bound():
    """The sphere test's discriminant is a difference of terms of size D^2, D =
    |o - c|: from (0, 0, 900) the id-ordered scan accepts rays that pass well
    beside a sphere -- farther than the culling margin 4e-5 * 900 that the
    sphere BVH's boxes once had, which is how the sphere kernels lost hits at
    ``narrow_far`` -- but never farther than sqrt(r^2 + 20 eps D^2), the
    padding rt_scene.cpp sphere_margin derives from the roundings of the test
    (measured here: 0.243 beside a sphere of radius 0.1, a ratio of 1.9)."""
    beside, ratio = scan_slack("narrow_far")
    print(f"narrow_far: a hit {beside:.3f} beside its sphere, (p^2 - r^2) / (eps D^2) = {ratio:.2f}")
    assert beside > 4e-5 * 900, "the view no longer shows what the old margin missed"
    assert ratio <= 20.0
    for pose in ("cornell", "diag_roll"):
        assert scan_slack(pose)[1] <= 20.0, pose


def test_the_own_light_flag_is_withheld_off_the_quads_plane():
    """Cluster flag 128 (the light's own cluster may be skipped) needs the light
    centre in the emissive quad's plane: every moved light withholds it, and
    changes no other flag."""
    s = Scene.cornell_box(ps.W, ps.H)
    flags = {l: ps.view(s, "cornell", l).cluster_kinds() for l in ps.LIGHTS}
    assert [f & 128 for f in flags["ceiling"]] == [0, 0, 0, 128], flags["ceiling"]
    for l in ps.MOVED_LIGHTS:  # ceiling_plane: y = 2.5 is the wall's plane, not the quad's (2.49)
        assert flags[l] == [f & ~128 for f in flags["ceiling"]], (l, flags[l])


# ---- the host twins -------------------------------------------------------------------

@pytest.mark.parametrize("pose,light", CASES, ids=IDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_candidate_masks_are_conservative_at_every_view(name, pose, light, monkeypatch):
    """Both check_scene functions (6 footprints a shape) on the candidate tests'
    70 x 45 frame; ``aspect3`` on its own 72 x 24, whose halfH feeds the beam:
    the footprints follow the frame of tests/test_camera_candidates.py, which
    is set for that case.
    Outside poses and every light: the occluder mask is undecided on at most a
    fifth of the footprints (measured: at most a tenth), so the check cannot
    pass vacuously.  Inside poses and ``away``: the documented fallback, the
    occluder mask undecided on every footprint with every byte set; for
    ``away`` the camera mask keeps every pair too."""
    if pose in ps.FRAME:
        monkeypatch.setattr(cc, "W", ps.FRAME[pose][0])
        monkeypatch.setattr(cc, "H", ps.FRAME[pose][1])
    s = table_scene(name, pose, light)
    k = CASES.index((pose, light))
    cc.check_scene(s, 100 + k, per_shape=6)
    if pose in ps.OUTSIDE or pose in ps.FRAME:
        shc.check_scene(s, 200 + k, per_shape=6, max_skipped=0.20)
        return
    skipped, n = shc.check_scene(s, 200 + k, per_shape=6)  # asserts every byte set where undecided
    assert skipped == n, f"{skipped} of {n} footprints undecided at an inside pose"
    if pose == "away":
        for rect, _, _ in cc.footprints(np.random.default_rng(300), 6):
            assert cc.candidates(s, *rect).all(), rect
