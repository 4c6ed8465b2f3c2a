"""CPU: the similarity transforms of tests/transform_scenes.py:
the whole scene -- geometry, camera and light -- scaled, moved and turned.
The reference first: the C oracle against its numpy restatements, bit for bit,
at every transform, so that a GPU parity test there is worth what it is at the
Cornell room (at ``tiny`` and ``x100`` the reference's own tmin / tmax clamps
are active).  Then the table's own claims: frames without NaNs that show
something, the box-cluster layout kept, the cluster kinds the scene compiler
reports written down per (scene, transform), tmax cutting the frame at
``x100``.  Then the host twins of the kernels' masks, the per-lane filter
checkers (tests/native/) on the scene file of every (scene, transform), the
container shrink where a container survives, and the ray sets with the
exactness domain.  The GPU side is tests/test_gpu_transforms.py."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib
import ray_sets as rs
import test_camera_candidates as cc
import test_shadow_candidates as shc
import transform_scenes as ts
from closest_order_scenes import write_scene_file
from conftest import native_toolchain
from gpuraytracer_amd import Scene
from lean_filter_scenes import CONTAINER, INSIDE, OWN_LIGHT, SINGLE, TURNED, kinds
from light_mask_scenes import emissive_ids
from test_lean_filter import EXPECTED as LEAN_EXPECTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = list(ts.TRANSFORMS)
SCENES = {"cornell": lambda w, h: Scene.cornell_box(w, h),
          "boxes0": lambda w, h: Scene.random_boxes(w, h, 4, seed=0),
          "boxes1": lambda w, h: Scene.random_boxes(w, h, 4, seed=1),
          "cornell_mis": lambda w, h: Scene.cornell_box_mis(w, h)}
CLUSTER_SCENES = ["cornell", "boxes0", "boxes1"]

ROOM, LIGHT = CONTAINER | INSIDE, SINGLE | OWN_LIGHT


def _k(*groups):
    """A sorted kinds list from (kind, count) groups."""
    return sorted(k for kind, n in groups for k in [kind] * n)


# The kind bits (8 container, 16 single face, 32 turned, 64 shrunk box, 128 own
# light) of every cluster, sorted, per (scene, transform): read off
# rt_debug_cluster_kinds once and written down.  A transform that changes a row
# changes what the kernels run.  Translations split boxes: fit_box takes two
# face normals, computed from the rounded vertices, for perpendicular only when
# |n . n0| <= 1e-6, and vertices rounded at 2^-18 (offset) or 2^-14 (offset900)
# tilt a normal by more, so a box falls into clusters of 1 to 5 faces.
def _rows(whole, no_own, offset, offset900, perm, roty30, rot123, rot_tiny):
    """A scene's table: the exact and inexact scales up to 100 keep the kinds of
    the control, x103 loses the own-light flag (extent 257.5 > 256), x100rot
    has the kinds of rot123."""
    rows = {tr: whole for tr in ("id", "half", "x1_16", "tiny", "x37", "x100")}
    rows.update(x103=no_own, offset=offset, offset900=offset900, perm=perm, roty30=roty30, rot123=rot123,
                rot_tiny=rot_tiny, x100rot=rot123)
    return rows


PLAIN = SINGLE   # the light's cluster without the own-light flag
_CORNELL = _rows(
    whole=_k((ROOM, 1), (TURNED, 2), (LIGHT, 1)),
    no_own=_k((ROOM, 1), (TURNED, 2), (PLAIN, 1)),
    offset=_k((ROOM, 1), (TURNED, 2), (0, 1), (LIGHT, 1)),           # 5 clusters
    offset900=_k((ROOM, 1), (TURNED, 2), (0, 1), (PLAIN, 3)),        # 7 clusters, no own-light
    perm=_k((ROOM, 1), (TURNED, 2), (PLAIN, 1)),                     # the quad's plane is z = 2.49, not the sampled y
    roty30=_k((TURNED, 3), (LIGHT, 1)),                              # the room is a turned box: no container
    rot123=_k((0, 3), (PLAIN, 1)),
    rot_tiny=_k((0, 2), (TURNED, 1), (PLAIN, 1)))
KINDS = {
    "cornell": _CORNELL,
    "cornell_mis": _CORNELL,
    "boxes0": _rows(
        whole=_k((ROOM, 1), (0, 4), (LIGHT, 1)),
        no_own=_k((ROOM, 1), (0, 4), (PLAIN, 1)),
        offset=_k((ROOM, 1), (0, 8), (LIGHT, 1)),                    # 10
        offset900=_k((ROOM, 1), (0, 7), (PLAIN, 11)),                # 19
        perm=_k((ROOM, 1), (0, 4), (PLAIN, 1)),
        roty30=_k((TURNED, 1), (0, 4), (LIGHT, 1)),
        rot123=_k((0, 5), (PLAIN, 1)),
        rot_tiny=_k((0, 4), (TURNED, 1), (PLAIN, 1))),
    "boxes1": _rows(
        whole=_k((ROOM, 1), (0, 4), (LIGHT, 1)),
        no_own=_k((ROOM, 1), (0, 4), (PLAIN, 1)),
        offset=_k((ROOM, 1), (0, 6), (LIGHT, 1)),                    # 8
        offset900=_k((ROOM, 1), (0, 9), (PLAIN, 3)),                 # 13
        perm=_k((ROOM, 1), (0, 4), (PLAIN, 1)),
        roty30=_k((TURNED, 1), (0, 4), (LIGHT, 1)),
        rot123=_k((0, 5), (PLAIN, 1)),
        rot_tiny=_k((0, 4), (TURNED, 1), (PLAIN, 1))),
}
COUNTS = {"cornell": {"offset": 5, "offset900": 7}, "cornell_mis": {"offset": 5, "offset900": 7},
          "boxes0": {"offset": 10, "offset900": 19}, "boxes1": {"offset": 8, "offset900": 13}}


@functools.lru_cache(maxsize=None)
def scene_at(name, tr, w=ts.W, h=ts.H):
    return ts.apply(SCENES[name](w, h), tr)


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def floats(buf, cols):
    return np.frombuffer(buf, f32).reshape(-1, cols)


# ---- the table itself -----------------------------------------------------------------

def test_the_control_row_is_the_scene_itself_and_copies_are_not_edits():
    s = Scene.cornell_box(ts.W, ts.H)
    before = bytes(s.vertices), bytes(s.camera), bytes(s.light)
    assert ts.apply(s, "id") is s
    assert sorted(ts.SCALES + ts.OFFSETS + ts.ROTATIONS + ["id", "x100rot"]) == sorted(ts.TRANSFORMS)
    assert set(ts.KEY) <= set(ts.TRANSFORMS) and set(ts.CORE) <= set(ts.KEY)
    for tr in ts.MOVED:
        m = ts.apply(s, tr)
        assert m.materials is s.materials and m.vertices is not s.vertices
        assert (m.width, m.height, m.camera.horizontalFov) == (s.width, s.height, s.camera.horizontalFov)
        assert (m.light.width, m.light.depth) == (s.light.width, s.light.depth)
    assert (bytes(s.vertices), bytes(s.camera), bytes(s.light)) == before


def test_exact_transforms_are_exact():
    """A power-of-two scale keeps every mantissa; the signed permutation moves
    components without rounding; a translation rounds each value once."""
    s = Scene.random_spheres(ts.W, ts.H, 20)
    v, sp = floats(s.vertices, 4)[:, :3], floats(s.spheres, 20)
    m = ts.apply(s, "tiny")
    assert np.array_equal(floats(m.vertices, 4)[:, :3], v * f32(2.0 ** -10))
    assert np.array_equal(floats(m.spheres, 20)[:, 16], sp[:, 16] * f32(2.0 ** -10))
    assert np.array_equal(floats(m.spheres, 20)[:, 0:3], sp[:, 0:3] * f32(2.0 ** -10))
    assert tuple(m.camera.direction) == tuple(s.camera.direction) and m.camera.position.z == 9.0 * 2.0 ** -10
    p = ts.apply(s, "perm")
    assert np.array_equal(floats(p.vertices, 4)[:, :3], np.stack([v[:, 0], -v[:, 2], v[:, 1]], 1))
    assert tuple(p.camera.position) == (0.0, -9.0, 0.0) and tuple(p.camera.direction) == (0.0, 1.0, 0.0)
    assert tuple(p.camera.up) == (0.0, 0.0, 1.0) and tuple(p.light.center) == (0.0, 0.0, f32(2.49))
    assert np.array_equal(floats(p.spheres, 20)[:, 16], sp[:, 16])
    o = ts.apply(s, "offset")
    want = (v.astype(np.float64) + np.array([40.0, -25.0, 60.0])).astype(f32)
    assert np.array_equal(floats(o.vertices, 4)[:, :3], want)
    r = ts.apply(s, "x100rot")
    want = ((100.0 * sp[:, 0:3].astype(np.float64)) @ ts.ROT123.T + np.array([30.0, 10.0, -20.0]))
    assert np.abs(floats(r.spheres, 20)[:, 0:3] - want).max() <= 2.0 ** -24 * 512, "one rounding to fp32"
    assert np.array_equal(floats(r.spheres, 20)[:, 16], (sp[:, 16].astype(np.float64) * 100.0).astype(f32))


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", ["cornell", "boxes0", "boxes1"])
def test_shared_vertices_keep_their_bits(name, tr):
    """Equal input vertices give equal output bits: the scene compiler pairs
    triangles by comparing bits, and every scene keeps all its pairs."""
    base, s = scene_at(name, "id"), scene_at(name, tr)
    a, b = floats(base.vertices, 4)[:, :3].view(np.uint32), floats(s.vertices, 4)[:, :3].view(np.uint32)
    _, ia = np.unique(a, axis=0, return_inverse=True)
    _, ib = np.unique(b, axis=0, return_inverse=True)
    assert len(set(zip(ia.ravel().tolist(), ib.ravel().tolist()))) == len(set(ia.ravel().tolist()))
    assert s.describe()["n_triangle_pairs"] == base.describe()["n_triangle_pairs"] == s.n_triangles // 2


# ---- the reference first ------------------------------------------------------------------

@pytest.mark.parametrize("tr", NAMES)
def test_oracle_equals_its_numpy_restatement(tr):
    import pt_oracle_np as P
    s = scene_at("cornell", tr, 16, 12)
    sd = oracle_lib.seeds(16, 12)
    out = oracle_lib.render(s, sd, 2, 3)
    ref = P.render(P.Scene(s.camera, s.materials, s.light, s.vertices), sd, 2, 3)
    assert same_words(out, ref), np.argwhere((out != ref).any(-1))[:4].tolist()


@pytest.mark.parametrize("tr", ts.CORE)
def test_mis_oracle_equals_its_numpy_restatement(tr):
    import pt_oracle_mis_np as M
    s = scene_at("cornell_mis", tr, 8, 6)
    out, out8 = oracle_lib.render_mis(s, 2, 9)
    with np.errstate(all="ignore"):  # the restatement computes both sides of its selects
        ref, ref8 = M.render_mis(M.Scene(s.camera, s.materials, s.light, s.vertices), 2, 9)
    assert same_words(out, ref) and np.array_equal(out8, ref8)
    assert np.isfinite(out).all() and out[..., :3].any()


# ---- the table's claims ---------------------------------------------------------------------

@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", ["cornell", "boxes0"])
def test_every_transform_shows_something_on_the_cluster_kernel(name, tr):
    """The oracle frame (64 x 48, 2 spp, 3 bounces) is NaN-free with at least a
    tenth of its pixels lit (the bar of tests/test_poses.py), and the scene
    stays on the box-cluster kernel: a transform must not push it onto the
    pair kernel unseen."""
    s = scene_at(name, tr)
    out = oracle_lib.render(s, oracle_lib.seeds(ts.W, ts.H), 2, 3)
    lit_share = float(out[..., :3].any(-1).mean())
    nan = int((~np.isfinite(out)).any(-1).sum())
    print(f"{name} at {tr}: lit {lit_share:.2f}, {nan} NaN pixels")
    assert nan == 0 and lit_share >= 0.10
    assert s.describe()["kernel_layout"] == 6


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", list(SCENES))
def test_cluster_kinds_are_the_tables(name, tr):
    s = scene_at(name, tr)
    got = kinds(s)
    print(f"{name} at {tr}: {len(got)} clusters, kinds {got}")
    assert s.describe()["n_box_clusters"] == len(got)
    assert got == KINDS[name][tr]
    assert len(got) == COUNTS[name].get(tr, 4 if name.startswith("cornell") else 6)


def test_the_id_rows_are_todays_expectations():
    """tests/test_lean_filter.py EXPECTED: Cornell, and four random boxes."""
    assert KINDS["cornell"]["id"] == LEAN_EXPECTED["cornell"]
    assert KINDS["boxes0"]["id"] == KINDS["boxes1"]["id"] == LEAN_EXPECTED["boxes4"]


def test_tmax_cuts_the_frame_at_x100():
    """At s = 100 the back wall lies 1150 from the camera: pixel centres that
    hit something at ``x37`` (the same view, all of it inside tmax) miss at
    ``x100``.  The reference's tmax is what a GPU parity test meets there."""
    far, near = oracle_lib.primary_ids(scene_at("cornell", "x100")), oracle_lib.primary_ids(scene_at("cornell", "x37"))
    cut = int(((far == -1) & (near >= 0)).sum())
    print(f"x100: {cut} pixel centres miss that hit at x37; {int((far >= 0).sum())} still hit")
    assert cut >= 1 and (far >= 0).any()


# ---- the host twins of the masks ----------------------------------------------------------------

@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", CLUSTER_SCENES)
def test_candidate_masks_are_conservative_at_every_transform(name, tr):
    """Both check_scene functions (6 footprints a shape) on the candidate tests'
    70 x 45 frame.  Every transform keeps the camera outside the room: the
    occluder mask is undecided on at most a fifth of the footprints."""
    s = scene_at(name, tr, cc.W, cc.H)
    k = NAMES.index(tr)
    cc.check_scene(s, 400 + k, per_shape=6)
    skipped, n = shc.check_scene(s, 500 + k, per_shape=6, max_skipped=0.20)
    print(f"{name} at {tr}: {skipped} of {n} footprints undecided")


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", CLUSTER_SCENES)
def test_light_mask_is_the_set_of_emissive_triangles(name, tr):
    """As tests/test_light_mask.py checks it: the mask is the set of emissive
    triangles, the records' flag words agree, colour and emissive words are bit
    copies of the materials."""
    s = scene_at(name, tr)
    mask, records = s.light_mask()
    lights = emissive_ids(s)
    assert lights == [s.n_triangles - 2, s.n_triangles - 1]
    assert mask == sum(1 << k for k in lights)
    rec = records.view(np.uint32)
    assert [k for k in range(s.n_triangles) if records[k, 3] != 0.0] == lights
    mm = floats(s.materials, 12).view(np.uint32)
    assert np.array_equal(rec[:, [7, 11, 15]], mm[:, 0:3]) and np.array_equal(rec[:, 12:15], mm[:, 8:11])


# ---- the per-lane filters ---------------------------------------------------------------------------

def _build(tmp, source, *defs):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    cxx, san, lib = native_toolchain(cxx)
    orc = os.environ.get("RTPT_SAN_DIR") or os.path.join(ROOT, "oracle")
    if not os.path.exists(os.path.join(orc, "liboracle.so")):
        pytest.skip("oracle/liboracle.so not built")
    out = tmp / source
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", *defs, *san,
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gpuraytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", source + ".cpp"),
                           "-L", lib, "-lrtpt", f"-Wl,-rpath,{lib}",
                           "-L", orc, "-loracle", f"-Wl,-rpath,{orc}", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("transforms")
    return {"lean": _build(tmp, "lean_filter_check", "-DRT_CLU_LEAN_ITEMS=7"),
            "closest": _build(tmp, "closest_order_check"),
            "cluster": _build(tmp, "cluster_check")}


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("transform_scenes")
    files = {}
    for name in CLUSTER_SCENES:
        for tr in NAMES:
            files[name, tr] = str(d / f"{name}-{tr}.bin")
            write_scene_file(scene_at(name, tr), files[name, tr])
    return files


def _run(*cmd):
    return subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", CLUSTER_SCENES)
def test_lean_candidates_hold_every_accepted_hit(checkers, scene_files, name, tr):
    """tests/native/lean_filter_check.cpp draws its rays from the scene's own
    surfaces, so it applies unchanged.  The counters show which paths ran: the
    own-light skip on every shadow query exactly where the kinds table has an
    own-light cluster, the exit-only path exactly where it has a container."""
    r = _run(checkers["lean"], scene_files[name, tr], 1, 0)
    print(f"{name} at {tr}: {r.stdout.strip()}")
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    c = {k: int(v) for k, v in (w.split("=") for w in r.stdout.split()[1:])}
    table = KINDS[name][tr]
    assert c["clusters"] == len(table)
    # without a container the classes drawn on a container's walls (W, T) are empty
    has_room = any(k & CONTAINER for k in table)
    assert c["closest"] + c["shadow"] >= (200_000 if has_room else 150_000) and c["occluded"] > 0, r.stdout
    assert c["own-skipped"] == (c["shadow"] if any(k & OWN_LIGHT for k in table) else 0), r.stdout
    assert (c["exit-only"] > 0) == has_room, r.stdout


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", CLUSTER_SCENES)
def test_ordered_query_equals_brute_force(checkers, scene_files, name, tr):
    r = _run(checkers["closest"], scene_files[name, tr], 1)
    print(f"{name} at {tr}: {r.stdout.strip()}")
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    assert int(r.stdout.split("far culled ")[1].split()[0]) > 0, r.stdout


def grow(ext):
    """The negative control of the container check: the stored box grown by
    2e-4 at extent 2.5 (the control of tests/test_cluster_host.py), scaled with
    max(1, ext), ext the largest |vertex coordinate| as build_clusters takes
    it.  The floor at 1 is the compiler's own (tol = 1e-5 * max(1, ext)): below
    it the shrink no longer follows the extent, and a growth that did would
    stay inside the shrink and show nothing."""
    return 2e-4 * max(1.0, ext) / 2.5


@pytest.mark.parametrize("tr", ["id", "tiny", "x100", "offset"])
def test_container_shrink_is_conservative_where_a_container_survives(checkers, scene_files, tr):
    """tests/native/cluster_check.cpp on the scene file: segments inside the
    stored shrunk room have no accepted hit on a room triangle; the same box
    grown (``grow``) has."""
    assert any(k & CONTAINER for k in KINDS["cornell"][tr])
    r = _run(checkers["cluster"], 0, 1, 0, scene_files["cornell", tr])
    print(f"cornell at {tr}: {r.stdout.strip()}")
    assert r.returncode == 0 and r.stdout.startswith("ok containers=1 "), r.stdout + r.stderr
    assert grow(2.5) == 2e-4
    g = grow(ts.extent(scene_at("cornell", tr)))
    r = _run(checkers["cluster"], 0, 1, repr(g), scene_files["cornell", tr])
    print(f"cornell at {tr}, grown by {g:.3g}: {r.stdout.strip()}")
    assert r.returncode != 0 and "hits triangle" in r.stdout, r.stdout + r.stderr


# ---- ray queries ------------------------------------------------------------------------------------

RAY_SCENES = {"cornell": lambda: Scene.cornell_box(ts.W, ts.H),
              "spheres": lambda: Scene.random_spheres(ts.W, ts.H, 200),
              "tri400": lambda: Scene.random_triangles(ts.W, ts.H, 400)}


@functools.lru_cache(maxsize=None)
def ray_case(name, tr):
    """(scene, numpy scene, domain, {set: rays}) of a ray-query scene under a
    transform: sets B and C mapped with the scene (ts.rays_bc), D and E built
    on the transformed scene by tests/ray_sets.py."""
    s = ts.apply(RAY_SCENES[name](), tr)
    sc, dom = rs.np_scene(s), s.ray_domain()
    B, C = ts.rays_bc(tr)
    D = rs.set_d(s, B, rs.reference(sc, B), origin=ts.point(tr, rs.INTERIOR))
    sets = {"B": B, "C": C, "D": D, "E": rs.set_e(B, dom)}
    for r in sets.values():
        r.setflags(write=False)
    return s, sc, dom, sets


@pytest.mark.parametrize("tr", NAMES)
@pytest.mark.parametrize("name", list(RAY_SCENES))
def test_ray_sets_lie_in_the_exactness_domain(name, tr):
    """rt_debug_ray_domain follows the scene: origin_max is the largest
    |coordinate| of the vertices, the sphere bounds and the camera, floored at
    2.5; the other bounds are constants.  At least half of every set lies
    inside, so the accelerated path is what the GPU test exercises: B whole, C
    wherever tmin < tmax holds (at ``tiny`` 3 % of its segments are shorter than
    the 1e-3 they are cut by), D but for the grazing rays that start 2 units
    beside a sphere at the far end of ``offset900``."""
    s, sc, dom, sets = ray_case(name, tr)
    cam = max(abs(c) for c in s.camera.position)
    assert dom == {"origin_max": float(f32(max(2.5, ts.extent(s), cam))), "dir_len2_min": 0.25, "dir_len2_max": 4.0,
                   "tmax_max": 1000.0}
    share = {k: float(rs.in_domain(r, dom).mean()) for k, r in sets.items()}
    print(f"{name} at {tr}: origin_max {dom['origin_max']:.6g}, in-domain share {share}")
    assert all(v >= 0.5 for v in share.values()), share
    assert share["B"] == 1.0 and share["E"] < 0.7
    C = sets["C"]
    assert np.array_equal(rs.in_domain(C, dom), C[:, 7] > 0)
    # the sets are worth tracing: B hits and misses, C is occluded and not
    t, ids = rs.reference(sc, sets["B"])
    occ = rs.reference(sc, C, any_hit=True)[1]
    print(f"  B hit {float((ids >= 0).mean()):.3f}, C occluded {float(occ.mean()):.3f}")
    assert (ids >= 0).mean() >= 0.25 and 0.02 <= occ.mean() <= 0.70
