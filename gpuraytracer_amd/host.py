"""Host-side mirror of the reference's Swift Scene/Renderer API.

``Scene``     <- RTrace/scene.swift (``initCornellBox``, scene.swift:14-62) and
                 RTrace/computeShader.swift conversions (convertCameras, ...).
``Renderer``  <- RTrace/renderer.swift: ``__init__`` = ``Renderer.init()``
                 (:29-115: upload scene, seed texture), ``draw()`` =
                 ``Renderer.draw()`` (:117-146: dispatch + wait + read back).

Everything executes in librtpt.so (C++ host + gfx950 kernel); this module
only marshals arrays through ctypes.  Failures raise :class:`RtError` (the
reference ``fatalError``s).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, fields

import numpy as np

from ._native import (MATH_FNS, RT_MATH_DEVICE, RT_MATH_HOST, RT_MATH_VALUES_MAX, LAYOUTS, RT_AOV_CENTER, RT_COMM_ID_BYTES, RT_KEEP_SUM, RT_OK, RT_OUT_DEVICE, RT_OUT_FP16,
                      RT_OUT_NONE, RT_OUT_RGBA8, RT_RAYS_ANY, RT_RAYS_EXACT, RT_UPDATE_REBUILD, TRI_BUILDS, WALKS,
                      AovBuffers, AovParams, BuildStats, CameraGPU, CreateOptions, DenoiseBuffers, DenoiseParams, LaunchInfo, MaterialGPU, MisParamsC, RayDomainInfo,
                      PathParamsC, PlanParams, PlanStats, RT_PLAN_RELATIVE, RenderParamsC, ReprojectBuffers, ReprojectParams,
                      RtError, SceneDesc, SceneInfo, SphereGPU, SquareLightGPU, TileLayout, TriBvhDump, UpdateStats, WaveMask, float3,
                      lib)

DEFAULT_SEED_KEY = 0x5EED00000000


def _check(status: int, ctx=None):
    if status != RT_OK:
        raise RtError(status, lib.rt_last_error(ctx).decode())


def seed_splitmix(width: int, height: int, key: int = DEFAULT_SEED_KEY) -> np.ndarray:
    """seed[p] = splitmix64(key + p) mod 2^20 — the deterministic stand-in for
    ``arc4random() % (1024*1024)`` (renderer.swift:99-101)."""
    n = int(width) * int(height)
    out = np.empty(n, dtype=np.uint32)
    lib.rt_seed_splitmix(ctypes.c_uint64(key), out.ctypes.data_as(ctypes.c_void_p), n)
    return out.reshape(height, width)


def tonemap_rgba8(rgba32f: np.ndarray) -> np.ndarray:
    """image.swift:35-65 epilogue: fp16 round trip, x2 exposure, Reinhard,
    gamma 1/2.2, truncating UInt8 (alpha 255)."""
    a = np.ascontiguousarray(rgba32f, dtype=np.float32)
    n = a.size // 4
    out = np.empty(a.shape[:-1] + (4,), dtype=np.uint8)
    lib.rt_tonemap_rgba8(a.ctypes.data_as(ctypes.c_void_p), n,
                         out.ctypes.data_as(ctypes.c_void_p))
    return out


WAVE_MASK_DTYPE = np.dtype([(n, np.uint32) for n in ("cam_mask", "shd_mask", "shd_cskip", "shd_available")] +
                           [(n, np.int32) for n in ("x0", "x1", "y0", "y1")])
assert WAVE_MASK_DTYPE.itemsize == ctypes.sizeof(WaveMask)


def _wave_records(call) -> np.ndarray:
    """The records of rt_debug_wave_rects / rt_debug_wave_masks as a
    (waves_y, waves_x) array: a first call for the counts, a second for the
    records."""
    wx, wy = ctypes.c_uint32(), ctypes.c_uint32()
    call(None, 0, wx, wy)
    out = np.zeros((wy.value, wx.value), dtype=WAVE_MASK_DTYPE)
    if out.size:
        call(out.ctypes.data_as(ctypes.c_void_p), out.size, wx, wy)
    return out


def wave_rects(width: int, height: int, lanes: int, row_start: int = 0, row_step: int = 1,
               row_count: int = 0) -> np.ndarray:
    """rt_debug_wave_rects (host only): the pixel rectangles (x0, x1, y0, y1,
    closed; image rows y0, y0 + row_step, .., y1) of the waves of a lockstep
    launch at ``lanes`` lanes per pixel, as a (waves_y, waves_x) record array
    whose mask fields are 0."""
    return _wave_records(lambda p, cap, wx, wy: _check(lib.rt_debug_wave_rects(
        width, height, row_start, row_step, row_count, lanes, p, cap, ctypes.byref(wx), ctypes.byref(wy))))


def _math_fn(fn: str, dim: int, where: str) -> tuple[int, int]:
    if fn not in MATH_FNS or where not in ("host", "device"):
        raise ValueError(f"unknown function {fn!r} or side {where!r}")
    return MATH_FNS[fn] | (int(dim) << 8), RT_MATH_DEVICE if where == "device" else RT_MATH_HOST


def math_values(fn: str, in_bits, where: str = "host", dim: int = 0) -> np.ndarray:
    """rt_debug_math_values: ``fn`` (a key of ``MATH_FNS``; ``dim`` is the
    dimension of a Halton form) on every 32-bit input pattern of ``in_bits``,
    by the x86 compile (``where="host"``) or by a kernel on the current device
    (``"device"``).  Returns the result patterns (uint32, NaNs canonical)."""
    word, side = _math_fn(fn, dim, where)
    a = np.ascontiguousarray(in_bits, dtype=np.uint32).ravel()
    out = np.empty(a.size, np.uint32)
    for lo in range(0, a.size, RT_MATH_VALUES_MAX):
        part = a[lo:lo + RT_MATH_VALUES_MAX]
        _check(lib.rt_debug_math_values(word, side, part.ctypes.data_as(ctypes.c_void_p), part.size,
                                        out[lo:].ctypes.data_as(ctypes.c_void_p)))
    return out


def math_sums(fn: str, first: int, count: int, chunk_log2: int = 16, where: str = "host", dim: int = 0,
              host_threads: int = 1) -> np.ndarray:
    """rt_debug_math_sums over the inputs ``first + j``, ``j < count``: a
    (chunks, 2) uint64 array, per chunk of 2^chunk_log2 inputs the sum of the
    results and the sum weighted by 2j'+1 (j' the offset in the chunk), both
    mod 2^64."""
    word, side = _math_fn(fn, dim, where)
    if not 6 <= chunk_log2 <= 31 or count < 0:
        raise ValueError("chunk_log2 outside 6..31 or a negative count")
    sums = np.zeros(((int(count) + (1 << chunk_log2) - 1) >> chunk_log2, 2), np.uint64)
    _check(lib.rt_debug_math_sums(word, side, first, count, chunk_log2, host_threads,
                                  sums.ctypes.data_as(ctypes.c_void_p)))
    return sums


def comm_unique_id() -> bytes:
    """rt_comm_unique_id: the RCCL communicator id rank 0 hands to every rank."""
    buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES)()
    _check(lib.rt_comm_unique_id(buf))
    return bytes(buf)


def _pixel_flags(fp16: bool = False, rgba8: bool = False) -> int:
    return (RT_OUT_FP16 if fp16 else 0) | (RT_OUT_RGBA8 if rgba8 else 0)


def tile_layout(width: int, height: int, world: int, rank: int, fp16: bool = False,
                rgba8: bool = False) -> dict:
    """rt_tile_layout: rank's rows of the rt_render_gather partition (y = rank +
    j*world) and the padded tile every rank sends (rows_max, tile_bytes)."""
    t = TileLayout()
    _check(lib.rt_tile_layout(width, height, world, rank, _pixel_flags(fp16, rgba8), ctypes.byref(t)))
    return {k: getattr(t, k) for k, _ in TileLayout._fields_}


def place_tiles_host(gathered: np.ndarray, width: int, height: int, world: int) -> np.ndarray:
    """rt_place_tiles_host: ``gathered`` = ``world`` padded tiles back to back
    (uint8/uint16/float32 RGBA pixels, any shape with 4 channels last); returns
    the (height, width, 4) frame rank 0 of rt_render_gather would assemble."""
    g = np.ascontiguousarray(gathered)
    fp16, rgba8 = g.dtype == np.uint16, g.dtype == np.uint8
    if g.dtype not in (np.float32, np.uint16, np.uint8):
        raise ValueError("gathered pixels must be float32, uint16 (fp16 bits) or uint8")
    lay = tile_layout(width, height, world, 0, fp16, rgba8)
    if g.nbytes != world * lay["tile_bytes"]:
        raise ValueError(f"gathered holds {g.nbytes} bytes, expected {world} x {lay['tile_bytes']}")
    frame = np.empty((height, width, 4), g.dtype)
    _check(lib.rt_place_tiles_host(g.ctypes.data_as(ctypes.c_void_p), width, height, world,
                                   _pixel_flags(fp16, rgba8), frame.ctypes.data_as(ctypes.c_void_p)))
    return frame


def _plan_params(budget, count_min, count_max, radius, relative, luminance_floor) -> PlanParams:
    p = PlanParams()
    lib.rt_plan_params_default(ctypes.byref(p))
    p.budget, p.count_min, p.count_max, p.radius = budget, count_min, count_max, radius
    p.luminance_floor = luminance_floor
    p.flags = RT_PLAN_RELATIVE if relative else 0
    return p


def _plan_images(first, all, width=None):
    f = np.ascontiguousarray(first, dtype=np.float32)
    a = np.ascontiguousarray(all, dtype=np.float32)
    if f.ndim != 3 or f.shape[2] != 4 or a.shape != f.shape or (width is not None and f.shape[1] != width):
        raise ValueError("first and all must be (rows, W, 4) float32 images of one shape")
    return f, a


def plan_samples_host(first, all, budget: int, count_min: int = 0, count_max: int = 1 << 24, radius: int = 1,
                      relative: bool = False, luminance_floor: float = 0.01, return_stats: bool = False):
    """rt_plan_samples_host: the sample planner of ``Renderer.plan_samples`` in
    plain C++ on the host (no device, no scene), bit for bit the same counts.
    ``first`` / ``all``: (rows, W, 4) float32.  Returns the (rows, W) uint32
    counts, with ``return_stats`` also the rt_plan_stats as a dict."""
    f, a = _plan_images(first, all)
    p = _plan_params(budget, count_min, count_max, radius, relative, luminance_floor)
    p.rows = f.shape[0]
    counts = np.empty(f.shape[:2], np.uint32)
    s = PlanStats()
    _check(lib.rt_plan_samples_host(f.shape[1], ctypes.byref(p), f.ctypes.data_as(ctypes.c_void_p),
                                    a.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(s)))
    return (counts, s.as_dict()) if return_stats else counts


def _reproject_params(max_history, normal_cos_min, plane_rel, weight_min) -> ReprojectParams:
    p = ReprojectParams()
    lib.rt_reproject_params_default(ctypes.byref(p))
    p.max_history, p.normal_cos_min, p.plane_rel, p.weight_min = max_history, normal_cos_min, plane_rel, weight_min
    return p


def _planes(x, name):
    """One frame or a sequence of one or two frames -> list."""
    planes = list(x) if isinstance(x, (list, tuple)) else [x]
    if len(planes) not in (1, 2):
        raise ValueError(f"{name}: one or two planes")
    return planes


def _reproject_host_buffers(shape, color, history, hit, normal_depth, prev_hit, prev_normal_depth, out):
    """rt_reproject_buffers over host arrays: (buffers, arrays to keep alive, outs)."""
    color, history = _planes(color, "color"), _planes(history, "history")
    if len(history) != len(color):
        raise ValueError("color and history must have the same number of planes")
    outs = [np.empty(shape, np.float32) for _ in color] if out is None else _planes(out, "out")
    if len(outs) != len(color):
        raise ValueError("out must have as many planes as color")
    b, keep = ReprojectBuffers(), []

    def frame(a, name):
        if not isinstance(a, np.ndarray) or a.shape != shape:
            raise ValueError(f"{name} must be a {shape} float32 array")
        a = np.ascontiguousarray(a, dtype=np.float32)
        keep.append(a)
        return a.ctypes.data

    def hits(a, name):
        if not isinstance(a, np.ndarray) or a.nbytes != 8 * shape[0] * shape[1] or a.shape[:2] != shape[:2]:
            raise ValueError(f"{name} must hold one 8-byte (t, id) record per pixel of the {shape[:2]} frame")
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data

    for k in range(len(color)):
        b.color[k] = frame(color[k], f"color[{k}]")
        b.history[k] = frame(history[k], f"history[{k}]")
        o = outs[k]
        if not isinstance(o, np.ndarray) or o.dtype != np.float32 or o.shape != shape or not o.flags.c_contiguous:
            raise ValueError(f"out[{k}] must be a contiguous {shape} float32 array")
        b.out[k] = o.ctypes.data
    b.hit, b.prev_hit = hits(hit, "hit"), hits(prev_hit, "prev_hit")
    b.normal_depth = frame(normal_depth, "normal_depth")
    b.prev_normal_depth = frame(prev_normal_depth, "prev_normal_depth")
    return b, keep, outs


def reproject_host(camera: CameraGPU, prev_camera, color, history, hit, normal_depth, prev_hit, prev_normal_depth,
                   max_history: int = 32, normal_cos_min: float = 0.9, plane_rel: float = 2.0 ** -7,
                   weight_min: float = 0.0625, out=None) -> list:
    """rt_reproject_host: ``Renderer.reproject`` in plain C++ on the host (no
    device, no context), bit for bit the same planes.  ``camera`` is the
    current CameraGPU, ``prev_camera`` the previous one (None: it did not
    move); the buffers are numpy arrays as for the host path of
    :meth:`Renderer.reproject`.  Returns the list of output planes."""
    shape = (camera.resolution.y, camera.resolution.x, 4)
    b, keep, outs = _reproject_host_buffers(shape, color, history, hit, normal_depth, prev_hit, prev_normal_depth, out)
    p = _reproject_params(max_history, normal_cos_min, plane_rel, weight_min)
    _check(lib.rt_reproject_host(ctypes.byref(camera), ctypes.byref(prev_camera) if prev_camera is not None else None,
                                 ctypes.byref(p), ctypes.byref(b)))
    return outs


def _tri_bvh_dump(call, n: int, nodes_cap: int) -> dict:
    """Run ``call(dump)`` with buffers for ``n`` triangles and ``nodes_cap``
    nodes per layout; the rt_tri_bvh_dump as a dict of numpy arrays."""
    nodes = np.zeros((8 * nodes_cap, 4), np.uint32)
    srt = np.zeros((n, 12), np.float32)
    perm = np.zeros(n, np.uint32)
    isect = np.zeros((n, 12), np.float32)
    d = TriBvhDump()
    d.nodes, d.sorted, d.perm, d.isect = (a.ctypes.data for a in (nodes, srt, perm, isect))
    call(d)
    total = int(d.nodes_per_layout)
    assert int(d.n_triangles) == n and total <= nodes_cap
    return {"n_triangles": n, "nodes_per_layout": total, "leaf_max": int(d.leaf_max),
            "margin": np.float32(d.margin), "nodes": nodes[:8 * total].reshape(8, total, 4).copy(),
            "sorted": srt, "perm": perm, "isect": isect}


@dataclass
class Options:
    """rt_create_options (include/rtpt.h): per-context, speed-only choices --
    none changes a rendered value.  Defaults are the library's measured best.
    ``layout`` in ``LAYOUTS`` (auto, pairs, single, global, pairsmem, sorted,
    bvh), ``tri_build`` in ``TRI_BUILDS`` (default, host, lbvh, gpusah),
    ``walk`` in ``WALKS`` (auto, lockstep, free, sorted);
    ``walk_leaf_den`` the free scheduler's leaf-round threshold (0 = default)."""

    layout: str = "auto"
    lanes: int = 0
    tri_build: str = "default"
    tri_leaf_max: int = 0
    tri_leaf_cost: float = 0.0
    sphere_leaf_max: int = 0
    sphere_median: bool = False
    walk: str = "auto"
    walk_leaf_den: int = 0

    def c(self) -> CreateOptions:
        o = CreateOptions()
        o.scene_layout = LAYOUTS[self.layout]
        o.lanes_per_pixel = self.lanes
        o.tri_bvh_build = TRI_BUILDS[self.tri_build]
        o.tri_leaf_max = self.tri_leaf_max
        o.tri_leaf_cost = self.tri_leaf_cost
        o.sphere_leaf_max = self.sphere_leaf_max
        o.sphere_median = 1 if self.sphere_median else 0
        o.walk_scheduler = WALKS[self.walk]
        o.walk_leaf_den = self.walk_leaf_den
        return o

    # tools and the bench take their A/B knobs from the environment; the
    # library itself reads none (a stray variable cannot change a context)
    _ENV = {"layout": "RTPT_SCENE_MEM", "lanes": "RTPT_LANES", "tri_build": "RTPT_TRI_BUILD",
            "tri_leaf_max": "RTPT_TRI_LEAF", "tri_leaf_cost": "RTPT_TRI_CT",
            "sphere_leaf_max": "RTPT_BVH_LEAF", "walk": "RTPT_WALK"}

    @classmethod
    def from_env(cls, env=None) -> "Options":
        """Options from RTPT_* variables (bench.py / tools only)."""
        env = os.environ if env is None else env
        o = cls()
        for f in fields(cls):
            v = env.get(cls._ENV.get(f.name, ""))
            if v:
                setattr(o, f.name, type(getattr(o, f.name))(v) if f.type != "str" else v)
        if env.get("RTPT_BVH_SAH") == "0":
            o.sphere_median = True
        return o


class Scene:
    """The shaderTypes.h arrays of one scene (what Renderer.init uploads)."""

    def __init__(self, camera: CameraGPU, materials, vertices, light: SquareLightGPU,
                 spheres=None):
        self.camera = camera
        self.materials = materials            # (MaterialGPU * n_tri)
        self.vertices = vertices              # (float3 * 3n_tri), 16-B stride
        self.light = light
        self.spheres = spheres                # (SphereGPU * n_sph) or None

    @property
    def n_triangles(self) -> int:
        return len(self.materials)

    @property
    def n_spheres(self) -> int:
        return 0 if self.spheres is None else len(self.spheres)

    @property
    def width(self) -> int:
        return int(self.camera.resolution.x)

    @property
    def height(self) -> int:
        return int(self.camera.resolution.y)

    @classmethod
    def cornell_box(cls, width: int = 800, height: int = 600) -> "Scene":
        """initCornellBox() (scene.swift:14-62), resolution overridden."""
        cam, light = CameraGPU(), SquareLightGPU()
        mats = (MaterialGPU * 36)()
        verts = (float3 * 108)()
        n = ctypes.c_uint32()
        _check(lib.rt_scene_cornell_box(width, height, ctypes.byref(cam), mats, verts,
                                        ctypes.byref(light), ctypes.byref(n)))
        assert n.value == 36
        return cls(cam, mats, verts, light)

    @classmethod
    def cornell_box_mis(cls, width: int = 800, height: int = 600) -> "Scene":
        """The SwiftPM build's scene (Sources/gpuRaytracer/main.swift:21-67):
        the same room with a 1.5 x 1.5 light."""
        cam, light = CameraGPU(), SquareLightGPU()
        mats = (MaterialGPU * 36)()
        verts = (float3 * 108)()
        n = ctypes.c_uint32()
        _check(lib.rt_scene_cornell_box_mis(width, height, ctypes.byref(cam), mats, verts,
                                            ctypes.byref(light), ctypes.byref(n)))
        assert n.value == 36
        return cls(cam, mats, verts, light)

    @classmethod
    def random_spheres(cls, width: int = 1920, height: int = 1080, n_spheres: int = 1000,
                       seed: int = 42) -> "Scene":
        """Config-4 scene: Cornell walls + light + PCG32(seed) spheres."""
        cam, light = CameraGPU(), SquareLightGPU()
        mats = (MaterialGPU * 12)()
        verts = (float3 * 36)()
        sph = (SphereGPU * max(n_spheres, 1))()
        n = ctypes.c_uint32()
        _check(lib.rt_scene_random_spheres(width, height, n_spheres, ctypes.c_uint64(seed),
                                           ctypes.byref(cam), mats, verts, ctypes.byref(light),
                                           ctypes.byref(n), sph))
        return cls(cam, mats, verts, light, sph if n_spheres else None)

    @classmethod
    def random_triangles(cls, width: int = 1920, height: int = 1080, n: int = 100_000,
                         seed: int = 7, size: float = 0.25) -> "Scene":
        """Stress scene for the triangle BVH: the Cornell room (ids 0-35, light
        34-35) plus ``n`` random small triangles (ids 36..) inside it, diffuse
        albedo in [0.1, 0.9] (numpy PCG64 ``seed``)."""
        base = cls.cornell_box(width, height)
        rng = np.random.default_rng(seed)
        mats = (MaterialGPU * (36 + n))()
        verts = (float3 * (3 * (36 + n)))()
        ctypes.memmove(ctypes.addressof(mats), ctypes.addressof(base.materials), 36 * 48)
        ctypes.memmove(ctypes.addressof(verts), ctypes.addressof(base.vertices), 108 * 16)
        c = rng.uniform(-2.3, 2.3, size=(n, 1, 3)).astype(np.float32)
        e = rng.uniform(-size, size, size=(n, 2, 3)).astype(np.float32)
        tri = np.concatenate([c, c + e], axis=1).reshape(-1, 3)          # v0, v0+a, v0+b
        vv = np.frombuffer(verts, np.float32).reshape(-1, 4)
        vv[108:, :3] = tri
        mm = np.frombuffer(mats, np.float32).reshape(-1, 12)
        mm[36:, 0:3] = rng.uniform(0.1, 0.9, size=(n, 3)).astype(np.float32)
        mm[36:, 3] = 1.0
        mm[36:, 5] = 0.5
        return cls(base.camera, mats, verts, base.light)

    @classmethod
    def random_boxes(cls, width: int = 1920, height: int = 1080, n_boxes: int = 4,
                     seed: int = 3) -> "Scene":
        """Box-cluster stress scene: the Cornell room (walls = ids 0-9) plus
        ``n_boxes`` randomly rotated boxes (12 triangles each, one shared-edge
        pair per face) and the light rectangle last (numpy PCG64 ``seed``)."""
        base = cls.cornell_box(width, height)
        rng = np.random.default_rng(seed)
        n = 10 + 12 * n_boxes + 2
        mats = (MaterialGPU * n)()
        verts = (float3 * (3 * n))()
        ctypes.memmove(ctypes.addressof(mats), ctypes.addressof(base.materials), 10 * 48)
        ctypes.memmove(ctypes.addressof(verts), ctypes.addressof(base.vertices), 30 * 16)
        vv = np.frombuffer(verts, np.float32).reshape(-1, 4)
        mm = np.frombuffer(mats, np.float32).reshape(-1, 12)
        for b in range(n_boxes):
            c = rng.uniform(-1.8, 1.8, 3)
            h = rng.uniform(0.15, 0.7, 3)
            R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            col = rng.uniform(0.1, 0.9, 3)
            for f in range(6):
                a, s = f // 2, (1.0 if f % 2 else -1.0)
                i, j = (a + 1) % 3, (a + 2) % 3
                P = [c + s * h[a] * R[a] + u * h[i] * R[i] + v * h[j] * R[j]
                     for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
                for t, tri in enumerate(((P[0], P[1], P[2]), (P[0], P[2], P[3]))):
                    k = 10 + 12 * b + 2 * f + t
                    vv[3 * k:3 * k + 3, :3] = np.array(tri, np.float32)
                    mm[k, 0:3] = col
                    mm[k, 3] = 1.0
                    mm[k, 5] = 0.5
        ctypes.memmove(ctypes.addressof(mats) + (n - 2) * 48, ctypes.addressof(base.materials) + 34 * 48, 96)
        ctypes.memmove(ctypes.addressof(verts) + 3 * (n - 2) * 16,
                       ctypes.addressof(base.vertices) + 3 * 34 * 16, 96)
        return cls(base.camera, mats, verts, base.light)

    def describe(self, options: Options | None = None) -> dict:
        """Device layout rt_create would choose (rt_scene_describe_ex).
        ``kernel_layout`` and ``kernel_lds_bytes`` follow ``options.walk``
        (layouts 8-11 for free and sorted on a BVH scene): the launcher's own
        choice, the kernel ``Renderer.last_launch()`` names after a render of
        >= 1 bounce.  Only ``n_triangle_bvh_nodes`` is an estimate."""
        info = SceneInfo()
        opt = None if options is None else ctypes.byref(options.c())
        _check(lib.rt_scene_describe_ex(ctypes.byref(self.desc()), opt, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in SceneInfo._fields_}

    def cluster_kinds(self) -> list:
        """The flag word of each box cluster the scene compiles to, in the
        kernel's order (rt_debug_cluster_kinds): bits 0-2 world axes,
        8 container, 16 single face, 32 turned about one world axis, 64
        container with a shrunk box, 128 the light's own cluster."""
        flags = (ctypes.c_uint32 * 32)()
        n = ctypes.c_uint32()
        _check(lib.rt_debug_cluster_kinds(ctypes.byref(self.desc()), flags, 32, ctypes.byref(n)))
        return [int(flags[c]) for c in range(n.value)]

    def light_mask(self):
        """``(mask, records)``: the light mask the box-cluster kernel tests
        (rt_debug_light_mask; bit id: triangle id is a light)
        and the (n_triangles, 16) float32 shading records it is made from."""
        n = self.n_triangles
        mask = ctypes.c_uint64()
        rec = (ctypes.c_float * (16 * n))()
        _check(lib.rt_debug_light_mask(ctypes.byref(self.desc()), ctypes.byref(mask), rec, n))
        return int(mask.value), np.frombuffer(rec, np.float32).reshape(-1, 16).copy()

    def tri_bvh_host(self, options: "Options | None" = None) -> dict:
        """The triangle BVH of the host binned-SAH build for this scene
        (rt_debug_tri_bvh_host; no device), as ``Renderer.tri_bvh`` returns a
        context's: what a ``tri_build="host"`` context with these options
        uploads.  Built at any triangle count >= 1."""
        n = self.n_triangles
        opt = None if options is None else ctypes.byref(options.c())
        desc = self.desc()
        return _tri_bvh_dump(lambda d: _check(lib.rt_debug_tri_bvh_host(ctypes.byref(desc), opt, ctypes.byref(d))),
                             n, max(2 * n - 1, 1))

    def tri_bvh_refit_host(self, updated: "Scene", options: "Options | None" = None) -> dict:
        """``tri_bvh_host(options)`` of this scene refitted onto the triangles
        of ``updated`` (rt_debug_tri_bvh_refit_host; no device): what a
        ``tri_build="host"`` context created from this scene holds after
        ``Renderer.update_scene(updated)``.  Same dict as ``tri_bvh_host``."""
        n = self.n_triangles
        opt = None if options is None else ctypes.byref(options.c())
        a, b = self.desc(), updated.desc()
        return _tri_bvh_dump(lambda d: _check(lib.rt_debug_tri_bvh_refit_host(ctypes.byref(a), opt, ctypes.byref(b),
                                                                              ctypes.byref(d))),
                             n, max(2 * n - 1, 1))

    def ray_domain(self) -> dict:
        """The exactness domain of ``Renderer.trace_rays`` for this scene
        (rt_debug_ray_domain): ``origin_max``,
        ``dir_len2_min``, ``dir_len2_max``, ``tmax_max``.  Rays inside it take
        the accelerated layout, every other ray the id-ordered loop; the
        answers are the same."""
        info = RayDomainInfo()
        _check(lib.rt_debug_ray_domain(ctypes.byref(self.desc()), ctypes.byref(info)))
        return {k: float(getattr(info, k)) for k, _ in RayDomainInfo._fields_}

    def desc(self, device: int = 0) -> SceneDesc:
        d = SceneDesc()
        d.camera = ctypes.pointer(self.camera)
        d.materials = ctypes.cast(self.materials, ctypes.POINTER(MaterialGPU))
        d.square_lights = ctypes.pointer(self.light)
        d.n_square_lights = 1
        d.vertices = ctypes.cast(self.vertices, ctypes.POINTER(float3))
        d.n_triangles = self.n_triangles
        if self.spheres is not None:
            d.spheres = ctypes.cast(self.spheres, ctypes.POINTER(SphereGPU))
            d.n_spheres = self.n_spheres
        d.device = device
        return d


@dataclass
class RenderParams:
    """rt_render_params (include/rtpt.h)."""

    spp: int = 400          # raytrace.metal:24
    bounces: int = 3        # raytrace.metal:25
    sample_base: int = 0
    row_start: int = 0
    row_step: int = 1
    row_count: int = 0      # 0 = every row from row_start with row_step
    accumulate: bool = False
    keep_sum: bool = False
    fp16: bool = False
    rgba8: bool = False     # the fused image.swift:35-65 epilogue (RT_OUT_RGBA8)

    def c(self, flags: int = 0) -> RenderParamsC:
        p = RenderParamsC()
        p.spp, p.bounces, p.sample_base = self.spp, self.bounces, self.sample_base
        p.row_start, p.row_step, p.row_count = self.row_start, self.row_step, self.row_count
        p.accumulate = 1 if self.accumulate else 0
        p.flags = (flags | (RT_KEEP_SUM if self.keep_sum else 0) | (RT_OUT_FP16 if self.fp16 else 0)
                   | (RT_OUT_RGBA8 if self.rgba8 else 0))
        return p

    def rows(self, height: int) -> int:
        if self.row_count:
            return self.row_count
        step = self.row_step or 1
        return (height - 1 - self.row_start) // step + 1


@dataclass
class MisParams:
    """rt_mis_params (include/rtpt.h): kernel drawTriangle of the SwiftPM build."""

    camera_rays: int = 6    # cameraRaysPerPixel, Sources/gpuRaytracer/shaders.metal:644
    mis_samples: int = 300  # misSamples, :648
    row_start: int = 0
    row_step: int = 1
    row_count: int = 0

    def c(self, flags: int = 0) -> MisParamsC:
        p = MisParamsC()
        p.camera_rays, p.mis_samples = self.camera_rays, self.mis_samples
        p.row_start, p.row_step, p.row_count = self.row_start, self.row_step, self.row_count
        p.flags = flags
        return p

    def rows(self, height: int) -> int:
        return RenderParams(row_start=self.row_start, row_step=self.row_step,
                            row_count=self.row_count).rows(height)


class Renderer:
    """renderer.swift's Renderer on the MI355X C-ABI."""

    def __init__(self, scene: Scene, device: int = 0, seeds=None,
                 seed_key: int = DEFAULT_SEED_KEY, options: Options | None = None):
        self.scene = scene
        self.device = device
        self.options = options or Options()
        ctx = ctypes.c_void_p()
        _check(lib.rt_create_ex(ctypes.byref(scene.desc(device)), ctypes.byref(self.options.c()),
                                ctypes.byref(ctx)))
        self._ctx = ctx
        if seeds is not None:
            s = np.ascontiguousarray(seeds, dtype=np.uint32)
            if s.size != scene.width * scene.height:
                raise ValueError("seed texture must have width*height entries")
            _check(lib.rt_set_seeds(ctx, s.ctypes.data_as(ctypes.c_void_p), scene.width,
                                    scene.height), ctx)
        else:
            _check(lib.rt_fill_seeds(ctx, ctypes.c_uint64(seed_key)), ctx)

    def close(self):
        if getattr(self, "_ctx", None):
            lib.rt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update_scene(self, scene: Scene, rebuild: bool = False):
        """rt_update_scene: replace the context's scene in place (same triangle
        and sphere counts and resolution).  Afterwards every call returns what
        a new ``Renderer(scene, options=...)`` with the same seeds returns, bit
        for bit.  The triangle BVH is refitted on the device (its topology
        kept), or rebuilt by the context's builder with ``rebuild``.  Seeds are
        kept, the running sum of ``keep_sum`` is dropped.  An argument error
        (RtError, RT_ERR_INVALID_ARG) leaves the context as it was."""
        _check(lib.rt_update_scene(self._ctx, ctypes.byref(scene.desc(self.device)),
                                   RT_UPDATE_REBUILD if rebuild else 0), self._ctx)
        self.scene = scene

    def update_info(self) -> dict:
        """rt_update_info of the last successful ``update_scene``: ``tri_bvh``
        (0 no tree, 1 refitted, 2 rebuilt), ``updates`` so far, and the wall ms
        of the compile, the upload and the whole call; ``tri_bvh_ms`` is the
        refit kernels' device time or the rebuild's wall time.  RtError
        (RT_ERR_STATE) before the first update."""
        u = UpdateStats()
        _check(lib.rt_update_info(self._ctx, ctypes.byref(u)), self._ctx)
        return {k: getattr(u, k) for k, _ in UpdateStats._fields_ if k != "reserved"}

    def set_seeds(self, seeds):
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        _check(lib.rt_set_seeds(self._ctx, s.ctypes.data_as(ctypes.c_void_p), self.scene.width,
                                self.scene.height), self._ctx)

    def render(self, params: RenderParams | None = None, out=None, stream=None):
        """Render into host memory (returns (rows, W, 4) float32, uint16 bits
        for fp16, uint8 for rgba8), or into a device tensor ``out`` (anything with
        ``data_ptr()``) enqueued on ``stream`` (a raw hipStream_t int / torch
        stream; default torch's current stream) without a host sync."""
        p = params or RenderParams()
        if out is None:
            rows = p.rows(self.scene.height)
            dt = np.uint8 if p.rgba8 else np.uint16 if p.fp16 else np.float32
            img = np.empty((rows, self.scene.width, 4), dtype=dt)
            _check(lib.rt_render(self._ctx, ctypes.byref(p.c()),
                                 img.ctypes.data_as(ctypes.c_void_p)), self._ctx)
            return img
        if stream is None:
            import torch  # plumbing only: the stream the caller's events see
            stream = torch.cuda.current_stream().cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        ptr = out if isinstance(out, int) else out.data_ptr()
        _check(lib.rt_render_async(self._ctx, ctypes.byref(p.c(RT_OUT_DEVICE)),
                                   ctypes.c_void_p(ptr), ctypes.c_void_p(stream)), self._ctx)
        return out

    def trace_rays(self, rays, any_hit: bool = False, exact: bool = False, out=None, stream=None):
        """Batched ray queries (rt_trace_rays): ``rays`` is (n, 8) float32,
        (origin.xyz, tmin, dir.xyz, tmax) per ray.  Closest hit: ``id`` is the
        primitive (triangles first, then the spheres; -1 for a miss) and ``t``
        its parameter (a miss: the ray's tmax); ``any_hit``: ``id`` is 1 or 0
        and ``t`` 0.  ``exact`` sends every ray through the id-ordered loop.

        A numpy array gives ``(t float32[n], id int32[n])`` synchronously.  A
        torch tensor on the context's device takes the device path and gives
        torch tensors (views of ``out``, an (n, 2) int32 tensor, when given);
        with ``stream`` the call is enqueued there without a host sync."""
        flags = (RT_RAYS_ANY if any_hit else 0) | (RT_RAYS_EXACT if exact else 0)
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, dtype=np.float32)
            if r.ndim != 2 or r.shape[1] != 8:
                raise ValueError("rays must have shape (n, 8)")
            n = r.shape[0]
            hits = np.empty((n, 2), np.int32) if out is None else out
            if hits.dtype != np.int32 or hits.shape != (n, 2) or not hits.flags.c_contiguous:
                raise ValueError("out must be a contiguous (n, 2) int32 array")
            _check(lib.rt_trace_rays(self._ctx, r.ctypes.data_as(ctypes.c_void_p), n, flags,
                                     hits.ctypes.data_as(ctypes.c_void_p)), self._ctx)
            return hits[:, 0].view(np.float32), hits[:, 1]
        import torch  # plumbing only: device memory and the caller's stream
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous (n, 8) float32 tensor")
        if not rays.is_cuda or rays.device.index != self.device:
            raise ValueError("rays must live on the context's device")
        n = rays.shape[0]
        hits = torch.empty((n, 2), dtype=torch.int32, device=rays.device) if out is None else out
        if (hits.dtype != torch.int32 or tuple(hits.shape) != (n, 2) or not hits.is_contiguous()
                or hits.device != rays.device):
            raise ValueError("out must be a contiguous (n, 2) int32 tensor on the rays' device")
        # without a stream: on torch's current stream (after whatever produced
        # the rays there), then wait for it
        cur = torch.cuda.current_stream(rays.device) if stream is None else None
        handle = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        _check(lib.rt_trace_rays_async(self._ctx, ctypes.c_void_p(rays.data_ptr()), n, flags,
                                       ctypes.c_void_p(hits.data_ptr()), ctypes.c_void_p(handle)), self._ctx)
        if cur is not None:
            cur.synchronize()
        return hits[:, 0].view(torch.float32), hits[:, 1]

    def trace_paths(self, rays, spp: int = 1, bounces: int = 3, sample_base: int = 0, seeds=None,
                    seed_key: int = DEFAULT_SEED_KEY, lanes: int = 0, first_hits: bool = False, out=None,
                    stream=None):
        """Path-traced radiance along the caller's rays (rt_trace_paths,
        DESIGN.md §3.28): ``rays`` is (n, 8) float32 as for :meth:`trace_rays`;
        ray r draws samples ``[sample_base, sample_base + spp)`` of the Halton
        index ``(seeds[r] & 0xFFFFF) + n`` (``seeds=None``: the value
        ``seed_splitmix(n, 1, seed_key)`` gives r) and the result is the
        (n, 4) float32 mean radiance with alpha 1; a ray outside the exactness
        domain is not traced and gets (0, 0, 0, 0).  ``lanes``: 0 (automatic),
        1 or 16 lanes per ray.  ``first_hits=True`` also returns the first
        segment's ``(t, id)`` as :meth:`trace_rays` gives it.

        Numpy arrays give numpy results synchronously.  Torch tensors on the
        context's device take the device path: ``out`` is an (n, 4) float32
        tensor, or with ``first_hits`` a pair of it and an (n, 2) int32 tensor;
        with ``stream`` the call is enqueued there without a host sync."""
        p = PathParamsC()
        lib.rt_path_params_default(ctypes.byref(p))
        p.spp, p.bounces, p.sample_base, p.lanes_per_ray, p.seed_key = spp, bounces, sample_base, lanes, seed_key
        out_rad, out_hits = (out if isinstance(out, (tuple, list)) else (out, None))
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, dtype=np.float32)
            if r.ndim != 2 or r.shape[1] != 8:
                raise ValueError("rays must have shape (n, 8)")
            n = r.shape[0]
            sd = None
            if seeds is not None:
                sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
                if sd.shape[0] != n:
                    raise ValueError("seeds must hold one value per ray")
            rad = np.empty((n, 4), np.float32) if out_rad is None else out_rad
            if rad.dtype != np.float32 or rad.shape != (n, 4) or not rad.flags.c_contiguous:
                raise ValueError("out must be a contiguous (n, 4) float32 array")
            hits = None
            if first_hits:
                hits = np.empty((n, 2), np.int32) if out_hits is None else out_hits
                if hits.dtype != np.int32 or hits.shape != (n, 2) or not hits.flags.c_contiguous:
                    raise ValueError("the first hits must be a contiguous (n, 2) int32 array")
            _check(lib.rt_trace_paths(self._ctx, ctypes.byref(p), r.ctypes.data_as(ctypes.c_void_p),
                                      None if sd is None else sd.ctypes.data_as(ctypes.c_void_p), n,
                                      rad.ctypes.data_as(ctypes.c_void_p),
                                      None if hits is None else hits.ctypes.data_as(ctypes.c_void_p)), self._ctx)
            return (rad, (hits[:, 0].view(np.float32), hits[:, 1])) if first_hits else rad
        import torch  # plumbing only: device memory and the caller's stream
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous (n, 8) float32 tensor")
        if not rays.is_cuda or rays.device.index != self.device:
            raise ValueError("rays must live on the context's device")
        n = rays.shape[0]

        def on_device(t, dtype, shape, what):
            if (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != rays.device):
                raise ValueError(f"{what} must be a contiguous {shape} {dtype} tensor on the rays' device")
            return t

        sd_ptr = None
        if seeds is not None:  # int32 tensors carry the 32 bits (torch has little uint32 support)
            if seeds.dtype not in (torch.int32, torch.uint32):
                raise ValueError("seeds must be an int32 or uint32 tensor")
            sd_ptr = on_device(seeds, seeds.dtype, (n,), "seeds").data_ptr()
        rad = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if out_rad is None else out_rad
        on_device(rad, torch.float32, (n, 4), "out")
        hits = None
        if first_hits:
            hits = torch.empty((n, 2), dtype=torch.int32, device=rays.device) if out_hits is None else out_hits
            on_device(hits, torch.int32, (n, 2), "the first hits")
        p.flags = RT_OUT_DEVICE
        cur = torch.cuda.current_stream(rays.device) if stream is None else None
        handle = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        _check(lib.rt_trace_paths_async(self._ctx, ctypes.byref(p), ctypes.c_void_p(rays.data_ptr()),
                                        None if sd_ptr is None else ctypes.c_void_p(sd_ptr), n,
                                        ctypes.c_void_p(rad.data_ptr()),
                                        None if hits is None else ctypes.c_void_p(hits.data_ptr()),
                                        ctypes.c_void_p(handle)), self._ctx)
        if cur is not None:
            cur.synchronize()
        return (rad, (hits[:, 0].view(torch.float32), hits[:, 1])) if first_hits else rad

    def render_aov(self, spp: int = 1, sample_base: int = 0, row_start: int = 0, row_step: int = 1,
                   row_count: int = 0, center: bool = False, albedo: bool = True,
                   normal_depth: bool = True, first_hit: bool = True, out=None, stream=None) -> dict:
        """First-hit feature buffers (rt_render_aov) of the
        camera rays of samples ``[sample_base, sample_base + spp)``: a dict with
        ``albedo`` (rows, W, 4) float32 = (mean diffuse.rgb, coverage),
        ``normal_depth`` (rows, W, 4) float32 = (mean N.xyz, mean t; misses
        count as zero) and ``first_hit`` (rows, W) structured ``(t, id)`` of
        sample ``sample_base`` (a miss: t = 1000, id = -1), for the buffers
        asked for.  ``center``: one ray through every pixel centre (spp 1, no
        seeds needed) -- the picking / id-buffer form.

        ``out``: a dict of contiguous torch tensors on the context's device,
        (rows, W, 4) float32 under ``albedo`` / ``normal_depth`` and (rows, W, 2)
        int32 (t bits, id) under ``first_hit``; only its keys are rendered, on
        ``stream`` without a host sync (default: torch's current stream, then
        waited for).  Returns ``out``."""
        p = AovParams()
        p.spp, p.sample_base = spp, sample_base
        p.row_start, p.row_step, p.row_count = row_start, row_step, row_count
        p.flags = RT_AOV_CENTER if center else 0
        rows = RenderParams(row_start=row_start, row_step=row_step, row_count=row_count).rows(self.scene.height)
        W = self.scene.width
        b = AovBuffers()
        if out is None:
            res = {}
            if albedo:
                res["albedo"] = np.empty((rows, W, 4), np.float32)
            if normal_depth:
                res["normal_depth"] = np.empty((rows, W, 4), np.float32)
            if first_hit:
                res["first_hit"] = np.empty((rows, W), np.dtype([("t", np.float32), ("id", np.int32)]))
            for k, a in res.items():
                setattr(b, k, a.ctypes.data)
            _check(lib.rt_render_aov(self._ctx, ctypes.byref(p), ctypes.byref(b)), self._ctx)
            return res
        import torch  # plumbing only: device memory and the caller's stream
        shapes = {"albedo": ((rows, W, 4), torch.float32), "normal_depth": ((rows, W, 4), torch.float32),
                  "first_hit": ((rows, W, 2), torch.int32)}
        for k, t in out.items():
            if k not in shapes:
                raise ValueError(f"unknown buffer {k!r}")
            shape, dt = shapes[k]
            if (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"out[{k!r}] must be a contiguous {shape} {dt} tensor on the context's device")
            setattr(b, k, t.data_ptr())
        p.flags |= RT_OUT_DEVICE
        cur = torch.cuda.current_stream(self.device) if stream is None else None
        handle = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        _check(lib.rt_render_aov_async(self._ctx, ctypes.byref(p), ctypes.byref(b), ctypes.c_void_p(handle)),
               self._ctx)
        if cur is not None:
            cur.synchronize()
        return out

    def denoise(self, color_a, color_b, albedo, normal_depth, iterations: int = 5, normal_power_log2: int = 7,
                sigma_luminance: float = 4.0, sigma_depth: float = 1.0, depth_floor: float = 0.01, out=None,
                stream=None):
        """Variance-guided a-trous denoiser (rt_denoise).
        ``color_a`` / ``color_b``: renders of the first and the second half of
        the samples, ``albedo`` / ``normal_depth``: ``render_aov`` of all of
        them; whole frames, (H, W, 4) float32 each.  Returns the filtered
        (H, W, 4) image: an estimate of the mean of the halves, alpha from
        ``color_a``.

        numpy arrays take the host path and block.  Contiguous float32 torch
        tensors on the context's device take the device path, enqueued on
        ``stream`` without a host sync (default: torch's current stream, then
        waited for).  ``out`` (same kind and shape) may be ``color_a`` or
        ``color_b``."""
        p = DenoiseParams()
        p.iterations, p.normal_power_log2 = iterations, normal_power_log2
        p.sigma_luminance, p.sigma_depth, p.depth_floor = sigma_luminance, sigma_depth, depth_floor
        shape = (self.scene.height, self.scene.width, 4)
        bufs = {"color_a": color_a, "color_b": color_b, "albedo": albedo, "normal_depth": normal_depth}
        b = DenoiseBuffers()
        if isinstance(color_a, np.ndarray):
            keep = []
            for k, a in bufs.items():
                if not isinstance(a, np.ndarray) or a.shape != shape:
                    raise ValueError(f"{k} must be a {shape} float32 array")
                a = np.ascontiguousarray(a, dtype=np.float32)
                keep.append(a)
                setattr(b, k, a.ctypes.data)
            res = np.empty(shape, np.float32) if out is None else out
            if (not isinstance(res, np.ndarray) or res.dtype != np.float32 or res.shape != shape
                    or not res.flags.c_contiguous):
                raise ValueError(f"out must be a contiguous {shape} float32 array")
            b.out = res.ctypes.data
            _check(lib.rt_denoise(self._ctx, ctypes.byref(p), ctypes.byref(b)), self._ctx)
            return res
        import torch  # plumbing only: device memory and the caller's stream
        res = torch.empty(shape, dtype=torch.float32, device=color_a.device) if out is None else out
        for k, t in dict(bufs, out=res).items():
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32
                    or not t.is_contiguous() or not t.is_cuda or t.device.index != self.device):
                raise ValueError(f"{k} must be a contiguous {shape} float32 tensor on the context's device")
            setattr(b, k, t.data_ptr())
        p.flags = RT_OUT_DEVICE
        cur = torch.cuda.current_stream(self.device) if stream is None else None
        handle = cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
        _check(lib.rt_denoise_async(self._ctx, ctypes.byref(p), ctypes.byref(b), ctypes.c_void_p(handle)), self._ctx)
        if cur is not None:
            cur.synchronize()
        return res

    def render_denoised(self, params: RenderParams | None = None, return_inputs: bool = False, stream=None,
                        **filter_args):
        """A denoised render of ``params.spp`` samples: two renders of
        ``spp / 2`` samples at ``sample_base`` and ``sample_base + spp / 2``,
        the feature buffers of all ``spp`` samples, and :meth:`denoise` (its
        keyword arguments pass through), all on device tensors and one stream
        (default: torch's current stream), then waited for.  Returns the
        (H, W, 4) float32 torch tensor; with ``return_inputs`` also the dict of
        the four inputs.  Needs an even ``spp`` >= 2 and whole float32 frames."""
        p = params or RenderParams()
        H, W = self.scene.height, self.scene.width
        if p.spp < 2 or p.spp % 2:
            raise ValueError("render_denoised needs an even spp >= 2 (two halves)")
        if p.row_start != 0 or p.row_step not in (0, 1) or p.row_count not in (0, H):
            raise ValueError("render_denoised needs whole frames (no row partition)")
        if p.accumulate or p.keep_sum or p.fp16 or p.rgba8:
            raise ValueError("render_denoised renders plain float32 frames (no accumulate, keep_sum, fp16, rgba8)")
        import torch  # plumbing only: device memory and the caller's stream
        dev = torch.device("cuda", self.device)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        half = p.spp // 2
        new = lambda: torch.empty((H, W, 4), dtype=torch.float32, device=dev)  # noqa: E731
        inputs = {"color_a": new(), "color_b": new(), "albedo": new(), "normal_depth": new()}
        self.render(RenderParams(spp=half, bounces=p.bounces, sample_base=p.sample_base), out=inputs["color_a"],
                    stream=s)
        self.render(RenderParams(spp=half, bounces=p.bounces, sample_base=p.sample_base + half),
                    out=inputs["color_b"], stream=s)
        self.render_aov(spp=p.spp, sample_base=p.sample_base,
                        out={k: inputs[k] for k in ("albedo", "normal_depth")}, stream=s)
        img = self.denoise(**inputs, stream=s, **filter_args)
        if hasattr(s, "synchronize"):
            s.synchronize()
        return (img, inputs) if return_inputs else img

    def reproject(self, color, history, hit, normal_depth, prev_hit, prev_normal_depth, prev_camera=None,
                  max_history: int = 32, normal_cos_min: float = 0.9, plane_rel: float = 2.0 ** -7,
                  weight_min: float = 0.0625, out=None, stream=None) -> list:
        """Temporal reprojection (rt_reproject): this frame's
        ``color`` plane(s) blended with the previous frame's ``history``
        plane(s), gathered where this frame's surface points were seen from
        ``prev_camera`` (a CameraGPU; None: the camera did not move).  The
        current camera is the context's.  ``color`` / ``history`` / ``out``: one
        (H, W, 4) float32 frame or a sequence of one or two; ``hit`` /
        ``normal_depth``: this frame's ``render_aov(center=True)`` buffers,
        ``prev_hit`` / ``prev_normal_depth``: the previous frame's.  Returns the
        list of output planes (rgb mean, alpha = history length); they are the
        next call's ``history``.

        numpy arrays take the host path and block.  Contiguous torch tensors on
        the context's device (hits as (H, W, 2) int32) take the device path,
        enqueued on ``stream`` without a host sync (default: torch's current
        stream, then waited for).  ``out[k]`` may be ``color[k]``; it must not
        overlap a history plane."""
        p = _reproject_params(max_history, normal_cos_min, plane_rel, weight_min)
        H, W = self.scene.height, self.scene.width
        shape = (H, W, 4)
        cam = ctypes.byref(prev_camera) if prev_camera is not None else None
        first = _planes(color, "color")[0]
        if isinstance(first, np.ndarray):
            b, keep, outs = _reproject_host_buffers(shape, color, history, hit, normal_depth, prev_hit,
                                                    prev_normal_depth, out)
            _check(lib.rt_reproject(self._ctx, ctypes.byref(p), cam, ctypes.byref(b)), self._ctx)
            return outs
        import torch  # plumbing only: device memory and the caller's stream
        color, history = _planes(color, "color"), _planes(history, "history")
        outs = [torch.empty(shape, dtype=torch.float32, device=first.device) for _ in color] if out is None \
            else _planes(out, "out")
        if len(history) != len(color) or len(outs) != len(color):
            raise ValueError("color, history and out must have the same number of planes")
        b = ReprojectBuffers()

        def ptr(t, name, shp=shape, dt=torch.float32):
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous()
                    or not t.is_cuda or t.device.index != self.device):
                raise ValueError(f"{name} must be a contiguous {shp} {dt} tensor on the context's device")
            return t.data_ptr()

        for k in range(len(color)):
            b.color[k] = ptr(color[k], f"color[{k}]")
            b.history[k] = ptr(history[k], f"history[{k}]")
            b.out[k] = ptr(outs[k], f"out[{k}]")
        b.hit = ptr(hit, "hit", (H, W, 2), torch.int32)
        b.prev_hit = ptr(prev_hit, "prev_hit", (H, W, 2), torch.int32)
        b.normal_depth = ptr(normal_depth, "normal_depth")
        b.prev_normal_depth = ptr(prev_normal_depth, "prev_normal_depth")
        p.flags = RT_OUT_DEVICE
        cur, handle = self._stream_handle(stream)
        _check(lib.rt_reproject_async(self._ctx, ctypes.byref(p), cam, ctypes.byref(b), ctypes.c_void_p(handle)),
               self._ctx)
        if cur is not None:
            cur.synchronize()
        return outs

    def render_temporal(self, params: RenderParams | None = None, state=None, denoise: bool = True, stream=None,
                        reproject_args: dict | None = None, **filter_args):
        """One frame of a temporally accumulated sequence: returns
        ``(image, state)``; pass ``state`` to the next call (after
        :meth:`update_scene` when the camera moved), ``state=None`` starts a
        sequence.  Frame ``f`` renders ``spp / 2 + spp / 2`` samples at
        ``sample_base + f * spp`` (so frames draw different samples) and the
        centre feature buffers, reprojects both planes against ``state`` (the
        previous camera, hit, normal_depth and both outputs;
        ``reproject_args`` pass to :meth:`reproject`) and, with ``denoise``,
        filters the accumulated planes with the jittered feature buffers of
        the frame's samples as :meth:`render_denoised` does (``filter_args``
        pass to :meth:`denoise`); without it ``image`` is the list of the two
        accumulated planes.  Everything runs on device tensors and one stream (default:
        torch's current stream), then waited for.  The image's alpha is plane
        0's history length (1: no history reused).  Needs an even ``spp`` >= 2 and whole float32
        frames."""
        p = params or RenderParams()
        H, W = self.scene.height, self.scene.width
        if p.spp < 2 or p.spp % 2:
            raise ValueError("render_temporal needs an even spp >= 2 (two halves)")
        if p.row_start != 0 or p.row_step not in (0, 1) or p.row_count not in (0, H):
            raise ValueError("render_temporal needs whole frames (no row partition)")
        if p.accumulate or p.keep_sum or p.fp16 or p.rgba8:
            raise ValueError("render_temporal renders plain float32 frames (no accumulate, keep_sum, fp16, rgba8)")
        import torch  # plumbing only: device memory and the caller's stream
        dev = torch.device("cuda", self.device)
        s = torch.cuda.current_stream(dev) if stream is None else stream
        frame = 0 if state is None else state["frame"] + 1
        half, base = p.spp // 2, p.sample_base + frame * p.spp
        new = lambda: torch.empty((H, W, 4), dtype=torch.float32, device=dev)  # noqa: E731
        planes = [new(), new()]
        self.render(RenderParams(spp=half, bounces=p.bounces, sample_base=base), out=planes[0], stream=s)
        self.render(RenderParams(spp=half, bounces=p.bounces, sample_base=base + half), out=planes[1], stream=s)
        centre = {"normal_depth": new(), "first_hit": torch.empty((H, W, 2), dtype=torch.int32, device=dev)}
        self.render_aov(center=True, out=centre, stream=s)
        if state is not None:
            self.reproject(planes, state["out"], centre["first_hit"], centre["normal_depth"], state["hit"],
                           state["normal_depth"], prev_camera=state["camera"], out=planes, stream=s,
                           **(reproject_args or {}))
        img = planes
        if denoise:
            aov = {"albedo": new(), "normal_depth": new()}
            self.render_aov(spp=p.spp, sample_base=base, out=aov, stream=s)
            img = self.denoise(planes[0], planes[1], aov["albedo"], aov["normal_depth"], stream=s, **filter_args)
        if hasattr(s, "synchronize"):
            s.synchronize()
        state = {"frame": frame, "camera": CameraGPU.from_buffer_copy(self.scene.camera), "out": planes,
                 "hit": centre["first_hit"], "normal_depth": centre["normal_depth"]}
        return img, state

    def _stream_handle(self, stream):
        """(torch stream to wait for or None, raw hipStream_t) for a device call."""
        import torch  # plumbing only: the caller's stream
        cur = torch.cuda.current_stream(self.device) if stream is None else None
        return cur, (cur.cuda_stream if stream is None else getattr(stream, "cuda_stream", stream))

    def render_counts(self, params: RenderParams, counts, out=None, totals=None, stream=None):
        """rt_render_counts: :meth:`render` with one sample
        count per pixel.  ``counts`` is (rows, W) uint32 in the layout of the
        image; ``params.spp`` is a cap, pixel p draws ``min(counts[p], spp)``
        samples after the ``k_p`` its running sum holds (``accumulate``), and
        equals the same pixel of ``render`` at ``spp = total_p`` from
        ``sample_base``, bit for bit.  ``options.lanes_per_pixel`` is ignored.

        A numpy ``counts`` takes the host path and blocks; a contiguous 4-byte
        integer torch tensor on the context's device takes the device path,
        enqueued on ``stream`` without a host sync (default: torch's current
        stream, then waited for), with ``out`` a device tensor (allocated when
        None).  ``totals``: True, or an array / tensor like ``counts``, to
        receive the per-pixel totals.  Returns the image, or ``(image,
        totals)`` when totals were asked for."""
        p = params
        rows, W = p.rows(self.scene.height), self.scene.width
        if isinstance(counts, np.ndarray):
            cn = np.ascontiguousarray(counts, dtype=np.uint32)
            if cn.shape != (rows, W):
                raise ValueError(f"counts must have shape {(rows, W)}")
            dt = np.uint8 if p.rgba8 else np.uint16 if p.fp16 else np.float32
            img = np.empty((rows, W, 4), dtype=dt) if out is None else out
            if not isinstance(img, np.ndarray) or img.dtype != dt or img.shape != (rows, W, 4) or not img.flags.c_contiguous:
                raise ValueError(f"out must be a contiguous {(rows, W, 4)} {np.dtype(dt)} array")
            tot = np.empty((rows, W), np.uint32) if totals is True else totals
            if tot is not None and (not isinstance(tot, np.ndarray) or tot.dtype != np.uint32 or tot.shape != (rows, W)
                                    or not tot.flags.c_contiguous):
                raise ValueError(f"totals must be a contiguous {(rows, W)} uint32 array")
            _check(lib.rt_render_counts(self._ctx, ctypes.byref(p.c()), cn.ctypes.data_as(ctypes.c_void_p),
                                        img.ctypes.data_as(ctypes.c_void_p),
                                        None if tot is None else tot.ctypes.data_as(ctypes.c_void_p)), self._ctx)
            return img if tot is None else (img, tot)
        import torch  # plumbing only: device memory and the caller's stream

        def word_tensor(t, name):
            if (not isinstance(t, torch.Tensor) or t.element_size() != 4 or t.is_floating_point()
                    or tuple(t.shape) != (rows, W) or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"{name} must be a contiguous {(rows, W)} 4-byte integer tensor on the context's device")
        word_tensor(counts, "counts")
        dt = torch.uint8 if p.rgba8 else torch.float16 if p.fp16 else torch.float32
        img = torch.empty((rows, W, 4), dtype=dt, device=counts.device) if out is None else out
        tot = torch.empty((rows, W), dtype=torch.int32, device=counts.device) if totals is True else totals
        if tot is not None:
            word_tensor(tot, "totals")
        cur, handle = self._stream_handle(stream)
        ptr = img if isinstance(img, int) else img.data_ptr()
        _check(lib.rt_render_counts_async(self._ctx, ctypes.byref(p.c(RT_OUT_DEVICE)), ctypes.c_void_p(counts.data_ptr()),
                                          ctypes.c_void_p(ptr), ctypes.c_void_p(None if tot is None else tot.data_ptr()),
                                          ctypes.c_void_p(handle)), self._ctx)
        if cur is not None:
            cur.synchronize()
        return img if tot is None else (img, tot)

    def plan_samples(self, first, all, budget: int, count_min: int = 0, count_max: int = 1 << 24, radius: int = 1,
                     relative: bool = False, luminance_floor: float = 0.01, counts=None, return_stats: bool = False,
                     stream=None):
        """rt_plan_samples: sample counts from a pilot
        render.  ``first`` / ``all``: (rows, W, 4) float32 images of the
        pilot's first half and of all its samples.  ``budget`` samples are
        handed out over the tile beyond ``count_min`` each, in proportion to
        the ``radius``-dilated luminance change between the two images
        (``relative``: divided by ``lum(all) + luminance_floor``), each count
        capped at ``count_max``.  numpy arrays take the host path; contiguous
        torch tensors on the context's device the device path on ``stream``
        (default: torch's current stream, then waited for).  Returns the
        (rows, W) counts (uint32 array / int32 tensor), with ``return_stats``
        also the rt_plan_stats as a dict (the device path then waits)."""
        p = _plan_params(budget, count_min, count_max, radius, relative, luminance_floor)
        W = self.scene.width
        s = PlanStats()
        if isinstance(first, np.ndarray):
            f, a = _plan_images(first, all, W)
            p.rows = f.shape[0]
            cn = np.empty(f.shape[:2], np.uint32) if counts is None else counts
            if not isinstance(cn, np.ndarray) or cn.dtype != np.uint32 or cn.shape != f.shape[:2] or not cn.flags.c_contiguous:
                raise ValueError(f"counts must be a contiguous {f.shape[:2]} uint32 array")
            _check(lib.rt_plan_samples(self._ctx, ctypes.byref(p), f.ctypes.data_as(ctypes.c_void_p),
                                       a.ctypes.data_as(ctypes.c_void_p), cn.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(s)), self._ctx)
            return (cn, s.as_dict()) if return_stats else cn
        import torch  # plumbing only: device memory and the caller's stream
        for k, t in (("first", first), ("all", all)):
            if (not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (W, 4) or t.shape != first.shape
                    or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"{k} must be a contiguous (rows, {W}, 4) float32 tensor on the context's device")
        rows = first.shape[0]
        p.rows = rows
        p.flags |= RT_OUT_DEVICE
        cn = torch.empty((rows, W), dtype=torch.int32, device=first.device) if counts is None else counts
        if (not isinstance(cn, torch.Tensor) or cn.element_size() != 4 or cn.is_floating_point()
                or tuple(cn.shape) != (rows, W) or not cn.is_contiguous() or cn.device != first.device):
            raise ValueError(f"counts must be a contiguous {(rows, W)} 4-byte integer tensor on the images' device")
        st = torch.empty(ctypes.sizeof(PlanStats), dtype=torch.uint8, device=first.device) if return_stats else None
        cur, handle = self._stream_handle(stream)
        _check(lib.rt_plan_samples_async(self._ctx, ctypes.byref(p), ctypes.c_void_p(first.data_ptr()),
                                         ctypes.c_void_p(all.data_ptr()), ctypes.c_void_p(cn.data_ptr()),
                                         ctypes.c_void_p(None if st is None else st.data_ptr()),
                                         ctypes.c_void_p(handle)), self._ctx)
        if cur is not None:
            cur.synchronize()
        if not return_stats:
            return cn
        if cur is None:
            torch.cuda.synchronize(first.device) if not hasattr(stream, "synchronize") else stream.synchronize()
        return cn, PlanStats.from_buffer_copy(st.cpu().numpy().tobytes()).as_dict()

    def render_adaptive(self, params: RenderParams, pilot_spp: int, mean_spp: int, radius: int = 1,
                        relative: bool = False, luminance_floor: float = 0.01, count_min: int = 0,
                        return_totals: bool = False, return_stats: bool = False, device: bool = False, stream=None):
        """An adaptively sampled render of ``mean_spp``
        samples per pixel on average, at most ``params.spp`` (the cap) at any
        pixel: a pilot of ``pilot_spp`` samples in two halves (``keep_sum``,
        then ``accumulate``, so no sample is rendered twice), the plan with
        ``budget = (mean_spp - pilot_spp) * pixels`` from the two pilot images,
        and one accumulating counts render.  Equal to those four calls made by
        hand.  Float32 images of ``params``' rows; the running sum is kept.

        Host path by default ((rows, W, 4) float32 array); ``device``: torch
        tensors on the context's device, everything enqueued on ``stream``
        (default: torch's current stream), then waited for.  Returns the
        image, followed by the totals (``return_totals``) and the plan's
        statistics (``return_stats``) when asked for."""
        p = params
        if pilot_spp < 2 or pilot_spp % 2:
            raise ValueError("render_adaptive needs an even pilot_spp >= 2 (two halves)")
        if mean_spp < pilot_spp or p.spp < pilot_spp:
            raise ValueError("render_adaptive needs pilot_spp <= mean_spp and pilot_spp <= params.spp (the cap)")
        if p.accumulate or p.fp16 or p.rgba8:
            raise ValueError("render_adaptive renders float32 frames from a new sum (no accumulate, fp16, rgba8)")
        rows, W, h = p.rows(self.scene.height), self.scene.width, pilot_spp // 2
        part = dict(bounces=p.bounces, row_start=p.row_start, row_step=p.row_step, row_count=p.row_count)
        first_p = RenderParams(spp=h, sample_base=p.sample_base, keep_sum=True, **part)
        all_p = RenderParams(spp=h, sample_base=p.sample_base + h, accumulate=True, keep_sum=True, **part)
        rest_p = RenderParams(spp=p.spp - pilot_spp, sample_base=p.sample_base, accumulate=True, keep_sum=True, **part)
        plan = dict(budget=(mean_spp - pilot_spp) * rows * W, count_min=count_min, count_max=max(p.spp - pilot_spp, count_min),
                    radius=radius, relative=relative, luminance_floor=luminance_floor, return_stats=True)
        if not device:
            first, both = self.render(first_p), self.render(all_p)
            counts, stats = self.plan_samples(first, both, **plan)
            img, totals = self.render_counts(rest_p, counts, totals=True)
        else:
            import torch  # plumbing only: device memory and the caller's stream
            dev = torch.device("cuda", self.device)
            s = torch.cuda.current_stream(dev) if stream is None else stream
            first = torch.empty((rows, W, 4), dtype=torch.float32, device=dev)
            both = torch.empty_like(first)
            self.render(first_p, out=first, stream=s)
            self.render(all_p, out=both, stream=s)
            counts, stats = self.plan_samples(first, both, stream=s, **plan)
            img, totals = self.render_counts(rest_p, counts, out=first, totals=True, stream=s)
            if hasattr(s, "synchronize"):
                s.synchronize()
        res = (img,) + ((totals,) if return_totals else ()) + ((stats,) if return_stats else ())
        return res if len(res) > 1 else img

    def render_progressive(self, params: RenderParams, batch_spp: int, out, stream=None,
                           gather: bool = False):
        """Progressive accumulation: ``params.spp`` samples as
        launches of ``batch_spp`` samples into the context's running fp32 sums
        (``RT_KEEP_SUM`` / ``accumulate`` with ``sample_base`` advancing), all
        enqueued on ``stream``; the last launch writes the averaged frame to the
        device tensor ``out``.  Bit-identical to one launch of ``params.spp``.
        ``gather``: every launch goes through rt_render_gather (this rank's rows
        of the communicator's partition), the last one gathers the frame into
        ``out`` on rank 0 -- one RCCL gather per frame."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        total, done = params.spp, 0
        ptr = out if (out is None or isinstance(out, int)) else out.data_ptr()
        while done < total:
            n = min(batch_spp, total - done)
            last = done + n == total
            p = RenderParams(spp=n, bounces=params.bounces, sample_base=params.sample_base + done,
                             row_start=params.row_start, row_step=params.row_step,
                             row_count=params.row_count, accumulate=done > 0, keep_sum=True,
                             fp16=params.fp16, rgba8=params.rgba8)
            flags = RT_OUT_DEVICE if last else (RT_OUT_DEVICE | RT_OUT_NONE)
            fn = lib.rt_render_gather if gather else lib.rt_render_async
            _check(fn(self._ctx, ctypes.byref(p.c(flags)), ctypes.c_void_p(ptr if last else None),
                      ctypes.c_void_p(stream)), self._ctx)
            done += n
        return out

    def accumulate(self, params: RenderParams):
        """Add samples to the context's running sums only (no image output)."""
        _check(lib.rt_render(self._ctx, ctypes.byref(params.c(RT_OUT_NONE | RT_KEEP_SUM)), None),
               self._ctx)

    def draw(self, spp: int = 400, bounces: int = 3) -> np.ndarray:
        """Renderer.draw(): the whole frame, synchronously; (H, W, 4) float32."""
        return self.render(RenderParams(spp=spp, bounces=bounces))

    def render_mis(self, params: MisParams | None = None, out=None, out8=None):
        """MIS integrator (rt_render_mis).  Host: returns (sum, rgba8) with
        sum (rows, W, 4) float32 = (radiance summed over camera rays, camera
        rays) and rgba8 (rows, W, 4) uint8.  Device: pass tensors ``out`` and/or
        ``out8`` (anything with ``data_ptr()``); the call is synchronous."""
        p = params or MisParams()
        if out is None and out8 is None:
            rows = p.rows(self.scene.height)
            img = np.empty((rows, self.scene.width, 4), dtype=np.float32)
            img8 = np.empty((rows, self.scene.width, 4), dtype=np.uint8)
            _check(lib.rt_render_mis(self._ctx, ctypes.byref(p.c()),
                                     img.ctypes.data_as(ctypes.c_void_p),
                                     img8.ctypes.data_as(ctypes.c_void_p)), self._ctx)
            return img, img8
        ptr = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        _check(lib.rt_render_mis(self._ctx, ctypes.byref(p.c(RT_OUT_DEVICE)), ptr(out), ptr(out8)),
               self._ctx)
        return out, out8

    def comm_init(self, rank: int, world: int, comm_id: bytes):
        """rt_comm_init: join the world-rank RCCL communicator (collective)."""
        if len(comm_id) != RT_COMM_ID_BYTES:
            raise ValueError("comm_id must be the 128 bytes of rt_comm_unique_id()")
        buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES).from_buffer_copy(comm_id)
        _check(lib.rt_comm_init(self._ctx, rank, world, buf), self._ctx)
        self.rank, self.world = rank, world

    def render_gather(self, params: RenderParams | None = None, out=None, stream=None):
        """rt_render_gather (collective): this rank renders rows y = rank (mod
        world), the tiles are gathered over RCCL into the frame on rank 0.
        Host: returns the (H, W, 4) frame on rank 0 (None elsewhere).  Device:
        ``out`` (rank 0; anything with ``data_ptr()``) is filled on ``stream``
        without a host sync."""
        p = params or RenderParams()
        if out is None:
            frame = None
            if getattr(self, "rank", 0) == 0 and not (p.c().flags & RT_OUT_NONE):
                dt = np.uint8 if p.rgba8 else np.uint16 if p.fp16 else np.float32
                frame = np.empty((self.scene.height, self.scene.width, 4), dtype=dt)
            ptr = None if frame is None else frame.ctypes.data_as(ctypes.c_void_p)
            _check(lib.rt_render_gather(self._ctx, ctypes.byref(p.c()), ptr, None), self._ctx)
            return frame
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        ptr = out if isinstance(out, int) else out.data_ptr()
        _check(lib.rt_render_gather(self._ctx, ctypes.byref(p.c(RT_OUT_DEVICE)), ctypes.c_void_p(ptr),
                                    ctypes.c_void_p(stream)), self._ctx)
        return out

    def comm_info(self) -> tuple[int, int]:
        """rt_comm_info: (ranks in the communicator, this rank) as RCCL reports them."""
        n, r = ctypes.c_int32(), ctypes.c_int32()
        _check(lib.rt_comm_info(self._ctx, ctypes.byref(n), ctypes.byref(r)), self._ctx)
        return n.value, r.value

    def place_tiles(self, gathered, world: int, out=None, fp16: bool = False, rgba8: bool = False,
                    stream=None):
        """rt_place_tiles: rank 0's placement step of rt_render_gather on a device
        buffer ``gathered`` (``world`` padded tiles back to back), ordered on
        ``stream`` (default: torch's current stream).  Returns the host frame
        (blocking), or fills the device tensor ``out`` without a host sync."""
        gp = gathered if isinstance(gathered, int) else gathered.data_ptr()
        flags = _pixel_flags(fp16, rgba8)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        if out is None:  # host frame: ordered on `stream` too, then the call blocks
            dt = np.uint8 if rgba8 else np.uint16 if fp16 else np.float32
            frame = np.empty((self.scene.height, self.scene.width, 4), dt)
            _check(lib.rt_place_tiles(self._ctx, ctypes.c_void_p(gp), world, flags,
                                      frame.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(stream)),
                   self._ctx)
            return frame
        ptr = out if isinstance(out, int) else out.data_ptr()
        _check(lib.rt_place_tiles(self._ctx, ctypes.c_void_p(gp), world, flags | RT_OUT_DEVICE,
                                  ctypes.c_void_p(ptr), ctypes.c_void_p(stream)), self._ctx)
        return out

    def last_launch(self) -> dict:
        """The kernel instantiation and launch shape of the last render or ray
        query (rt_last_launch): kernel name as rocprofv3 reports it, lanes per
        pixel, whether the LDS Halton tables were filled, grid, LDS bytes."""
        info = LaunchInfo()
        _check(lib.rt_last_launch(self._ctx, ctypes.byref(info)), self._ctx)
        return info.as_dict()

    def wave_masks(self, params: RenderParams | None = None, lanes: int = 0):
        """rt_debug_wave_masks: the per-wave candidate masks the render of
        ``params`` reads (with ``lanes`` lanes per pixel instead of the
        context's when not 0), read back from the context's table, as a
        (waves_y, waves_x) record array of WAVE_MASK_DTYPE -- empty when that
        launch reads no table -- and how often the context has filled its
        table so far."""
        p = (params or RenderParams()).c()
        fills = ctypes.c_uint64()
        rec = _wave_records(lambda ptr, cap, wx, wy: _check(lib.rt_debug_wave_masks(
            self._ctx, ctypes.byref(p), lanes, ptr, cap, ctypes.byref(wx), ctypes.byref(wy), ctypes.byref(fills)),
            self._ctx))
        return rec, int(fills.value)

    def build_info(self) -> dict:
        """rt_build_info: which triangle-BVH build ran (0 none, 1 host SAH, 2 GPU
        LBVH, 3 GPU SAH), its nodes per layout and the build / scene-compile
        wall times in ms."""
        b = BuildStats()
        _check(lib.rt_build_info(self._ctx, ctypes.byref(b)), self._ctx)
        return {k: getattr(b, k) for k, _ in BuildStats._fields_}

    def tri_bvh(self) -> dict:
        """The context's triangle BVH as the walks read it (rt_debug_tri_bvh),
        copied to the host: ``nodes`` (8, nodes_per_layout, 4) uint32 -- per
        octant layout the entries of three fp16 near/far words and an escape
        or leaf word --, ``sorted`` (n, 12) float32 records in leaf order,
        ``perm`` (n,) uint32 leaf order -> id, ``isect`` (n, 12) float32 records
        in id order, and ``n_triangles``, ``nodes_per_layout``, ``margin``,
        ``leaf_max``.  RtError (RT_ERR_STATE) when the context built none."""
        sizes = TriBvhDump()
        _check(lib.rt_debug_tri_bvh(self._ctx, ctypes.byref(sizes)), self._ctx)
        return _tri_bvh_dump(lambda d: _check(lib.rt_debug_tri_bvh(self._ctx, ctypes.byref(d)), self._ctx),
                             int(sizes.n_triangles), int(sizes.nodes_per_layout))

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float()
        _check(lib.rt_last_kernel_ms(self._ctx, ctypes.byref(ms)), self._ctx)
        return float(ms.value)
