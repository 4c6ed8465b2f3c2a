#!/usr/bin/env python3
"""Path-query rates (Renderer.trace_paths) on one GPU, in
Mpaths/s = rays x spp / rt_last_kernel_ms, rays and results in device memory:

  (a) the pixel-centre camera rays of the Cornell box at --width x --height, 3
      bounces, spp 1 / 8 / 64, against rt_render of as many samples on the same
      context (the yardstick is the existing kernel: the query form has no
      per-wave camera and shadow masks and no packet walks, and reads a ray and
      a seed per path);
  (b) an incoherent baking load: --bake rays, cosine-distributed about the
      surface normal from random surface points, 1 spp, on the Cornell box,
      1000 spheres and 100k triangles;
  (c) a probe load: 4096 of those rays x 256 spp, one lane per ray against 16;
  (d) the table behind the automatic rule: lanes 1 and 16 over spp and ray count.

Every figure is the median (min-max) of --reps launches after one warm-up.

    python tools/bench_paths.py [--reps 5] [--out profiles/r21/paths.md]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
f32 = np.float32


def unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, dtype=f32))[..., None]


def baking_rays(scene, renderer, n, seed=2025):
    """n rays from random surface points, cosine-distributed about the normal on
    the side the point was seen from: the points are the closest hits of random
    rays from inside the room (Renderer.trace_rays)."""
    rng = np.random.default_rng(seed)
    rays = np.empty((0, 8), f32)
    tri = np.frombuffer(bytes(scene.vertices), f32).reshape(-1, 3, 4)[:, :, :3]
    sph = (np.frombuffer(bytes(scene.spheres), f32).reshape(-1, 20) if scene.n_spheres else np.zeros((0, 20), f32))
    while len(rays) < n:
        m = n - len(rays) + 1024
        probe = np.empty((m, 8), f32)
        probe[:, 0:3] = rng.uniform(-2.4, 2.4, (m, 3))
        probe[:, 4:7] = unit(rng.standard_normal((m, 3)).astype(f32))
        probe[:, 3], probe[:, 7] = f32(0.001), f32(1000.0)
        t, ids = renderer.trace_rays(probe)
        hit = ids >= 0
        o, d, t, ids = probe[hit, 0:3], probe[hit, 4:7], t[hit], ids[hit]
        p = o + d * t[:, None]
        nrm = np.empty_like(p)
        is_tri = ids < scene.n_triangles
        v = tri[ids[is_tri]]
        nrm[is_tri] = unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(f32))
        nrm[~is_tri] = unit(p[~is_tri] - sph[ids[~is_tri] - scene.n_triangles, 0:3])
        nrm = np.where((np.sum(nrm * d, axis=1) > 0)[:, None], -nrm, nrm)
        # cosine-distributed about nrm (Malley): a disc sample lifted to the hemisphere
        u1, u2 = rng.random(len(p), dtype=f32), rng.random(len(p), dtype=f32)
        rad, phi = np.sqrt(u1), f32(2.0 * np.pi) * u2
        a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0, 1, 0]], f32), np.array([[1, 0, 0]], f32))
        tx = unit(np.cross(nrm, a).astype(f32))
        ty = np.cross(nrm, tx).astype(f32)
        w = (tx * (rad * np.cos(phi))[:, None] + ty * (rad * np.sin(phi))[:, None] +
             nrm * np.sqrt(np.maximum(f32(0.0), f32(1.0) - u1))[:, None])
        out = np.empty((len(p), 8), f32)
        out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p + nrm * f32(1e-3), f32(0.001), unit(w.astype(f32)), f32(1000.0)
        rays = np.concatenate([rays, out])
    return np.ascontiguousarray(rays[:n])


def stat(ms, paths):
    rate = [paths / m / 1e3 for m in ms]
    sig = lambda x: float(f"{x:.4g}")  # noqa: E731
    return {"ms": round(statistics.median(ms), 4), "mpaths_s": sig(statistics.median(rate)), "min": sig(min(rate)),
            "max": sig(max(rate))}


def time_paths(r, d_rays, out, reps, **kw):
    r.trace_paths(d_rays, out=out, **kw)  # warm-up
    info = r.last_launch()
    ms = []
    for _ in range(reps):
        r.trace_paths(d_rays, out=out, **kw)
        ms.append(r.last_kernel_ms())
    row = stat(ms, len(d_rays) * kw.get("spp", 1))
    row.update(kernel=info["kernel"], lanes=info["lanes_per_pixel"], tables=info["halton_tables"], grid=info["grid_x"])
    return row


def fmt(w):
    num = lambda x: f"{x:,.0f}" if x >= 100 else f"{x:.4g}"  # noqa: E731
    return f"{num(w['mpaths_s'])} ({num(w['min'])}-{num(w['max'])})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bake", type=int, default=2_000_000)
    ap.add_argument("--spheres", type=int, default=1000)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--max-paths", type=int, default=1 << 26, help="largest rays x spp of a cell of table (d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "paths.md"))
    a = ap.parse_args(argv)
    import torch

    from bench_rays import camera_rays
    from gpuraytracer_amd import RenderParams, Renderer, Scene
    if not torch.cuda.is_available():
        raise SystemExit("bench_paths: no GPU (rates are measured on the device only)")
    dev = torch.cuda.get_device_name(0)
    L = [f"# Path-query rates ({dev}, {a.reps} launches each after a warm-up)", "",
         "Mpaths/s = rays x spp / device time of the kernel (rt_last_kernel_ms): median (min-max).  3 bounces.", ""]
    scenes = [("cornell", Scene.cornell_box(a.width, a.height)),
              (f"{a.spheres} spheres", Scene.random_spheres(a.width, a.height, a.spheres, seed=42)),
              (f"{a.triangles} triangles", Scene.random_triangles(a.width, a.height, a.triangles))]

    # (a) camera rays of the Cornell box against rt_render
    L += [f"## (a) Cornell {a.width}x{a.height}: pixel-centre camera rays against rt_render", "",
          "| spp | lanes | query Mpaths/s | kernel | rt_render Msamples/s | kernel | query / render |", "|---|---|---|---|---|---|---|"]
    name, scene = scenes[0]
    with Renderer(scene) as r:
        d_rays = torch.from_numpy(camera_rays(scene)).cuda()
        out = torch.empty((len(d_rays), 4), dtype=torch.float32, device="cuda")
        img = torch.empty((a.height, a.width, 4), dtype=torch.float32, device="cuda")
        for spp in (1, 8, 64):
            p = RenderParams(spp=spp, bounces=3)
            r.render(p, out=img)
            torch.cuda.synchronize()
            rk = r.last_launch()["kernel"]
            ms = []
            for _ in range(a.reps):
                r.render(p, out=img)
                torch.cuda.synchronize()
                ms.append(r.last_kernel_ms())
            ren = stat(ms, len(d_rays) * spp)
            for lanes in (0, 1, 16):
                q = time_paths(r, d_rays, out, a.reps, spp=spp, lanes=lanes)
                print(json.dumps(dict(part="a", spp=spp, asked=lanes, query=q, render=ren, render_kernel=rk)), flush=True)
                L.append(f"| {spp} | {'auto: ' if lanes == 0 else ''}{q['lanes']} | {fmt(q)} | `{q['kernel']}` | {fmt(ren)} | "
                         f"`{rk}` | {q['mpaths_s'] / ren['mpaths_s']:.3f} |")
    L.append("")

    # (b), (c), (d) on the baking rays of each scene
    bake, probe, table = [], [], []
    for name, scene in scenes:
        with Renderer(scene) as r:
            rays = baking_rays(scene, r, a.bake)
            d_rays = torch.from_numpy(rays).cuda()
            out = torch.empty((len(d_rays), 4), dtype=torch.float32, device="cuda")
            for lanes in (1, 16):
                q = time_paths(r, d_rays, out, a.reps, spp=1, lanes=lanes)
                print(json.dumps(dict(part="b", scene=name, query=q)), flush=True)
                bake.append(f"| {name} | {len(d_rays):,} | {q['lanes']} | {fmt(q)} | {q['ms']} | `{q['kernel']}` |")
            cell = {}
            for lanes in (1, 16):
                q = time_paths(r, d_rays[:4096], out[:4096], a.reps, spp=256, lanes=lanes)
                print(json.dumps(dict(part="c", scene=name, query=q)), flush=True)
                cell[lanes] = q
                probe.append(f"| {name} | {q['lanes']} | {fmt(q)} | {q['ms']} | {q['grid']} | `{q['kernel']}` |")
            probe.append(f"| {name} | 16 / 1 | {cell[16]['mpaths_s'] / cell[1]['mpaths_s']:.2f}x | | | |")
            for n in (4096, 65536, 1 << 20):
                for spp in (1, 4, 8, 16, 32, 64, 128):
                    if n * spp > a.max_paths or n > len(d_rays):
                        continue
                    q1 = time_paths(r, d_rays[:n], out[:n], a.reps, spp=spp, lanes=1)
                    q16 = time_paths(r, d_rays[:n], out[:n], a.reps, spp=spp, lanes=16)
                    ratio = q16["mpaths_s"] / q1["mpaths_s"]
                    print(json.dumps(dict(part="d", scene=name, n=n, spp=spp, l1=q1, l16=q16)), flush=True)
                    table.append(f"| {name} | {n:,} | {spp} | {fmt(q1)} | {fmt(q16)} | {ratio:.2f} | "
                                 f"{'16' if ratio > 1.0 else '1'} |")
    L += [f"## (b) Baking: {a.bake:,} cosine-distributed rays from random surface points, 1 spp", "",
          "| scene | rays | lanes | Mpaths/s | ms | kernel |", "|---|---|---|---|---|---|"] + bake + [""]
    L += ["## (c) Probes: 4096 rays x 256 spp", "", "| scene | lanes | Mpaths/s | ms | workgroups | kernel |",
          "|---|---|---|---|---|---|"] + probe + [""]
    L += ["## (d) Lanes per ray over spp and ray count (the baking rays' first n)", "",
          "| scene | rays | spp | 1 lane Mpaths/s | 16 lanes Mpaths/s | 16 / 1 | faster |", "|---|---|---|---|---|---|---|"] + table
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
