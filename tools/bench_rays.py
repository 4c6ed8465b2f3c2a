#!/usr/bin/env python3
"""Ray-query rates (Renderer.trace_rays) on one GPU: Mrays/s of the context's
accelerated layout against the id-ordered loop (RT_RAYS_EXACT) in the same
process, for three scenes -- the Cornell box, 1000 spheres, 100k triangles --
and two ray sets of width x height rays each:

  camera      the frame's pixel-centre camera rays (coherent: a wave holds 64
              neighbours of one image row)
  incoherent  random origins in the room, random directions (numpy PCG64 2024,
              the recipe of tests/ray_sets.py set B)

The two paths alternate, after a warm-up of each, and are timed with the
context's device events around the query kernel (rt_last_kernel_ms); the table
gives the median and the spread (min-max) over --reps repeats.  The rays and
hits stay in device memory.  On a scene of more than --exact-cap primitives the
id-ordered loop is timed on every 16th workgroup chunk of the rays (its cost
per ray does not depend on the ray); the two paths' answers are compared on
those rays, bit for bit.

    python tools/bench_rays.py [--width 1920 --height 1080 --reps 5] [--out profiles/r12/rays.md]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32


def camera_rays(scene):
    """Pixel-centre camera rays (sampling.metal:125-157 with jitter 0.5), row-major."""
    cam = scene.camera
    W, H = scene.width, scene.height
    unit = lambda v: v / np.sqrt(np.sum(v * v, dtype=f32))  # noqa: E731
    pos = np.array(list(cam.position), f32)
    w = -unit(np.array(list(cam.direction), f32))
    u = unit(np.cross(np.array(list(cam.up), f32), w).astype(f32))
    v = unit(np.cross(w, u).astype(f32))
    half_w = f32(np.tan(f32(cam.horizontalFov) / f32(2.0)))
    half_h = half_w / f32(W // H)
    ys, xs = np.mgrid[0:H, 0:W]
    s = ((xs.ravel().astype(f32) + f32(0.5)) / f32(W)) * f32(2.0) - f32(1.0)
    t = -(((ys.ravel().astype(f32) + f32(0.5)) / f32(H)) * f32(2.0) - f32(1.0))
    d = (s * half_w)[:, None] * u + (t * half_h)[:, None] * v - w
    d = d / np.sqrt(np.sum(d * d, axis=1, dtype=f32))[:, None]
    r = np.empty((W * H, 8), f32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = pos, f32(0.001), d, f32(1000.0)
    return r


def incoherent_rays(n):
    rng = np.random.default_rng(2024)
    o = rng.uniform(-2.4, 2.4, (n, 3)).astype(f32)
    g = rng.standard_normal((n, 3)).astype(f32)
    r = np.empty((n, 8), f32)
    r[:, 0:3], r[:, 3], r[:, 7] = o, f32(0.001), f32(1000.0)
    r[:, 4:7] = g / np.sqrt(np.sum(g * g, axis=1, dtype=f32))[:, None]
    return r


def table(rows, device, width, height, reps):
    """The markdown table of the result rows."""
    num = lambda x: f"{x:,.0f}" if x >= 100 else f"{x:.4g}"  # noqa: E731
    lines = [f"# Ray-query rates ({device}, {width}x{height} rays per set, {reps} repeats, alternating)", "",
             "Mrays/s from the device time of the query kernel alone (rays and hits in device memory): median",
             "(min-max).  `exact` is `RT_RAYS_EXACT`, the id-ordered loop over the global records.", "",
             "| scene | rays | query | kernel | accelerated Mrays/s | exact Mrays/s | speed-up | answers equal |",
             "|---|---|---|---|---|---|---|---|"]
    for w in rows:
        up = w["accelerated_mrays_s"] / w["exact_mrays_s"]
        sub = "" if w["n_exact"] == w["n_accelerated"] else f" on {w['n_exact']:,} rays"
        lines.append(f"| {w['scene']} | {w['rays']} | {w['query']} | `{w['kernel']}` | "
                     f"{num(w['accelerated_mrays_s'])} ({num(w['accelerated_min'])}-{num(w['accelerated_max'])}) | "
                     f"{num(w['exact_mrays_s'])} ({num(w['exact_min'])}-{num(w['exact_max'])}){sub} | "
                     f"{up:,.2f}x{' (the loop wins)' if up < 1.0 else ''} | {'yes' if w['answers_equal'] else 'NO'} |")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spheres", type=int, default=1000)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--exact-cap", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "rays.md"))
    a = ap.parse_args(argv)
    import torch

    from gpuraytracer_amd import RT_RAYS_CHUNK, Renderer, Scene
    if not torch.cuda.is_available():
        raise SystemExit("bench_rays: no GPU (rates are measured on the device only)")
    scenes = [("cornell (36 triangles)", Scene.cornell_box(a.width, a.height)),
              (f"{a.spheres} spheres + 12 triangles", Scene.random_spheres(a.width, a.height, a.spheres, seed=42)),
              (f"{a.triangles} triangles + room", Scene.random_triangles(a.width, a.height, a.triangles))]
    n = a.width * a.height
    rows = []
    for label, scene in scenes:
        prims = scene.n_triangles + scene.n_spheres
        sets = {"camera": camera_rays(scene), "incoherent": incoherent_rays(n)}
        with Renderer(scene) as r:
            for set_name, rays in sets.items():
                for any_hit in (False, True):
                    if any_hit and set_name == "camera":
                        continue
                    d_all = torch.from_numpy(rays).cuda()
                    if prims > a.exact_cap:  # every 16th workgroup chunk for the id-ordered loop
                        blocks = d_all[: (n // RT_RAYS_CHUNK) * RT_RAYS_CHUNK].view(-1, RT_RAYS_CHUNK, 8)[::16]
                        d_sub = blocks.reshape(-1, 8).contiguous()
                    else:
                        d_sub = d_all
                    out_all = torch.empty((len(d_all), 2), dtype=torch.int32, device="cuda")
                    out_sub = torch.empty((len(d_sub), 2), dtype=torch.int32, device="cuda")
                    ref_sub = torch.empty_like(out_sub)
                    # warm-up of both paths, and their answers on the same rays
                    r.trace_rays(d_all, any_hit=any_hit, out=out_all)
                    r.trace_rays(d_sub, any_hit=any_hit, out=out_sub)
                    kernel = r.last_launch()["kernel"]
                    r.trace_rays(d_sub, any_hit=any_hit, exact=True, out=ref_sub)
                    equal = bool(torch.equal(out_sub, ref_sub))
                    ms = {"accelerated": [], "exact": []}
                    for _ in range(a.reps):
                        r.trace_rays(d_all, any_hit=any_hit, out=out_all)
                        ms["accelerated"].append(r.last_kernel_ms())
                        r.trace_rays(d_sub, any_hit=any_hit, exact=True, out=ref_sub)
                        ms["exact"].append(r.last_kernel_ms())
                    rate = {"accelerated": [len(d_all) / m / 1e3 for m in ms["accelerated"]],
                            "exact": [len(d_sub) / m / 1e3 for m in ms["exact"]]}
                    row = {"scene": label, "rays": set_name, "query": "any" if any_hit else "closest",
                           "kernel": kernel, "n_accelerated": len(d_all), "n_exact": len(d_sub),
                           "answers_equal": equal}
                    sig = lambda x: float(f"{x:.4g}")  # noqa: E731  (four significant digits)
                    for k in ("accelerated", "exact"):
                        row[k + "_mrays_s"] = sig(statistics.median(rate[k]))
                        row[k + "_min"] = sig(min(rate[k]))
                        row[k + "_max"] = sig(max(rate[k]))
                        row[k + "_ms"] = round(statistics.median(ms[k]), 3)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    lines = table(rows, torch.cuda.get_device_name(0), a.width, a.height, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")
    if not all(w["answers_equal"] for w in rows):
        raise SystemExit("bench_rays: the accelerated path and the id-ordered loop disagree")


if __name__ == "__main__":
    main()
