#!/usr/bin/env python3
"""Feature-buffer launch times (Renderer.render_aov) on one GPU against the
render of the same samples at one bounce, for three scenes -- the Cornell box,
1000 spheres, 100k triangles -- at width x height x spp.

The AOV launch traces the camera rays and closest queries of that render and
nothing else (no light sample, no shadow query), so it should take no longer.
Both launches run on one context and alternate in one process after a warm-up
of each; the time is the context's device events around the kernel alone
(rt_last_kernel_ms), all outputs in device memory.  The table gives the median
and the spread (min-max) over --reps launches of each, the AOV launch's camera
rays per second, and the closest-hit rate of rt_trace_rays on pixel-centre
camera rays from profiles/r12/rays.md for comparison (rays read from memory
instead of generated).

    python tools/bench_aov.py [--width 1920 --height 1080 --spp 256 --reps 20] [--out profiles/r15/aov.md]
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def query_rates():
    """scene label -> Mrays/s of the camera-ray closest query in profiles/r12/rays.md."""
    rates = {}
    path = os.path.join(ROOT, "profiles", "r12", "rays.md")
    if not os.path.exists(path):
        return rates
    for line in open(path):
        m = re.match(r"\| ([^|]+) \| camera \| closest \| `[^`]+` \| ([\d,.]+) ", line)
        if m:
            rates[m.group(1).strip()] = float(m.group(2).replace(",", ""))
    return rates


def table(rows, device, a):
    lines = [f"# Feature-buffer launches ({device}, {a.width}x{a.height} x {a.spp} spp, {a.reps} launches each, "
             "alternating)", "",
             "Kernel ms from the context's device events (`rt_last_kernel_ms`), outputs in device memory: median",
             "(min-max).  `render` is `rt_render` at `bounces = 1` of the same samples on the same context.",
             "`rt_trace_rays` is the closest-hit rate of pixel-centre camera rays from `profiles/r12/rays.md`.", "",
             "| scene | AOV kernel | AOV ms | render kernel | render ms | AOV / render | AOV Mrays/s | rt_trace_rays Mrays/s |",
             "|---|---|---|---|---|---|---|---|"]
    for w in rows:
        q = f"{w['query_mrays_s']:,.0f}" if w["query_mrays_s"] else "-"
        lines.append(f"| {w['scene']} | `{w['aov_kernel']}` | {w['aov_ms']:.3f} ({w['aov_min']:.3f}-{w['aov_max']:.3f}) | "
                     f"`{w['render_kernel']}` | {w['render_ms']:.3f} ({w['render_min']:.3f}-{w['render_max']:.3f}) | "
                     f"{w['ratio']:.3f}{'' if w['ratio'] <= 1.0 else ' (SLOWER)'} | {w['aov_mrays_s']:,.0f} | {q} |")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spheres", type=int, default=1000)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "aov.md"))
    a = ap.parse_args(argv)
    import torch

    from gpuraytracer_amd import RenderParams, Renderer, Scene
    if not torch.cuda.is_available():
        raise SystemExit("bench_aov: no GPU (times are measured on the device only)")
    scenes = [("cornell (36 triangles)", Scene.cornell_box(a.width, a.height)),
              (f"{a.spheres} spheres + 12 triangles", Scene.random_spheres(a.width, a.height, a.spheres, seed=42)),
              (f"{a.triangles} triangles + room", Scene.random_triangles(a.width, a.height, a.triangles))]
    rates = query_rates()
    rows = []
    for label, scene in scenes:
        with Renderer(scene) as r:
            shape = (a.height, a.width)
            out = {"albedo": torch.empty(shape + (4,), dtype=torch.float32, device="cuda"),
                   "normal_depth": torch.empty(shape + (4,), dtype=torch.float32, device="cuda"),
                   "first_hit": torch.empty(shape + (2,), dtype=torch.int32, device="cuda")}
            img = torch.empty(shape + (4,), dtype=torch.float32, device="cuda")
            params = RenderParams(spp=a.spp, bounces=1)
            ms = {"aov": [], "render": []}
            kernel = {}
            for k in range(a.warmup + a.reps):
                r.render_aov(spp=a.spp, out=out)
                t_aov = r.last_kernel_ms()
                kernel["aov"] = r.last_launch()["kernel"]
                r.render(params, out=img)
                t_render = r.last_kernel_ms()  # waits for the launch's end event
                kernel["render"] = r.last_launch()["kernel"]
                if k >= a.warmup:
                    ms["aov"].append(t_aov)
                    ms["render"].append(t_render)
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"scene": label, "aov_kernel": kernel["aov"], "render_kernel": kernel["render"],
                   "aov_ms": round(med["aov"], 4), "aov_min": round(min(ms["aov"]), 4),
                   "aov_max": round(max(ms["aov"]), 4), "render_ms": round(med["render"], 4),
                   "render_min": round(min(ms["render"]), 4), "render_max": round(max(ms["render"]), 4),
                   "ratio": round(med["aov"] / med["render"], 4),
                   "aov_mrays_s": round(a.width * a.height * a.spp / med["aov"] / 1e3, 1),
                   "query_mrays_s": rates.get(label)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = table(rows, torch.cuda.get_device_name(0), a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")
    slower = [w["scene"] for w in rows if w["ratio"] > 1.0]
    if slower:
        raise SystemExit("bench_aov: the AOV launch took longer than the one-bounce render on: " + ", ".join(slower))


if __name__ == "__main__":
    main()
