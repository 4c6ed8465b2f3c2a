#!/usr/bin/env python3
"""What an in-place scene update (rt_update_scene) costs on one GPU, against the
two other ways to get the same context, and what a refitted tree costs in
render rate, on Scene.random_triangles at --triangles counts, width x height.

The scene is deformed by moving every random triangle by a uniform offset of
+-(jitter / 2) x the room's side (5.0) per axis, kept inside the room.  All
from one process, after a warm-up of every call, the calls alternating; each
number is the median (min-max) over --reps calls:

  * refit:    wall ms of Renderer.update_scene(deformed) and its parts from
              rt_update_info (host compile, upload, the refit kernels' device ms);
  * rebuild:  wall ms of update_scene(deformed, rebuild=True);
  * recreate: wall ms of rt_destroy + rt_create_ex + rt_fill_seeds, what a
              caller without rt_update_scene does;
  * floor:    a device-to-device copy of the bytes the refit has to move: the
              triangle records once (48 B each, read in id order, written in
              leaf order) and the node array read and written once (8 layouts
              x 16 B an entry), next to the refit kernels' device ms;
  * render:   Msamples/s of a 16 spp render (device output, rt_last_kernel_ms)
              on the refitted tree and on the rebuilt tree of the same deformed
              scene, at jitters of 1 %, 10 % and 100 % of the room: the quality
              a refit loses, so a caller knows when to pass rebuild=True.

    python tools/bench_update.py [--triangles 10000 100000 --reps 20] [--out profiles/r17/update.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOM = 5.0


def deformed(scene, jitter, seed):
    """``scene`` (Scene.random_triangles) with every triangle past the room's 36 moved as a whole."""
    import ctypes

    import numpy as np

    from gpuraytracer_amd import Scene, float3
    n = scene.n_triangles
    verts = (float3 * (3 * n))()
    ctypes.memmove(ctypes.addressof(verts), ctypes.addressof(scene.vertices), 48 * n)
    vv = np.frombuffer(verts, np.float32).reshape(-1, 3, 4)
    rng = np.random.default_rng(seed)
    off = rng.uniform(-0.5 * jitter * ROOM, 0.5 * jitter * ROOM, size=(n - 36, 1, 3)).astype(np.float32)
    v0 = vv[36:, 0:1, :3]
    off = np.clip(v0 + off, -2.3, 2.3) - v0  # the first vertex stays in the room
    vv[36:, :, :3] += off
    return Scene(scene.camera, scene.materials, verts, scene.light)


def med(v):
    return statistics.median(v)


def span(v, digits=3):
    return f"{med(v):.{digits}f} ({min(v):.{digits}f}-{max(v):.{digits}f})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--jitters", type=float, nargs="+", default=[0.01, 0.1, 1.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, library_path
    if not torch.cuda.is_available():
        raise SystemExit("bench_update: no GPU (times are measured on the device only)")
    opt = Options.from_env()
    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    results, lines = [], []
    for n in a.triangles:
        base = Scene.random_triangles(W, H, n)
        moved = [deformed(base, 0.1, seed) for seed in (1, 2)]  # alternate: no update meets its own data
        nT = base.n_triangles
        t = {k: [] for k in ("refit", "refit_fresh", "rebuild", "recreate", "floor", "compile", "upload", "refit_dev",
                                "rebuild_bvh", "rebuild_compile", "rebuild_upload")}
        r = Renderer(base, options=opt)
        total = r.build_info()["tri_bvh_nodes"]
        copy_bytes = 48 * nT + 8 * 16 * total
        src = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def update(sc, rebuild):
            t0 = time.perf_counter()
            r.update_scene(sc, rebuild=rebuild)
            dt = (time.perf_counter() - t0) * 1e3
            u = r.update_info()
            assert u["tri_bvh"] == (2 if rebuild else 1), u
            return dt, u

        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            # a frame loop updates a context that was updated before: the first update of a new context apart
            fresh, _ = update(moved[0], False)
            dt, u = update(moved[1], False)
            if keep:
                t["refit_fresh"].append(fresh)
                t["refit"].append(dt)
                t["compile"].append(u["compile_ms"])
                t["upload"].append(u["upload_ms"])
                t["refit_dev"].append(u["tri_bvh_ms"])
            update(moved[0], True)
            dt, u = update(moved[1], True)
            if keep:
                t["rebuild"].append(dt)
                t["rebuild_bvh"].append(u["tri_bvh_ms"])
                t["rebuild_compile"].append(u["compile_ms"])
                t["rebuild_upload"].append(u["upload_ms"])
            sc = moved[rep % 2]
            t0 = time.perf_counter()
            r.close()
            r = Renderer(sc, options=opt)  # rt_create_ex + rt_fill_seeds
            dt = (time.perf_counter() - t0) * 1e3
            if keep:
                t["recreate"].append(dt)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            e1.synchronize()
            if keep:
                t["floor"].append(e0.elapsed_time(e1))
        r.close()
        del src, dst

        # render rate on the refitted and on the rebuilt tree of the same deformed scene
        out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        p = RenderParams(spp=a.spp, bounces=3)
        rates = {}
        for j in a.jitters:
            sc = deformed(base, j, 3)
            ms = {"refit": [], "rebuild": []}
            with Renderer(base, options=opt) as ra, Renderer(base, options=opt) as rb:
                ra.update_scene(sc)
                rb.update_scene(sc, rebuild=True)
                for rep in range(1 + a.render_reps):
                    for k, rr in (("refit", ra), ("rebuild", rb)):
                        rr.render(p, out=out, stream=stream)
                        stream.synchronize()
                        if rep >= 1:
                            ms[k].append(rr.last_kernel_ms())
            rates[j] = {k: [W * H * a.spp / v / 1e3 for v in vs] for k, vs in ms.items()}
        res = {"triangles": nT, "nodes_per_layout": total, "copy_bytes": copy_bytes,
               "median_ms": {k: med(v) for k, v in t.items()}, "spread_ms": {k: [min(v), max(v)] for k, v in t.items()},
               "render_msamples_s": {str(j): {k: med(v) for k, v in d.items()} for j, d in rates.items()}}
        results.append(res)
        m = res["median_ms"]
        lines += [f"## {nT:,} triangles ({total:,} nodes a layout)", "",
                  "| call | wall ms, median (min-max) | parts |", "|---|---|---|",
                  f"| update, refit | {span(t['refit'])} | compile {span(t['compile'])}, upload {span(t['upload'])}, "
                  f"refit kernels (device) {span(t['refit_dev'])}; the first update of a new context "
                  f"{span(t['refit_fresh'])} |",
                  f"| update, rebuild | {span(t['rebuild'])} | compile {span(t['rebuild_compile'])}, upload "
                  f"{span(t['rebuild_upload'])}, tree build (wall) {span(t['rebuild_bvh'])} |",
                  f"| destroy + create + fill seeds | {span(t['recreate'])} | |", "",
                  f"Refit kernels {m['refit_dev']:.3f} ms on the device; a device copy of the {copy_bytes / 1e6:.1f} MB they "
                  f"have to move takes {span(t['floor'])} ms: refit / copy = {m['refit_dev'] / m['floor']:.1f}.  "
                  f"Refit update / rebuild update = {m['refit'] / m['rebuild']:.2f}, refit update / recreate = "
                  f"{m['refit'] / m['recreate']:.2f}.", "",
                  f"| jitter of the room | Msamples/s on the refitted tree | on the rebuilt tree | refit / rebuild |",
                  "|---|---|---|---|"]
        for j, d in rates.items():
            lines.append(f"| {100 * j:g} % | {span(d['refit'], 1)} | {span(d['rebuild'], 1)} | "
                         f"{med(d['refit']) / med(d['rebuild']):.2f} |")
        lines.append("")
    head = [f"# Scene updates ({torch.cuda.get_device_name(dev)}, Scene.random_triangles {W}x{H}, builder "
            f"`{opt.tri_build}`, {a.reps} calls each, alternating; `{os.path.relpath(library_path, ROOT)}`)", "",
            "Wall times are host clocks around synchronous calls; the deformed scenes of the update rows move every "
            f"random triangle by up to 5 % of the room per axis.  Renders: {a.spp} spp, 3 bounces, kernel time "
            f"(hipEvents), {a.render_reps} launches each.", ""]
    text = "\n".join(head + lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "width": W, "height": H, "reps": a.reps,
                      "results": results}))
    return results


if __name__ == "__main__":
    main()
