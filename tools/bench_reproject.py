#!/usr/bin/env python3
"""Reprojection call time (Renderer.reproject) on one GPU against a
memory-copy floor and against the render_temporal frame it is part of, on the
Cornell box at width x height, the previous camera an orbit step of 0.05 rad
away.

All from one process, device buffers, hipEvents on one stream around each
call, after a warm-up of every call, the calls alternating until every reprojection
call has at least --window seconds of measured time and --reps samples (the
frame's other calls stop at 5 * reps samples); each number is the median
(min-max):

  * reproject1 / reproject2: rt_reproject_async with the defaults on one and
    two colour planes (inputs: a rendered frame, its centre feature buffers
    and those of the previous pose, the previous frame's planes as history);
  * floor1 / floor2: a device-to-device copy that moves the call's compulsory
    bytes (compulsory_bytes below: every input texel read once, every output
    written once), i.e. a copy of half that many bytes (a copy reads and
    writes each byte once);
  * the other calls of a render_temporal frame of 1+1 spp -- the two renders,
    the centre feature buffers, the jittered feature buffers, the denoiser --
    and reprojection's share of their sum.

    python tools/bench_reproject.py [--width 1920 --height 1080 --reps 20 --window 0.5] [--out profiles/r24/reproject_run.md]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compulsory_bytes(pixels, planes):
    """Bytes a call has to move: (read, written).  Per pixel the colour and the
    history texel of every plane (16 B each), both hit records (8 B each) and
    both normal_depth texels (16 B each); one 16-B output per plane."""
    return pixels * (32 * planes + 2 * 8 + 2 * 16), pixels * 16 * planes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 20 or a.window < 0.5:
        raise SystemExit("bench_reproject: --reps must be >= 20 and --window >= 0.5")
    import torch

    import pose_scenes as ps
    from gpuraytracer_amd import RenderParams, Renderer, Scene, library_path
    if not torch.cuda.is_available():
        raise SystemExit("bench_reproject: no GPU (times are measured on the device only)")
    W, H = a.width, a.height
    base = Scene.cornell_box(W, H)
    pose = lambda t: ps.posed(base, eye=(9 * math.sin(t), 0.3 * math.sin(2 * t), 9 * math.cos(t)),  # noqa: E731
                              look_at=(0, 0, 0))
    prev, cur = pose(0.0), pose(0.05)
    with Renderer(prev) as r:
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.current_stream(dev)
        _, state = r.render_temporal(RenderParams(spp=2, bounces=a.bounces))
        r.update_scene(cur)
        new = lambda: torch.empty((H, W, 4), dtype=torch.float32, device=dev)  # noqa: E731
        color, out = [new(), new()], [new(), new()]
        centre = {"normal_depth": new(), "first_hit": torch.empty((H, W, 2), dtype=torch.int32, device=dev)}
        aov = {"albedo": new(), "normal_depth": new()}
        den = new()

        def reproject(planes):
            return lambda: r.reproject(color[:planes], state["out"][:planes], centre["first_hit"],
                                       centre["normal_depth"], state["hit"], state["normal_depth"],
                                       prev_camera=state["camera"], out=out[:planes], stream=stream)

        floors = {}
        for planes in (1, 2):
            rd, wr = compulsory_bytes(W * H, planes)
            src = torch.empty((rd + wr) // 2, dtype=torch.uint8, device=dev)
            floors[planes] = (src, torch.empty_like(src), rd, wr)
        calls = {
            "renders": lambda: (r.render(RenderParams(spp=1, bounces=a.bounces, sample_base=2), out=color[0],
                                         stream=stream),
                                r.render(RenderParams(spp=1, bounces=a.bounces, sample_base=3), out=color[1],
                                         stream=stream)),
            "centre_aov": lambda: r.render_aov(center=True, out=centre, stream=stream),
            "reproject1": reproject(1), "floor1": lambda: floors[1][1].copy_(floors[1][0]),
            "reproject2": reproject(2), "floor2": lambda: floors[2][1].copy_(floors[2][0]),
            "aov": lambda: r.render_aov(spp=2, sample_base=2, out=aov, stream=stream),
            "denoise": lambda: r.denoise(out[0], out[1], aov["albedo"], aov["normal_depth"], out=den, stream=stream),
        }
        times = {k: [] for k in calls}
        timed = ("reproject1", "reproject2")   # the calls the window is for; the floors run alongside them
        rep = 0
        while rep < a.warmup + a.reps or min(sum(times[k]) for k in timed) < 1e3 * a.window:
            for k, f in calls.items():
                if k not in timed and not k.startswith("floor") and len(times[k]) >= 5 * a.reps:
                    continue   # the frame's other calls: 5 * reps samples are enough
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
            rep += 1
        reused = float((out[0][..., 3] > 1).float().mean())
        calls["reproject2"]()
        stream.synchronize()
        launch = r.last_launch()
    med = {k: statistics.median(v) for k, v in times.items()}
    frame = med["renders"] + med["centre_aov"] + med["reproject2"] + med["aov"] + med["denoise"]
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.relpath(library_path, ROOT),
           "width": W, "height": H, "bounces": a.bounces, "samples_per_call": len(times["reproject2"]),
           "reused_share_of_pixels": reused, "kernel": launch["kernel"], "lds_bytes": launch["lds_bytes"],
           "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in times.items()},
           "frame_ms": frame, "reproject_share": med["reproject2"] / frame}
    for planes in (1, 2):
        rd, wr = floors[planes][2:]
        res[f"compulsory_bytes{planes}"] = [rd, wr]
        res[f"over_floor{planes}"] = med[f"reproject{planes}"] / med[f"floor{planes}"]
        res[f"achieved_gb_s{planes}"] = (rd + wr) / med[f"reproject{planes}"] / 1e6
        res[f"copy_gb_s{planes}"] = (rd + wr) / med[f"floor{planes}"] / 1e6
    sp = res["spread_ms"]
    row = lambda k: f"{med[k]:.3f} ({sp[k][0]:.3f}-{sp[k][1]:.3f})"  # noqa: E731
    lines = [f"# Reprojection call time ({res['device']}, Cornell {W}x{H}, orbit step 0.05 rad, "
             f"{res['samples_per_call']} calls each, alternating; `{res['library']}`)", "",
             "hipEvents around each call on one stream, device buffers: median (min-max) ms.  "
             f"{100 * reused:.1f} % of the pixels reuse history; `{launch['kernel']}`, {launch['lds_bytes']} B LDS.", "",
             "| call | ms | compulsory bytes (read + written) | GB/s | copy of half those bytes, ms | GB/s | call / copy |",
             "|---|---|---|---|---|---|---|"]
    for planes in (1, 2):
        rd, wr = floors[planes][2:]
        lines.append(f"| reproject, {planes} plane{'s' if planes > 1 else ''} | {row(f'reproject{planes}')} | "
                     f"{rd / 1e6:.1f} + {wr / 1e6:.1f} MB | {res[f'achieved_gb_s{planes}']:.0f} | "
                     f"{row(f'floor{planes}')} | {res[f'copy_gb_s{planes}']:.0f} | {res[f'over_floor{planes}']:.2f} |")
    lines += ["", "A render_temporal frame of 1+1 spp:", "", "| call | ms |", "|---|---|",
              f"| two renders of 1 spp, {a.bounces} bounces | {row('renders')} |",
              f"| centre feature buffers | {row('centre_aov')} |",
              f"| reproject, 2 planes | {row('reproject2')} |",
              f"| jittered feature buffers of the 2 samples | {row('aov')} |",
              f"| denoise, 5 passes | {row('denoise')} |",
              f"| sum | {frame:.3f} |", "",
              f"Reprojection is {100 * res['reproject_share']:.1f} % of the frame."]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
