#!/usr/bin/env python3
"""Denoiser call time (Renderer.denoise) on one GPU against the low-spp
pipeline it ends and against a memory-copy floor, on the Cornell box at
width x height.

Three numbers, all from one process, device buffers, hipEvents on one stream
around each call, after a warm-up of every call, the calls alternating; each
is the median (min-max) over --reps calls:

  * denoise: rt_denoise_async with the defaults at --iterations passes
    (prepare + variance pre-filter + the a-trous passes);
  * inputs: the two rt_render_async launches of spp/2 samples at --bounces and
    the rt_render_aov_async launch of all spp samples that make its inputs, and
    the denoiser's share of inputs + denoise;
  * floor: a device-to-device copy that moves the filter's compulsory bytes --
    per pixel 48 B read + 16 B written by prepare, 16 + 16 by the variance
    pre-filter, 32 + 16 by every pass, and 32 B more read by the last pass
    (colour a, albedo) -- i.e. a copy of half that many bytes (a copy reads and
    writes each byte once).

The table of cumulative times at 1..6 passes gives the cost of each step by
difference (the A/B of RT_DENOISE_LDS_MAX_STEP builds reads it, see
profiles/r16/denoise.md).

    python tools/bench_denoise.py [--width 1920 --height 1080 --spp 4 --reps 20] [--out profiles/r16/denoise_run.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compulsory_bytes(pixels, iterations):
    """Bytes the filter has to move: (read, written)."""
    return pixels * (48 + 16 + 32 * iterations + 32), pixels * (16 + 16 + 16 * iterations)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("bench_denoise: --reps must be >= 20")
    import torch

    from gpuraytracer_amd import RenderParams, Renderer, Scene, library_path
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise: no GPU (times are measured on the device only)")
    W, H, half = a.width, a.height, a.spp // 2
    with Renderer(Scene.cornell_box(W, H)) as r:
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.current_stream(dev)
        _, bufs = r.render_denoised(RenderParams(spp=a.spp, bounces=a.bounces), return_inputs=True,
                                    iterations=a.iterations)
        out = torch.empty_like(bufs["color_a"])
        rd, wr = compulsory_bytes(W * H, a.iterations)
        src = torch.empty((rd + wr) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def inputs():
            r.render(RenderParams(spp=half, bounces=a.bounces), out=bufs["color_a"], stream=stream)
            r.render(RenderParams(spp=half, bounces=a.bounces, sample_base=half), out=bufs["color_b"], stream=stream)
            r.render_aov(spp=a.spp, out={k: bufs[k] for k in ("albedo", "normal_depth")}, stream=stream)

        calls = {"inputs": inputs, "floor": lambda: dst.copy_(src)}
        for it in range(1, 7):
            calls[f"denoise{it}"] = (lambda it: lambda: r.denoise(**bufs, iterations=it, out=out, stream=stream))(it)
        times = {k: [] for k in calls}
        for rep in range(a.warmup + a.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        r.denoise(**bufs, iterations=a.iterations, out=out, stream=stream)
        stream.synchronize()
        launch = r.last_launch()
    med = {k: statistics.median(v) for k, v in times.items()}
    den = med[f"denoise{a.iterations}"]
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.relpath(library_path, ROOT),
           "width": W, "height": H, "spp": a.spp, "bounces": a.bounces, "iterations": a.iterations, "reps": a.reps,
           "denoise_ms": den, "inputs_ms": med["inputs"], "denoise_share": den / (den + med["inputs"]),
           "floor_ms": med["floor"], "denoise_over_floor": den / med["floor"],
           "compulsory_read_bytes": rd, "compulsory_written_bytes": wr,
           "achieved_gb_s": (rd + wr) / den / 1e6, "copy_gb_s": (rd + wr) / med["floor"] / 1e6,
           "last_kernel": launch["kernel"], "last_lds_bytes": launch["lds_bytes"],
           "cumulative_ms": {str(it): med[f"denoise{it}"] for it in range(1, 7)},
           "spread_ms": {k: [min(v), max(v)] for k, v in times.items()}}
    sp = res["spread_ms"]
    lines = [f"# Denoiser call time ({res['device']}, Cornell {W}x{H}, {a.spp // 2}+{a.spp // 2} spp, "
             f"{a.bounces} bounces, {a.reps} calls each, alternating; `{res['library']}`)", "",
             "hipEvents around each call on one stream, device buffers: median (min-max) ms.", "",
             "| call | ms | note |", "|---|---|---|",
             f"| denoise, {a.iterations} passes | {den:.3f} ({sp[f'denoise{a.iterations}'][0]:.3f}-"
             f"{sp[f'denoise{a.iterations}'][1]:.3f}) | {res['achieved_gb_s']:.0f} GB/s of compulsory bytes; last pass "
             f"`{launch['kernel']}`, {launch['lds_bytes']} B LDS |",
             f"| inputs: 2 renders + AOV | {med['inputs']:.3f} ({sp['inputs'][0]:.3f}-{sp['inputs'][1]:.3f}) | "
             f"denoiser's share of the pipeline {100 * res['denoise_share']:.1f} % |",
             f"| floor: copy of {(rd + wr) / 2 / 1e6:.1f} MB | {med['floor']:.3f} ({sp['floor'][0]:.3f}-"
             f"{sp['floor'][1]:.3f}) | {res['copy_gb_s']:.0f} GB/s read + written; denoise / floor = "
             f"{res['denoise_over_floor']:.2f} |", "",
             "| passes | " + " | ".join(str(i) for i in range(1, 7)) + " |", "|---|" + "---|" * 6,
             "| cumulative ms | " + " | ".join(f"{med[f'denoise{i}']:.3f}" for i in range(1, 7)) + " |"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
