#!/usr/bin/env python3
"""Adaptive sampling on one GPU: what the counts form of the
path kernel costs, what the divergence of a planned count map costs, and the
planner's time against a memory-copy floor, on the Cornell box at width x
height.

All from one process, device buffers, hipEvents on one stream around each
call, after a warm-up of every call, the calls alternating in one loop; each
number is the median (min-max) over --reps calls:

  (a) render_counts with uniform counts of --spp against rt_render at --spp
      with 16 lanes per pixel (the same wave shape) and against rt_render's
      automatic choice: the cost of the counts form;
  (b) the pipeline of render_adaptive made by hand -- the pilot's two halves
      (--pilot / 2 samples each), the plan with budget (--mean - --pilot) *
      pixels, the accumulating counts render -- per stage, and the counts
      render against rt_render of round(mean count) samples: the cost of
      divergence.  The wave utilisation is computed on the host from the
      counts: the mean over the 2 x 2-pixel waves that trace anything of
      (mean rounds of the wave's pixels) / (rounds the wave runs);
  (c) the plan against a device-to-device copy of its compulsory bytes, 32 B
      read and 4 B written per pixel, i.e. a copy of half that many bytes.

    python tools/bench_adaptive.py [--width 1920 --height 1080 --reps 20] [--out profiles/r20/adaptive.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wave_utilisation(counts, lanes=16, tile=2):
    """Mean over the tile x tile-pixel waves with a sample of mean rounds / max rounds."""
    import numpy as np
    h, w = counts.shape
    hp, wp = -(-h // tile) * tile, -(-w // tile) * tile
    r = np.zeros((hp, wp), np.float64)
    r[:h, :w] = -(-counts.astype(np.int64) // lanes)
    inside = np.zeros((hp, wp), bool)
    inside[:h, :w] = True
    blk = lambda a: a.reshape(hp // tile, tile, wp // tile, tile).transpose(0, 2, 1, 3).reshape(-1, tile * tile)  # noqa: E731
    rb, ib = blk(r), blk(inside)
    mx = rb.max(1)
    busy = mx > 0
    mean = rb.sum(1) / ib.sum(1)
    return float((mean[busy] / mx[busy]).mean()), float(busy.mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--pilot", type=int, default=8)
    ap.add_argument("--mean", type=int, default=16)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("bench_adaptive: --reps must be >= 20")
    import torch

    from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, library_path
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaptive: no GPU (times are measured on the device only)")
    W, H, B, h = a.width, a.height, a.bounces, a.pilot // 2
    scene = Scene.cornell_box(W, H)
    with Renderer(scene) as r, Renderer(scene, options=Options(lanes=16)) as r16:
        dev = torch.device("cuda", r.device)
        stream = torch.cuda.current_stream(dev)
        new = lambda: torch.empty((H, W, 4), dtype=torch.float32, device=dev)  # noqa: E731
        first, both, img, uni = new(), new(), new(), new()
        counts = torch.empty((H, W), dtype=torch.int32, device=dev)
        flat = torch.full((H, W), a.spp, dtype=torch.int32, device=dev)
        src = torch.empty(W * H * 18, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        budget = (a.mean - a.pilot) * W * H
        plan = dict(budget=budget, count_max=a.cap - a.pilot, counts=counts, stream=stream)

        def pilot_first():
            r.render(RenderParams(spp=h, bounces=B, keep_sum=True), out=first, stream=stream)

        def pilot_second():
            r.render(RenderParams(spp=h, bounces=B, sample_base=h, accumulate=True, keep_sum=True), out=both,
                     stream=stream)

        # the pipeline once: the count map every timed call below uses
        pilot_first()
        pilot_second()
        _, stats = r.plan_samples(first, both, return_stats=True, **plan)
        stream.synchronize()
        cn = counts.cpu().numpy()
        mean_count = float(cn.mean())
        mspp = max(1, int(round(mean_count)))
        util, busy = wave_utilisation(cn)

        calls = {
            "pilot_first": pilot_first,
            "pilot_second": pilot_second,
            "plan": lambda: r.plan_samples(first, both, **plan),
            "counts_planned": lambda: r.render_counts(
                RenderParams(spp=a.cap - a.pilot, bounces=B, accumulate=True, keep_sum=True), counts, out=img,
                stream=stream),
            "uniform_mean_auto": lambda: r.render(RenderParams(spp=mspp, bounces=B, sample_base=a.pilot), out=uni,
                                                  stream=stream),
            "uniform_mean_l16": lambda: r16.render(RenderParams(spp=mspp, bounces=B, sample_base=a.pilot), out=uni,
                                                   stream=stream),
            "counts_flat": lambda: r.render_counts(RenderParams(spp=a.spp, bounces=B), flat, out=uni, stream=stream),
            "render_l16": lambda: r16.render(RenderParams(spp=a.spp, bounces=B), out=uni, stream=stream),
            "render_auto": lambda: r.render(RenderParams(spp=a.spp, bounces=B), out=uni, stream=stream),
            "floor": lambda: dst.copy_(src),
        }
        times = {k: [] for k in calls}
        kernels = {}
        for rep in range(a.warmup + a.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
                if k in ("counts_planned", "uniform_mean_auto", "counts_flat", "render_auto", "plan"):
                    kernels[k] = r.last_launch()["kernel"]
                elif k in ("uniform_mean_l16", "render_l16"):
                    kernels[k] = r16.last_launch()["kernel"]
    med = {k: statistics.median(v) for k, v in times.items()}
    sp = {k: (min(v), max(v)) for k, v in times.items()}
    t = lambda k: f"{med[k]:.3f} ({sp[k][0]:.3f}-{sp[k][1]:.3f})"  # noqa: E731
    pipeline = med["pilot_first"] + med["pilot_second"] + med["plan"] + med["counts_planned"]
    planned_samples = mean_count * W * H
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.relpath(library_path, ROOT), "width": W,
           "height": H, "bounces": B, "reps": a.reps, "spp": a.spp, "pilot": a.pilot, "mean": a.mean, "cap": a.cap,
           "median_ms": med, "spread_ms": {k: list(v) for k, v in sp.items()}, "kernels": kernels,
           "plan_stats": stats, "mean_count": mean_count, "uniform_mean_spp": mspp, "wave_utilisation": util,
           "waves_with_samples": busy, "pipeline_ms": pipeline,
           "counts_flat_over_render_l16": med["counts_flat"] / med["render_l16"],
           "counts_flat_over_render_auto": med["counts_flat"] / med["render_auto"],
           "counts_planned_ms_per_msample": med["counts_planned"] / (planned_samples / 1e6),
           "uniform_mean_l16_ms_per_msample": med["uniform_mean_l16"] / (mspp * W * H / 1e6),
           "uniform_mean_auto_ms_per_msample": med["uniform_mean_auto"] / (mspp * W * H / 1e6),
           "plan_over_floor": med["plan"] / med["floor"],
           "plan_gb_s": 36 * W * H / med["plan"] / 1e6, "copy_gb_s": 36 * W * H / med["floor"] / 1e6}
    lines = [
        f"# Adaptive sampling ({res['device']}, Cornell {W}x{H}, {B} bounces, {a.reps} calls each, alternating; "
        f"`{res['library']}`)", "",
        "hipEvents around each call on one stream, device buffers: median (min-max) ms.", "",
        f"## (a) The counts form: uniform counts of {a.spp} against rt_render at {a.spp} spp", "",
        "| call | ms | kernel |", "|---|---|---|",
        f"| render_counts, every count {a.spp} | {t('counts_flat')} | `{kernels['counts_flat']}` |",
        f"| rt_render, 16 lanes per pixel | {t('render_l16')} | `{kernels['render_l16']}` |",
        f"| rt_render, automatic lanes | {t('render_auto')} | `{kernels['render_auto']}` |", "",
        f"counts / rt_render at 16 lanes = {res['counts_flat_over_render_l16']:.3f}, "
        f"counts / rt_render automatic = {res['counts_flat_over_render_auto']:.3f}.", "",
        f"## (b) The pipeline: {h}+{h} pilot, mean {a.mean}, cap {a.cap}", "",
        "| stage | ms |", "|---|---|",
        f"| pilot, first {h} samples (RT_KEEP_SUM) | {t('pilot_first')} |",
        f"| pilot, second {h} samples (accumulate) | {t('pilot_second')} |",
        f"| plan (budget {budget}) | {t('plan')} |",
        f"| counts render (accumulate) | {t('counts_planned')} |",
        f"| sum of the medians | {pipeline:.3f} |", "",
        f"The plan: mean count {mean_count:.3f} beyond the pilot (largest {stats['count_max_seen']}, "
        f"{stats['at_cap']} pixels cut by the cap, {stats['samples']} samples of {budget}).  "
        f"Wave utilisation from the counts (2x2-pixel waves, 16 lanes per pixel): mean rounds / max rounds = "
        f"{util:.3f} over the {100 * busy:.1f} % of waves that trace a sample.", "",
        "| call | ms | ms per 10^6 samples | kernel |", "|---|---|---|---|",
        f"| counts render of the plan ({mean_count:.2f} samples per pixel) | {t('counts_planned')} | "
        f"{res['counts_planned_ms_per_msample']:.4f} | `{kernels['counts_planned']}` |",
        f"| rt_render, {mspp} spp, 16 lanes per pixel | {t('uniform_mean_l16')} | "
        f"{res['uniform_mean_l16_ms_per_msample']:.4f} | `{kernels['uniform_mean_l16']}` |",
        f"| rt_render, {mspp} spp, automatic lanes | {t('uniform_mean_auto')} | "
        f"{res['uniform_mean_auto_ms_per_msample']:.4f} | `{kernels['uniform_mean_auto']}` |", "",
        "## (c) The planner against a copy of its compulsory bytes", "",
        "| call | ms | GB/s of compulsory bytes |", "|---|---|---|",
        f"| plan (2 kernels + a 32-B memset) | {t('plan')} | {res['plan_gb_s']:.0f} |",
        f"| floor: copy of {18 * W * H / 1e6:.1f} MB | {t('floor')} | {res['copy_gb_s']:.0f} |", "",
        f"plan / floor = {res['plan_over_floor']:.2f}.",
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
