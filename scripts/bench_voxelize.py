#!/usr/bin/env python3
"""voxelize_points (one memset and five launches for the batch) vs two baselines that give the same bits:

  (a) `host round trip`: device -> host copy of the points, the library's own sequential host entry, host -> device copy of
      the outputs (what a loader-side voxelizer costs a step);
  (b) `torch composition`: the deterministic composition of the definition on the device (examples/voxelize_step.py
      composed_voxels: `unique` with inverse over the keys, first occurrence by `scatter_reduce("amin")`, a stable `argsort`
      for the ranks).

Shapes (seed 1): B = 1 and B = 8 frames; P ragged around 34 000 points a frame (one nuScenes sweep) and around 250 000 (ten
sweeps); pillars (0.2 m over +-51.2 m, g_z = 1, T = 20, V = 40 000, 4 channels) and voxels (0.075 m over +-54 m by 8 m,
T = 10, V = 120 000, 5 channels); the augmentation rows of bev_augment_boxes folded inside in every row.

Every row is timed in `--blocks` blocks, the rows taking turns inside a block; a block is `--iters` windows of `--calls`
(`--baseline-calls` for the baselines) back-to-back calls between two device events, after `--warmup` calls; a block's figure
is the median of its windows.  A row's median is the median of its block medians, its spread their max - min.  The verdict per
baseline: the fused median below the baseline's by more than the margin, the larger spread of the two rows (what the
measurement cannot resolve).  Launch counts come from torch's profiler in a separate pass (memsets and copies are not
counted; the host round trip launches none by construction and is not profiled); host round trips are counted from the code.  Before anything is timed the five fused outputs are compared with both
baselines bit for bit (the number of output tensors that differ).  `count + number alone` is the device time of the fused
call's two prefix-sum launches through the profiler (their share of the call), or "not measured".
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_voxelize.py [--warmup 5] [--blocks 3] [--iters 20] [--calls 10] [--baseline-calls 1] [--out FILE]
"""
import json

import torch

from measure import block_summary, emit, gpu, kernel_times, launches, parser, shown, timed_windows

SHAPES = ((8, 34000), (8, 250000), (1, 34000), (1, 250000))
FUSED, HOST, TORCH = "fused", "host round trip", "torch composition"
ROUND_TRIPS = {FUSED: 0, HOST: 2, TORCH: 1}


def main():
    ap = parser(warmup=5, iters=20, calls=10)
    ap.add_argument("--blocks", type=int, default=3, help="blocks per row; the rows take turns inside a block")
    ap.add_argument("--baseline-calls", type=int, default=1, help="back-to-back baseline calls per window")
    ap.add_argument("--baseline-iters", type=int, default=5, help="timed windows per block of a baseline row")
    args = ap.parse_args()
    dev = gpu()
    from voxelize_step import PILLARS, VOXELS, composed_voxels, differing, host_round_trip, make_cloud

    from accvlab.draw_heatmap import sample_bev_augmentation
    from accvlab.point_cloud import voxelize_points

    lines, results = [], []
    for grid_name, cfg, channels in (("pillars", PILLARS, 4), ("voxels", VOXELS, 5)):
        for B, P in SHAPES:
            points = make_cloud(B, P, channels, dev, seed=1)
            rows = sample_bev_augmentation(B, (-0.3925, 0.3925), (0.95, 1.05), (0.5, 0.5, 0.5), generator=torch.Generator(device=dev).manual_seed(1))
            full = dict(cfg, return_point_voxel=True)
            calls = {FUSED: lambda: voxelize_points(points, augmentation=rows, **full),
                     HOST: lambda: host_round_trip(points, rows, full),
                     TORCH: lambda: composed_voxels(points, rows, cfg)}
            names = [FUSED, HOST, TORCH]
            got = calls[FUSED]()
            differ = {r: differing(got, calls[r]()) for r in (HOST, TORCH)}
            counts, voxel_counts = points.sample_sizes.tolist(), got.voxel_counts.tolist()
            stored, in_voxels = int(got.num_points.sum()), int((got.point_voxel >= 0).sum())
            torch.cuda.synchronize()
            blocks = {r: [] for r in names}
            for _ in range(args.blocks):
                for r in names:
                    base = r != FUSED
                    blocks[r].append(timed_windows(calls[r], 1 if base else args.warmup, args.baseline_iters if base else args.iters,
                                                   args.baseline_calls if base else args.calls))
            n_launch = {r: 0 if r == HOST else shown(launches(calls[r])) for r in names}      # the round trip: copies only, by construction
            times = kernel_times(calls[FUSED])
            number_ms = round(sum(v for k, v in times.items() if "voxelize_number" in k or "voxelize_count" in k), 5) if times else None
            ms = {r: block_summary(blocks[r]) for r in names}
            verdicts = {}
            for r in (HOST, TORCH):
                margin = max(ms[FUSED]["spread_ms"], ms[r]["spread_ms"])
                verdicts[r] = dict(margin_ms=margin, fused_below_by_more_than_margin=bool(ms[FUSED]["median_ms"] < ms[r]["median_ms"] - margin))
            res = dict(shape=dict(grid=grid_name, B=B, P=int(points.tensor.shape[1]), D=channels, points_min=min(counts), points_max=max(counts),
                                  max_points=cfg["max_points"], max_voxels=cfg["max_voxels"], voxel_size=cfg["voxel_size"],
                                  point_cloud_range=cfg["point_cloud_range"]),
                       rows=ms, launches=n_launch, host_round_trips=ROUND_TRIPS, verdicts=verdicts, count_and_number_launches_alone_ms=number_ms,
                       output_tensors_differing=differ, voxels_min=min(voxel_counts), voxels_max=max(voxel_counts),
                       points_in_voxels=in_voxels, points_stored=stored)
            results.append(res)
            lines += [f"voxelize_points  {grid_name}: {cfg['voxel_size']} m over {cfg['point_cloud_range']}, T={cfg['max_points']}, "
                      f"V={cfg['max_voxels']}; B={B} frames, {min(counts)}..{max(counts)} points a frame (P={points.tensor.shape[1]}, {channels} "
                      f"channels), rows folded inside; {min(voxel_counts)}..{max(voxel_counts)} voxels a frame, {in_voxels} points in voxels, "
                      f"{stored} stored",
                      f"  {args.blocks} blocks a row of {args.iters} windows of {args.calls} calls ({args.baseline_iters} windows of "
                      f"{args.baseline_calls} for the baselines)"]
            for r in names:
                m = ms[r]
                lines.append(f"  {r:<18} median {m['median_ms']:.4f} ms  min {m['min_ms']:.4f} ms  block medians "
                             f"{' '.join(f'{v:.4f}' for v in m['block_medians_ms'])}  spread {m['spread_ms']:.4f}  launches {n_launch[r]}  "
                             f"host round trips {ROUND_TRIPS[r]}")
            for r in (HOST, TORCH):
                v = verdicts[r]
                lines.append(f"  fused {ms[FUSED]['median_ms']:.4f} ms vs {r} {ms[r]['median_ms']:.4f} ms "
                             f"({ms[r]['median_ms'] / ms[FUSED]['median_ms']:.1f}x), margin (larger spread of the two rows) {v['margin_ms']:.4f} ms: "
                             f"fused below it by more than the margin: {v['fused_below_by_more_than_margin']}")
            lines.append(f"  count + number alone (the prefix sum over the frame's points): "
                         f"{'not measured' if number_ms is None else f'{number_ms:.4f} ms'}; output tensors differing from the host round trip: "
                         f"{differ[HOST]} of 5; from the torch composition: {differ[TORCH]} of 5")
            emit(lines[-8:])
    result = dict(metric="voxelize_points_ms", unit="ms", value=results[0]["rows"][FUSED]["median_ms"], warmup=args.warmup, blocks=args.blocks,
                  iters=args.iters, calls_per_window=args.calls, baseline_iters=args.baseline_iters,
                  baseline_calls_per_window=args.baseline_calls, sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out, printed=len(lines) - 1)


if __name__ == "__main__":
    main()
