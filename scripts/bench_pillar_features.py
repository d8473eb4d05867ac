#!/usr/bin/env python3
"""pillar_features (one launch) vs the torch composition of mmdet3d's PillarFeatureNet.forward up to its PFN layers
(examples/pillar_step.py torch_pillar_features: a sum, a divide, three strided slice assignments into a zeros_like, a cat, a
mask build and a multiply).

Shapes (seed 1): T = 20, D = 4 (0.2 m pillars over +-51.2 m) and T = 32, D = 5 (KITTI's 0.16 m pillars), at B = 8 and B = 1
frames of about 34 000 points (the synthetic clouds of bench_voxelize.py); the voxels of voxelize_points, concatenated
(`[M, T, D]`, `[M, 4]`, `[M]`).  with_cluster_center and with_voxel_center on, with_distance off (mmdet3d's defaults).

Every row is timed in `--blocks` blocks, the rows taking turns inside a block; a block is `--iters` windows of `--calls`
back-to-back calls between two device events, after `--warmup` calls; a block's figure is the median of its windows.  A row's
median is the median of its block medians, its spread their max - min.  The verdict: the fused median below the
baseline's by more than the margin, the larger spread of the two rows.  Launch counts come from torch's profiler in a
separate pass, host synchronisations from torch's sync debug mode.  Before anything is timed the outputs are compared: the
input channels must be equal; the cluster channels are held to (2 n + 2) * 2^-24 * max_j |p_jk| (torch's sum has no defined
order); the centre channels are compared twice, with the composition's offsets v / 2 + lo evaluated in float64 and rounded
once as mmdet3d does, and evaluated in float32 as the library's definition does (0.2, 0.16 and 51.2 are not exact in
float32, so the two offsets can differ in their last bit).  Bytes moved by the fused call: voxels, num_points and coors
read, the output written.
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_pillar_features.py [--warmup 5] [--blocks 3] [--iters 20] [--calls 10] [--out FILE]
"""
import json

import torch

from measure import block_summary, emit, gpu, launches, parser, round_trips, shown, timed_windows

SHAPES = (("nuscenes", 8), ("nuscenes", 1), ("kitti", 8), ("kitti", 1))
FUSED, TORCH = "fused", "torch composition"
PEAK = 8.0e12


def main():
    ap = parser(warmup=5, iters=20, calls=10)
    ap.add_argument("--blocks", type=int, default=3, help="blocks per row; the rows take turns inside a block")
    args = ap.parse_args()
    dev = gpu()
    from pillar_step import KITTI, NUSCENES, grid_of, torch_pillar_features
    from voxelize_step import make_cloud

    from accvlab.point_cloud import concatenate_voxels, pillar_features, voxelize_points

    lines, results = [], []
    for grid_name, B in SHAPES:
        cfg, D = (NUSCENES, 4) if grid_name == "nuscenes" else (KITTI, 5)
        voxels, coors, num = concatenate_voxels(voxelize_points(make_cloud(B, 34000, D, dev, seed=1), **cfg))
        M, T = int(voxels.shape[0]), int(voxels.shape[1])
        grid = grid_of(cfg)
        calls = {FUSED: lambda: pillar_features(voxels, num, coors, **grid),
                 TORCH: lambda: torch_pillar_features(voxels, num, coors, cfg["voxel_size"], cfg["point_cloud_range"])}
        got, ref = calls[FUSED](), calls[TORCH]()
        ref32 = torch_pillar_features(voxels, num, coors, cfg["voxel_size"], cfg["point_cloud_range"], float32_offsets=True)
        live = torch.arange(T, device=dev).view(1, T, 1) < num.view(M, 1, 1)
        bar = (2.0 * num.view(M, 1, 1).double() + 2.0) * 2.0 ** -24 * (voxels[..., :3].abs() * live).amax(dim=1, keepdim=True).double()
        checks = dict(input_elements_differing=int((got[..., :D] != ref[..., :D]).sum()),
                      cluster_elements_beyond_the_bar=int(((got[..., D:D + 3].double() - ref[..., D:D + 3].double()).abs() > bar).sum()),
                      centre_elements_differing_float64_offsets=int((got[..., D + 3:] != ref[..., D + 3:]).sum()),
                      centre_elements_differing_float32_offsets=int((got[..., D + 3:] != ref32[..., D + 3:]).sum()),
                      centre_max_abs_difference_float64_offsets=float((got[..., D + 3:] - ref[..., D + 3:]).abs().max()))
        del got, ref, ref32, bar
        torch.cuda.synchronize()
        blocks = {r: [] for r in calls}
        for _ in range(args.blocks):
            for r in calls:
                blocks[r].append(timed_windows(calls[r], args.warmup, args.iters, args.calls))
        ms = {r: block_summary(blocks[r]) for r in calls}
        margin = max(m["spread_ms"] for m in ms.values())
        below = bool(ms[FUSED]["median_ms"] < ms[TORCH]["median_ms"] - margin)
        n_launch = {r: shown(launches(calls[r])) for r in calls}
        trips = {r: shown(round_trips(calls[r])) for r in calls}
        moved = M * T * D * 4 + M * 4 + M * 16 + M * T * (D + 6) * 4
        frac = moved / (ms[FUSED]["median_ms"] * 1e-3) / PEAK
        res = dict(shape=dict(grid=grid_name, B=B, M=M, T=T, D=D, F=D + 6), rows=ms, margin_ms=margin, fused_below_by_more_than_margin=below,
                   launches=n_launch, host_round_trips=trips, bytes_moved=moved, fraction_of_8TBs=round(frac, 4), **checks)
        results.append(res)
        lines.append(f"pillar_features  {grid_name}: B={B}, M={M} voxels, T={T}, D={D} -> F={D + 6}; {args.blocks} blocks a row of {args.iters} "
                     f"windows of {args.calls} calls")
        for r in calls:
            m = ms[r]
            lines.append(f"  {r:<18} median {m['median_ms']:.4f} ms  min {m['min_ms']:.4f} ms  block medians "
                         f"{' '.join(f'{v:.4f}' for v in m['block_medians_ms'])}  spread {m['spread_ms']:.4f}  launches {n_launch[r]}  "
                         f"host round trips {trips[r]}")
        lines.append(f"  fused {ms[FUSED]['median_ms']:.4f} ms vs torch {ms[TORCH]['median_ms']:.4f} ms "
                     f"({ms[TORCH]['median_ms'] / ms[FUSED]['median_ms']:.1f}x), margin (larger spread) {margin:.4f} ms: fused below it by more than "
                     f"the margin: {below}; {moved / 1e6:.1f} MB moved = {frac:.3f} of 8 TB/s")
        lines.append(f"  input elements differing: {checks['input_elements_differing']}; cluster elements beyond the bar: "
                     f"{checks['cluster_elements_beyond_the_bar']}; centre elements differing from float64 offsets rounded once: "
                     f"{checks['centre_elements_differing_float64_offsets']} (max {checks['centre_max_abs_difference_float64_offsets']:.3e}), "
                     f"from float32 offsets: {checks['centre_elements_differing_float32_offsets']}")
        emit(lines[-5:])
    result = dict(metric="pillar_features_ms", unit="ms", value=results[0]["rows"][FUSED]["median_ms"], warmup=args.warmup, blocks=args.blocks,
                  iters=args.iters, calls_per_window=args.calls, sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out, printed=len(lines) - 1)


if __name__ == "__main__":
    main()
