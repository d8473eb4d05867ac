#!/usr/bin/env python3
"""lidar_depth_targets (one launch) vs the torch composition of its definition on the device
(examples/depth_targets_step.py composed_targets: fold the matrices, matmul, divide, masks, cell index,
scatter_reduce_("amin"), bins), and the fused call under other band rules.

Shapes (seed 1): C = 6 cameras, 900 x 1600 sources prepared to 256 x 704, stride 16 (maps of 16 x 44), 112 bins of 0.5 m from
2 m, image matrices folded inside; B = 8 and B = 1 frames; P ragged around 34 000 points per frame (one nuScenes sweep) and
around 250 000 (ten sweeps), 4 channels.

Rows: `fused` is the library's band rule (bands beyond those that are needed only while the launch stays at or below 64
workgroups: one band of 16 rows at B = 8, eight bands of 2 rows at B = 1); `fused, bands of R rows` forces bands of R rows
through the private `_band_rows` (16 rows: one band a map), which makes 16 / R workgroups a map, each projecting all points
of the frame; `torch composition` is the baseline.  Every row is timed in `--blocks` blocks, the rows taking turns
inside a block; a block is `--iters` windows of `--calls` (`--baseline-calls` for the torch row) back-to-back calls between two
device events, after `--warmup` calls; a block's figure is the median of its windows.  A row's median is the median of its
block medians, its spread their max - min.  The verdict per comparison: one median below the other by more than the margin,
the larger spread of the two rows (what the measurement cannot resolve).  Launch counts come from torch's profiler in a
separate pass; host round trips are counted from the code.  Before anything is timed the fused outputs are compared with the
composition in the definition's own operation order (bit for bit: the number of output tensors that differ) and with the
matmul composition that is timed (cells filled on one side only, the largest depth difference, bins that differ), and the
band rules with each other.
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_depth_targets.py [--warmup 10] [--blocks 3] [--iters 40] [--calls 20] [--baseline-calls 2] [--out FILE]
"""
import json

import torch

from measure import block_summary, emit, gpu, launches, parser, shown, timed_windows

SOURCE_HW, OUTPUT_HW, CAMERAS = (900, 1600), (256, 704), 6
SHAPES = ((8, 34000), (8, 250000), (1, 34000), (1, 250000))
BAND_ROWS = (16, 4, 1)
TORCH = "torch composition"


def main():
    ap = parser(warmup=10, iters=40, calls=20)
    ap.add_argument("--blocks", type=int, default=3, help="blocks per row; the rows take turns inside a block")
    ap.add_argument("--baseline-calls", type=int, default=2, help="back-to-back torch-composition calls per window")
    args = ap.parse_args()
    dev = gpu()
    from depth_targets_step import STRIDE, composed_targets, fused_targets, image_matrices, make_scene

    h, w = -(-OUTPUT_HW[0] // STRIDE), -(-OUTPUT_HW[1] // STRIDE)
    lines, results = [], []
    for B, P in SHAPES:
        points, lidar2img = make_scene(B, CAMERAS, P, SOURCE_HW, dev, seed=1)
        matrices = image_matrices(B, CAMERAS, SOURCE_HW, OUTPUT_HW, dev)
        rows = ["fused"] + [f"fused, bands of {r} rows" for r in BAND_ROWS] + [TORCH]
        calls = {"fused": lambda: fused_targets(points, lidar2img, matrices, OUTPUT_HW),
                 TORCH: lambda: composed_targets(points, lidar2img, matrices, OUTPUT_HW)}
        for r in BAND_ROWS:
            calls[f"fused, bands of {r} rows"] = lambda r=r: fused_targets(points, lidar2img, matrices, OUTPUT_HW, band_rows=r)
        got = calls["fused"]()
        exact = composed_targets(points, lidar2img, matrices, OUTPUT_HW, definition_order=True)
        loose = calls[TORCH]()
        differ_exact = int(not torch.equal(got.depth.view(torch.int32), exact[0].view(torch.int32))) + int(not torch.equal(got.bins, exact[1]))
        one_sided = int(((got.depth != 0) != (loose[0] != 0)).sum())
        depth_diff = float((got.depth - loose[0]).abs().max())
        bins_differ = int((got.bins != loose[1]).sum())
        differ_bands = sum(int(not torch.equal(got.depth.view(torch.int32), o.depth.view(torch.int32))) + int(not torch.equal(got.bins, o.bins))
                           for o in (calls[f"fused, bands of {r} rows"]() for r in BAND_ROWS))
        filled = int((got.depth != 0).sum())
        torch.cuda.synchronize()
        blocks = {r: [] for r in rows}
        for _ in range(args.blocks):
            for r in rows:
                n = args.baseline_calls if r == TORCH else args.calls
                blocks[r].append(timed_windows(calls[r], 3 if r == TORCH else args.warmup, args.iters, n))
        n_launch = {r: shown(launches(calls[r])) for r in rows}
        ms = {r: block_summary(blocks[r]) for r in rows}
        rule_rows = -(-h // max(1, min(h, 64 // (B * CAMERAS))))       # the library's rule, restated
        workgroups = {"fused": B * CAMERAS * -(-h // rule_rows), TORCH: None}
        workgroups.update({f"fused, bands of {r} rows": B * CAMERAS * -(-h // r) for r in BAND_ROWS})

        def below(a, b):
            margin = max(ms[a]["spread_ms"], ms[b]["spread_ms"])
            return margin, bool(ms[a]["median_ms"] < ms[b]["median_ms"] - margin)

        margin, faster = below("fused", TORCH)
        band_verdicts = {}
        for r in BAND_ROWS:
            name = f"fused, bands of {r} rows"
            mg, wins = below(name, "fused")
            _, loses = below("fused", name)
            band_verdicts[name] = dict(margin_ms=mg, below_the_rule_by_more_than_margin=wins, above_the_rule_by_more_than_margin=loses)
        counts = points.sample_sizes.tolist()
        res = dict(shape=dict(B=B, C=CAMERAS, P=int(points.tensor.shape[1]), D=4, points_min=min(counts), points_max=max(counts),
                              image_h=OUTPUT_HW[0], image_w=OUTPUT_HW[1], stride=STRIDE, map_h=h, map_w=w, bins=112),
                   rows=ms, launches=n_launch, host_round_trips={r: 0 for r in rows}, workgroups=workgroups,
                   margin_ms=margin, fused_below_composition_by_more_than_margin=faster, band_rules=band_verdicts,
                   output_tensors_differing_from_definition_order_composition=differ_exact,
                   output_tensors_differing_between_band_rules=differ_bands,
                   matmul_composition=dict(cells_filled_on_one_side_only=one_sided, largest_depth_difference=depth_diff, bins_differing=bins_differ),
                   filled_cells=filled)
        results.append(res)
        lines += [f"lidar_depth_targets  B={B} frames x C={CAMERAS} cameras, {min(counts)}..{max(counts)} points a frame (P={points.tensor.shape[1]}, "
                  f"4 channels), {OUTPUT_HW[0]}x{OUTPUT_HW[1]} at stride {STRIDE}: maps of {h}x{w}, 112 bins, image matrices folded inside; "
                  f"{filled} of {B * CAMERAS * h * w} cells filled",
                  f"  {args.blocks} blocks a row of {args.iters} windows of {args.calls} calls ({args.baseline_calls} for the torch row)"]
        for r in rows:
            m = ms[r]
            wg = "" if workgroups[r] is None else f"  workgroups {workgroups[r]}"
            lines.append(f"  {r:<26} median {m['median_ms']:.4f} ms  min {m['min_ms']:.4f} ms  block medians "
                         f"{' '.join(f'{v:.4f}' for v in m['block_medians_ms'])}  spread {m['spread_ms']:.4f}  launches {n_launch[r]}  "
                         f"host round trips 0{wg}")
        lines.append(f"  fused {ms['fused']['median_ms']:.4f} ms vs torch composition {ms[TORCH]['median_ms']:.4f} ms "
                     f"({ms[TORCH]['median_ms'] / ms['fused']['median_ms']:.1f}x), margin (larger spread of the two rows) {margin:.4f} ms: "
                     f"fused below the composition by more than the margin: {faster}")
        for name, v in band_verdicts.items():
            word = "wins" if v["below_the_rule_by_more_than_margin"] else "loses" if v["above_the_rule_by_more_than_margin"] else "ties (within the margin)"
            lines.append(f"  {name} {ms[name]['median_ms']:.4f} ms vs the library's rule {ms['fused']['median_ms']:.4f} ms, margin {v['margin_ms']:.4f} ms: {word}")
        lines.append(f"  output tensors differing from the composition in the definition's order: {differ_exact} of 2; between band rules: "
                     f"{differ_bands} of {2 * len(BAND_ROWS)}; against the timed matmul composition: {one_sided} cells filled on one side only, "
                     f"largest depth difference {depth_diff:.2e}, {bins_differ} bins differ")
    result = dict(metric="lidar_depth_targets_ms", unit="ms", value=results[0]["rows"]["fused"]["median_ms"], warmup=args.warmup,
                  blocks=args.blocks, iters=args.iters, calls_per_window=args.calls, baseline_calls_per_window=args.baseline_calls,
                  sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
