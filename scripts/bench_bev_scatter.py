#!/usr/bin/env python3
"""scatter_to_bev (one memset and two launches; one more launch for the backward) vs two torch baselines with equal outputs:

  (b) `torch loop`: mmdet3d's PointPillarsScatter, per frame a zeros canvas, a mask, a transposed index assignment, then a
      stack (examples/pillar_step.py torch_scatter_loop);
  (c) `torch flat`: the same without the loop, one zeros and one flat index_put_ (torch_scatter_flat; its NHWC -> NCHW copy
      is part of it, since the backbone reads NCHW).

Shapes (seed 1): C = 64 on 512 x 512 (0.2 m over +-51.2 m) at B = 8 and B = 1 and on 496 x 432 (KITTI's 0.16 m) at B = 8, in
float32 and bfloat16; the rows are the voxels of voxelize_points on the synthetic clouds of bench_voxelize.py, about 34 000
points a frame, concatenated (`[M, C]`, `[M, 4]`).  Forward, and forward + backward (the upstream gradient is a fixed
tensor; the backward of the baselines is torch autograd).

Every row is timed in `--blocks` blocks, the rows taking turns inside a block; a block is `--iters` windows of `--calls`
back-to-back calls between two device events, after `--warmup` calls; a block's figure is the median of its windows.  A row's
median is the median of its block medians, its spread their max - min.  The verdict per baseline: the fused median below
the baseline's by more than the margin, the largest spread of the rows compared.  Launch counts and the backward kernel's
own device time come from torch's profiler in a separate pass (memsets and copies are not counted), host synchronisations
from torch's sync debug mode.  Before anything is timed the canvas and the gradient are compared with both baselines
(torch.equal; the number of output tensors that differ).  Bytes of the fused forward: the canvas written, the index cleared,
marked and read, the coors and the placed feature rows read; shown as a fraction of 8 TB/s.
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_bev_scatter.py [--warmup 3] [--blocks 3] [--iters 10] [--calls 5] [--out FILE]
"""
import json

import torch

from measure import block_summary, emit, gpu, kernel_times, launches, parser, round_trips, shown, timed_windows

SHAPES = (("nuscenes", 8), ("nuscenes", 1), ("kitti", 8))
FUSED, LOOP, FLAT = "fused", "torch loop", "torch flat"
PEAK = 8.0e12


def main():
    ap = parser(warmup=3, iters=10, calls=5)
    ap.add_argument("--blocks", type=int, default=3, help="blocks per row; the rows take turns inside a block")
    ap.add_argument("--channels", type=int, default=64)
    args = ap.parse_args()
    dev = gpu()
    from pillar_step import GRID_HW, KITTI, NUSCENES, torch_scatter_flat, torch_scatter_loop
    from voxelize_step import make_cloud

    from accvlab.point_cloud import concatenate_voxels, scatter_to_bev, voxelize_points

    C = args.channels
    lines, results = [], []
    for grid_name, B in SHAPES:
        cfg, (ny, nx) = (NUSCENES if grid_name == "nuscenes" else KITTI), GRID_HW[grid_name]
        _, coors, _ = concatenate_voxels(voxelize_points(make_cloud(B, 34000, 4, dev, seed=1), **cfg))
        M = int(coors.shape[0])
        for dtype in (torch.float32, torch.bfloat16):
            es = torch.empty((), dtype=dtype).element_size()
            feats = torch.randn(M, C, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dtype).requires_grad_(True)
            go = torch.randn(B, C, ny, nx, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(dtype)
            fwd = {FUSED: lambda: scatter_to_bev(feats, coors, grid_hw=(ny, nx), batch_size=B),
                   LOOP: lambda: torch_scatter_loop(feats, coors, B, ny, nx),
                   FLAT: lambda: torch_scatter_flat(feats, coors, B, ny, nx)}
            both = {r: (lambda f=f: torch.autograd.grad(f(), feats, go)[0]) for r, f in fwd.items()}
            plain = {r: _no_grad(f) for r, f in fwd.items()}
            names = [FUSED, LOOP, FLAT]
            got, grad = fwd[FUSED](), both[FUSED]()
            differ = {r: int(not torch.equal(got, fwd[r]())) + int(not torch.equal(grad, both[r]())) for r in (LOOP, FLAT)}
            del got, grad
            torch.cuda.synchronize()
            res = dict(shape=dict(grid=grid_name, B=B, C=C, ny=ny, nx=nx, rows=M, dtype=str(dtype).replace("torch.", "")))
            for what, calls in (("forward", plain), ("forward_backward", both)):
                blocks = {r: [] for r in names}
                for _ in range(args.blocks):
                    for r in names:
                        blocks[r].append(timed_windows(calls[r], args.warmup, args.iters, args.calls))
                ms = {r: block_summary(blocks[r]) for r in names}
                margin = max(m["spread_ms"] for m in ms.values())
                verdict = {r: bool(ms[FUSED]["median_ms"] < ms[r]["median_ms"] - margin) for r in (LOOP, FLAT)}
                res[what] = dict(rows=ms, margin_ms=margin, fused_below_by_more_than_margin=verdict)
            res["launches"] = {r: shown(launches(plain[r])) for r in names}
            res["launches_forward_backward"] = {r: shown(launches(both[r])) for r in names}
            res["host_round_trips"] = {r: shown(round_trips(plain[r])) for r in names}
            times = kernel_times(both[FUSED])
            bwd_ms = round(sum(v for k, v in times.items() if "bev_gather" in k), 5) if times else None
            fwd_bytes = B * C * ny * nx * es + 3 * B * ny * nx * 4 + M * 16 + M * C * es
            bwd_bytes = M * C * es + M * 16 + M * 4 + M * C * 32       # a 32-byte sector per gathered element
            frac = fwd_bytes / (res["forward"]["rows"][FUSED]["median_ms"] * 1e-3) / PEAK
            res.update(output_tensors_differing=differ, forward_bytes=fwd_bytes, forward_fraction_of_8TBs=round(frac, 4),
                       backward_kernel_ms=bwd_ms, backward_bytes_useful=M * C * es * 2 + M * 20, backward_bytes_with_sectors=bwd_bytes)
            results.append(res)
            lines.append(f"scatter_to_bev  {grid_name} {ny} x {nx}, B={B}, C={C}, {res['shape']['dtype']}, {M} rows; {args.blocks} blocks a row of "
                         f"{args.iters} windows of {args.calls} calls")
            for what in ("forward", "forward_backward"):
                for r in names:
                    m = res[what]["rows"][r]
                    n_l = res["launches" if what == "forward" else "launches_forward_backward"][r]
                    lines.append(f"  {what:<16} {r:<11} median {m['median_ms']:.4f} ms  min {m['min_ms']:.4f} ms  block medians "
                                 f"{' '.join(f'{v:.4f}' for v in m['block_medians_ms'])}  spread {m['spread_ms']:.4f}  launches {n_l}"
                                 + (f"  host round trips {res['host_round_trips'][r]}" if what == "forward" else ""))
                f = res[what]["rows"][FUSED]["median_ms"]
                lines.append(f"  {what}: fused {f:.4f} ms vs loop {res[what]['rows'][LOOP]['median_ms'] / f:.2f}x, vs flat "
                             f"{res[what]['rows'][FLAT]['median_ms'] / f:.2f}x; margin (largest spread) {res[what]['margin_ms']:.4f} ms: fused below "
                             f"by more than the margin: loop {res[what]['fused_below_by_more_than_margin'][LOOP]}, flat "
                             f"{res[what]['fused_below_by_more_than_margin'][FLAT]}")
            lines.append(f"  forward bytes {fwd_bytes / 1e6:.1f} MB = {frac:.3f} of 8 TB/s; backward kernel alone "
                         f"{'not measured' if bwd_ms is None else f'{bwd_ms:.4f} ms'} for {res['backward_bytes_useful'] / 1e6:.1f} MB useful "
                         f"({bwd_bytes / 1e6:.1f} MB with a 32-byte sector per gathered element); output tensors differing from the loop: "
                         f"{differ[LOOP]} of 2, from the flat composition: {differ[FLAT]} of 2")
            emit(lines[-10:])
            del feats, go
            torch.cuda.empty_cache()
    result = dict(metric="scatter_to_bev_forward_ms", unit="ms", value=results[0]["forward"]["rows"][FUSED]["median_ms"], warmup=args.warmup,
                  blocks=args.blocks, iters=args.iters, calls_per_window=args.calls, sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out, printed=len(lines) - 1)


def _no_grad(f):
    def call():
        with torch.no_grad():
            return f()
    return call


if __name__ == "__main__":
    main()
