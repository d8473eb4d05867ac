#!/usr/bin/env python3
"""visible_bbox_mask (one launch, no canvas) vs the two ways to get the same mask without it, both written here.

Sizes (ragged, seed 42, occlusion check plus minimum_size = 2):
    B = 48 frames of 900 x 1600 (6 cameras x 8 samples), N in [1, 64] boxes per frame;
    B = 64 frames of 1080 x 1920, N in [1, 128].

Baselines, both the per-sample canvas painter of the reference's VisibleBboxSelector (an H x W int32 canvas, the boxes
painted from far to near, `unique` on the canvas), with this package's tie rule (stable sort) so that the masks are equal:
    numpy   device -> host copy of boxes, depths and sizes, the painter in numpy frame by frame, host -> device copy of the mask;
    torch   the painter on the device: the integer rectangles computed by tensor operations and read back once for the slice
            bounds, one slice assignment per box, one `torch.unique` per frame (its result shape is a host round trip).

The fused side is timed as in bench_center_targets.py: `--iters` windows of `--calls` back-to-back calls between two device
events.  A baseline call takes from tens of milliseconds to seconds, so the baselines are timed call by call with the host
clock around a device synchronisation, `--baseline-iters` calls each.  Launch counts come from torch's profiler in a
separate pass (kernel events per call; copies and memsets are not counted; the numpy baseline launches none by
construction and is not profiled); "not measured" if the profiler is unavailable.
Host round trips are counted from the code: every copy to the host or operation whose result shape the host needs.
Prints a few lines of log per size and ONE JSON line.

    python3 scripts/bench_visible_bboxes.py [--warmup 20] [--iters 100] [--calls 20] [--baseline-iters 3] [--out FILE]
"""
import json

import numpy as np
import torch

from measure import emit, gpu, launches, parser, shown, summary, timed_windows, wall_times

SIZES = ((48, 900, 1600, 64), (64, 1080, 1920, 128))
MIN_SIZE = 2.0


def make_inputs(B, H, W, n_max, dev, seed=42):
    """boxes of a few pixels to a third of the image around centres that may lie up to a tenth outside it, fractional
    corners, a tenth of them flipped; depths in [1, 80) metres"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, n_max + 1, (B,), generator=g)
    N = int(sizes.max())
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    cx, cy = (u(B, N) * 1.2 - 0.1) * W, (u(B, N) * 1.2 - 0.1) * H
    w, h = 4 + u(B, N) ** 3 * W / 3, 4 + u(B, N) ** 3 * H / 3
    boxes = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
    flip = u(B, N) < 0.1
    boxes[flip] = boxes[flip][:, [2, 3, 0, 1]]
    depths = 1 + u(B, N) * 79
    return boxes.to(torch.float32).contiguous().to(dev), depths.to(torch.float32).to(dev), sizes.to(dev)


def numpy_painter(boxes, depths, sizes, H, W):
    """D2H, the canvas painter frame by frame, H2D"""
    bx, dp, ns = boxes.cpu().numpy(), depths.cpu().numpy(), sizes.cpu().numpy()
    out = np.zeros(dp.shape, bool)
    for b in range(len(ns)):
        n = int(ns[b])
        canvas = np.full((H, W), -1, np.int32)
        for i in np.argsort(-dp[b, :n], kind="stable"):
            x1, y1, x2, y2 = bx[b, i]
            x0, x1 = (x1, x2) if x1 < x2 else (x2, x1)
            y0, y1 = (y1, y2) if y1 < y2 else (y2, y1)
            x0, y0, x1, y1 = int(np.floor(x0)), int(np.floor(y0)), int(np.ceil(x1)), int(np.ceil(y1))
            if x0 > W or x1 < 0 or y0 > H or y1 < 0:
                continue
            canvas[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = i
        seen = np.unique(canvas)
        out[b, seen[seen >= 0]] = True
        c = bx[b, :n].copy()
        c[:, 0::2] = np.clip(c[:, 0::2], 0.0, W)
        c[:, 1::2] = np.clip(c[:, 1::2], 0.0, H)
        out[b, :n] &= (np.abs(c[:, 2] - c[:, 0]) >= MIN_SIZE) & (np.abs(c[:, 3] - c[:, 1]) >= MIN_SIZE)
    return torch.from_numpy(out).to(boxes.device)


def torch_painter(boxes, depths, sizes, H, W):
    """the canvas on the device: one slice assignment per box, one unique per frame"""
    B, N = depths.shape
    lo = torch.minimum(boxes[..., :2], boxes[..., 2:]).floor()
    hi = torch.maximum(boxes[..., :2], boxes[..., 2:]).ceil()
    lim = torch.tensor([W, H], dtype=torch.float32, device=boxes.device)
    inside = ((lo <= lim) & (hi >= 0)).all(-1)
    rect = torch.cat([lo.clamp(min=0), torch.minimum(hi, lim)], -1).to(torch.int32)
    live = torch.arange(N, device=boxes.device)[None] < sizes[:, None]
    order = torch.argsort(torch.where(live, -depths, float("inf")), dim=1, stable=True)
    rect_h, order_h, inside_h, ns = rect.tolist(), order.tolist(), inside.tolist(), sizes.tolist()   # the one read-back of bounds
    out = torch.zeros((B, N), dtype=torch.bool, device=boxes.device)
    canvas = torch.empty((H, W), dtype=torch.int32, device=boxes.device)
    for b in range(B):
        canvas.fill_(-1)
        for i in order_h[b][:ns[b]]:
            if inside_h[b][i]:
                x0, y0, x1, y1 = rect_h[b][i]
                canvas[y0:y1, x0:x1] = i
        seen = torch.unique(canvas)
        out[b, seen[seen >= 0].long()] = True
    c = torch.stack([boxes[..., 0].clamp(0, W), boxes[..., 1].clamp(0, H), boxes[..., 2].clamp(0, W), boxes[..., 3].clamp(0, H)], -1)
    big = ((c[..., 2] - c[..., 0]).abs() >= MIN_SIZE) & ((c[..., 3] - c[..., 1]).abs() >= MIN_SIZE)
    return out & big & live


def main():
    ap = parser(warmup=20, iters=100, calls=20)
    ap.add_argument("--baseline-iters", type=int, default=3, help="timed calls of each baseline")
    args = ap.parse_args()
    dev = gpu()
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import visible_bbox_mask

    lines, results = [], []
    for B, H, W, n_max in SIZES:
        boxes, depths, sizes = make_inputs(B, H, W, n_max, dev)
        rb = RaggedBatch(boxes, sample_sizes=sizes)
        hw = torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev)
        fused = lambda: visible_bbox_mask(rb, depths, image_hw=hw, minimum_size=MIN_SIZE)          # noqa: E731
        via_numpy = lambda: numpy_painter(boxes, depths, sizes, H, W)                              # noqa: E731
        via_torch = lambda: torch_painter(boxes, depths, sizes, H, W)                              # noqa: E731
        got, ref_np, ref_t = fused().tensor, via_numpy(), via_torch()
        torch.cuda.synchronize()
        differ = dict(numpy=int(not torch.equal(got, ref_np)), torch=int(not torch.equal(got, ref_t)))
        elements = dict(numpy=int((got != ref_np).sum()), torch=int((got != ref_t).sum()))
        ms = dict(fused=timed_windows(fused, args.warmup, args.iters, args.calls),
                  numpy=summary(wall_times(via_numpy, args.baseline_iters), digits=3),
                  torch=summary(wall_times(via_torch, args.baseline_iters), digits=3))
        n = {k: shown(launches(f)) for k, f in (("fused", fused), ("torch", via_torch))}
        n["numpy"] = 0                                            # copies only, by construction
        trips = dict(fused=0, numpy=2, torch=1 + B)
        res = dict(shape=dict(B=B, H=H, W=W, N=int(boxes.shape[1])), boxes=int(sizes.sum()), kept=int(got.sum()),
                   fused=ms["fused"], numpy=ms["numpy"], torch=ms["torch"], launches=n, host_round_trips=trips,
                   speedup_median_vs_numpy=round(ms["numpy"]["median_ms"] / ms["fused"]["median_ms"], 1),
                   speedup_median_vs_torch=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 1),
                   output_tensors_that_differ=differ, elements_that_differ=elements)
        results.append(res)
        lines += [f"visible_bbox_mask  B={B} frames of {H}x{W}, N<={boxes.shape[1]}, occlusion + minimum_size {MIN_SIZE:g}: "
                  f"{res['boxes']} boxes, {res['kept']} kept",
                  f"  fused: {args.iters} windows of {args.calls} calls, timed {ms['fused']['timed_s']} s; baselines: "
                  f"{args.baseline_iters} calls each, timed {ms['numpy']['timed_s']} s numpy, {ms['torch']['timed_s']} s torch",
                  f"  fused          median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {n['fused']}  host round trips 0",
                  f"  numpy canvas   median {ms['numpy']['median_ms']:.3f} ms  min {ms['numpy']['min_ms']:.3f} ms  launches {n['numpy']}  host round trips 2",
                  f"  torch canvas   median {ms['torch']['median_ms']:.3f} ms  min {ms['torch']['min_ms']:.3f} ms  launches {n['torch']}  host round trips {1 + B}",
                  f"  output tensors that differ from the baselines: numpy {differ['numpy']}, torch {differ['torch']} "
                  f"(elements: {elements['numpy']}, {elements['torch']})"]
    result = dict(metric="visible_bbox_mask_ms", unit="ms", value=results[0]["fused"]["median_ms"], warmup=args.warmup,
                  iters=args.iters, calls_per_window=args.calls, baseline_iters=args.baseline_iters, sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)
    if any(v for r in results for v in r["output_tensors_that_differ"].values()):
        raise SystemExit("the masks differ from a baseline")


if __name__ == "__main__":
    main()
