#!/usr/bin/env python3
"""heatmap_peaks + box_heatmap_decode (two + one launches, no host round trip) vs a torch composition of the same
definition, written here after mmdet's CenterNetHead._decode_heatmap and a per-frame greedy NMS on the host — the ROCm
build of torch comes without torchvision, so there is no device NMS to call.

Size: F = 48 camera frames, 10 categories, maps of 112 x 200 (images of 448 x 800, stride 4), K = 100 and K = 500 peaks
per frame, score threshold 0.1, IoU threshold 0.5, class-aware, post_max_size 100; float32 heat map (probabilities) and
heads (offset 2, size 2 as separate tensors), seed 42.

Both sides start from the heat map.  The fused side ranks it (`heatmap_peaks(kernel=1)`: a plain top-K, what the
composition does) and decodes.  The composition does topk, the two gathers, the corner arithmetic, the clamp and the
score mask on the device in the operator's float32 operation order; then per frame the boolean index, the boxes and
labels to the host, the greedy NMS there and the kept indices back.  Its host NMS is the greedy loop with the inner loop
vectorised in numpy float32, in the operator's operation order (a pure Python double loop would flatter the operator), so
the outputs of the two can be compared bit for bit: "output tensors that differ" counts, of boxes, scores, labels, source
and sample_sizes, those that are not bitwise equal.

Both alternate inside one process: a timed block is `--calls` back-to-back calls of one side between two device events
(the composition synchronises inside; the events still enclose all of its work), its time divided by the number of calls;
`--iters` blocks per side; median and minimum per call over the blocks.  Launch counts come from torch's profiler in a
separate pass (kernel events per call; copies and memsets are not counted); host round trips are the synchronisations
torch's sync debug mode reports during one call; "not measured" if either is unavailable.
Prints a few lines of log per K and ONE JSON line.

    python3 scripts/bench_box_decode.py [--warmup 20] [--iters 10] [--calls 10] [--out FILE]
"""
import json

import numpy as np
import torch

from measure import emit, gpu, launches, parser, round_trips, shown, summary, window_times

FRAMES, CATEGORIES = 48, 10
HM, WM = 112, 200
IMAGE_HW = (448, 800)
OPTS = dict(score_threshold=0.1, iou_threshold=0.5, post_max_size=100)


def make_inputs(dev, seed=42):
    g = torch.Generator().manual_seed(seed)
    heat = (torch.randn(FRAMES, CATEGORIES, HM, WM, generator=g) - 3.0).sigmoid().to(dev)
    offset = torch.rand(FRAMES, 2, HM, WM, generator=g).to(dev)
    size = (2.0 + 20.0 * torch.rand(FRAMES, 2, HM, WM, generator=g)).to(dev)
    return heat, [offset, size]


def greedy_nms_host(boxes, labels, thresh, post_max_size):
    """greedy IoU NMS on host float32 arrays already in descending score order, class-aware: the kept indices"""
    n = boxes.shape[0]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = np.zeros(n, bool)
    keep = []
    zero = np.float32(0)
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        if len(keep) >= post_max_size:
            break
        rest = boxes[i + 1:]
        iw = np.minimum(boxes[i, 2], rest[:, 2]) - np.maximum(boxes[i, 0], rest[:, 0])
        ih = np.minimum(boxes[i, 3], rest[:, 3]) - np.maximum(boxes[i, 1], rest[:, 1])
        inter = np.maximum(iw, zero) * np.maximum(ih, zero)
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / ((area[i] + area[i + 1:]) - inter)
        dead[i + 1:] |= (iou > np.float32(thresh)) & (labels[i + 1:] == labels[i])
    return keep


def composition(heat, heads, K):
    """(boxes [F, M, 4], scores, labels, source [F, M], sizes [F]) with the operator's padding"""
    dev = heat.device
    F = heat.shape[0]
    M = min(K, OPTS["post_max_size"])
    scores, inds = heat.view(F, -1).topk(K)
    clses, inds = inds // (HM * WM), inds % (HM * WM)
    ys, xs = (inds // WM).float(), (inds % WM).float()
    off, hw = (f.view(F, 2, -1).permute(0, 2, 1).gather(1, inds[..., None].expand(-1, -1, 2)) for f in heads)
    cx, cy = xs + off[..., 0], ys + off[..., 1]
    half_w, half_h = 0.5 * hw[..., 1], 0.5 * hw[..., 0]
    ux = torch.tensor(float(IMAGE_HW[1]), device=dev) / torch.tensor(float(WM), device=dev)
    uy = torch.tensor(float(IMAGE_HW[0]), device=dev) / torch.tensor(float(HM), device=dev)
    boxes = torch.stack([((cx - half_w) * ux).clamp(0, IMAGE_HW[1]), ((cy - half_h) * uy).clamp(0, IMAGE_HW[0]),
                         ((cx + half_w) * ux).clamp(0, IMAGE_HW[1]), ((cy + half_h) * uy).clamp(0, IMAGE_HW[0])], -1)
    mask = scores > OPTS["score_threshold"]
    out_boxes = torch.zeros((F, M, 4), device=dev)
    out_scores = torch.zeros((F, M), device=dev)
    out_labels = torch.zeros((F, M), dtype=torch.int64, device=dev)
    out_source = torch.full((F, M), -1, dtype=torch.int32, device=dev)
    sizes = torch.zeros((F,), dtype=torch.int64)
    for f in range(F):
        rank = mask[f].nonzero()[:, 0]                                         # boolean index: a host synchronisation
        bx, lb = boxes[f][rank], clses[f][rank]
        keep = greedy_nms_host(bx.cpu().numpy(), lb.cpu().numpy(), OPTS["iou_threshold"], OPTS["post_max_size"])
        keep = torch.tensor(keep, dtype=torch.long, device=dev)
        n = keep.numel()
        out_boxes[f, :n], out_scores[f, :n], out_labels[f, :n] = bx[keep], scores[f][rank][keep], lb[keep]
        out_source[f, :n] = rank[keep].int()
        sizes[f] = n
    return out_boxes, out_scores, out_labels, out_source, sizes.to(dev)


def main():
    ap = parser(warmup=20, iters=10, calls=10)
    ap.add_argument("--k", type=int, nargs="+", default=[100, 500])
    args = ap.parse_args()
    dev = gpu()
    from accvlab.draw_heatmap import box_heatmap_decode, heatmap_peaks

    heat, heads = make_inputs(dev)
    lines, results = [], []
    for K in args.k:
        def fused():
            return box_heatmap_decode(heatmap_peaks(heat, K, kernel=1), heads, image_hw=IMAGE_HW, **OPTS)

        def decode_only(peaks=heatmap_peaks(heat, K, kernel=1)):   # noqa: B008 - the peaks are computed once
            return box_heatmap_decode(peaks, heads, image_hw=IMAGE_HW, **OPTS)

        comp = lambda: composition(heat, heads, K)   # noqa: E731
        got, ref = fused(), comp()
        torch.cuda.synchronize()
        mine = (got.boxes.tensor, got.scores.tensor, got.labels.tensor, got.source.tensor, got.boxes.sample_sizes)
        differ = sum(0 if a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) else 1
                     for a, b in zip(mine, ref))
        dets = int(got.boxes.sample_sizes.sum())
        ms = window_times({"fused": fused, "decode_only": decode_only, "torch": comp}, args.warmup, args.iters, args.calls)
        ms = {k: summary(v, args.calls, with_max=True) for k, v in ms.items()}
        n_fused, n_decode, n_torch = launches(fused), launches(decode_only), launches(comp)
        r_fused, r_decode, r_torch = round_trips(fused), round_trips(decode_only), round_trips(comp)
        results.append(dict(K=K, detections=dets, fused=ms["fused"], decode_only=ms["decode_only"], torch=ms["torch"],
                            speedup_median=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                            launches_fused=shown(n_fused), launches_decode_only=shown(n_decode), launches_torch=shown(n_torch),
                            host_round_trips_fused=shown(r_fused), host_round_trips_decode_only=shown(r_decode),
                            host_round_trips_torch=shown(r_torch), output_tensors_that_differ=differ))
        lines += [f"box_heatmap_decode  F={FRAMES} C={CATEGORIES} {HM}x{WM} K={K} post_max_size={OPTS['post_max_size']}: {dets} detections",
                  f"  {args.warmup} warm-up calls, {args.iters} blocks of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s "
                  f"fused, {ms['torch']['timed_s']} s torch",
                  f"  peaks + decode  median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {shown(n_fused)}  "
                  f"host round trips {shown(r_fused)}",
                  f"  decode alone    median {ms['decode_only']['median_ms']:.4f} ms  min {ms['decode_only']['min_ms']:.4f} ms  launches "
                  f"{shown(n_decode)}  host round trips {shown(r_decode)}",
                  f"  torch + host    median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {shown(n_torch)}  "
                  f"host round trips {shown(r_torch)}",
                  f"  against the torch composition: {differ} of 5 output tensors differ"]
    result = dict(metric="box_heatmap_decode_ms", unit="ms", value=results[-1]["fused"]["median_ms"], warmup=args.warmup, iters=args.iters,
                  calls_per_block=args.calls, shape=dict(F=FRAMES, C=CATEGORIES, H=HM, W=WM, post_max_size=OPTS["post_max_size"]), runs=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
