#!/usr/bin/env python3
"""query_box_decode_3d (one launch, no host round trip) vs the torch composition it replaces and vs the route the library
offered before it.

Shapes: B in {1, 8} frames, (Q, C, max_num) in {(900, 10, 300), (900, 80, 300), (300, 80, 100)}: StreamPETR / PETR on
nuScenes, the same head over 80 classes, a DETR-sized head.  float32 logits (distinct values, so torch.topk has no tie to
order) and 10-value box rows, score threshold 0.1, post_center_range (-61.2, -61.2, -10, 61.2, 61.2, 10), seed 42.

  (a) fused          query_box_decode_3d on the raw logits
  (b) torch          mmdet3d's NMSFreeCoder.decode with denormalize_bbox, written here after it: per frame the sigmoid over
                     all Q * C logits, topk, div and mod, the row gather, exp / atan2 / cat, the score and range masks and
                     the boolean index (a host round trip per frame); the kept rows are then padded into the operator's
                     output layout so the two can be compared
  (c) peaks + torch  what the library offered before: heatmap_peaks(cls.view(B, 1, Q, C), K, kernel=1) on the logits (two
                     launches, defined order) and the same torch decode behind it

"output tensors that differ" counts, of boxes, scores, labels, source and sample_sizes of (a) against (b), those that are
not bitwise equal, and names them: exp, atan2 and the sigmoid of torch and of the kernel agree to a few ulp, not bit for bit.

All sides alternate inside one process: a timed block is `--calls` back-to-back calls of one side between two device events,
its time divided by the number of calls; `--iters` blocks per side; median and minimum per call over the blocks.  Launch
counts come from torch's profiler in a separate pass; host round trips are the synchronisations torch's sync debug mode
reports during one call; "not measured" if either is unavailable.  Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_query_decode.py [--warmup 20] [--iters 10] [--calls 10] [--out FILE]
"""
import json

import torch

from measure import emit, gpu, launches, parser, round_trips, shown, summary, window_times

BATCHES = (1, 8)
SHAPES = ((900, 10, 300), (900, 80, 300), (300, 80, 100))
D = 10
RANGE = (-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)
THR = 0.1
NAMES = ("boxes", "scores", "labels", "source", "sample_sizes")


def make_inputs(B, Q, C, dev, seed=42):
    g = torch.Generator().manual_seed(seed)
    N = Q * C
    base = torch.linspace(-9.0, 1.0, N)
    cls = torch.stack([base[torch.randperm(N, generator=g)] for _ in range(B)]).view(B, Q, C)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, Q, generator=g)   # noqa: E731
    ang = u(-3.14, 3.14)
    rows = torch.stack([u(-70, 70), u(-70, 70), u(-0.5, 1.5), u(0.0, 2.0), u(-5, 3), u(0.0, 1.0), ang.sin(), ang.cos(), u(-5, 5), u(-5, 5)], 2)
    return cls.contiguous().to(dev), rows.contiguous().to(dev)


def denormalize(rows):
    """mmdet3d's denormalize_bbox on gathered rows [K, 10]"""
    rot = torch.atan2(rows[:, 6:7], rows[:, 7:8])
    return torch.cat([rows[:, 0:1], rows[:, 1:2], rows[:, 4:5], rows[:, 2:3].exp(), rows[:, 3:4].exp(), rows[:, 5:6].exp(), rot, rows[:, 8:10]], 1)


def filter_and_pad(out, b, scores, labels, q, final, lo, hi):
    """the two masks and the boolean index of NMSFreeCoder.decode_single, then the operator's output layout"""
    boxes, out_scores, out_labels, out_source, sizes = out
    mask = scores > THR
    mask &= (final[:, :3] >= lo).all(1)
    mask &= (final[:, :3] <= hi).all(1)
    kept = final[mask]                                       # boolean index: a host synchronisation
    n = kept.shape[0]
    boxes[b, :n], out_scores[b, :n], out_labels[b, :n], out_source[b, :n] = kept, scores[mask], labels[mask], q[mask].int()
    sizes[b] = n


def empty_outputs(B, M, dev):
    return (torch.zeros((B, M, D - 1), device=dev), torch.zeros((B, M), device=dev), torch.zeros((B, M), dtype=torch.int64, device=dev),
            torch.full((B, M), -1, dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev))


def composition(cls, rows, K):
    B, Q, C = cls.shape
    out = empty_outputs(B, K, cls.device)
    lo, hi = torch.tensor(RANGE[:3], device=cls.device), torch.tensor(RANGE[3:], device=cls.device)
    for b in range(B):
        scores, idx = cls[b].sigmoid().view(-1).topk(K)
        labels, q = idx % C, idx // C
        filter_and_pad(out, b, scores, labels, q, denormalize(rows[b][q]), lo, hi)
    return out


def peaks_route(cls, rows, K, heatmap_peaks):
    B, Q, C = cls.shape
    out = empty_outputs(B, K, cls.device)
    lo, hi = torch.tensor(RANGE[:3], device=cls.device), torch.tensor(RANGE[3:], device=cls.device)
    peaks = heatmap_peaks(cls.view(B, 1, Q, C), K, kernel=1)
    for b in range(B):
        filter_and_pad(out, b, peaks.scores[b].sigmoid(), peaks.xs[b], peaks.ys[b], denormalize(rows[b][peaks.ys[b]]), lo, hi)
    return out


def main():
    args = parser(warmup=20, iters=10, calls=10).parse_args()
    dev = gpu()
    from accvlab.draw_heatmap import heatmap_peaks, query_box_decode_3d

    lines, results = [], []
    for Q, C, K in SHAPES:
        for B in BATCHES:
            cls, rows = make_inputs(B, Q, C, dev)
            fused = lambda: query_box_decode_3d(cls, rows, K, score_threshold=THR, post_center_range=RANGE)   # noqa: E731
            comp = lambda: composition(cls, rows, K)   # noqa: E731
            prev = lambda: peaks_route(cls, rows, K, heatmap_peaks)   # noqa: E731
            got, ref = fused(), comp()
            torch.cuda.synchronize()
            mine = (got.boxes.tensor, got.scores.tensor, got.labels.tensor, got.source.tensor, got.boxes.sample_sizes)
            differ = [n for n, a, b in zip(NAMES, mine, ref)
                      if not (a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))]
            worst = max(float((mine[0] - ref[0]).abs().max()), float((mine[1] - ref[1]).abs().max()))
            dets = int(got.boxes.sample_sizes.sum())
            sides = {"fused": fused, "torch": comp, "peaks_torch": prev}
            ms = {k: summary(v, args.calls, with_max=True) for k, v in window_times(sides, args.warmup, args.iters, args.calls).items()}
            n = {k: launches(f) for k, f in sides.items()}
            r = {k: round_trips(f) for k, f in sides.items()}
            results.append(dict(B=B, Q=Q, C=C, max_num=K, detections=dets, **ms,
                                speedup_median_vs_torch=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                                speedup_median_vs_peaks_torch=round(ms["peaks_torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                                launches={k: shown(v) for k, v in n.items()}, host_round_trips={k: shown(v) for k, v in r.items()},
                                output_tensors_that_differ=len(differ), tensors_that_differ=differ, largest_difference=worst))
            lines += [f"query_box_decode_3d  B={B} Q={Q} C={C} max_num={K}: {dets} detections",
                      f"  {args.warmup} warm-up calls, {args.iters} blocks of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s "
                      f"fused, {ms['torch']['timed_s']} s torch, {ms['peaks_torch']['timed_s']} s peaks + torch"]
            for key, label in (("fused", "(a) fused        "), ("torch", "(b) torch        "), ("peaks_torch", "(c) peaks + torch")):
                lines.append(f"  {label} median {ms[key]['median_ms']:.4f} ms  min {ms[key]['min_ms']:.4f} ms  launches {shown(n[key])}  "
                             f"host round trips {shown(r[key])}")
            lines.append(f"  against the torch composition: {len(differ)} of 5 output tensors differ ({', '.join(differ) or 'none'}; largest "
                         f"difference {worst:.3e})")
    result = dict(metric="query_box_decode_3d_ms", unit="ms", value=results[0]["fused"]["median_ms"], warmup=args.warmup, iters=args.iters,
                  calls_per_block=args.calls, runs=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
