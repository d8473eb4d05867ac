#!/usr/bin/env python3
"""heatmap_peaks + center_point_decode (two + one launches per head, no host round trip) vs a torch composition of the
same definition, written here after mmdet3d's CenterPointBBoxCoder.decode and the `circle` branch of
CenterHead.get_bboxes.

Size: B = 4 frames, the six nuScenes tasks over ten classes, 180 x 180 maps (pc_range +-54 m, voxel 0.075 m, stride 8),
K = 500 peaks per task and frame, score threshold 0.1, post_center_range +-61.2 m, mmdet3d's nuScenes min_radius list,
post_max_size 83; float32 logits and heads (reg 2, height 1, dim 3, rot 2, vel 2 as separate tensors), seed 42.

Both sides start from the logits.  The fused side ranks the raw logits (`heatmap_peaks(kernel=1)`: mmdet3d's decoder
takes a plain top-K) and decodes with `scores_are_logits=True`.  The composition does, per task, sigmoid, topk, the five
gathers, exp / atan2 / the affine map and the two masks on the device; then per frame the boolean index, the centres to
the host, the circle NMS there and the kept indices back — mmdet3d's flow.  Its host NMS is the greedy loop with the inner
loop vectorised in numpy (mmdet3d's is numba-jitted; neither is a pure Python double loop, which would flatter the
operator).

Both alternate inside one process: a timed block is `--calls` back-to-back calls of one side between two device events
(the composition synchronises inside; the events still enclose all of its work), its time divided by the number of calls;
`--iters` blocks per side; median and minimum per call over the blocks.  Launch counts come from torch's profiler in a
separate pass (kernel events per call; copies and memsets are not counted); "not measured" if the profiler is unavailable.
Prints a few lines of log and ONE JSON line.

    python3 scripts/bench_center_decode.py [--warmup 100] [--iters 20] [--calls 100] [--out FILE]
"""
import json

import numpy as np
import torch

from measure import emit, gpu, launches, parser, shown, summary, window_times

TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))
MIN_RADIUS = [4, 12, 10, 1, 0.85, 0.175]
CFG = dict(pc_range=[-54.0, -54.0], voxel_size=[0.075, 0.075], out_size_factor=8)
OPTS = dict(score_threshold=0.1, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], nms_threshold=MIN_RADIUS, post_max_size=83)
H = W = 180


def make_inputs(B, dev, seed=42):
    g = torch.Generator().manual_seed(seed)
    logits, heads = [], []
    for ids in TASKS:
        logits.append((torch.randn(B, len(ids), H, W, generator=g) - 3.0).to(dev))
        ang = (torch.rand(B, 1, H, W, generator=g) * 2 - 1) * np.pi
        heads.append([t.contiguous().to(dev) for t in (
            torch.rand(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g) * 8 - 5,
            torch.rand(B, 3, H, W, generator=g) * 3 - 1, torch.cat([ang.sin(), ang.cos()], 1),
            torch.rand(B, 2, H, W, generator=g) * 20 - 10)])
    return logits, heads


def circle_nms_host(xy, thresh, post_max_size):
    """mmdet3d's circle_nms on host arrays already in descending score order: the kept indices"""
    n = xy.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        if len(keep) >= post_max_size:
            break
        d = xy[i + 1:] - xy[i]
        dead[i + 1:] |= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= thresh
    return keep


def composition(logits, heads, K):
    """per task and frame (boxes [n, 9], scores [n], labels [n]) as mmdet3d produces them"""
    out = []
    rng = torch.tensor(OPTS["post_center_range"], device=logits[0].device)
    for t, (lg, hd) in enumerate(zip(logits, heads)):
        B = lg.shape[0]
        heat = lg.sigmoid()
        scores, inds = heat.view(B, -1).topk(K)
        clses, inds = inds // (H * W), inds % (H * W)
        ys, xs = (inds // W).float(), (inds % W).float()
        reg, hei, dim, rot, vel = (f.view(B, f.shape[1], -1).permute(0, 2, 1).gather(1, inds[..., None].expand(-1, -1, f.shape[1]))
                                   for f in hd)
        xs = (xs + reg[..., 0]) * CFG["out_size_factor"] * CFG["voxel_size"][0] + CFG["pc_range"][0]
        ys = (ys + reg[..., 1]) * CFG["out_size_factor"] * CFG["voxel_size"][1] + CFG["pc_range"][1]
        boxes = torch.cat([xs[..., None], ys[..., None], hei, dim.exp(), torch.atan2(rot[..., 0:1], rot[..., 1:2]), vel], -1)
        mask = (scores > OPTS["score_threshold"]) & (boxes[..., :3] >= rng[:3]).all(-1) & (boxes[..., :3] <= rng[3:]).all(-1)
        ids = torch.tensor(TASKS[t], device=lg.device)
        frames = []
        for b in range(B):
            bx, sc, lb = boxes[b][mask[b]], scores[b][mask[b]], ids[clses[b][mask[b]]]      # boolean index: a host synchronisation
            keep = circle_nms_host(bx[:, :2].cpu().numpy(), MIN_RADIUS[t], OPTS["post_max_size"])
            keep = torch.tensor(keep, dtype=torch.long, device=lg.device)
            frames.append((bx[keep], sc[keep], lb[keep]))
        out.append(frames)
    return out


def main():
    ap = parser(warmup=100, iters=20, calls=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--k", type=int, default=500)
    args = ap.parse_args()
    dev = gpu()
    from accvlab.draw_heatmap import center_point_decode, heatmap_peaks

    logits, heads = make_inputs(args.batch, dev)
    K = args.k

    def fused():
        return center_point_decode([heatmap_peaks(lg, K, kernel=1) for lg in logits], heads, TASKS, **CFG, scores_are_logits=True, **OPTS)

    def decode_only(peaks=[heatmap_peaks(lg, K, kernel=1) for lg in logits]):   # noqa: B006 - the peaks are computed once
        return center_point_decode(peaks, heads, TASKS, **CFG, scores_are_logits=True, **OPTS)

    comp = lambda: composition(logits, heads, K)   # noqa: E731
    got, ref = fused(), comp()
    torch.cuda.synchronize()
    count_mismatch, label_mismatch, box_err, score_err, dets = 0, 0, 0.0, 0.0, 0
    for d, frames in zip(got, ref):
        for b, (bx, sc, lb) in enumerate(frames):
            n = int(d.boxes.sample_sizes[b])
            dets += n
            if n != bx.shape[0]:
                count_mismatch += 1
                continue
            label_mismatch += int((d.labels.tensor[b, :n] != lb).sum())
            if n:
                box_err = max(box_err, float((d.boxes.tensor[b, :n] - bx).abs().max()))
                score_err = max(score_err, float((d.scores.tensor[b, :n] - sc).abs().max()))
    ms = window_times({"fused": fused, "decode_only": decode_only, "torch": comp}, args.warmup, args.iters, args.calls)
    ms = {k: summary(v, args.calls, with_max=True) for k, v in ms.items()}
    n_fused, n_decode, n_torch = launches(fused), launches(decode_only), launches(comp)
    result = dict(metric="center_point_decode_ms", unit="ms", value=ms["fused"]["median_ms"], warmup=args.warmup, iters=args.iters,
                  calls_per_block=args.calls, shape=dict(B=args.batch, T=len(TASKS), H=H, W=W, K=K, post_max_size=OPTS["post_max_size"]),
                  detections=dets, fused=ms["fused"], decode_only=ms["decode_only"], torch=ms["torch"],
                  speedup_median=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                  launches_fused=shown(n_fused), launches_decode_only=shown(n_decode), launches_torch=shown(n_torch),
                  host_round_trips_torch=len(TASKS) * args.batch,
                  frames_with_other_count_vs_torch=count_mismatch, label_mismatches_vs_torch=label_mismatch,
                  boxes_max_abs_diff_vs_torch=box_err, scores_max_abs_diff_vs_torch=score_err)
    lines = [f"center_point_decode  B={args.batch} T={len(TASKS)} {H}x{W} K={K} post_max_size={OPTS['post_max_size']}: {dets} detections",
             f"  {args.warmup} warm-up calls, {args.iters} blocks of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s fused, "
             f"{ms['torch']['timed_s']} s torch",
             f"  peaks + decode  median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {shown(n_fused)}",
             f"  decode alone    median {ms['decode_only']['median_ms']:.4f} ms  min {ms['decode_only']['min_ms']:.4f} ms  launches {shown(n_decode)}",
             f"  torch + host    median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {shown(n_torch)}  "
             f"host round trips {len(TASKS) * args.batch}",
             f"  against the torch composition: {count_mismatch} frames with another count, {label_mismatch} labels differ, boxes max abs diff "
             f"{box_err:.3e}, scores {score_err:.3e}",
             json.dumps(result)]
    emit(lines, args.out)


if __name__ == "__main__":
    main()
