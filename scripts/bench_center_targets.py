#!/usr/bin/env python3
"""center_point_targets (one launch) vs a vectorised torch composition of its definition, written here.

Size: B = 64 frames, N in [1, 128] objects per frame (ragged, seed 42), D = 9, the six nuScenes tasks over ten classes, a
180 x 180 map (pc_range +-54 m, voxel 0.075 m, stride 8), max_objs 500.  The composition is what a user gets without a
Python loop and without a host synchronisation: masks, cumsum ranks and one scatter per output, all tasks at once.  It is
NOT the per-object loop of mmdet3d, which would flatter the operator.

The composition's float32 constants and class tables are device tensors built once, outside the timed function.  Both
alternate inside one process: a timed window is `--calls` back-to-back calls of one side between two device events, its
time divided by the number of calls; `--iters` windows per side; median and minimum per call over the windows.  Launch
counts come from torch's profiler in a separate pass (kernel events per call; copies and memsets are not counted); "not
measured" if the profiler is unavailable.  Prints a few lines of log and ONE JSON line.

    python3 scripts/bench_center_targets.py [--warmup 20] [--iters 200] [--calls 50] [--out FILE]
"""
import json
import math

import torch

from measure import emit, gpu, launches, parser, shown, summary, window_times

TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))
CFG = dict(pc_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], out_size_factor=8, grid_size=(180, 180),
           gaussian_overlap=0.1, min_radius=2, max_objs=500, norm_bbox=True)


def make_inputs(B, n_max, dev, seed=42):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, n_max + 1, (B,), generator=g)
    N = int(sizes.max())
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    xy = (u(B, N, 2) * 1.2 - 0.6) * 108.0                       # a sixth of the centres fall outside the range
    boxes = torch.cat([xy, u(B, N, 1) * 8 - 5, 0.3 + u(B, N, 3) * 11.7, (u(B, N, 1) * 2 - 1) * math.pi, u(B, N, 2) * 20 - 10], -1)
    labels = torch.randint(-1, 10, (B, N), generator=g)
    return boxes.to(torch.float32).contiguous().to(dev), labels.to(dev), sizes.to(dev)


def constants(cfg, dev):
    """what the composition needs on the device and does not change between calls: built once, outside the timed function"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)   # noqa: E731
    task_of = torch.full((64,), 255, dtype=torch.int64)
    pos_of = torch.zeros((64,), dtype=torch.int64)
    for t, ids in enumerate(TASKS):
        for p, c in enumerate(ids):
            task_of[c], pos_of[c] = t, p
    return dict(task_of=task_of.to(dev), pos_of=pos_of.to(dev), tasks=torch.arange(len(TASKS), device=dev)[:, None, None],
                pc0=f32(cfg["pc_range"][0]), pc1=f32(cfg["pc_range"][1]), vs0=f32(cfg["voxel_size"][0]), vs1=f32(cfg["voxel_size"][1]),
                f=f32(cfg["out_size_factor"]), m=f32(cfg["gaussian_overlap"]))


def composition(boxes, labels, sizes, k, T, cfg):
    """the definition over whole tensors; returns the operator's seven outputs as [T, B, M, ...] tensors.  No host
    synchronisation: every scalar that meets a tensor is a Python number or one of the device constants `k`."""
    B, N, D = boxes.shape
    W, H = cfg["grid_size"]
    M = min(cfg["max_objs"], N)
    task_of, pos_of = k["task_of"], k["pos_of"]
    slot = torch.arange(N, device=boxes.device)
    ok = (slot[None] < sizes[:, None]) & (labels >= 0) & (labels < 64)
    lab = labels.clamp(0, 63)
    task = torch.where(ok, task_of[lab], 255)
    cand = task[None] == k["tasks"]                                                      # [T, B, N]
    passed = cand & (cand.cumsum(-1) <= cfg["max_objs"])
    x, y, dx, dy = boxes[..., 0], boxes[..., 1], boxes[..., 3], boxes[..., 4]
    vs0, vs1, f, m = k["vs0"], k["vs1"], k["f"], k["m"]
    w, l = dx / vs0 / f, dy / vs1 / f
    cx, cy = (x - k["pc0"]) / vs0 / f, (y - k["pc1"]) / vs1 / f
    valid = (w > 0) & (l > 0) & (cx > -1) & (cx < W) & (cy > -1) & (cy < H)
    keep = passed & valid[None]
    out_slot = torch.where(keep, keep.cumsum(-1) - 1, M)                                 # dropped objects go to a spare slot
    kept = keep.sum(-1)
    ix, iy = cx.to(torch.int32), cy.to(torch.int32)
    s = l + w
    r1 = (s + torch.sqrt(s * s - 4 * (w * l * (1 - m) / (1 + m)))) / 2
    r2 = (2 * s + torch.sqrt(4 * s * s - 16 * ((1 - m) * w * l))) / 2
    b3 = -2 * m * s
    r3 = (b3 + torch.sqrt(b3 * b3 - 16 * m * ((m - 1) * w * l))) / 2
    radius = torch.minimum(torch.minimum(r1, r2), r3).nan_to_num(0.0).to(torch.int32).clamp(min=cfg["min_radius"])
    dims = boxes[..., 3:6].log() if cfg["norm_bbox"] else boxes[..., 3:6]
    rows = torch.cat([(cx - ix)[..., None], (cy - iy)[..., None], boxes[..., 2:3], dims, boxes[..., 6:7].sin(), boxes[..., 6:7].cos(),
                      boxes[..., 7:]], -1)

    def compact(values, fill, dtype):
        tail = values.shape[2:]
        out = torch.full((T, B, M + 1) + tail, fill, dtype=dtype, device=boxes.device)
        idx = out_slot.reshape(T, B, N, *([1] * len(tail))).expand(T, B, N, *tail)
        out.scatter_(2, idx, values[None].expand(T, B, N, *tail).to(dtype))
        out[:, :, M] = fill                                      # what the dropped objects wrote
        return out[:, :, :M]

    centers = compact(torch.stack([ix, iy], -1), 0, torch.int32)
    return (centers, compact(radius, 0, torch.int32), compact(pos_of[lab], 0, torch.int32), compact(rows, 0.0, torch.float32),
            compact(iy.long() * W + ix.long(), 0, torch.int64), compact(slot[None].expand(B, N), -1, torch.int32), kept)


def main():
    ap = parser(warmup=20, iters=200, calls=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-max", type=int, default=128)
    args = ap.parse_args()
    dev = gpu()
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import center_point_targets

    boxes, labels, sizes = make_inputs(args.batch, args.n_max, dev)
    rb, rl = RaggedBatch(boxes, sample_sizes=sizes), RaggedBatch(labels, sample_sizes=sizes)
    k = constants(CFG, dev)

    fused = lambda: center_point_targets(rb, rl, TASKS, **CFG)                                  # noqa: E731
    comp = lambda: composition(boxes, labels, sizes, k, len(TASKS), CFG)                        # noqa: E731
    got, ref = fused(), comp()
    torch.cuda.synchronize()
    names = ("centers", "radii", "labels", "targets", "indices", "source")
    mismatch = {n: int((torch.stack([getattr(r, n).tensor for r in got]) != ref[i]).sum()) for i, n in enumerate(names) if n != "targets"}
    mismatch["sizes"] = int((torch.stack([r.centers.sample_sizes for r in got]) != ref[6]).sum())
    terr = float((torch.stack([r.targets.tensor for r in got]) - ref[3]).abs().max())
    ms = {k: summary(v, args.calls) for k, v in window_times({"fused": fused, "torch": comp}, args.warmup, args.iters, args.calls).items()}
    result = dict(metric="center_point_targets_ms", unit="ms", value=ms["fused"]["median_ms"], warmup=args.warmup, iters=args.iters, calls_per_window=args.calls,
                  shape=dict(B=args.batch, N=int(boxes.shape[1]), D=9, T=len(TASKS), grid=list(CFG["grid_size"])),
                  objects=int(sizes.sum()), kept=int(ref[6].sum()), fused=ms["fused"], torch=ms["torch"],
                  speedup_median=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                  launches_fused=shown(launches(fused)), launches_torch=shown(launches(comp)),
                  integer_mismatches_vs_torch=mismatch, targets_max_abs_diff_vs_torch=terr)
    lines = [f"center_point_targets  B={args.batch} N<={boxes.shape[1]} D=9 T={len(TASKS)} grid 180x180: {int(sizes.sum())} objects, "
             f"{int(ref[6].sum())} kept",
             f"  {args.iters} windows of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s fused, {ms['torch']['timed_s']} s torch",
             f"  fused   median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {result['launches_fused']}",
             f"  torch   median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {result['launches_torch']}",
             f"  integer outputs that differ from the torch composition: {mismatch}; targets max abs diff {terr:.3e}",
             json.dumps(result)]
    emit(lines, args.out)


if __name__ == "__main__":
    main()
