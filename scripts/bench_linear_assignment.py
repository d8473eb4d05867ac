#!/usr/bin/env python3
"""Batched linear sum assignment on the GPU vs the scipy round trip of examples/matched_loss.py:match_batched.

Cases (examples/matched_loss.make_inputs, 10 classes, seed 0): the F3 inputs 8 x 900 queries x <= 100 targets; 64 x 300
x <= 50; 8 x 900 x 300 (every frame full); 8 x 100 x 300 (more targets than queries).  Per case, on the matcher's own
cost matrices (built once, outside the timed region):
  - roundtrip: what match_batched does after the cost build — to_device(cpu), split, scipy per frame, combine_data x 2,
    copy back — wall time with a synchronisation at the end of every iteration;
  - op_check / op_nocheck: batched_linear_sum_assignment with check=True (one status read) / check=False, wall time
    with the same synchronisation;
  - op_kernel_t64 / t256 / t1024: device-event time of check=False with one wave, 256 and 1024 lanes per frame;
  - steps: Dijkstra steps of the whole batch (a numpy count with the same algorithm) and the per-step cost
    op_kernel / max steps of one frame (frames run in parallel, the longest frame bounds the launch).
Plus F3 forward + backward (run_batched vs run_batched_on_device, fused and composed loss).  Median and minimum of
--iters iterations after --warmup.  Prints ONE JSON line.

    python3 scripts/bench_linear_assignment.py [--warmup 5] [--iters 30] [--out FILE]
"""
import json

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from measure import call_times, emit, gpu, parser, summary, wall_times

CASES = [
    # name, batch, queries, max_gt, min_gt
    ("f3_8x900xle100", 8, 900, 100, 0),
    ("b64_300xle50", 64, 300, 50, 0),
    ("b8_900x300", 8, 900, 300, 300),
    ("b8_100x300_g_gt_q", 8, 100, 300, 300),
]


def dijkstra_steps(cost):
    """Dijkstra steps of the shortest-augmenting-path solve of one frame (numpy; the algorithm of the kernel)."""
    c = np.asarray(cost, dtype=np.float64)
    if c.shape[0] > c.shape[1]:
        c = c.T
    n, m = c.shape
    u, v = np.zeros(n), np.zeros(m)
    row4col, col4row = -np.ones(m, np.int64), -np.ones(n, np.int64)
    steps = 0
    for cur in range(n):
        spc, path = np.full(m, np.inf), -np.ones(m, np.int64)
        sc, sr = np.zeros(m, bool), np.zeros(n, bool)
        sr[cur] = True
        i, min_val, sink = cur, 0.0, -1
        while sink < 0:
            steps += 1
            r = min_val + c[i] - u[i] - v
            upd = (~sc) & (r < spc)
            spc[upd], path[upd] = r[upd], i
            key = np.where(sc, np.inf, spc)
            low = key.min()
            cand = np.flatnonzero(key == low)
            free = cand[row4col[cand] < 0]
            j = int(free[0] if free.size else cand[0])
            min_val = low
            sc[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
                sr[i] = True
        u[cur] += min_val
        rows = np.flatnonzero(sr)
        rows = rows[rows != cur]
        u[rows] += min_val - spc[col4row[rows]]
        v[sc] -= min_val - spc[sc]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return steps


def main():
    args = parser(warmup=5, iters=30).parse_args()
    dev = gpu()

    import matched_loss as ml

    import accvlab.batching_helpers as bh

    stats = lambda ms: {k: v for k, v in summary(ms, digits=4).items() if k != "timed_s"}    # noqa: E731 - median and minimum
    wall = lambda fn: stats(wall_times(fn, args.iters, args.warmup))                          # noqa: E731
    device = lambda fn: stats(call_times({"fn": fn}, args.warmup, args.iters)["fn"])          # noqa: E731
    result = {"metric": "linear_assignment_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters, "cases": {}}

    def roundtrip(cost):
        per_frame = cost.to_device(torch.device("cpu")).split()
        gt_idx, pred_idx = [], []
        for m in per_frame:
            rows, cols = linear_sum_assignment(m.numpy())
            pred_idx.append(torch.as_tensor(rows, dtype=torch.int64))
            gt_idx.append(torch.as_tensor(cols, dtype=torch.int64))
        gt_rb = bh.combine_data(gt_idx)
        pred_rb = bh.combine_data(pred_idx, other_with_same_sample_sizes=gt_rb)
        return gt_rb.to_device(dev), pred_rb.to_device(dev)

    for name, B, Q, G, G0 in CASES:
        inp = ml.make_inputs(B, Q, 10, G, dev, seed=0, min_gt=G0)
        gt_boxes = bh.combine_data(inp[0])
        gt_labels = bh.combine_data(inp[1], other_with_same_sample_sizes=gt_boxes)
        pred_boxes, pred_scores = inp[3], inp[4]
        num_classes = pred_scores.shape[-1]
        cost = (1.0 - ml._iou(pred_boxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
               (1.0 - torch.einsum("bqc,bgc->bqg", pred_scores, ml._one_hot(gt_labels.tensor, num_classes)))
        cost = gt_labels.create_with_sample_sizes_like_self(cost.detach(), non_uniform_dim=2)

        want_gt, want_pred = roundtrip(cost)
        pred_rb, gt_rb = bh.batched_linear_sum_assignment(cost)
        same = bool(torch.equal(want_gt.sample_sizes, gt_rb.sample_sizes)) and all(
            torch.equal(w.tensor[w.mask], g.tensor[:, :w.tensor.shape[1]][w.mask])
            for w, g in ((want_gt, gt_rb), (want_pred, pred_rb)))
        frames = cost.to_device(torch.device("cpu")).split()
        steps = [dijkstra_steps(f.numpy()) for f in frames]

        entry = {"B": B, "queries": Q, "max_gt": G, "min_gt": G0, "gt_sizes": cost.sample_sizes.tolist(),
                 "indices_equal_scipy": same, "steps_per_frame": steps}
        entry["roundtrip"] = wall(lambda: roundtrip(cost))
        entry["op_check"] = wall(lambda: bh.batched_linear_sum_assignment(cost))
        entry["op_nocheck"] = wall(lambda: bh.batched_linear_sum_assignment(cost, check=False))
        for t in (64, 256, 1024):
            entry[f"op_kernel_t{t}"] = device(lambda: bh.batched_linear_sum_assignment(cost, check=False, _threads=t))
        best = min(entry[f"op_kernel_t{t}"]["median_ms"] for t in (64, 256, 1024))
        entry["us_per_step_longest_frame_t256"] = round(entry["op_kernel_t256"]["median_ms"] * 1e3 / max(max(steps), 1), 3)
        entry["speedup_check_vs_roundtrip"] = round(entry["roundtrip"]["median_ms"] / entry["op_check"]["median_ms"], 2)
        entry["best_kernel_median_ms"] = best

        if name.startswith("f3"):
            for fused in (False, True):
                def step(run, fused=fused):
                    p = [t.clone().requires_grad_(True) for t in inp[3:]]
                    run(*inp[:3], *p, fused=fused).sum().backward()
                tag = "fused" if fused else "composed"
                entry[f"f3_fwd_bwd_{tag}_scipy"] = wall(lambda: step(ml.run_batched))
                entry[f"f3_fwd_bwd_{tag}_on_device"] = wall(lambda: step(ml.run_batched_on_device))
        result["cases"][name] = entry
    f3 = result["cases"][CASES[0][0]]
    result["value"] = f3["op_check"]["median_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
