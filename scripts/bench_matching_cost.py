#!/usr/bin/env python3
"""Fused matching-cost matrices (batched_matching_cost) vs the torch compositions matchers write today.

Cases (examples/matched_loss.make_inputs-style inputs, seed 0, ragged ground truth):
  - f3: 8 x 900 queries x <= 100 targets, 10 classes, 1 - p + (1 - IoU) — examples/matched_loss.py's cost;
  - detr: 16 x 100 x <= 50, 92 classes, -p + 5 L1 (cxcywh) - 2 GIoU — DETR's HungarianMatcher;
  - streampetr: 8 x 900 x <= 150, 10 classes, 2 focal + 0.25 L1 on [..., :8] of a [B, Q, 10] box-code tensor;
  - large: 64 x 900 x <= 300, 10 classes, the f3 cost.
Per case: `torch` the composition (wall time, synchronised per iteration), `op` batched_matching_cost (the same), `op_kernel`
the op between two device events; the maximum difference between the two results.  Plus the F3 forward + backward with
the composed cost + on-device solver + fused loss (examples/matched_loss.run_batched_on_device) against the fused cost
(run_batched_fused_cost).  Median and minimum of --iters iterations after --warmup.  Prints ONE JSON line.
--op-only runs just the op of every case (for a rocprofv3 --kernel-trace --stats run).

    python3 scripts/bench_matching_cost.py [--warmup 10] [--iters 50] [--out FILE] [--op-only]
"""
import json

import torch

from measure import call_times, emit, gpu, parser, summary, wall_times

CASES = [
    # name, batch, queries, classes, max_gt
    ("f3", 8, 900, 10, 100),
    ("detr", 16, 100, 92, 50),
    ("streampetr", 8, 900, 10, 150),
    ("large", 64, 900, 10, 300),
]


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou(p, g, eps=1e-6):
    area_p = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
    area_g = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    wh = (torch.minimum(p[..., 2:], g[..., 2:]) - torch.maximum(p[..., :2], g[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = (area_p + area_g - inter).clamp(min=eps)
    ewh = (torch.maximum(p[..., 2:], g[..., 2:]) - torch.minimum(p[..., :2], g[..., :2])).clamp(min=0)
    enclose = (ewh[..., 0] * ewh[..., 1]).clamp(min=eps)
    return inter / union - (enclose - union) / enclose


def make(name, B, Q, C, G, dev):
    """inputs, torch composition, op keyword arguments"""
    import matched_loss as ml

    import accvlab.batching_helpers as bh

    g = torch.Generator().manual_seed(0)
    gb_l, gl_l, _, pboxes, pscores, _ = ml.make_inputs(B, Q, C, G, dev, seed=0)
    gt_boxes = bh.combine_data(gb_l)
    gt_labels = bh.combine_data(gl_l, other_with_same_sample_sizes=gt_boxes)
    if name in ("f3", "large"):
        def torch_cost():
            return (1.0 - ml._iou(pboxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
                   (1.0 - torch.einsum("bqc,bgc->bqg", pscores, ml._one_hot(gt_labels.tensor, C)))
        return (pscores, gt_labels, pboxes, gt_boxes), torch_cost, dict(iou_weight=1.0, iou_eps=ml.EPS)
    if name == "detr":
        to_cxcywh = lambda b: torch.cat([(b[..., :2] + b[..., 2:]) * 0.5, b[..., 2:] - b[..., :2]], -1)
        pb, gb = to_cxcywh(pboxes) / 120.0, to_cxcywh(gt_boxes.tensor) / 120.0
        gt_b = gt_boxes.create_with_sample_sizes_like_self(gb)

        def torch_cost():
            lab = gt_labels.tensor.unsqueeze(1).expand(B, Q, gt_labels.tensor.shape[1])
            return (-pscores.gather(2, lab) + 5.0 * torch.cdist(pb, gb, p=1)
                    - 2.0 * giou(xyxy(pb).unsqueeze(2), xyxy(gb).unsqueeze(1)))
        return (pscores, gt_labels, pb, gt_b), torch_cost, dict(class_cost="neg_prob", l1_weight=5.0, giou_weight=2.0,
                                                                 box_format="cxcywh")
    # streampetr: logits, a 10-wide box code of which the matcher reads the first 8
    logits = torch.randn(B, Q, C, generator=g).mul(3.0).to(dev)
    code = torch.randn(B, Q, 10, generator=g).to(dev)
    gcode = bh.combine_data([torch.randn(int(n), 8, generator=g).to(dev) for n in gt_labels.sample_sizes.tolist()])
    gt_code = gt_labels.create_with_sample_sizes_like_self(gcode.tensor)
    bcode = code[..., :8]

    def torch_cost():
        s = logits.sigmoid()
        neg = -(1 - s + 1e-12).log() * (1 - 0.25) * s.pow(2.0)
        pos = -(s + 1e-12).log() * 0.25 * (1 - s).pow(2.0)
        lab = gt_labels.tensor.unsqueeze(1).expand(B, Q, gt_labels.tensor.shape[1])
        return 2.0 * (pos.gather(2, lab) - neg.gather(2, lab)) + 0.25 * torch.cdist(bcode, gcode.tensor, p=1)
    return (logits, gt_labels, bcode, gt_code), torch_cost, dict(class_cost="focal", class_weight=2.0, l1_weight=0.25)


def main():
    ap = parser(warmup=10, iters=50)
    ap.add_argument("--op-only", action="store_true")
    args = ap.parse_args()
    dev = gpu()

    import matched_loss as ml

    import accvlab.batching_helpers as bh

    stats = lambda ms: {k: v for k, v in summary(ms).items() if k != "timed_s"}               # noqa: E731 - median and minimum
    wall = lambda fn: stats(wall_times(fn, args.iters, args.warmup))                          # noqa: E731
    device = lambda fn: stats(call_times({"fn": fn}, args.warmup, args.iters)["fn"])          # noqa: E731
    result = {"metric": "matching_cost_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters, "cases": {}}
    for name, B, Q, C, G in CASES:
        inp, torch_cost, kw = make(name, B, Q, C, G, dev)
        op = lambda: bh.batched_matching_cost(*inp, **kw)
        if args.op_only:
            wall(op)
            continue
        got = op()
        want = torch_cost()
        mask = got.mask.unsqueeze(1).expand_as(want)
        entry = {"B": B, "queries": Q, "classes": C, "max_gt": G, "gt_sizes": got.sample_sizes.tolist(),
                 "max_abs_diff_vs_torch": float((got.tensor - want)[mask].abs().max()) if mask.any() else 0.0}
        entry["torch"] = wall(torch_cost)
        entry["op"] = wall(op)
        entry["torch_kernel"] = device(torch_cost)
        entry["op_kernel"] = device(op)
        entry["speedup_wall"] = round(entry["torch"]["median_ms"] / entry["op"]["median_ms"], 2)
        entry["speedup_device"] = round(entry["torch_kernel"]["median_ms"] / entry["op_kernel"]["median_ms"], 2)
        result["cases"][name] = entry
        if name == "f3":
            inp_f3 = ml.make_inputs(B, Q, C, G, dev, seed=0)
            for tag, run in (("composed_cost", ml.run_batched_on_device), ("fused_cost", ml.run_batched_fused_cost)):
                def step(run=run):
                    p = [t.clone().requires_grad_(True) for t in inp_f3[3:]]
                    run(*inp_f3[:3], *p, fused=True).sum().backward()
                entry[f"f3_fwd_bwd_{tag}_on_device_fused_loss"] = wall(step)
    if args.op_only:
        print(json.dumps({"op_only": True}))
        return
    result["value"] = result["cases"]["f3"]["op"]["median_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
