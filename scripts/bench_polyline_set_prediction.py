#!/usr/bin/env python3
"""Polyline set prediction (accvlab.lane_helpers.polyline: batched_polyline_matching_cost, matched_polyline_loss) vs the
torch composition of tests/polyline_match_cases.py (composed_cost: the [B, Q, G, V, P, D] broadcast; composed_loss: the
[M, V, P, D] variants of the matched lines).

Shape: MapTR-like B = 8, Q = 350, G in [5, 40], P = 20, D = 2, float32; variants: open reversible lines (V = 2) and all
closed lines (V = 40).  For each: the cost, the loss forward and forward + backward of both, all alternating inside every
timed iteration of one process; device events; medians next to minima.  Prints ONE JSON line.

    python3 scripts/bench_polyline_set_prediction.py [--warmup 20] [--iters 100] [--out FILE]
"""
import json

import torch

from measure import call_times, emit, gpu, parser, summary   # puts tests/ on the path

import polyline_match_cases as pm  # noqa: E402
from accvlab.lane_helpers import polyline  # noqa: E402

B, Q, P, D, G_MIN, G_MAX = 8, 350, 20, 2, 5, 40


def run_case(closed, dev, warmup, iters):
    g = torch.Generator().manual_seed(7)
    sizes = [int(v) for v in torch.randint(G_MIN, G_MAX + 1, (B,), generator=g)]
    sizes[0] = G_MAX
    lines, gt, pind, gind, closed_rb = pm.make_case(B, Q, P, D, sizes, sizes, torch.float32, seed=3,
                                                    closed="closed" if closed else "open", device=dev)
    x = lines.detach().requires_grad_(True)
    go = torch.ones(B, device=dev)
    fused_loss = lambda: polyline.matched_polyline_loss(x, gt, pind, gind, gt_closed=closed_rb)     # noqa: E731
    torch_loss = lambda: pm.composed_loss(x, gt, pind, gind, closed)                                  # noqa: E731

    def no_grad(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), x, (go, go))

    with torch.no_grad():
        cf = polyline.batched_polyline_matching_cost(lines, gt, gt_closed=closed_rb).tensor
        ct = pm.composed_cost(lines, gt, closed)
        lf, lt = [float(t.sum()) for t in fused_loss()], [float(t.sum()) for t in torch_loss()]
    ms = {}
    for k, v in call_times({"fused_cost": no_grad(lambda: polyline.batched_polyline_matching_cost(lines, gt, gt_closed=closed_rb)),
                            "torch_cost": no_grad(lambda: pm.composed_cost(lines, gt, closed)),
                            "fused_fwd": no_grad(fused_loss), "torch_fwd": no_grad(torch_loss),
                            "fused_fwd_bwd": fwd_bwd(fused_loss), "torch_fwd_bwd": fwd_bwd(torch_loss)}, warmup, iters).items():
        s = summary(v, digits=4)
        ms[k + "_ms"], ms[k + "_min_ms"] = s["median_ms"], s["min_ms"]
    variants = 2 * P if closed else 2
    return dict(ms, shape=[B, Q, P, D], lines=sizes, orders=variants, pairs=sum(sizes),
                variants_bytes=B * Q * G_MAX * variants * P * D * 4,
                cost_max_abs_diff=float((cf - ct).abs().max()), loss_fused=lf, loss_torch=lt,
                speedup_cost=round(ms["torch_cost_ms"] / ms["fused_cost_ms"], 2),
                speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
                speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2))


def main():
    args = parser(warmup=20, iters=100).parse_args()
    dev = gpu()
    if args.iters < 100:
        raise SystemExit("medians of at least 100 iterations are reported")
    result = {"metric": "polyline_matching_cost_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters}
    result["open_reversible"] = run_case(False, dev, args.warmup, args.iters)
    result["closed"] = run_case(True, dev, args.warmup, args.iters)
    result["value"] = result["closed"]["fused_cost_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
