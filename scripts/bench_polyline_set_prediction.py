#!/usr/bin/env python3
"""Polyline set prediction (accvlab.lane_helpers.polyline: batched_polyline_matching_cost, matched_polyline_loss) vs the
torch composition of tests/polyline_match_cases.py (composed_cost: the [B, Q, G, V, P, D] broadcast; composed_loss: the
[M, V, P, D] variants of the matched lines).

Shape: MapTR-like B = 8, Q = 350, G in [5, 40], P = 20, D = 2, float32; variants: open reversible lines (V = 2) and all
closed lines (V = 40).  For each: the cost, the loss forward and forward + backward of both, all alternating inside every
timed iteration of one process; device events; medians next to minima.  Prints ONE JSON line.

    python3 scripts/bench_polyline_set_prediction.py [--warmup 20] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import polyline_match_cases as pm  # noqa: E402
from accvlab.lane_helpers import polyline  # noqa: E402

B, Q, P, D, G_MIN, G_MAX = 8, 350, 20, 2, 5, 40


def timed(fns, warmup, iters):
    """(median, minimum) in ms of the callables, run one after the other inside every iteration"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    events = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, v in events.items():
        ms = [a.elapsed_time(b) for a, b in v]
        out[k + "_ms"], out[k + "_min_ms"] = round(statistics.median(ms), 4), round(min(ms), 4)
    return out


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
    ms = timed({"fused_cost": no_grad(lambda: polyline.batched_polyline_matching_cost(lines, gt, gt_closed=closed_rb)),
                "torch_cost": no_grad(lambda: pm.composed_cost(lines, gt, closed)),
                "fused_fwd": no_grad(fused_loss), "torch_fwd": no_grad(torch_loss),
                "fused_fwd_bwd": fwd_bwd(fused_loss), "torch_fwd_bwd": fwd_bwd(torch_loss)}, warmup, iters)
    variants = 2 * P if closed else 2
    return dict(ms, shape=[B, Q, P, D], lines=sizes, orders=variants, pairs=sum(sizes),
                variants_bytes=B * Q * G_MAX * variants * P * D * 4,
                cost_max_abs_diff=float((cf - ct).abs().max()), loss_fused=lf, loss_torch=lt,
                speedup_cost=round(ms["torch_cost_ms"] / ms["fused_cost_ms"], 2),
                speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
                speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polyline_set_prediction.py measures on a GPU; none is visible")
    if args.iters < 100:
        raise SystemExit("medians of at least 100 iterations are reported")
    dev = torch.device("cuda", 0)
    result = {"metric": "polyline_matching_cost_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters}
    result["open_reversible"] = run_case(False, dev, args.warmup, args.iters)
    result["closed"] = run_case(True, dev, args.warmup, args.iters)
    result["value"] = result["closed"]["fused_cost_ms"]
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
