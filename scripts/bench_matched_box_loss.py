#!/usr/bin/env python3
"""Fused matched box loss (accvlab.batching_helpers.matched_box_loss) vs the composition it replaces
(examples/matched_loss.py::box_loss_composed: two ragged gathers, the cxcywh conversion, L1, GIoU as mmdet's aligned
bbox_overlaps, masked per-frame sums, division by the number of pairs).

Cases, float32 and bfloat16 each: (a) 8 x 900 x 4 with up to 100 objects, (b) 16 x 300 x 4, (c) 48 x 900 x 10, L1 only with
code_weights (six decoder layers of batch 8 stacked on the batch axis, mmdet3d box codes), (d) 32 x 8400 x 4 with up to 60
objects.  For each: forward and forward + backward of both; all four alternate inside every timed iteration of one
process; device events; medians.  `--trace N` runs N plain forward + backward iterations of both instead (for a kernel
trace); `--launch-count` counts the kernel launches of one forward and one forward + backward of both with torch's
profiler.  Prints ONE JSON line.

    python3 scripts/bench_matched_box_loss.py [--warmup 20] [--iters 100] [--out FILE] [--cases a_f32,d_bf16]
"""
import json
import statistics

import torch

from measure import call_times, emit, gpu, parser   # puts tests/ and examples/ on the path

import matched_box_loss_cases as mb  # noqa: E402
import matched_loss as ml  # noqa: E402

SHAPES = {"a": (8, 900, 4, 100), "b": (16, 300, 4, 40), "c": (48, 900, 10, 60), "d": (32, 8400, 4, 60)}
CASES = {f"{k}_{n}": dict(shape=v, dtype=d) for k, v in SHAPES.items() for n, d in (("f32", torch.float32), ("bf16", torch.bfloat16))}
CODE_WEIGHTS_10 = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]


def make(cfg, dev):
    B, Q, D, objects = cfg["shape"]
    l1_only = D != 4
    fmt = "xyxy" if l1_only else "cxcywh"
    boxes, gt, pind, gind, _ = mb.shape_case(B, Q, D, objects, cfg["dtype"], seed=B, device=dev, box_format=fmt)
    x = boxes.detach().requires_grad_(True)
    kw = dict(box_format=fmt, iou_kind=None if l1_only else "giou", code_weights=CODE_WEIGHTS_10 if l1_only else None)
    cw_dev = torch.tensor(CODE_WEIGHTS_10, dtype=cfg["dtype"], device=dev) if l1_only else None   # the composition's operand
    fused = lambda: ml.box_loss_fused(x, gt, pind, gind, **kw)                                           # noqa: E731
    comp = lambda: ml.box_loss_composed(x, gt, pind, gind, **dict(kw, code_weights=cw_dev))             # noqa: E731
    return x, fused, comp, int(pind.sample_sizes.sum()), l1_only


def run_case(cfg, dev, warmup, iters):
    x, fused, comp, pairs, l1_only = make(cfg, dev)
    go = torch.ones(x.shape[0], device=dev)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            l1, iou = f()
            return torch.autograd.grad((l1,) if l1_only else (l1, iou), x, (go,) if l1_only else (go, go))
        return run

    with torch.no_grad():
        lf, lc = [float(t.sum()) for t in fused()], [float(t.sum()) for t in comp()]
    ms = call_times({"fused_fwd_ms": fwd(fused), "torch_fwd_ms": fwd(comp), "fused_fwd_bwd_ms": fwd_bwd(fused),
                     "torch_fwd_bwd_ms": fwd_bwd(comp)}, warmup, iters)
    ms = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    return dict(ms, shape=list(x.shape), dtype=str(x.dtype).split(".")[-1], pairs=pairs, terms="l1" if l1_only else "l1+giou",
                speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
                speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2), loss_fused=lf, loss_torch=lc)


def trace_case(cfg, dev, iters, count):
    """plain iterations for a kernel trace (iters), or the launch counts of both from torch's profiler (count)"""
    x, fused, comp, _, l1_only = make(cfg, dev)
    go = torch.ones(x.shape[0], device=dev)

    def step(f):
        l1, iou = f()
        return torch.autograd.grad((l1,) if l1_only else (l1, iou), x, (go,) if l1_only else (go, go))

    def device_events(fn):         # every device event of one call, copies included: what the recorded --launch-count figures are
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])

    counts = {}
    for name, f in (("fused", fused), ("composed", comp)):
        for _ in range(3):
            step(f)
        torch.cuda.synchronize()
        if count:
            def forward_only():
                with torch.no_grad():
                    f()
            counts[name + "_launches_fwd"] = device_events(forward_only)
            counts[name + "_launches_fwd_bwd"] = device_events(lambda: step(f))
        for _ in range(iters):
            step(f)
        torch.cuda.synchronize()
    return counts


def main():
    ap = parser(warmup=20, iters=100)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--trace", type=int, default=0, help="run this many plain iterations per case instead of timing")
    ap.add_argument("--launch-count", action="store_true", help="count the launches of both with torch's profiler instead")
    args = ap.parse_args()
    dev = gpu()
    plain = args.trace or args.launch_count
    if args.iters < 100 and not plain:
        raise SystemExit("medians of at least 100 iterations are reported")
    result = {"metric": "matched_box_loss_fwd_bwd_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters}
    for name in args.cases.split(","):
        result[name] = (trace_case(CASES[name], dev, args.trace, args.launch_count) if plain
                        else run_case(CASES[name], dev, args.warmup, args.iters))
    if not plain:
        result["value"] = result[args.cases.split(",")[0]]["fused_fwd_bwd_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
