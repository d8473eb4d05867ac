#!/usr/bin/env python3
"""Fused sigmoid focal classification loss (accvlab.batching_helpers.matched_focal_loss) vs the composition it replaces
(examples/matched_loss.py::focal_class_loss_composed: ragged gather of the labels, ragged write into a [B, Q] label
tensor, one_hot, sigmoid_focal_loss, division by the number of pairs).

Cases, float32 and bfloat16 each: (a) 8 x 900 x 10 with up to 100 objects (the F3 shape of DESIGN.md §4), (b) 16 x 300 x
91, (c) 48 x 900 x 80 (six decoder layers of batch 8 stacked on the batch axis), (d) 32 x 8400 x 80, the one streaming
case.  For each: forward and forward + backward of both; all four alternate inside every timed iteration of one process;
device events; medians.  `--trace N` runs N plain forward + backward iterations of both instead (for a kernel trace);
`--launch-count` counts the kernel launches of one forward + backward of both with torch's profiler.  Prints ONE JSON
line.

    python3 scripts/bench_matched_focal_loss.py [--warmup 20] [--iters 100] [--out FILE] [--cases a_f32,d_bf16]
"""
import json
import statistics

import torch

from measure import call_times, emit, gpu, parser   # puts tests/ and examples/ on the path

import matched_focal_loss_cases as mf  # noqa: E402
import matched_loss as ml  # noqa: E402

SHAPES = {"a": (8, 900, 10, 100), "b": (16, 300, 91, 40), "c": (48, 900, 80, 60), "d": (32, 8400, 80, 60)}
CASES = {f"{k}_{n}": dict(shape=v, dtype=d) for k, v in SHAPES.items() for n, d in (("f32", torch.float32), ("bf16", torch.bfloat16))}
COPY_CEILING_TBPS = 6.29   # float4 copy, DESIGN.md §9b


def make(cfg, dev):
    B, Q, C, objects = cfg["shape"]
    logits, labels, pind, gind, _ = mf.shape_case(B, Q, C, objects, cfg["dtype"], seed=B, device=dev)
    x = logits.detach().requires_grad_(True)
    fused = lambda: ml.focal_class_loss_fused(x, labels, pind, gind)          # noqa: E731
    comp = lambda: ml.focal_class_loss_composed(x, labels, pind, gind)        # noqa: E731
    return x, fused, comp, int(pind.sample_sizes.sum())


def run_case(cfg, dev, warmup, iters):
    x, fused, comp, pairs = make(cfg, dev)
    go = torch.ones(x.shape[0], device=dev)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), x, go)

    with torch.no_grad():
        lf, lc = float(fused().sum()), float(comp().sum())
    ms = call_times({"fused_fwd_ms": fwd(fused), "torch_fwd_ms": fwd(comp), "fused_fwd_bwd_ms": fwd_bwd(fused),
                     "torch_fwd_bwd_ms": fwd_bwd(comp)}, warmup, iters)
    ms = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    nbytes = x.numel() * x.element_size()
    fused_bwd = max(ms["fused_fwd_bwd_ms"] - ms["fused_fwd_ms"], 1e-6)
    return dict(ms, shape=list(x.shape), dtype=str(x.dtype).split(".")[-1], pairs=pairs, logit_bytes=nbytes,
                speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
                speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2),
                # bytes the two streaming kernels move (logits read twice, gradient written once) over forward + backward
                fwd_bwd_tbps=round(3 * nbytes / (ms["fused_fwd_bwd_ms"] * 1e-3) / 1e12, 3),
                fwd_bwd_share_of_copy_ceiling=round(3 * nbytes / (ms["fused_fwd_bwd_ms"] * 1e-3) / 1e12 / COPY_CEILING_TBPS, 3),
                fwd_read_tbps=round(nbytes / (ms["fused_fwd_ms"] * 1e-3) / 1e12, 3),
                bwd_tbps_by_difference=round(2 * nbytes / (fused_bwd * 1e-3) / 1e12, 3), loss_fused=lf, loss_torch=lc)


def trace_case(cfg, dev, iters, count):
    """plain iterations for a kernel trace (iters), or the launch counts of both from torch's profiler (count)"""
    x, fused, comp, _ = make(cfg, dev)
    go = torch.ones(x.shape[0], device=dev)
    counts = {}
    for name, f in (("fused", fused), ("composed", comp)):
        for _ in range(3):
            torch.autograd.grad(f(), x, go)
        torch.cuda.synchronize()
        if count:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                torch.autograd.grad(f(), x, go)
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            counts[name + "_launches_fwd_bwd"] = len(kernels)
        for _ in range(iters):
            torch.autograd.grad(f(), x, go)
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
    result = {"metric": "matched_focal_loss_fwd_bwd_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters}
    for name in args.cases.split(","):
        result[name] = (trace_case(CASES[name], dev, args.trace, args.launch_count) if plain
                        else run_case(CASES[name], dev, args.warmup, args.iters))
    if not plain:
        result["value"] = result[args.cases.split(",")[0]]["fused_fwd_bwd_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
