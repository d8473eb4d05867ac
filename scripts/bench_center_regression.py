#!/usr/bin/env python3
"""Fused centre-point regression (accvlab.draw_heatmap.center_regression_loss) vs the torch composition it replaces.

Cases: (a) the headline geometry, 64 frames of 270 x 480 (1920 x 1080 at stride 4) with heads [2, 2] (offset, size),
float32 and bfloat16, centres from bench_workloads' seed-42 rule-A objects; (b) CenterPoint-like 4 x [2, 1, 3, 2, 2] x
180 x 180 with up to 500 objects, float32; (c) stride 1, 8 x 4 x 1080 x 1920, float32.  For each: forward, forward +
backward and backward alone of the fused operator and of the composition (tests/center_regression_cases.composition_loss,
the float32 form of the oracle, torch.cat included when there are several heads), and torch's zero_() on gradient tensors
of the same sizes as the floor of the backward.  All of them alternate inside every timed iteration of one process;
device events; medians.  Prints ONE JSON line.

    python3 scripts/bench_center_regression.py [--warmup 10] [--iters 100] [--out FILE] [--cases a_f32,b_f32]
"""
import json
import statistics

import torch

from measure import call_times, emit, gpu, parser   # puts the repository root and tests/ on the path

import bench_workloads as wl  # noqa: E402
import center_regression_cases as cr  # noqa: E402

CASES = {
    "a_f32": dict(B=64, H=270, W=480, heads=[2, 2], n_max=128, dtype=torch.float32),
    "a_bf16": dict(B=64, H=270, W=480, heads=[2, 2], n_max=128, dtype=torch.bfloat16),
    "b_f32": dict(B=4, H=180, W=180, heads=[2, 1, 3, 2, 2], n_max=500, dtype=torch.float32),
    "c_f32": dict(B=8, H=1080, W=1920, heads=[4], n_max=128, dtype=torch.float32),
}


def run_case(name, cfg, dev, warmup, iters):
    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import center_regression_loss

    B, H, W, heads, dtype = cfg["B"], cfg["H"], cfg["W"], cfg["heads"], cfg["dtype"]
    C = sum(heads)
    centers_l, _ = wl.heatmap_objects(B, H, W, 1, cfg["n_max"], "A", seed=42)
    centers = combine_data(centers_l, device=dev)
    xy, sizes = centers.tensor, centers.sample_sizes
    N = xy.shape[1]
    maps = [m.requires_grad_(True) for m in cr.make_maps(B, heads, H, W, dtype, dev, seed=1)]
    g = torch.Generator().manual_seed(2)
    targets = (torch.randn(B, N, C, generator=g) * 3.0).to(dev)
    weights = torch.rand(B, N, generator=g).to(dev)
    grads = [torch.empty_like(m) for m in maps]
    feats = maps if len(maps) > 1 else maps[0]

    def fused():
        return center_regression_loss(feats, centers, targets, weights)

    def comp():
        return cr.composition_loss(maps, xy, sizes, targets, weights)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), maps)

    def bwd(f):
        run = lambda loss: torch.autograd.grad(loss, maps)  # noqa: E731
        run.prepare = f
        return run

    def zero():
        for t in grads:
            t.zero_()

    with torch.no_grad():
        lf, lc = float(fused()), float(comp())
    ms = call_times({"fused_fwd_ms": fwd(fused), "torch_fwd_ms": fwd(comp), "fused_fwd_bwd_ms": fwd_bwd(fused),
                     "torch_fwd_bwd_ms": fwd_bwd(comp), "fused_bwd_ms": bwd(fused), "torch_bwd_ms": bwd(comp), "zero_ms": zero},
                    warmup, iters)
    ms = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    grad_bytes = sum(t.numel() * t.element_size() for t in grads)
    return dict(ms, shape=[B, heads, H, W], dtype=str(dtype).split(".")[-1], n_max=N, objects=int(sizes.sum()),
                grad_bytes=grad_bytes, speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
                speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2),
                bwd_over_zero=round(ms["fused_bwd_ms"] / ms["zero_ms"], 3),
                bwd_write_tbps=round(grad_bytes / (ms["fused_bwd_ms"] * 1e-3) / 1e12, 3), loss_fused=lf, loss_torch=lc)


def main():
    ap = parser(warmup=10, iters=100)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    dev = gpu()
    result = {"metric": "center_regression_fwd_bwd_ms", "unit": "ms", "warmup": args.warmup, "iters": args.iters}
    for name in args.cases.split(","):
        result[name] = run_case(name, CASES[name], dev, args.warmup, args.iters)
    first = args.cases.split(",")[0]
    result["value"] = result[first]["fused_fwd_bwd_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
