#!/usr/bin/env python3
"""Fused Gaussian focal loss vs the torch composition it replaces, at configs[1] size (64 x 1080 x 1920).

The target is drawn by draw_heatmap_batched(..., clear=True) from bench_workloads' seed-42 rule-A objects (the headline
workload's map); logits are uniform in [-10, 10], float32 and bfloat16.  For each logits dtype: forward and
forward + backward ms of accvlab.draw_heatmap.gaussian_focal_loss and of the composition (with its num_pos.item()),
medians over device-event-timed iterations, the algorithmic bytes (forward: logits + target read; backward: logits +
target read + gradient written) and the fused op's share of the 8 TB/s HBM peak by those bytes.  The map (530 MB f32)
is larger than the 256 MB Infinity Cache, so back-to-back iterations read from HBM.  Prints ONE JSON line.

    python3 scripts/bench_heatmap_loss.py [--warmup 20] [--iters 200] [--out FILE]
"""
import json
import statistics

import torch

from measure import call_times, emit, gpu, parser   # puts the repository root on the path

import bench_workloads as wl  # noqa: E402

B, H, W = 64, 1080, 1920
HBM_BPS = 8.0e12


def composition(logits, target, alpha=2.0, gamma=4.0, clamp_eps=1e-4):
    """what a head writes today: element-wise torch ops, num_pos read back to the host"""
    p = logits.float().sigmoid().clamp(clamp_eps, 1 - clamp_eps)
    pos = target.eq(1)
    pos_loss = -(p + 1e-12).log() * (1 - p).pow(alpha) * pos
    neg_loss = -(1 - p + 1e-12).log() * p.pow(alpha) * (1 - target).pow(gamma)
    num_pos = max(int(pos.sum().item()), 1)
    return (pos_loss + neg_loss).sum() / num_pos


def main():
    args = parser(warmup=20, iters=200).parse_args()

    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import draw_heatmap_batched, gaussian_focal_loss

    dev = gpu()
    centers_l, radii_l = wl.heatmap_objects(B, H, W, 1, 128, "A", seed=42)
    centers = combine_data(centers_l, device=dev)
    radii = combine_data(radii_l, device=dev, other_with_same_sample_sizes=centers)
    target = torch.empty((B, H, W), device=dev)
    draw_heatmap_batched(target, centers, radii, 6.0, 1.0, clear=True)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    base = (torch.rand((B, H, W), device=dev, generator=g) * 2 - 1) * 10
    n = target.numel()

    result = {"metric": "gaussian_focal_loss_fwd_bwd_ms", "unit": "ms", "shape": [B, H, W],
              "num_pos": int((target == 1).sum()), "warmup": args.warmup, "iters": args.iters, "hbm_peak_tbps": 8.0}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        x = base.to(dtype).requires_grad_(True)
        es = x.element_size()
        fwd_bytes = n * (es + 4)
        bwd_bytes = n * (es + 4 + es)

        def fused_fwd():
            with torch.no_grad():
                gaussian_focal_loss(x, target)

        def fused_fwd_bwd():
            torch.autograd.grad(gaussian_focal_loss(x, target), x)

        def comp_fwd():
            with torch.no_grad():
                composition(x, target)

        def comp_fwd_bwd():
            torch.autograd.grad(composition(x, target), x)

        with torch.no_grad():
            fl = float(gaussian_focal_loss(x, target))
            cl = float(composition(x, target))
        ms = {k: round(statistics.median(call_times({k: f}, args.warmup, args.iters)[k]), 4)      # one after the other, not in turns
              for k, f in (("fused_fwd_ms", fused_fwd), ("fused_fwd_bwd_ms", fused_fwd_bwd), ("torch_fwd_ms", comp_fwd),
                           ("torch_fwd_bwd_ms", comp_fwd_bwd))}
        result[name] = dict(
            ms,
            fwd_bytes=fwd_bytes,
            fwd_bwd_bytes=fwd_bytes + bwd_bytes,
            fused_fwd_hbm_fraction=round(fwd_bytes / (ms["fused_fwd_ms"] * 1e-3) / HBM_BPS, 3),
            fused_fwd_bwd_hbm_fraction=round((fwd_bytes + bwd_bytes) / (ms["fused_fwd_bwd_ms"] * 1e-3) / HBM_BPS, 3),
            speedup_fwd=round(ms["torch_fwd_ms"] / ms["fused_fwd_ms"], 2),
            speedup_fwd_bwd=round(ms["torch_fwd_bwd_ms"] / ms["fused_fwd_bwd_ms"], 2),
            loss_fused=fl,
            loss_torch=cl,
        )
        del x
    result["value"] = result["f32"]["fused_fwd_bwd_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
