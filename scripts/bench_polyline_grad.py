#!/usr/bin/env python3
"""Polyline interpolate / lengths forward + backward through autograd (the HIP backward accv_polyline_grad) against the
same function written as a torch composition in the same dtype with torch autograd.

Shapes (batch x points x queries, 2-D points, float32, relative queries k / (queries - 1) as a lane head samples them):
config-3 lanes 256 x 24 x 256 (32 frames x 8 lanes), 64 x 100 x 100, 64 x 5000 x 5000 and 1 x 5000 x 5000.  Points are
a seeded random walk.  Per shape: forward only (no grad) and forward + backward ms of accvlab's operators and of the
composition, medians over device-event-timed iterations after warm-up; the loss is <samples, g> + <lengths, g_len> so
that both backward inputs are used.  Prints ONE JSON line (``--out`` also writes it to a file).

    python3 scripts/bench_polyline_grad.py [--warmup 20] [--iters 200] [--out FILE] [--only-ours]

``--only-ours`` skips the composition (the kernel trace in profiles/ was taken that way, with few iterations).
"""
import json
import statistics

import torch

from measure import call_times, emit, gpu, parser

SHAPES = [("config3_lanes", 256, 24, 256), ("b64_p100_q100", 64, 100, 100), ("b64_p5000_q5000", 64, 5000, 5000),
          ("b1_p5000_q5000", 1, 5000, 5000)]


def composition(points, fractions):
    """interpolate(points, fractions, relative=True) and lengths(points) as differentiable torch ops (searchsorted picks
    the segment, as the CPU formulation in ops.py does)"""
    b, p, d = points.shape
    seg = torch.linalg.vector_norm(points[:, 1:] - points[:, :-1], dim=2)
    acc = torch.cat([seg.new_zeros((b, 1)), torch.cumsum(seg, 1)], 1)
    total = acc[:, -1]
    dist = fractions * total.unsqueeze(1)
    with torch.no_grad():
        idx = torch.searchsorted(acc.detach().contiguous(), dist.detach().contiguous(), right=True) - 1
        i = idx.clamp(0, p - 2)
        inside = (idx >= 0) & (idx < p - 1)
        seg_i = seg.detach().gather(1, i)
        interp = inside & (seg_i >= torch.finfo(points.dtype).eps)
        j = torch.where(idx < 0, torch.zeros_like(idx), idx.clamp(max=p - 1))
    c_i = acc.gather(1, i)
    l_i = torch.where(interp, seg.gather(1, i), torch.ones_like(c_i))
    w1 = torch.where(interp, (dist - c_i) / l_i, torch.zeros_like(c_i)).unsqueeze(-1)
    p0 = points.gather(1, i.unsqueeze(-1).expand(b, -1, d))
    p1 = points.gather(1, (i + 1).unsqueeze(-1).expand(b, -1, d))
    pj = points.gather(1, j.unsqueeze(-1).expand(b, -1, d))
    return torch.where(interp.unsqueeze(-1), p0 + w1 * (p1 - p0), pj), total


def main():
    ap = parser(warmup=20, iters=200)
    ap.add_argument("--only-ours", action="store_true", help="time accvlab's operators only")
    args = ap.parse_args()

    from accvlab.lane_helpers.polyline import interpolate, lengths

    dev = gpu()
    result = {"metric": "polyline_interpolate_lengths_fwd_bwd_ms", "unit": "ms", "dtype": "float32", "dims": 2,
              "relative": True, "warmup": args.warmup, "iters": args.iters, "shapes": {}}
    for name, b, p, q in SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(p + q)
        pts = torch.randn((b, p, 2), device=dev, generator=g).cumsum(1)
        fr = torch.linspace(0, 1, q, device=dev).expand(b, q).contiguous()
        go = torch.randn((b, q, 2), device=dev, generator=g)
        gl = torch.randn((b,), device=dev, generator=g)
        x = pts.clone().requires_grad_(True)
        f = fr.clone().requires_grad_(True)

        def ours_fwd():
            with torch.no_grad():
                interpolate(x, f, relative=True)
                lengths(x)

        def ours_fwd_bwd():
            torch.autograd.grad([interpolate(x, f, relative=True), lengths(x)], [x, f], [go, gl])

        def comp_fwd_bwd():
            torch.autograd.grad(list(composition(x, f)), [x, f], [go, gl])

        runs = [("ours_fwd_ms", ours_fwd), ("ours_fwd_bwd_ms", ours_fwd_bwd)]
        if not args.only_ours:
            runs.append(("torch_fwd_bwd_ms", comp_fwd_bwd))
        ms = {k: round(statistics.median(call_times({k: fn}, args.warmup, args.iters)[k]), 4) for k, fn in runs}   # one after the other
        entry = dict(ms, batch=b, points=p, queries=q)
        if not args.only_ours:
            entry["speedup_fwd_bwd"] = round(ms["torch_fwd_bwd_ms"] / ms["ours_fwd_bwd_ms"], 2)
        result["shapes"][name] = entry
    result["value"] = result["shapes"]["config3_lanes"]["ours_fwd_bwd_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
