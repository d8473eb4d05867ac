#!/usr/bin/env python3
"""boxes_to_heatmap (one launch) vs the two ways to get the same targets without it, both written here from the operator's
definition (its docstring).

Sizes (ragged, seed 42, 10 categories, default centres, min_object_size (1, 1), the operator's default radii):
    B = 48 frames of 900 x 1600 (6 cameras x 8 samples), map 112 x 200, N in [1, 64] boxes per frame;
    B = 64 frames of 1080 x 1920, map 270 x 480, N in [1, 128].

Baselines:
    torch   a vectorised composition on the device: the per-object definition by tensor operations over [B, N], every
            object's (2 * 10 + 1)^2 patch as one [B, N, 21, 21] tensor, and one scatter_reduce_("amax") into a zeroed map;
            no host round trip;
    numpy   device -> host copy of boxes, categories and sizes, the definition object by object in numpy (float32 scalars for
            the per-object outputs, a float64 patch per object), host -> device copy of the seven outputs.

The fused side is timed as in bench_visible_bboxes.py: `--iters` windows of `--calls` back-to-back calls between two device
events; the torch baseline likewise with `--baseline-calls` calls per window.  The numpy baseline takes from tens to hundreds
of milliseconds, so it is timed call by call with the host clock around a device synchronisation, `--baseline-iters` calls.
Launch counts come from torch's profiler in a separate pass (kernel events per call; copies and memsets are not counted; the
numpy baseline launches none by construction and is not profiled); "not measured" if the profiler is unavailable.
Host round trips are counted from the code.  Differences are counted per output tensor against the project's bars: the six
per-object tensors bit for bit, the map within 1e-5 absolute.
Prints a few lines of log per size and ONE JSON line.

    python3 scripts/bench_box_heatmap.py [--warmup 20] [--iters 100] [--calls 20] [--baseline-iters 3] [--out FILE]
"""
import json

import numpy as np
import torch

from measure import emit, gpu, launches, parser, shown, summary, timed_windows, wall_times

SIZES = ((48, 900, 1600, 112, 200, 64), (64, 1080, 1920, 270, 480, 128))
CLASSES = 10
MIN_HW = (1.0, 1.0)
THR, R_MIN, R_MAX, R_SCALE, R_SIGMA = 0.25, 0.5, 10.0, 0.8, 1.0 / 3.0
FIELDS = ("heatmap", "is_active", "center", "center_offset", "height_width", "bboxes_heatmap", "radii")
F = np.float32


def make_inputs(B, H, W, n_max, dev, seed=42):
    """boxes of a few pixels to a third of the image around centres that may lie up to a tenth outside it, fractional
    corners, a tenth of them flipped; categories in [0, 10)"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, n_max + 1, (B,), generator=g)
    N = int(sizes.max())
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    cx, cy = (u(B, N) * 1.2 - 0.1) * W, (u(B, N) * 1.2 - 0.1) * H
    w, h = 4 + u(B, N) ** 3 * W / 3, 4 + u(B, N) ** 3 * H / 3
    boxes = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
    flip = u(B, N) < 0.1
    boxes[flip] = boxes[flip][:, [2, 3, 0, 1]]
    cats = torch.randint(0, CLASSES, (B, N), generator=g)
    return boxes.to(torch.float32).contiguous().to(dev), cats.to(dev), sizes.to(dev)


def numpy_loop(boxes, cats, sizes, H, W, Hm, Wm):
    """D2H, the definition object by object, H2D"""
    bx, ct, ns = boxes.cpu().numpy(), cats.cpu().numpy(), sizes.cpu().numpy()
    B, N = ct.shape
    hm = np.zeros((B, CLASSES, Hm, Wm), F)
    active, center, radii = np.zeros((B, N), bool), np.zeros((B, N, 2), np.int32), np.zeros((B, N), F)
    offset, hw, clipped = np.zeros((B, N, 2), F), np.zeros((B, N, 2), F), np.zeros((B, N, 4), F)
    sx, sy, xm, ym = F(Wm) / F(W), F(Hm) / F(H), F(Wm - 1), F(Hm - 1)
    clip = lambda v, m: F(0) if v < F(0) else (m if v > m else v)   # noqa: E731
    for b in range(B):
        for i in range(int(ns[b])):
            x1, y1, x2, y2 = bx[b, i]
            X1, Y1, X2, Y2 = sx * x1, sy * y1, sx * x2, sy * y2
            CX, CY = sx * ((x1 + x2) / F(2)), sy * ((y1 + y2) / F(2))
            if not all(np.isfinite(v) for v in (X1, Y1, X2, Y2, CX, CY)):
                continue
            a, c, e, d = clip(X1, xm), clip(Y1, ym), clip(X2, xm), clip(Y2, ym)
            h, w = abs(d - c), abs(e - a)
            cx, cy = clip(CX, xm), clip(CY, ym)
            fx, fy = np.floor(cx), np.floor(cy)
            ix, iy = int(fx), int(fy)
            dist = max(F(0), min(cx - min(a, e), cy - min(c, d), max(a, e) - cx, max(c, d) - cy))
            radius = min(max(dist * F(R_SCALE), F(R_MIN)), F(R_MAX))
            clipped[b, i], hw[b, i], center[b, i], offset[b, i], radii[b, i] = (a, c, e, d), (h, w), (ix, iy), (cx - fx, cy - fy), radius
            with np.errstate(all="ignore"):
                fraction = (h * w) / (abs(Y2 - Y1) * abs(X2 - X1))
            k = int(ct[b, i])
            active[b, i] = fraction >= F(THR) and h >= F(MIN_HW[0]) and w >= F(MIN_HW[1]) and 0 <= k < CLASSES
            if not active[b, i]:
                continue
            R, sigma = int(np.ceil(radius)), float(radius) * float(F(R_SIGMA))
            ya, yb, xa, xb = max(iy - R, 0), min(iy + R, Hm - 1), max(ix - R, 0), min(ix + R, Wm - 1)
            yy, xx = np.ogrid[ya:yb + 1, xa:xb + 1]
            g = np.exp(-((yy - iy) ** 2 + (xx - ix) ** 2) / (2.0 * sigma * sigma))
            view = hm[b, k, ya:yb + 1, xa:xb + 1]
            np.maximum(view, g, out=view)
    dev = boxes.device
    return tuple(torch.from_numpy(v).to(dev) for v in (hm, active, center, offset, hw, clipped, radii))


def torch_composition(boxes, cats, sizes, H, W, Hm, Wm):
    """the definition by tensor operations over [B, N] and one scatter of every patch"""
    dev = boxes.device
    B, N = cats.shape
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)   # noqa: E731
    sx, sy = f32(Wm) / f32(W), f32(Hm) / f32(H)
    live = torch.arange(N, device=dev)[None] < sizes[:, None]
    X, Y = boxes[..., 0::2] * sx, boxes[..., 1::2] * sy
    CX, CY = (boxes[..., 0] + boxes[..., 2]) / 2 * sx, (boxes[..., 1] + boxes[..., 3]) / 2 * sy
    finite = live & torch.isfinite(X).all(-1) & torch.isfinite(Y).all(-1) & torch.isfinite(CX) & torch.isfinite(CY)
    Xc, Yc = X.clamp(0, Wm - 1), Y.clamp(0, Hm - 1)
    h, w = (Yc[..., 1] - Yc[..., 0]).abs(), (Xc[..., 1] - Xc[..., 0]).abs()
    fraction = (h * w) / ((Y[..., 1] - Y[..., 0]).abs() * (X[..., 1] - X[..., 0]).abs())
    cx, cy = CX.clamp(0, Wm - 1), CY.clamp(0, Hm - 1)
    fx, fy = cx.floor(), cy.floor()
    dist = torch.stack([cx - Xc.amin(-1), cy - Yc.amin(-1), Xc.amax(-1) - cx, Yc.amax(-1) - cy], -1).amin(-1).clamp(min=0)
    radius = (dist * R_SCALE).clamp(min=R_MIN).clamp(max=R_MAX)
    active = finite & (fraction >= THR) & (h >= MIN_HW[0]) & (w >= MIN_HW[1]) & (cats >= 0) & (cats < CLASSES)
    zero = lambda t: torch.where(finite.reshape(finite.shape + (1,) * (t.dim() - 2)), t, torch.zeros_like(t))   # noqa: E731
    center = zero(torch.stack([fx, fy], -1)).to(torch.int32)
    offset, hw = zero(torch.stack([cx - fx, cy - fy], -1)), zero(torch.stack([h, w], -1))
    clipped, radii = zero(torch.stack([Xc[..., 0], Yc[..., 0], Xc[..., 1], Yc[..., 1]], -1)), zero(radius)
    # every patch at once
    K = int(np.ceil(R_MAX))
    d = torch.arange(-K, K + 1, device=dev)
    dy, dx = d[:, None], d[None, :]
    ix, iy, R = center[..., 0, None, None].long(), center[..., 1, None, None].long(), radius.ceil()[..., None, None]
    px, py = ix + dx, iy + dy
    inside = (active[..., None, None] & (dx.abs() <= R) & (dy.abs() <= R) & (px >= 0) & (px < Wm) & (py >= 0) & (py < Hm))
    sigma = (radius * R_SIGMA)[..., None, None]
    val = torch.exp(-(dx * dx + dy * dy).to(torch.float32) / (2 * sigma * sigma))
    plane = torch.arange(B, device=dev)[:, None] * CLASSES + cats.clamp(0, CLASSES - 1)
    idx = (plane[..., None, None] * Hm + py) * Wm + px
    idx, val = torch.where(inside, idx, torch.zeros_like(idx)), torch.where(inside, val, torch.zeros_like(val))
    hm = torch.zeros(B * CLASSES * Hm * Wm, device=dev).scatter_reduce_(0, idx.reshape(-1), val.reshape(-1), "amax")
    return hm.view(B, CLASSES, Hm, Wm), active, center, offset, hw, clipped, radii


def differing(got, ref):
    """per output tensor: 1 when it differs from the baseline beyond the bar (the map 1e-5 absolute, the rest bit for bit)"""
    out = {}
    for name, g, r in zip(FIELDS, got, ref):
        if name == "heatmap":
            out[name] = int(not bool(((g - r).abs() <= 1e-5).all()))
        else:
            g, r = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (g, r))
            out[name] = int(not torch.equal(g, r))
    return out


def main():
    ap = parser(warmup=20, iters=100, calls=20)
    ap.add_argument("--baseline-calls", type=int, default=2, help="back-to-back torch-baseline calls per window")
    ap.add_argument("--baseline-iters", type=int, default=3, help="timed calls of the numpy baseline")
    args = ap.parse_args()
    dev = gpu()
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import boxes_to_heatmap

    lines, results = [], []
    for B, H, W, Hm, Wm, n_max in SIZES:
        boxes, cats, sizes = make_inputs(B, H, W, n_max, dev)
        rb = RaggedBatch(boxes, sample_sizes=sizes)
        out = torch.empty((B, CLASSES, Hm, Wm), device=dev)
        kw = dict(image_hw=(H, W), heatmap_hw=(Hm, Wm), categories=cats, num_categories=CLASSES, min_object_size=MIN_HW,
                  min_fraction_area_clipping=THR, min_radius=R_MIN, max_radius=R_MAX, radius_scaling_factor=R_SCALE,
                  radius_to_sigma_factor=R_SIGMA, out=out)
        fused = lambda: boxes_to_heatmap(rb, **kw)                                             # noqa: E731
        via_numpy = lambda: numpy_loop(boxes, cats, sizes, H, W, Hm, Wm)                       # noqa: E731
        via_torch = lambda: torch_composition(boxes, cats, sizes, H, W, Hm, Wm)                # noqa: E731
        t = fused()
        got = (t.heatmap.clone(),) + tuple(r.tensor for r in t[1:])
        ref_np, ref_t = via_numpy(), via_torch()
        torch.cuda.synchronize()
        differ = dict(numpy=differing(got, ref_np), torch=differing(got, ref_t))
        count = {k: sum(v.values()) for k, v in differ.items()}
        map_err = dict(numpy=float((got[0] - ref_np[0]).abs().max()), torch=float((got[0] - ref_t[0]).abs().max()))
        ms = dict(fused=timed_windows(fused, args.warmup, args.iters, args.calls),
                  torch=timed_windows(via_torch, 3, args.iters, args.baseline_calls),
                  numpy=summary(wall_times(via_numpy, args.baseline_iters), digits=3))
        n = {k: shown(launches(f)) for k, f in (("fused", fused), ("torch", via_torch))}
        n["numpy"] = 0                                            # copies only, by construction
        trips = dict(fused=0, torch=0, numpy=2)
        res = dict(shape=dict(B=B, H=H, W=W, map_h=Hm, map_w=Wm, N=int(boxes.shape[1]), classes=CLASSES), boxes=int(sizes.sum()),
                   active=int(got[1].sum()), fused=ms["fused"], torch=ms["torch"], numpy=ms["numpy"], launches=n,
                   host_round_trips=trips,
                   speedup_median_vs_torch=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 1),
                   speedup_median_vs_numpy=round(ms["numpy"]["median_ms"] / ms["fused"]["median_ms"], 1),
                   output_tensors_that_differ=count, which=differ, map_max_abs_difference=map_err)
        results.append(res)
        named = lambda d: ", ".join(k for k, v in d.items() if v) or "none"   # noqa: E731
        lines += [f"boxes_to_heatmap  B={B} frames of {H}x{W} -> {CLASSES} x {Hm}x{Wm}, N<={boxes.shape[1]}: {res['boxes']} boxes, "
                  f"{res['active']} active",
                  f"  fused: {args.iters} windows of {args.calls} calls, timed {ms['fused']['timed_s']} s; torch: {args.iters} windows of "
                  f"{args.baseline_calls} calls, timed {ms['torch']['timed_s']} s; numpy: {args.baseline_iters} calls, timed "
                  f"{ms['numpy']['timed_s']} s",
                  f"  fused              median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {n['fused']}  host round trips 0",
                  f"  torch composition  median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {n['torch']}  host round trips 0",
                  f"  numpy loop         median {ms['numpy']['median_ms']:.3f} ms  min {ms['numpy']['min_ms']:.3f} ms  launches {n['numpy']}  host round trips 2",
                  f"  output tensors (of 7) that differ from the baselines beyond the bars: torch {count['torch']} ({named(differ['torch'])}), "
                  f"numpy {count['numpy']} ({named(differ['numpy'])}); largest map difference {map_err['torch']:.2e}, {map_err['numpy']:.2e}"]
    result = dict(metric="boxes_to_heatmap_ms", unit="ms", value=results[0]["fused"]["median_ms"], warmup=args.warmup,
                  iters=args.iters, calls_per_window=args.calls, baseline_calls_per_window=args.baseline_calls,
                  baseline_iters=args.baseline_iters, sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
