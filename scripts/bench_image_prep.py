#!/usr/bin/env python3
"""prepare_images (one launch) vs the torch composition it replaces (examples/image_prep_step.py: `to(float)`, `permute`,
`affine_grid` + `grid_sample`, the colour chain in tensor operations, `F.pad`, normalise).

Shapes (seed 42, float32 CHW output, ImageNet mean / std, a photometric row per sample shared by its cameras):
    warp      8 samples x 6 cameras of 900 x 1600 -> 256 x 704, tile 32: `output_size_transform(crop, center)` (scale 0.44), every
              second sample flipped in x;
    no_warp   48 images of 900 x 1600 at full resolution, no matrix, tile 32 (900 -> 928 rows of which 28 are padding).

Both sides are timed alike: `--iters` windows of `--calls` (fused) or `--baseline-calls` (torch) back-to-back calls between
two device events, after `--warmup` calls.  Launch counts come from torch's profiler in a separate pass (kernel events per
call; copies and memsets are not counted); "not measured" if the profiler is unavailable.  Host round trips are counted from
the code.  Bytes are counted from the shapes: the source bytes the call samples (every source pixel that is a bilinear
neighbour of some output pixel, counted once, 3 bytes; all of the valid source without a matrix) plus the output bytes written;
bytes over the fused median is the achieved rate, given also as a fraction of the 8 TB/s HBM peak.  The source count is the
least the algorithm needs, not what the memory system fetched.

The one output tensor is compared against the baseline with a bar written down here, not taken from the result.  Value
arithmetic: both sides are float32 chains of at most K = 23 rounded operations (tests/image_prep_cases.py), so
2 * K * 2^-24 * (1 + max saturation) * 255 / min(std).  Sample positions: the two sides compute (sx, sy) by different float32
sequences (`grid_sample` through normalised coordinates); with P = 8 rounded operations a side at a magnitude of at most the
source extent E, the positions differ by at most 2 * P * 2^-24 * E pixels per axis, and a bilinear sample moves by at most 255
per pixel per axis: + 2 * (2 * P * 2^-24 * E) * 255 / min(std) with a matrix.
With `--probe` the warp shape is also timed in variants that take one cost away at a time (no colour rows; every colour
stage on; a 90 x 160 source with the same output, which stays in cache; `zero_()` of the output as the store floor): what
bounds the kernel, for the decision about a second kernel path.
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_image_prep.py [--warmup 10] [--iters 100] [--calls 50] [--baseline-calls 2] [--probe] [--out FILE]
"""
import json

import torch

from measure import emit, gpu, launches, parser, shown, timed_windows

SOURCE_HW = (900, 1600)
SHAPES = (("warp", 8, 6, (256, 704)), ("no_warp", 8, 6, None))
TILE = 32
K_VALUE, P_POSITION = 23, 8
HBM_PEAK = 8.0e12


def sampled_source_bytes(transform, source_hw, output_hw):
    """3 bytes per source pixel that is a bilinear neighbour of an output pixel, for one matrix (float64 positions)"""
    Hs, Ws = source_hw
    Ho, Wo = output_hw
    m = torch.zeros((3, 3), dtype=torch.float64)
    m[:2], m[2, 2] = transform.double().cpu(), 1.0
    inv = torch.linalg.inv(m)
    X, Y = torch.meshgrid(torch.arange(Wo, dtype=torch.float64) + 0.5, torch.arange(Ho, dtype=torch.float64) + 0.5, indexing="xy")
    sx = inv[0, 0] * X + inv[0, 1] * Y + inv[0, 2] - 0.5
    sy = inv[1, 0] * X + inv[1, 1] * Y + inv[1, 2] - 0.5
    x0, y0 = sx.floor().long(), sy.floor().long()
    touched = torch.zeros((Hs, Ws), dtype=torch.bool)
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
            touched[y[ok], x[ok]] = True
    return 3 * int(touched.sum())


def probe_warp_shape(dev, args):
    from image_prep_step import MEAN, STD, step_parameters

    from accvlab.image_prep import output_size_transform, prepare_images

    _, samples, cameras, output_hw = SHAPES[0]
    B = samples * cameras
    images = torch.randint(0, 256, (B, *SOURCE_HW, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(42)).to(dev)
    transforms, rows = (t.to(dev) for t in step_parameters(samples, cameras, SOURCE_HW, output_hw, seed=42))
    small_hw = (SOURCE_HW[0] // 10, SOURCE_HW[1] // 10)
    small = images[:, :small_hw[0], :small_hw[1]].contiguous()
    small_t = torch.tensor([output_size_transform(small_hw, output_hw, "crop", "center")] * B, dtype=torch.float32, device=dev)
    every = torch.tensor([[0.1, 1.1, 1.2, 20.0, 1.0, 3.0]] * B, device=dev)
    out = torch.empty((B, 3, *output_hw), device=dev)
    kw = dict(output_hw=output_hw, mean=MEAN, std=STD, tile_hw=TILE, out=out)
    variants = {
        "as benched": lambda: prepare_images(images, transforms=transforms, photometric=rows, **kw),
        "photometric=None": lambda: prepare_images(images, transforms=transforms, **kw),
        "every colour stage on": lambda: prepare_images(images, transforms=transforms, photometric=every, **kw),
        f"{small_hw[0]}x{small_hw[1]} source (stays in cache), photometric=None": lambda: prepare_images(small, transforms=small_t, **kw),
        f"{small_hw[0]}x{small_hw[1]} source (stays in cache), every colour stage on":
            lambda: prepare_images(small, transforms=small_t, photometric=every, **kw),
        "out.zero_() (the store floor)": lambda: out.zero_(),
    }
    return {k: timed_windows(f, args.warmup, args.iters, args.calls) for k, f in variants.items()}


def main():
    ap = parser(warmup=10, iters=100, calls=50)
    ap.add_argument("--probe", action="store_true", help="also time the warp shape with one cost taken away at a time")
    ap.add_argument("--baseline-calls", type=int, default=2, help="back-to-back torch-composition calls per window")
    args = ap.parse_args()
    dev = gpu()
    from image_prep_step import MEAN, STD, step_parameters, torch_composition

    from accvlab.image_prep import padded_hw, prepare_images

    lines, results = [], []
    for name, samples, cameras, output_hw in SHAPES:
        B = samples * cameras
        images = torch.randint(0, 256, (B, *SOURCE_HW, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(42)).to(dev)
        transforms, photometric = step_parameters(samples, cameras, SOURCE_HW, output_hw or SOURCE_HW, seed=42)
        if output_hw is None:
            transforms = None
            source_bytes = B * 3 * SOURCE_HW[0] * SOURCE_HW[1]
        else:
            per_matrix = {}
            for m in transforms:
                key = tuple(m.flatten().tolist())
                if key not in per_matrix:
                    per_matrix[key] = sampled_source_bytes(m, SOURCE_HW, output_hw)
            source_bytes = sum(per_matrix[tuple(m.flatten().tolist())] for m in transforms)
            transforms = transforms.to(dev)
        photometric = photometric.to(dev)
        Ho, Wo = output_hw or SOURCE_HW
        Hp, Wp = padded_hw((Ho, Wo), TILE)
        out = torch.empty((B, 3, Hp, Wp), device=dev)
        fused = lambda: prepare_images(images, output_hw=output_hw, transforms=transforms, photometric=photometric,   # noqa: E731
                                       mean=MEAN, std=STD, tile_hw=TILE, out=out)
        composed = lambda: torch_composition(images, transforms, photometric, (Ho, Wo), mean=MEAN, std=STD, tile_hw=TILE)   # noqa: E731
        got, ref = fused().clone(), composed()
        torch.cuda.synchronize()
        sat = max(1.0, float(photometric[:, 2].max()))
        bar = 2 * K_VALUE * 2.0 ** -24 * (1 + sat) * 255 / min(STD)
        if transforms is not None:
            bar += 2 * (2 * P_POSITION * 2.0 ** -24 * max(SOURCE_HW)) * 255 / min(STD)
        diff = float((got - ref).abs().max())
        differ = int(not diff <= bar)
        del ref
        ms = dict(fused=timed_windows(fused, args.warmup, args.iters, args.calls), torch=timed_windows(composed, 3, args.iters, args.baseline_calls))
        n = {k: shown(launches(f)) for k, f in (("fused", fused), ("torch", composed))}
        out_bytes = out.numel() * out.element_size()
        rate = (source_bytes + out_bytes) / (ms["fused"]["median_ms"] * 1e-3)
        res = dict(shape=dict(name=name, B=B, source_h=SOURCE_HW[0], source_w=SOURCE_HW[1], output_h=Ho, output_w=Wo, padded_h=Hp,
                              padded_w=Wp, tile=TILE), fused=ms["fused"], torch=ms["torch"], launches=n,
                   host_round_trips=dict(fused=0, torch=0), source_bytes_sampled=source_bytes, output_bytes=out_bytes,
                   fused_bytes_per_s=round(rate, 0), fraction_of_hbm_peak=round(rate / HBM_PEAK, 4),
                   speedup_median_vs_torch=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 1),
                   output_tensors_that_differ=differ, max_abs_difference=diff, bar=bar)
        results.append(res)
        lines += [f"prepare_images  {name}: B={B} images of {SOURCE_HW[0]}x{SOURCE_HW[1]} -> float32 CHW {Hp}x{Wp} ({Ho}x{Wo} before "
                  f"padding to {TILE}){', crop + flip' if transforms is not None else ', no matrix'}, photometric rows per sample",
                  f"  fused: {args.iters} windows of {args.calls} calls, timed {ms['fused']['timed_s']} s; torch: {args.iters} windows of "
                  f"{args.baseline_calls} calls, timed {ms['torch']['timed_s']} s",
                  f"  fused              median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {n['fused']}  host round trips 0",
                  f"  torch composition  median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {n['torch']}  host round trips 0",
                  f"  fused moves {source_bytes / 1e6:.1f} MB of source sampled + {out_bytes / 1e6:.1f} MB of output = "
                  f"{rate / 1e12:.3f} TB/s, {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak",
                  f"  output tensors (of 1) that differ from the torch composition beyond the bar: {differ}; largest difference "
                  f"{diff:.2e}, bar {bar:.2e}"]
    probe = None
    if args.probe:
        probe = probe_warp_shape(dev, args)
        lines.append("prepare_images  warp shape with one cost taken away at a time (median ms, min ms):")
        lines += [f"  {k:<58} {v['median_ms']:.4f}  {v['min_ms']:.4f}" for k, v in probe.items()]
    result = dict(metric="prepare_images_ms", unit="ms", value=results[0]["fused"]["median_ms"], warmup=args.warmup, iters=args.iters,
                  calls_per_window=args.calls, baseline_calls_per_window=args.baseline_calls, kernel_paths=["gather"], sizes=results, probe=probe)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
