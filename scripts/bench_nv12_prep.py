#!/usr/bin/env python3
"""prepare_images_nv12 (one launch, NV12 planes in) vs the two routes that materialise the RGB batch first: `nv12_to_rgb` +
`prepare_images` (two launches) and the torch composition of the conversion a user would write without either
(examples/nv12_prep_step.py: chroma upsampling, a float matrix product, round, clamp) + `prepare_images`.

Shapes (seed 42, limited range, float32 CHW output, ImageNet mean / std, a photometric row per sample shared by its cameras;
surfaces of pitch 1664 whose UV plane starts at row 912, the luma height rounded up to 16):
    warp      8 samples x 6 cameras of 900 x 1600 -> 256 x 704, tile 32: `output_size_transform(crop, center)`, every second
              sample flipped in x;
    no_warp   48 images of 900 x 1600 at full resolution, no matrix, tile 32.

Every row is timed in `--blocks` blocks, the rows taking turns inside a block; a block is `--iters` windows of `--calls`
(`--baseline-calls` for the torch row) back-to-back calls between two device events, after `--warmup` calls; a block's
figure is the median of its windows.  A row's median is the median of its block medians, its spread their max - min.  The
verdict: the fused median against the sum of the `nv12_to_rgb` and `prepare_images` medians of the same run, with the largest
spread of those three rows as the margin (what the measurement cannot resolve).  Launch counts come from torch's profiler in
a separate pass; host round trips are counted from the code.  Bytes are counted from the shapes, the least the algorithm
needs: per route, the source bytes sampled (a luma byte per source pixel that is a bilinear neighbour of an output pixel and
the two bytes of each chroma sample under one, all of the planes without a matrix; the conversion as a step of its own reads
all of both planes and writes 3 bytes per pixel, which `prepare_images` then samples) plus the output bytes; over the
route's median that is its rate, given also as a fraction of the 8 TB/s HBM peak.
The fused result is checked bit for bit against the two-launch route before anything is timed.
Prints a few lines of log per shape and ONE JSON line.

    python3 scripts/bench_nv12_prep.py [--warmup 10] [--blocks 3] [--iters 40] [--calls 20] [--baseline-calls 2] [--out FILE]
"""
import json

import torch

from measure import block_summary, emit, gpu, launches, parser, shown, timed_windows

SOURCE_HW = (900, 1600)
PITCH = 1664
SHAPES = (("warp", 8, 6, (256, 704)), ("no_warp", 8, 6, None))
TILE = 32
HBM_PEAK = 8.0e12
ROWS = ("fused", "nv12_to_rgb", "prepare_images", "torch + prepare_images")


def touched_source(transform, source_hw, output_hw):
    """bool [Hs, Ws]: the source pixels that are a bilinear neighbour of an output pixel, for one matrix (float64 positions)"""
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
    return touched


def sampled_counts(transforms, source_hw, output_hw, B):
    """(luma pixels, chroma samples) sampled over the batch"""
    Hs, Ws = source_hw
    if transforms is None:
        return B * Hs * Ws, B * ((Hs + 1) // 2) * ((Ws + 1) // 2)
    per_matrix, luma, chroma = {}, 0, 0
    for m in transforms:
        key = tuple(m.flatten().tolist())
        if key not in per_matrix:
            t = touched_source(m, source_hw, output_hw)
            pad = torch.zeros((Hs + Hs % 2, Ws + Ws % 2), dtype=torch.bool)
            pad[:Hs, :Ws] = t
            c = pad[0::2, 0::2] | pad[0::2, 1::2] | pad[1::2, 0::2] | pad[1::2, 1::2]
            per_matrix[key] = (int(t.sum()), int(c.sum()))
        luma, chroma = luma + per_matrix[key][0], chroma + per_matrix[key][1]
    return luma, chroma


def main():
    ap = parser(warmup=10, iters=40, calls=20)
    ap.add_argument("--blocks", type=int, default=3, help="blocks per row; the rows take turns inside a block")
    ap.add_argument("--baseline-calls", type=int, default=2, help="back-to-back torch-composition calls per window")
    args = ap.parse_args()
    dev = gpu()
    from image_prep_step import MEAN, STD, step_parameters
    from nv12_prep_step import random_surfaces, torch_nv12_to_rgb

    from accvlab.image_prep import nv12_planes, nv12_to_rgb, padded_hw, prepare_images, prepare_images_nv12

    Hs, Ws = SOURCE_HW
    lines, results = [], []
    for name, samples, cameras, output_hw in SHAPES:
        B = samples * cameras
        surfaces, uv_row = random_surfaces(B, SOURCE_HW, PITCH, seed=42, aligned_rows=16)
        surfaces = surfaces.to(dev)
        y, uv = nv12_planes(surfaces, SOURCE_HW, uv_row=uv_row)
        transforms, photometric = step_parameters(samples, cameras, SOURCE_HW, output_hw or SOURCE_HW, seed=42)
        if output_hw is None:
            transforms = None
        luma, chroma = sampled_counts(transforms, SOURCE_HW, output_hw or SOURCE_HW, B)
        transforms = None if transforms is None else transforms.to(dev)
        photometric = photometric.to(dev)
        Ho, Wo = output_hw or SOURCE_HW
        Hp, Wp = padded_hw((Ho, Wo), TILE)
        out = torch.empty((B, 3, Hp, Wp), device=dev)
        rgb = torch.empty((B, Hs, Ws, 3), dtype=torch.uint8, device=dev)
        kw = dict(output_hw=output_hw, transforms=transforms, photometric=photometric, mean=MEAN, std=STD, tile_hw=TILE, out=out)
        calls = {"fused": lambda: prepare_images_nv12(y, uv, **kw),
                 "nv12_to_rgb": lambda: nv12_to_rgb(y, uv, out=rgb),
                 "prepare_images": lambda: prepare_images(rgb, **kw),
                 "torch + prepare_images": lambda: prepare_images(torch_nv12_to_rgb(y, uv), **kw)}
        got = calls["fused"]().clone()
        calls["nv12_to_rgb"]()
        equal = bool(torch.equal(got.view(torch.int32), calls["prepare_images"]().view(torch.int32)))
        byte_diff = int((torch_nv12_to_rgb(y, uv).to(torch.int16) - rgb.to(torch.int16)).abs().max())
        torch.cuda.synchronize()
        blocks = {r: [] for r in ROWS}
        for _ in range(args.blocks):
            for r in ROWS:
                n = args.baseline_calls if r.startswith("torch") else args.calls
                blocks[r].append(timed_windows(calls[r], 3 if r.startswith("torch") else args.warmup, args.iters, n))
        calls["nv12_to_rgb"]()      # the torch row does not write rgb; keep it the conversion's for the profiler pass
        n_launch = {r: shown(launches(calls[r])) for r in ROWS}
        ms = {r: block_summary(blocks[r]) for r in ROWS}
        out_bytes = out.numel() * out.element_size()
        full_planes = B * (Hs * Ws + 2 * ((Hs + 1) // 2) * ((Ws + 1) // 2))
        moved = {"fused": luma + 2 * chroma + out_bytes,
                 "nv12_to_rgb": full_planes + rgb.numel(),
                 "prepare_images": 3 * luma + out_bytes}
        rate = {r: moved[r] / (ms[r]["median_ms"] * 1e-3) for r in moved}
        two = round(ms["nv12_to_rgb"]["median_ms"] + ms["prepare_images"]["median_ms"], 5)
        margin = max(ms[r]["spread_ms"] for r in ROWS[:3])
        faster = bool(ms["fused"]["median_ms"] < two - margin)
        res = dict(shape=dict(name=name, B=B, source_h=Hs, source_w=Ws, pitch=PITCH, uv_row=uv_row, output_h=Ho, output_w=Wo,
                              padded_h=Hp, padded_w=Wp, tile=TILE),
                   rows=ms, launches=n_launch, host_round_trips={r: 0 for r in ROWS}, bytes_moved=moved,
                   bytes_per_s={r: round(v, 0) for r, v in rate.items()},
                   fraction_of_hbm_peak={r: round(v / HBM_PEAK, 4) for r, v in rate.items()},
                   two_launch_sum_ms=two, margin_ms=margin, fused_below_sum_by_more_than_margin=faster,
                   fused_equals_two_launch_route_bit_for_bit=equal, torch_conversion_largest_byte_difference=byte_diff)
        results.append(res)
        lines += [f"prepare_images_nv12  {name}: B={B} surfaces of pitch {PITCH} holding {Hs}x{Ws} -> float32 CHW {Hp}x{Wp} ({Ho}x{Wo} "
                  f"before padding to {TILE}){', crop + flip' if transforms is not None else ', no matrix'}, photometric rows per sample",
                  f"  {args.blocks} blocks a row of {args.iters} windows of {args.calls} calls ({args.baseline_calls} for the torch row)"]
        for r in ROWS:
            m = ms[r]
            lines.append(f"  {r:<24} median {m['median_ms']:.4f} ms  min {m['min_ms']:.4f} ms  block medians "
                         f"{' '.join(f'{v:.4f}' for v in m['block_medians_ms'])}  spread {m['spread_ms']:.4f}  launches {n_launch[r]}  "
                         "host round trips 0")
        lines += [f"  {r:<24} moves {moved[r] / 1e6:.1f} MB = {rate[r] / 1e12:.3f} TB/s, {100 * rate[r] / HBM_PEAK:.1f} % of the 8 TB/s peak"
                  for r in moved]
        lines += [f"  fused {ms['fused']['median_ms']:.4f} ms vs nv12_to_rgb + prepare_images {two:.4f} ms, margin (largest spread of the "
                  f"three rows) {margin:.4f} ms: fused below the sum by more than the margin: {faster}",
                  f"  fused equals the two-launch route bit for bit: {equal}; the torch conversion differs from nv12_to_rgb by at most "
                  f"{byte_diff} in a byte"]
    result = dict(metric="prepare_images_nv12_ms", unit="ms", value=results[0]["rows"]["fused"]["median_ms"], warmup=args.warmup,
                  blocks=args.blocks, iters=args.iters, calls_per_window=args.calls, baseline_calls_per_window=args.baseline_calls,
                  sizes=results)
    lines.append(json.dumps(result))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
