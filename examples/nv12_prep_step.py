#!/usr/bin/env python3
"""The entry of the camera leg for decoder surfaces: NV12 surfaces `[B, rows, pitch]`, as a hardware video or JPEG decoder
hands them out, -> `nv12_planes` -> `prepare_images_nv12` (one launch, the RGB batch never exists), next to the conversion
as a step of its own followed by `prepare_images` (two launches, bit-equal to the fused call) and next to the torch
composition a user would write without either: chroma upsampling, float matrix products, round and clamp, then the
composition of examples/image_prep_step.py.

    python3 examples/nv12_prep_step.py [--samples 2] [--cameras 6] [--source 900 1600] [--pitch 1664] [--output 256 704] [--cpu]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd"), os.path.join(ROOT, "examples")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from image_prep_step import MEAN, STD, step_parameters, torch_composition  # noqa: E402


def random_surfaces(B, source_hw, pitch, seed=1, aligned_rows=None):
    """uint8 [B, rows, pitch]: the luma rows (height rounded up to `aligned_rows` when given), then the UV rows; returns the
    surfaces and the row the UV plane starts at"""
    H, W = source_hw
    uv_row = H if aligned_rows is None else -(-H // aligned_rows) * aligned_rows
    rows = uv_row + (H + 1) // 2
    s = torch.randint(0, 256, (B, rows, pitch), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    return s, uv_row


def torch_nv12_to_rgb(y, uv):
    """What a user writes today for limited-range BT.601: nearest chroma upsampling, a float matrix product, round and clamp.
    It materialises float planes and the uint8 RGB batch; it rounds differently from the integer arithmetic of
    `nv12_to_rgb`, so its bytes can differ by one."""
    B, H, W = y.shape
    up = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W].to(torch.float32)
    yy = (y.to(torch.float32) - 16.0).clamp(min=0.0) * (1220542 / 2 ** 20)
    uu, vv = up[..., 0] - 128.0, up[..., 1] - 128.0
    m = torch.tensor([[0.0, 1673527.0], [-409993.0, -852492.0], [2116026.0, 0.0]], device=y.device) / 2 ** 20
    rgb = yy.unsqueeze(-1) + torch.stack((uu, vv), dim=-1) @ m.T
    return rgb.round().clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--source", type=int, nargs=2, default=(900, 1600))
    ap.add_argument("--pitch", type=int, default=1664)
    ap.add_argument("--output", type=int, nargs=2, default=(256, 704))
    ap.add_argument("--cpu", action="store_true", help="run the library's host entries instead of the kernels")
    args = ap.parse_args()
    from accvlab.image_prep import nv12_planes, nv12_to_rgb, prepare_images, prepare_images_nv12

    dev = torch.device("cpu" if args.cpu else "cuda")
    source_hw, output_hw = tuple(args.source), tuple(args.output)
    B = args.samples * args.cameras
    surfaces, uv_row = random_surfaces(B, source_hw, args.pitch, aligned_rows=16)
    y, uv = nv12_planes(surfaces.to(dev), source_hw, uv_row=uv_row)       # views: nothing is copied
    transforms, photometric = (t.to(dev) for t in step_parameters(args.samples, args.cameras, source_hw, output_hw))
    kw = dict(output_hw=output_hw, transforms=transforms, photometric=photometric, mean=MEAN, std=STD, tile_hw=32)

    fused = prepare_images_nv12(y, uv, **kw)
    two_steps = prepare_images(nv12_to_rgb(y, uv), **kw)
    print(f"{B} surfaces of {tuple(surfaces.shape[1:])} bytes (pitch {args.pitch}, UV from row {uv_row}) holding "
          f"{source_hw[0]}x{source_hw[1]} -> {tuple(fused.shape)} {fused.dtype} on {dev}")
    print(f"prepare_images_nv12 equals nv12_to_rgb + prepare_images bit for bit: {torch.equal(fused, two_steps)}")
    composed = torch_composition(torch_nv12_to_rgb(y, uv), transforms, photometric, output_hw)
    print(f"largest difference to the torch composition: {float((fused - composed).abs().max()):.2e} (its float conversion "
          "rounds a byte differently here and there, and its sample positions are computed another way)")
    half = prepare_images_nv12(y, uv, layout="HWC", dtype=torch.bfloat16, **kw)
    print(f"channels-last bf16 for a half-precision backbone: {tuple(half.shape)} {half.dtype}")


if __name__ == "__main__":
    main()
