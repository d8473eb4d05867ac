#!/usr/bin/env python3
"""The image side of a StreamPETR-style camera pipeline in one call: a decoder-shaped uint8 batch (samples x cameras of
H x W x 3) -> resize / crop by `output_size_transform`, a horizontal flip for half of the samples, the photometric
augmentation shared by the cameras of a sample, mean / std normalisation and padding to multiples of 32
(`accvlab.image_prep.prepare_images`), next to the torch composition it replaces: `to(float)`, `permute`, `affine_grid` +
`grid_sample`, the colour chain in tensor operations, normalise, `F.pad`.

    python3 examples/image_prep_step.py [--samples 2] [--cameras 6] [--source 900 1600] [--output 256 704] [--cpu]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
RANGES = dict(min_max_brightness=(-32.0, 32.0), min_max_hue=(-18.0, 18.0), min_max_contrast=(0.5, 1.5),
              min_max_saturation=(0.5, 1.5))


def step_parameters(samples, cameras, source_hw, output_hw, seed=0):
    """CPU tensors: the forward matrices [B, 2, 3] (resize / crop about the centre, every second sample flipped in x) and
    the photometric rows [B, 6], one draw per sample"""
    from accvlab.image_prep import output_size_transform, sample_photometric_params

    resize = torch.tensor(output_size_transform(source_hw, output_hw, "crop", "center") + [[0.0, 0.0, 1.0]], dtype=torch.float64)
    flip = torch.tensor([[-1.0, 0.0, float(output_hw[1])], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    per_sample = [(flip @ resize if s % 2 else resize)[:2] for s in range(samples)]
    transforms = torch.stack(per_sample).repeat_interleave(cameras, dim=0).to(torch.float32).contiguous()
    photometric = sample_photometric_params(samples, cameras, generator=torch.Generator().manual_seed(seed), **RANGES)
    return transforms, photometric


def torch_composition(images, transforms, photometric, output_hw, *, is_bgr=False, mean=MEAN, std=STD, tile_hw=32):
    """What a user writes without the fused operator; every line is at least one pass over a float image.  `transforms` and
    `photometric` may be None.  Padding comes before the normalisation, as in the StreamPETR pipeline."""
    B, Hs, Ws, _ = images.shape
    dev = images.device
    x = images.to(torch.float32).permute(0, 3, 1, 2)                     # [B, 3, Hs, Ws]
    if transforms is not None:
        Ho, Wo = output_hw
        fwd = torch.zeros((B, 3, 3), dtype=torch.float64, device=dev)
        fwd[:, :2], fwd[:, 2, 2] = transforms.double(), 1.0
        inv = torch.linalg.inv(fwd)                                      # output -> source, pixel-centre coordinates
        # affine_grid works on coordinates normalised to [-1, 1] over the extent (align_corners=False)
        to_px = torch.tensor([[Wo / 2, 0, Wo / 2], [0, Ho / 2, Ho / 2], [0, 0, 1]], dtype=torch.float64, device=dev)
        to_norm = torch.tensor([[2 / Ws, 0, -1], [0, 2 / Hs, -1], [0, 0, 1]], dtype=torch.float64, device=dev)
        theta = (to_norm @ inv @ to_px)[:, :2].to(torch.float32)
        grid = F.affine_grid(theta, (B, 3, Ho, Wo), align_corners=False)
        x = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    v = x / 255.0
    if photometric is not None:
        col = lambda i: photometric[:, i].view(B, 1, 1)                  # noqa: E731
        v = (v + col(0).unsqueeze(1)).clamp(0, 1)
        v = (v * col(1).unsqueeze(1)).clamp(0, 1)
        r, g, b = (v[:, 2], v[:, 1], v[:, 0]) if is_bgr else (v[:, 0], v[:, 1], v[:, 2])
        mx, mn = torch.maximum(torch.maximum(r, g), b), torch.minimum(torch.minimum(r, g), b)
        dc = mx - mn
        safe = torch.where(dc > 0, dc, torch.ones_like(dc))
        h = torch.where(mx == r, (g - b) / safe, torch.where(mx == g, 2 + (b - r) / safe, 4 + (r - g) / safe))
        h = torch.where(dc > 0, h, torch.zeros_like(h))
        s = torch.where(dc > 0, dc / torch.where(mx > 0, mx, torch.ones_like(mx)), torch.zeros_like(dc)) * col(2)
        h = h + col(3) / 60.0
        chan = lambda n: mx - mx * s * torch.minimum(torch.minimum((n + h) % 6, 4 - (n + h) % 6), torch.ones_like(h)).clamp(min=0)   # noqa: E731
        r, g, b = chan(5.0), chan(3.0), chan(1.0)
        v = torch.stack((b, g, r) if is_bgr else (r, g, b), dim=1)
        v = (v * col(4).unsqueeze(1)).clamp(0, 1)
        from accvlab.image_prep import CHANNEL_PERMUTATIONS

        table = torch.tensor(CHANNEL_PERMUTATIONS, device=dev)
        index = photometric[:, 5].long()
        index = torch.where((index >= 0) & (index <= 5) & (photometric[:, 5] == index), index, torch.zeros_like(index))
        v = torch.gather(v, 1, table[index].view(B, 3, 1, 1).expand(-1, -1, v.shape[2], v.shape[3]))
    v = v.clamp(0, 1) * 255.0
    th, tw = (tile_hw, tile_hw) if isinstance(tile_hw, int) else tile_hw
    H, W = v.shape[2:]
    v = F.pad(v, (0, -W % tw, 0, -H % th), value=0.0)
    mean_t = torch.tensor(mean, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    return ((v - mean_t) / std_t).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--source", type=int, nargs=2, default=(900, 1600))
    ap.add_argument("--output", type=int, nargs=2, default=(256, 704))
    ap.add_argument("--cpu", action="store_true", help="run the library's host entry instead of the kernel")
    args = ap.parse_args()
    from accvlab.image_prep import prepare_images

    dev = torch.device("cpu" if args.cpu else "cuda")
    source_hw, output_hw = tuple(args.source), tuple(args.output)
    B = args.samples * args.cameras
    images = torch.randint(0, 256, (B, *source_hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    transforms, photometric = step_parameters(args.samples, args.cameras, source_hw, output_hw)
    transforms, photometric = transforms.to(dev), photometric.to(dev)

    fused = prepare_images(images, output_hw=output_hw, transforms=transforms, photometric=photometric, mean=MEAN, std=STD,
                           tile_hw=32)
    composed = torch_composition(images, transforms, photometric, output_hw)
    diff = float((fused - composed).abs().max())
    print(f"{B} images of {source_hw[0]}x{source_hw[1]} -> {tuple(fused.shape)} {fused.dtype} on {dev}")
    print(f"largest difference between the fused call and the torch composition: {diff:.2e} "
          "(float32 sample positions computed two ways; see scripts/bench_image_prep.py for the bar)")
    half = prepare_images(images, output_hw=output_hw, transforms=transforms, photometric=photometric, mean=MEAN, std=STD,
                          tile_hw=32, layout="HWC", dtype=torch.bfloat16)
    print(f"channels-last bf16 for a half-precision backbone: {tuple(half.shape)} {half.dtype}")


if __name__ == "__main__":
    main()
