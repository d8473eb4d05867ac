#!/usr/bin/env python3
"""The camera leg of a StreamPETR-style pipeline between the decoder and the data combiner, every step native and without a
host round trip: `sample_image_transforms` draws one flip / scale / align-bottom matrix per sample, `prepare_images` warps,
normalises and pads the images with it, `camera_augment_boxes` moves the 2D annotations and the projection matrices with
the same matrix, drops what is hidden, too small or not annotated, compacts and crops, and `boxes_to_heatmap` turns the
result into CenterNet-style targets.

    python3 examples/camera_boxes_step.py [--samples 2] [--cameras 6] [--source 900 1600] [--output 256 704] [--cpu]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def annotations(frames, g_max, source_hw, seed=1):
    """ragged 2D ground truth of `frames` camera images: boxes, their centres, depths and categories (-1: not annotated)"""
    from accvlab.batching_helpers import RaggedBatch

    g = torch.Generator().manual_seed(seed)
    H, W = source_hw
    sizes = torch.randint(1, g_max + 1, (frames,), generator=g)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    cx, cy = u(frames, g_max) * W, u(frames, g_max) * H
    w, h = 8 + u(frames, g_max) ** 2 * W / 3, 8 + u(frames, g_max) ** 2 * H / 3
    boxes = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).contiguous()
    cats = torch.randint(-1, 10, (frames, g_max), generator=g)
    return RaggedBatch(boxes, sample_sizes=sizes), torch.stack([cx, cy], -1).contiguous(), 1 + u(frames, g_max) * 60, cats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--source", type=int, nargs=2, default=(900, 1600))
    ap.add_argument("--output", type=int, nargs=2, default=(256, 704))
    ap.add_argument("--cpu", action="store_true", help="run the library's host entries instead of the kernels")
    args = ap.parse_args()
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import boxes_to_heatmap, camera_augment_boxes
    from accvlab.image_prep import (NonUniformScaling, ShiftToAlignWithOriginalImageBorder, UniformScaling, padded_hw,
                                    prepare_images, sample_image_transforms)

    dev = torch.device("cpu" if args.cpu else "cuda")
    source_hw, output_hw = tuple(args.source), tuple(args.output)
    frames = args.samples * args.cameras
    steps = [NonUniformScaling(0.5, (-1.0, 1.0)),                       # the horizontal flip
             UniformScaling(1.0, 0.9, 1.1), ShiftToAlignWithOriginalImageBorder(1.0, "bottom")]
    transforms = sample_image_transforms(args.samples, args.cameras, steps, source_hw=source_hw, output_hw=output_hw, mode="crop",
                                         anchor="bottom_or_right", generator=torch.Generator().manual_seed(0)).to(dev)

    images = torch.randint(0, 256, (frames, *source_hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    prepared = prepare_images(images, output_hw=output_hw, transforms=transforms, mean=MEAN, std=STD, tile_hw=32)
    hw = padded_hw(output_hw, 32)                                       # what the selector and the croppers see

    boxes, centers, depths, cats = annotations(frames, 40, source_hw)
    boxes = RaggedBatch(boxes.tensor.to(dev), sample_sizes=boxes.sample_sizes.to(dev))
    lidar2img = torch.eye(4).repeat(frames, 1, 1).to(dev)
    out = camera_augment_boxes(boxes, transforms, image_hw=hw, centers=centers.to(dev), depths=depths.to(dev),
                               categories=cats.to(dev), minimum_size=2, projection_matrices=(lidar2img,))
    targets = boxes_to_heatmap(out.bboxes, centers=out.centers, categories=out.categories, image_hw=hw,
                               heatmap_hw=(hw[0] // 16, hw[1] // 16), num_categories=10)
    print(f"{frames} images of {source_hw[0]}x{source_hw[1]} -> {tuple(prepared.shape)} on {dev}")
    print(f"{int(boxes.sample_sizes.sum())} boxes, {int(out.visible.tensor.sum())} visible, {int(out.bboxes.sample_sizes.sum())} kept "
          f"(per frame {out.bboxes.sample_sizes.tolist()}); first kept box of frame 0 came from slot {int(out.source.tensor[0, 0])}")
    print(f"lidar2img row 0 of frame 0 after the warp: {[round(v, 3) for v in out.projection_matrices[0][0, 0].tolist()]}")
    print(f"heat maps {tuple(targets.heatmap.shape)}, {int(targets.is_active.tensor.sum())} active objects")


if __name__ == "__main__":
    main()
