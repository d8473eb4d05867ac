"""The depth leg of a BEVDepth-style training step, next to the image leg it shares its matrices with:

    sample_image_transforms   one resize / crop / flip matrix per camera image
    prepare_images            warps, normalises and pads the images with it
    lidar_depth_targets       the frame's lidar points -> nearest depth and depth bin per cell of every camera's feature map,
                              through lidar2img and the SAME image matrix (image_transforms=...): ONE launch

`fused_targets` is that path; nothing in it synchronises with the host.  `composed_targets` is the torch composition of the
definition on the device that it replaces (BEVDepth does the first half per camera on the CPU in its loader:
map_pointcloud_to_image and depth_transform; the second half is get_downsampled_gt_depth): fold the matrices, a matmul, the
divide, six masks, the cell index, a scatter_reduce_("amin") over [B, C, h * w] and the bins, about two dozen launches.  With
`definition_order=True` it evaluates the projection element-wise in the operator's own operation order and is then equal
bit for bit; with the matmul a user would write, depths agree to float32 rounding.

    python3 examples/depth_targets_step.py [--samples 2] [--cameras 6] [--points 34000] [--source 900 1600] [--output 256 704]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import lidar_depth_targets

STRIDE = 16
DEPTH_RANGE = (2.0, 58.0)       # BEVDepth's d_bound = [2.0, 58.0, 0.5]
BINS = (2.0, 0.5, 112)


def make_scene(samples: int, cameras: int, points: int, source_hw, device, seed: int = 1):
    """(points RaggedBatch [B, P, 4] with ragged counts around `points`, lidar2img float32 [B, C, 4, 4]): a ring of pinhole
    cameras with nuScenes-like intrinsics around a spinning lidar"""
    g = torch.Generator().manual_seed(seed)
    H, W = source_hw
    counts = (points * (0.9 + 0.2 * torch.rand(samples, generator=g))).long()
    P = int(counts.max())
    rng, az = 2.0 + 58.0 * torch.rand(samples, P, generator=g) ** 2, 2 * math.pi * torch.rand(samples, P, generator=g)
    el = math.radians(-30.0) + math.radians(40.0) * torch.rand(samples, P, generator=g)
    xyz = torch.stack([rng * el.cos() * az.cos(), rng * el.cos() * az.sin(), rng * el.sin(), torch.rand(samples, P, generator=g)], 2)
    K = torch.tensor([[1266.0 * W / 1600, 0.0, 816.0 * W / 1600], [0.0, 1266.0 * W / 1600, 491.0 * H / 900], [0.0, 0.0, 1.0]], dtype=torch.float64)
    l2i = torch.zeros(samples, cameras, 4, 4, dtype=torch.float64)
    for b in range(samples):
        for c in range(cameras):
            yaw = 2 * math.pi * c / cameras + 0.05 * float(torch.randn((), generator=g))
            rot = torch.tensor([[math.sin(yaw), -math.cos(yaw), 0.0], [0.0, 0.0, -1.0], [math.cos(yaw), math.sin(yaw), 0.0]], dtype=torch.float64)
            t = torch.tensor([0.0, 0.3, -0.5], dtype=torch.float64) + 0.1 * torch.randn(3, generator=g).double()
            l2i[b, c, :3, :3], l2i[b, c, :3, 3], l2i[b, c, 3, 3] = K @ rot, K @ t, 1.0
    return RaggedBatch(xyz.contiguous().to(device), sample_sizes=counts.to(device)), l2i.float().to(device)


def fused_targets(points, lidar2img, matrices, image_hw, band_rows=0):
    return lidar_depth_targets(points, lidar2img, image_hw=image_hw, downsample=STRIDE, depth_range=DEPTH_RANGE, depth_bins=BINS,
                               image_transforms=matrices, _band_rows=band_rows)


def composed_targets(points, lidar2img, matrices, image_hw, definition_order=False):
    """(depth [B, C, h, w] float32, bins int32) by torch operators on the points' device, without a host round trip"""
    pts, sizes = points.tensor, points.sample_sizes
    B, P, _ = pts.shape
    C = lidar2img.shape[1]
    H, W = image_hw
    h, w = -(-H // STRIDE), -(-W // STRIDE)
    m = lidar2img[:, :, :3, :]                                                    # [B, C, 3, 4]
    a = matrices.view(B, C, 2, 3)
    if definition_order:
        row = lambda i: (a[:, :, i, 0:1] * m[:, :, 0] + a[:, :, i, 1:2] * m[:, :, 1]) + a[:, :, i, 2:3] * m[:, :, 2]     # noqa: E731
        m = torch.stack([row(0), row(1), m[:, :, 2]], 2)
        x, y, z = (pts[:, None, :, i] for i in range(3))                          # [B, 1, P]
        p = [((m[:, :, k, 0:1] * x + m[:, :, k, 1:2] * y) + m[:, :, k, 2:3] * z) + m[:, :, k, 3:4] for k in range(3)]
        d, u, v = p[2], p[0] / p[2], p[1] / p[2]
    else:
        a3 = torch.cat([a, torch.tensor([0.0, 0.0, 1.0], device=a.device).expand(B, C, 1, 3)], 2)
        m = a3 @ m
        hom = torch.cat([pts[:, :, :3], torch.ones_like(pts[:, :, :1])], 2)       # [B, P, 4]
        p = m @ hom.transpose(1, 2)[:, None]                                      # [B, C, 3, P]
        d = p[:, :, 2]
        u, v = p[:, :, 0] / d, p[:, :, 1] / d
    real = (torch.arange(P, device=pts.device)[None] < sizes[:, None])[:, None]   # [B, 1, P]
    ok = real & (d >= DEPTH_RANGE[0]) & (d < DEPTH_RANGE[1]) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    cell = (v.clamp(0, H - 1).long() // STRIDE) * w + u.clamp(0, W - 1).long() // STRIDE
    cell = torch.where(ok, cell, torch.full_like(cell, h * w))                    # what does not count goes to a spare cell
    depth = torch.full((B, C, h * w + 1), float("inf"), device=pts.device)
    depth.scatter_reduce_(2, cell, torch.where(ok, d, torch.full_like(d, float("inf"))), "amin")
    depth = depth[:, :, :h * w]
    has = depth != float("inf")
    depth = torch.where(has, depth, torch.zeros_like(depth)).view(B, C, h, w)
    t = (depth - BINS[0]) / BINS[1]
    good = has.view(B, C, h, w) & (t >= 0) & (t < BINS[2])
    bins = torch.where(good, t.clamp(0, BINS[2]).int(), torch.full_like(t, -1, dtype=torch.int32))
    return depth, bins


def image_matrices(samples, cameras, source_hw, output_hw, device, seed=0):
    from accvlab.image_prep import NonUniformScaling, UniformScaling, sample_image_transforms

    steps = [NonUniformScaling(0.5, (-1.0, 1.0)), UniformScaling(1.0, 0.94, 1.11)]    # the flip and BEVDepth's resize range
    return sample_image_transforms(samples, cameras, steps, source_hw=source_hw, output_hw=output_hw, mode="crop", anchor="bottom_or_right",
                                   generator=torch.Generator().manual_seed(seed)).view(samples, cameras, 2, 3).contiguous().to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--points", type=int, default=34000)
    ap.add_argument("--source", type=int, nargs=2, default=(900, 1600))
    ap.add_argument("--output", type=int, nargs=2, default=(256, 704))
    args = ap.parse_args()
    from accvlab.image_prep import prepare_images

    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    source_hw, output_hw = tuple(args.source), tuple(args.output)
    points, lidar2img = make_scene(args.samples, args.cameras, args.points, source_hw, dev)
    matrices = image_matrices(args.samples, args.cameras, source_hw, output_hw, dev)
    frames = args.samples * args.cameras
    images = torch.randint(0, 256, (frames, *source_hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(dev)
    batch = prepare_images(images, output_hw=output_hw, transforms=matrices.view(frames, 2, 3), mean=(123.675, 116.28, 103.53),
                           std=(58.395, 57.12, 57.375))
    got = fused_targets(points, lidar2img, matrices, output_hw)
    exact = composed_targets(points, lidar2img, matrices, output_hw, definition_order=True)
    loose = composed_targets(points, lidar2img, matrices, output_hw)
    print(f"images {tuple(batch.shape)}, depth {tuple(got.depth.shape)}, bins {tuple(got.bins.shape)}")
    for b in range(args.samples):
        filled = (got.depth[b] != 0).sum(dim=(1, 2)).tolist()
        print(f"sample {b}: {int(points.sample_sizes[b])} points, filled cells per camera {filled}")
    print(f"against the composition in the definition's order: depth equal {bool(torch.equal(got.depth, exact[0]))}, bins equal "
          f"{bool(torch.equal(got.bins, exact[1]))}")
    print(f"against the matmul composition: {int(((got.depth != 0) != (loose[0] != 0)).sum())} cells filled on one side only, "
          f"largest depth difference {float((got.depth - loose[0]).abs().max()):.2e}, {int((got.bins != loose[1]).sum())} bins differ")
    one_hot = torch.nn.functional.one_hot(got.bins.long() + 1, BINS[2] + 1)[..., 1:]          # BEVDepth's target
    print(f"one-hot target {tuple(one_hot.shape)}, {int(one_hot.sum())} supervised cells")


if __name__ == "__main__":
    main()
