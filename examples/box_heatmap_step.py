"""The 2D target step of a CenterNet-style camera head, and its losses, without leaving the GPU:

    select_visible_bboxes    ragged boxes + depths -> the boxes that stay (occlusion, minimum size), compacted
    boxes_to_heatmap         the kept boxes -> per-category Gaussian maps, is_active, integer centres, sub-pixel offsets,
                             clipped sizes and boxes, float radii, ONE launch
    gaussian_focal_loss      the head's heat-map logits against the maps
    center_regression_loss   the head's offset and size maps at `center` against `center_offset` and `height_width`,
                             weighted by `is_active` (gather_at_centers reads the same cells)

`per_sample_numpy_loop` is the step boxes_to_heatmap replaces, as the reference's BoundingBoxToHeatmapConverter runs it: per
sample on the host, scaling, clipping, the active decision and a Gaussian per object painted into the map.  Run the file
directly to see both agree.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import (boxes_to_heatmap, center_regression_loss, gather_at_centers, gaussian_focal_loss,
                                  select_visible_bboxes)

CAMERAS, SAMPLES = 6, 2
H, W = 900, 1600
MAP_H, MAP_W, CLASSES = 112, 200, 10
MIN_SIZE = 2.0
STEP = dict(num_categories=CLASSES, min_object_size=(1.0, 1.0), radius_scaling_factor=0.8)

F = np.float32


def make_batch(device, max_boxes: int = 32, seed: int = 0):
    """B = cameras x samples frames with a ragged number of 2D boxes each (image pixels), depths (metres) and categories"""
    g = torch.Generator().manual_seed(seed)
    B = CAMERAS * SAMPLES
    sizes = torch.randint(0, max_boxes + 1, (B,), generator=g)
    N = int(sizes.max())
    c = (torch.rand(B, N, 2, generator=g) * 1.2 - 0.1) * torch.tensor([float(W), float(H)])
    half = 2.0 + torch.rand(B, N, 2, generator=g) ** 3 * torch.tensor([W / 5.0, H / 5.0])
    boxes = torch.cat([c - half, c + half], -1)
    depths = 1.0 + torch.rand(B, N, generator=g) * 79.0
    cats = torch.randint(0, CLASSES, (B, N), generator=g)
    sizes = sizes.to(device)
    return tuple(RaggedBatch(t.to(device), sample_sizes=sizes) for t in (boxes, depths, cats))


def target_step(boxes, depths, cats):
    """the whole target step on the device"""
    _, boxes, depths, cats = select_visible_bboxes(boxes, depths, cats, image_hw=(H, W), minimum_size=MIN_SIZE)
    return boxes, cats, boxes_to_heatmap(boxes, image_hw=(H, W), heatmap_hw=(MAP_H, MAP_W), categories=cats, **STEP)


def losses(head, targets):
    """head: dict of the raw outputs `heat` [B, C, h, w], `offset` [B, 2, h, w], `size` [B, 2, h, w]"""
    weights = targets.is_active.tensor.to(torch.float32)
    num_pos = weights.sum().clamp(min=1.0)
    heat = gaussian_focal_loss(head["heat"], targets.heatmap, avg_factor=num_pos)
    regression = torch.cat([targets.center_offset.tensor, targets.height_width.tensor], -1)      # (ox, oy, h, w)
    reg = center_regression_loss([head["offset"], head["size"]], targets.center, regression, weights, avg_factor=num_pos)
    return heat, reg


def per_sample_numpy_loop(boxes, cats):
    """what boxes_to_heatmap replaces: a device -> host copy and one pass per sample and object on the host"""
    bx, ct, ns = boxes.tensor.cpu().numpy(), cats.tensor.cpu().numpy(), boxes.sample_sizes.cpu().numpy()
    B, N = ct.shape
    hm = np.zeros((B, CLASSES, MAP_H, MAP_W), F)
    active, center = np.zeros((B, N), bool), np.zeros((B, N, 2), np.int32)
    offset, hw = np.zeros((B, N, 2), F), np.zeros((B, N, 2), F)
    sx, sy, xm, ym = F(MAP_W) / F(W), F(MAP_H) / F(H), F(MAP_W - 1), F(MAP_H - 1)
    for b, n in enumerate(ns):
        for i in range(n):
            x1, y1, x2, y2 = bx[b, i]
            X1, Y1, X2, Y2 = sx * x1, sy * y1, sx * x2, sy * y2
            CX, CY = sx * ((x1 + x2) / F(2)), sy * ((y1 + y2) / F(2))
            a, c, e, d = np.clip(X1, 0, xm), np.clip(Y1, 0, ym), np.clip(X2, 0, xm), np.clip(Y2, 0, ym)
            h, w = abs(d - c), abs(e - a)
            cx, cy = np.clip(CX, 0, xm), np.clip(CY, 0, ym)
            ix, iy = int(np.floor(cx)), int(np.floor(cy))
            center[b, i], offset[b, i], hw[b, i] = (ix, iy), (cx - F(ix), cy - F(iy)), (h, w)
            with np.errstate(all="ignore"):
                fraction = (h * w) / (abs(Y2 - Y1) * abs(X2 - X1))
            active[b, i] = fraction >= F(0.25) and h >= STEP["min_object_size"][0] and w >= STEP["min_object_size"][1]
            if not active[b, i]:
                continue
            dist = max(F(0), min(cx - min(a, e), cy - min(c, d), max(a, e) - cx, max(c, d) - cy))
            radius = min(max(dist * F(STEP["radius_scaling_factor"]), F(0.5)), F(10.0))
            R, sigma = int(np.ceil(radius)), float(radius) * float(F(1.0 / 3.0))
            ya, yb, xa, xb = max(iy - R, 0), min(iy + R, MAP_H - 1), max(ix - R, 0), min(ix + R, MAP_W - 1)
            yy, xx = np.ogrid[ya:yb + 1, xa:xb + 1]
            g = np.exp(-((yy - iy) ** 2 + (xx - ix) ** 2) / (2.0 * sigma * sigma))
            view = hm[b, ct[b, i], ya:yb + 1, xa:xb + 1]
            np.maximum(view, g, out=view)
    return hm, active, center, offset, hw


def main():
    if not torch.cuda.is_available():
        raise SystemExit("box_heatmap_step.py draws heat maps on a GPU; none is visible")
    device = torch.device("cuda", 0)
    boxes, cats, t = target_step(*make_batch(device))
    B = len(boxes.sample_sizes)
    g = torch.Generator().manual_seed(1)
    head = {k: torch.randn((B, c, MAP_H, MAP_W), generator=g).to(device).requires_grad_() for k, c in
            (("heat", CLASSES), ("offset", 2), ("size", 2))}
    heat, reg = losses(head, t)
    (heat + reg).backward()
    heat, reg = heat.detach(), reg.detach()
    at = gather_at_centers([head["offset"].detach(), head["size"].detach()], t.center)
    hm, active, center, offset, hw = per_sample_numpy_loop(boxes, cats)
    same = (np.array_equal(t.is_active.tensor.cpu().numpy(), active) and np.array_equal(t.center.tensor.cpu().numpy(), center)
            and np.array_equal(t.center_offset.tensor.cpu().numpy(), offset)
            and np.array_equal(t.height_width.tensor.cpu().numpy(), hw))
    err = float(np.abs(t.heatmap.cpu().numpy() - hm).max())
    total, drawn = int(boxes.sample_sizes.sum()), int(t.is_active.tensor.sum())
    print(f"{device}: {total} visible boxes in {B} frames, {drawn} drawn on {CLASSES} planes of {MAP_H}x{MAP_W}; "
          f"focal loss {float(heat):.4f}, regression loss {float(reg):.4f}, gathered rows {tuple(at.tensor.shape)}, "
          f"gradients finite: {all(bool(torch.isfinite(v.grad).all()) for v in head.values())}")
    print(f"per-object targets equal the per-sample numpy loop: {same}; largest map difference {err:.2e}")
    assert same and err <= 1e-5


if __name__ == "__main__":
    main()
