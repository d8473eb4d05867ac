"""Which boxes of a camera batch become heat-map targets, and the targets themselves, without leaving the GPU:

    visible_bbox_mask        ragged boxes + depths -> bool mask (occlusion by nearer boxes, minimum size), ONE launch
    batched_bool_indexing    the mask compacts boxes, depths and centres (select_visible_bboxes does both steps)
    get_centers_and_radii    float centres and boxes -> integer centres and Gaussian radii at the map's stride
    draw_heatmap_batched     clear=True: the maps in a single write-only pass

`per_sample_canvas_loop` is the step it replaces, as the reference's VisibleBboxSelector runs it: per sample on the host,
an H x W int32 canvas painted from far to near and np.unique on it.  Run the file directly to see both agree.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import draw_heatmap_batched, get_centers_and_radii, select_visible_bboxes

CAMERAS, SAMPLES = 6, 2
H, W, STRIDE = 900, 1600, 4.0
MIN_SIZE = 2.0


def make_batch(device, max_boxes: int = 32, seed: int = 0):
    """B = cameras x samples frames with a ragged number of 2D boxes each (image pixels) and their depths (metres)"""
    g = torch.Generator().manual_seed(seed)
    B = CAMERAS * SAMPLES
    sizes = torch.randint(0, max_boxes + 1, (B,), generator=g)
    N = int(sizes.max())
    c = (torch.rand(B, N, 2, generator=g) * 1.2 - 0.1) * torch.tensor([float(W), float(H)])
    half = 2.0 + torch.rand(B, N, 2, generator=g) ** 3 * torch.tensor([W / 5.0, H / 5.0])
    boxes = torch.cat([c - half, c + half], -1)
    depths = 1.0 + torch.rand(B, N, generator=g) * 79.0
    sizes = sizes.to(device)
    return (RaggedBatch(boxes.to(device), sample_sizes=sizes), RaggedBatch(depths.to(device), sample_sizes=sizes),
            RaggedBatch(c.to(device), sample_sizes=sizes))


def target_step(boxes, depths, centers, heatmap):
    """the whole step on the device; returns the mask and the kept boxes"""
    mask, boxes, depths, centers = select_visible_bboxes(boxes, depths, centers, image_hw=(H, W), minimum_size=MIN_SIZE)
    c, r = get_centers_and_radii(centers, boxes, STRIDE)
    draw_heatmap_batched(heatmap, c, r, clear=True)
    return mask, boxes


def per_sample_canvas_loop(boxes, depths):
    """what the step replaces: a device -> host copy, one canvas per sample, a host -> device copy of the mask"""
    bx, dp, ns = boxes.tensor.cpu().numpy(), depths.tensor.cpu().numpy(), boxes.sample_sizes.cpu().numpy()
    out = np.zeros(dp.shape, bool)
    for b, n in enumerate(ns):
        canvas = np.full((H, W), -1, np.int32)                      # 5.8 MB per frame
        for i in np.argsort(-dp[b, :n], kind="stable"):
            x0, x1 = sorted((bx[b, i, 0], bx[b, i, 2]))
            y0, y1 = sorted((bx[b, i, 1], bx[b, i, 3]))
            x0, y0, x1, y1 = int(np.floor(x0)), int(np.floor(y0)), int(np.ceil(x1)), int(np.ceil(y1))
            if x0 > W or x1 < 0 or y0 > H or y1 < 0:
                continue
            canvas[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = i
        seen = np.unique(canvas)
        out[b, seen[seen >= 0]] = True
        cl = bx[b, :n].copy()
        cl[:, 0::2], cl[:, 1::2] = np.clip(cl[:, 0::2], 0, W), np.clip(cl[:, 1::2], 0, H)
        out[b, :n] &= (np.abs(cl[:, 2] - cl[:, 0]) >= MIN_SIZE) & (np.abs(cl[:, 3] - cl[:, 1]) >= MIN_SIZE)
    return torch.from_numpy(out).to(boxes.tensor.device)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("visible_boxes_step.py draws heat maps on a GPU; none is visible")
    device = torch.device("cuda", 0)
    boxes, depths, centers = make_batch(device)
    heatmap = torch.empty((CAMERAS * SAMPLES, int(H / STRIDE), int(W / STRIDE)), device=device)
    mask, kept = target_step(boxes, depths, centers, heatmap)
    loop = per_sample_canvas_loop(boxes, depths)
    total, stay = int(boxes.sample_sizes.sum()), int(mask.tensor.sum())
    print(f"{device}: {total} boxes in {len(boxes.sample_sizes)} frames, {stay} stay, {total - stay} dropped; "
          f"kept per frame {kept.sample_sizes.tolist()}")
    print(f"mask equals the per-sample canvas loop: {torch.equal(mask.tensor, loop)}; heat-map peak {float(heatmap.max()):.1f}")
    assert torch.equal(mask.tensor, loop)


if __name__ == "__main__":
    main()
