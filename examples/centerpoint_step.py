"""The target side and the loss of one CenterPoint training step, from raw ragged ground-truth 3D boxes:

    center_point_targets    boxes, labels -> centres, radii, in-task labels, regression targets of every task: ONE launch
    draw_heatmap_batched    class-wise Gaussian targets per task (fused clear + draw)
    gaussian_focal_loss     heat-map term
    center_regression_loss  regression term at the object centres

`fused_step` is that path.  `loop_step` is the same step with the target side written as the per-object loop it replaces
(mmdet3d's CenterHead.get_targets_single: frames x tasks x objects in Python, numpy float32 scalars), feeding the same
draw and loss operators.  Both print the same losses.

    python3 examples/centerpoint_step.py
"""
from __future__ import annotations

import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import center_point_targets, center_regression_loss, draw_heatmap_batched, gaussian_focal_loss

TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))            # the six nuScenes tasks over ten classes
CFG = dict(pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0], out_size_factor=4, grid_size=(128, 128),
           gaussian_overlap=0.1, min_radius=2, max_objs=500, norm_bbox=True)


def make_batch(batch: int, max_objects: int, device, seed: int = 0):
    """synthetic ground truth: (x, y, z, dx, dy, dz, yaw, vx, vy) and a class per object, ragged over the frames"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, max_objects + 1, (batch,), generator=g)
    n = max(int(sizes.max()), 1)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    boxes = torch.cat([(u(batch, n, 2) * 1.1 - 0.55) * 102.4, u(batch, n, 1) * 8 - 5, 0.5 + u(batch, n, 3) * 9.5,
                       (u(batch, n, 1) * 2 - 1) * math.pi, u(batch, n, 2) * 10 - 5], -1).contiguous()
    labels = torch.randint(0, 10, (batch, n), generator=g)
    return (RaggedBatch(boxes.to(device), sample_sizes=sizes.to(device)), RaggedBatch(labels.to(device), sample_sizes=sizes.to(device)))


def make_heads(batch: int, device, seed: int = 1):
    """what the network would predict: per task the heat-map logits and the five regression heads (reg, height, dim, rot, vel)"""
    g = torch.Generator().manual_seed(seed)
    w, h = CFG["grid_size"]
    heads = []
    for ids in TASKS:
        logits = (torch.randn(batch, len(ids), h, w, generator=g) - 2.0).to(device)
        regression = [torch.randn(batch, c, h, w, generator=g).to(device) for c in (2, 1, 3, 2, 2)]
        heads.append((logits, regression))
    return heads


def losses(targets, heads):
    """draw + heat-map loss + regression loss per task, from the targets of either path"""
    heat, reg = [], []
    for r, (logits, regression) in zip(targets, heads):
        hm = torch.empty_like(logits)
        draw_heatmap_batched(hm, r.centers, r.radii, labels=r.labels, clear=True)
        heat.append(gaussian_focal_loss(logits, hm))
        reg.append(center_regression_loss(regression, r.centers, r.targets))
    return torch.stack(heat), torch.stack(reg)


def fused_step(boxes, labels, heads):
    return losses(center_point_targets(boxes, labels, TASKS, **CFG), heads)


def gaussian_radius(height, width, m):
    f = np.float32
    b1 = height + width
    r1 = (b1 + np.sqrt(b1 * b1 - f(4) * (width * height * (f(1) - m) / (f(1) + m)))) / f(2)
    b2 = f(2) * b1
    r2 = (b2 + np.sqrt(b2 * b2 - f(16) * ((f(1) - m) * width * height))) / f(2)
    b3 = f(-2) * m * b1
    r3 = (b3 + np.sqrt(b3 * b3 - f(4) * (f(4) * m) * ((m - f(1)) * width * height))) / f(2)
    return min(r1, r2, r3)


def loop_targets(boxes, labels):
    """get_targets_single, per frame, task and object; the tensors a user would then stack and copy to the device"""
    from accvlab.draw_heatmap import CenterPointTargets

    f = np.float32
    dev = boxes.tensor.device
    bx, lb, sizes = boxes.tensor.cpu().numpy(), labels.tensor.cpu().numpy(), boxes.sample_sizes.cpu().tolist()
    batch, n, _ = bx.shape
    m_slots = min(CFG["max_objs"], n)
    w_map, h_map = CFG["grid_size"]
    pc, vs, stride, m = CFG["pc_range"], CFG["voxel_size"], f(CFG["out_size_factor"]), f(CFG["gaussian_overlap"])
    out = []
    for ids in TASKS:
        centers = np.zeros((batch, m_slots, 2), np.int32)
        radii = np.zeros((batch, m_slots), np.int32)
        cls = np.zeros((batch, m_slots), np.int32)
        rows = np.zeros((batch, m_slots, 10), np.float32)
        ind = np.zeros((batch, m_slots), np.int64)
        src = np.full((batch, m_slots), -1, np.int32)
        kept = np.zeros((batch,), np.int64)
        for b in range(batch):
            mine = [i for i in range(sizes[b]) if lb[b, i] in ids][:CFG["max_objs"]]
            k = 0
            for i in mine:
                x, y, z, dx, dy, dz, yaw, vx, vy = bx[b, i]
                width, length = dx / f(vs[0]) / stride, dy / f(vs[1]) / stride
                cx, cy = (x - f(pc[0])) / f(vs[0]) / stride, (y - f(pc[1])) / f(vs[1]) / stride
                if not (width > 0 and length > 0 and -1 < cx < w_map and -1 < cy < h_map):
                    continue
                ix, iy = int(cx), int(cy)
                centers[b, k], radii[b, k] = (ix, iy), max(CFG["min_radius"], int(gaussian_radius(length, width, m)))
                cls[b, k], ind[b, k], src[b, k] = ids.index(lb[b, i]), iy * w_map + ix, i
                rows[b, k] = [cx - f(ix), cy - f(iy), z, math.log(dx), math.log(dy), math.log(dz), math.sin(yaw), math.cos(yaw), vx, vy]
                k += 1
            kept[b] = k
        sizes_t = torch.from_numpy(kept).to(dev)
        out.append(CenterPointTargets(*(RaggedBatch(torch.from_numpy(a).to(dev), sample_sizes=sizes_t)
                                        for a in (centers, radii, cls, rows, ind, src))))
    return out


def loop_step(boxes, labels, heads):
    return losses(loop_targets(boxes, labels), heads)


if __name__ == "__main__":
    device = torch.device("cuda", 0)
    boxes, labels = make_batch(4, 60, device)
    heads = make_heads(4, device)
    for name, step in (("fused", fused_step), ("loop", loop_step)):
        heat, reg = step(boxes, labels, heads)
        print(f"{name:5s}  heat-map loss per task {[round(v, 5) for v in heat.tolist()]}  regression loss per task "
              f"{[round(v, 5) for v in reg.tolist()]}")
