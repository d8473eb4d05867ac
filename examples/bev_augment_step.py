"""The 3D side of a target step, from the raw sample data to the centre-point targets, without leaving the GPU:

    sample_bev_augmentation  one (angle, scale, translation) per sample -> parameter rows [B, 7]
    bev_augment_boxes        raw ragged boxes + labels + the camera and ego matrices -> rotated, scaled and translated
                             boxes, range-filtered and compacted, and the matrices of the augmented frame, ONE launch
    center_point_targets     the kept boxes -> centres, radii, labels and regression targets of every task, ONE launch

`per_sample_loop` is what it replaces, as the reference's BEVBBoxesTransformer3D, PointsInRangeCheck and
ConditionalElementRemover run it: per sample on the host, one 4 x 4 matrix product per field and step.  Run the file
directly to see both agree.
"""
from __future__ import annotations

import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import bev_augment_boxes, center_point_targets, sample_bev_augmentation

SAMPLES, CAMERAS = 8, 6
RANGE = ((-51.2, -51.2, -5.0), (51.2, 51.2, 3.0))
TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))
HEAD = dict(pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0], out_size_factor=8, grid_size=(64, 64))


def make_batch(device, max_boxes: int = 96, seed: int = 0):
    """ragged 3D boxes (x, y, z, dx, dy, dz, yaw, vx, vy) with labels and a lidar-point count per box, lidar2img
    [B, cameras, 4, 4] and ego_to_world / world_to_ego [B, 1, 4, 4]"""
    g = torch.Generator().manual_seed(seed)
    B = SAMPLES
    sizes = torch.randint(1, max_boxes + 1, (B,), generator=g)
    N = int(sizes.max())
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    boxes = torch.cat([(u(B, N, 2) * 2 - 1) * 70.0, u(B, N, 1) * 10 - 6, 0.5 + u(B, N, 3) * 8, (u(B, N, 1) * 2 - 1) * math.pi,
                       u(B, N, 2) * 10 - 5], -1)
    labels = torch.randint(0, 10, (B, N), generator=g)
    lidar_points = torch.randint(0, 20, (B, N), generator=g)

    def poses(K, spread):
        q, _ = torch.linalg.qr(torch.randn(B, K, 3, 3, generator=g, dtype=torch.float64))
        m = torch.zeros(B, K, 4, 4, dtype=torch.float64)
        m[..., :3, :3], m[..., 3, 3] = q, 1.0
        m[..., :3, 3] = (u(B, K, 3).double() * 2 - 1) * spread
        return m

    ego = poses(1, 1500.0)
    intrinsics = torch.tensor([[1260.0, 0, 800, 0], [0, 1260.0, 450, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    mats = [(intrinsics @ poses(CAMERAS, 2.0)).float(), ego.float(), torch.linalg.inv(ego).float()]
    sizes = sizes.to(device)
    return (RaggedBatch(boxes.float().contiguous().to(device), sample_sizes=sizes), RaggedBatch(labels.to(device), sample_sizes=sizes),
            lidar_points.to(device), [m.contiguous().to(device) for m in mats])


def target_step(boxes, labels, lidar_points, mats, rows):
    """the whole step on the device: no host round trip between the raw boxes and the targets"""
    lidar2img, ego_to_world, world_to_ego = mats
    aug = bev_augment_boxes(boxes, rows, labels=labels, valid=(lidar_points >= 1) & (labels.tensor >= 0), point_range=RANGE,
                            point_transforms=(lidar2img, ego_to_world), frame_transforms=(world_to_ego,))
    return aug, center_point_targets(aug.boxes, aug.labels, TASKS, **HEAD)


def per_sample_loop(boxes, labels, lidar_points, mats, rows):
    """what the step replaces: a device -> host copy, per sample three matrix steps per field, the range check on the
    raw centres and the removal of the inactive objects; float64, so it also says how exact the fused step is"""
    bx, lb, lp = boxes.tensor.double().cpu().numpy(), labels.tensor.cpu().numpy(), lidar_points.cpu().numpy()
    ms = [m.double().cpu().numpy() for m in mats]
    out = []
    for b, n in enumerate(boxes.sample_sizes.cpu().numpy()):
        th, _, _, k, tx, ty, tz = rows[b].double().cpu().numpy()
        R = np.array([[math.cos(th), -math.sin(th), 0, 0], [math.sin(th), math.cos(th), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        S, T = np.diag([k, k, k, 1.0]), np.eye(4)
        T[:3, 3] = (tx, ty, tz)
        o = bx[b, :n]
        active = (lp[b, :n] >= 1) & (lb[b, :n] >= 0) & np.all((o[:, :3] >= RANGE[0]) & (o[:, :3] <= RANGE[1]), 1)
        p = np.concatenate([o[:, :3], np.ones((n, 1))], 1).T
        for M in (R, S, T):                                           # one apply_matrix per step
            p = M @ p
        v = S @ R @ np.concatenate([o[:, 7:9], np.zeros((n, 2))], 1).T
        yaw = (o[:, 6] + th + math.pi) % (2 * math.pi) - math.pi
        new = np.concatenate([p[:3].T, o[:, 3:6] * k, yaw[:, None], v[:2].T], 1)
        A = T @ S @ R
        out.append((new[active], lb[b, :n][active], ms[0][b] @ np.linalg.inv(A), ms[1][b] @ np.linalg.inv(A), A @ ms[2][b]))
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bev_augment_step.py runs its target step on a GPU; none is visible")
    device = torch.device("cuda", 0)
    boxes, labels, lidar_points, mats = make_batch(device)
    rows = sample_bev_augmentation(SAMPLES, (-0.3925, 0.3925), (0.95, 1.05), (0.5, 0.5, 0.5),
                                   generator=torch.Generator(device=device).manual_seed(1))
    aug, targets = target_step(boxes, labels, lidar_points, mats, rows)
    loop = per_sample_loop(boxes, labels, lidar_points, mats, rows)
    kept = aug.boxes.sample_sizes.tolist()
    worst = 0.0
    for b, (bx, lb, l2i, e2w, w2e) in enumerate(loop):
        assert kept[b] == len(bx) and aug.labels.tensor[b, :kept[b]].tolist() == lb.tolist()
        diff = np.abs(aug.boxes.tensor[b, :kept[b]].double().cpu().numpy() - bx)
        diff[:, 6] = np.minimum(diff[:, 6], np.abs(diff[:, 6] - 2 * math.pi))
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
        for got, want in ((aug.point_transforms[0][b], l2i), (aug.point_transforms[1][b], e2w), (aug.frame_transforms[0][b], w2e)):
            assert np.allclose(got.double().cpu().numpy(), want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    total = int(boxes.sample_sizes.sum())
    print(f"{device}: {total} boxes in {SAMPLES} samples, {sum(kept)} kept; kept per sample {kept}")
    print(f"boxes equal the per-sample float64 loop to {worst:.2e}; objects per task "
          f"{[int(t.centers.sample_sizes.sum()) for t in targets]}")
    assert worst < 1e-4


if __name__ == "__main__":
    main()
