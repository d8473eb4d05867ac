"""Set-prediction criterion of a lane / vectorised-map head (MapTR-style), on the device end to end.

Ground-truth lanes arrive with a different number of points each.  They are resampled to ``P`` points at equal arc length
with ``polyline.interpolate_var_size_batch``, matched to the query lines by ``batched_polyline_hungarian_match`` (class
cost + the point-wise L1 distance minimised over the equivalent orders of each lane) and the criterion is

    w_cls * matched_focal_loss + w_pts * loss_pts + w_dir * loss_dir

with ``matched_polyline_loss`` for the two line terms.  ``criterion_composed`` is the same criterion written as the torch
composition a user would otherwise write: every order of every matched lane built by ``gather``, the best one picked by
``torch.min``.

    python examples/lane_set_prediction.py            # runs on cuda:0 when there is one, else on the CPU
"""
from __future__ import annotations

import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "accv-lab_amd"))

import accvlab.batching_helpers as bh  # noqa: E402
from accvlab.lane_helpers import polyline  # noqa: E402

WEIGHTS = {"cls": 2.0, "pts": 5.0, "dir": 0.005}    # MapTR's loss weights
MATCH_WEIGHTS = {"cls": 2.0, "pts": 5.0}


def resample(raw_lanes, num_points):
    """list of [n_i, D] lanes (n_i >= 2) -> [N, num_points, D] at equal arc length, one launch for all of them"""
    pts = bh.combine_data(raw_lanes)                                         # [N, max n_i, D], sizes n_i
    frac = torch.linspace(0.0, 1.0, num_points, dtype=pts.tensor.dtype, device=pts.tensor.device)
    dist = bh.RaggedBatch(frac.expand(len(raw_lanes), num_points).contiguous(),
                          sample_sizes=torch.full_like(pts.sample_sizes, num_points))
    return polyline.interpolate_var_size_batch(pts, dist, relative=True).tensor


def make_inputs(batch, num_queries, num_classes, max_lanes, num_points, device, seed=0, dtype=torch.float32):
    """-> (pred_lines [B, Q, P, 2], pred_logits [B, Q, C], gt_lines, gt_labels, gt_closed): ragged ground truth resampled
    from raw lanes of 3 .. 12 points; about a third of the lanes are closed polygons"""
    g = torch.Generator().manual_seed(seed)
    lines_l, labels_l, closed_l = [], [], []
    for _ in range(batch):
        n = int(torch.randint(0, max_lanes + 1, (1,), generator=g))
        raw, closed = [], torch.rand(n, generator=g) < 0.33
        for i in range(n):
            k = int(torch.randint(3, 13, (1,), generator=g))
            if bool(closed[i]):
                ang = (torch.arange(k + 1) % k + 0.5 * torch.rand(k, generator=g)[torch.arange(k + 1) % k]) * (6.2831853 / k)
                rad = (0.1 + 0.2 * torch.rand(k, generator=g))[torch.arange(k + 1) % k]
                pts = 0.5 + torch.stack([rad * ang.cos(), rad * ang.sin()], -1)     # the ring, closed for the resampling
            else:
                step = torch.stack([0.3 + torch.rand(k, generator=g), 0.5 * torch.randn(k, generator=g)], -1) / k
                pts = torch.rand(2, generator=g) * 0.2 + step.cumsum(0)
            raw.append(pts.to(dtype).to(device))
        # a closed lane is resampled over its ring at P + 1 points and loses the repeated end point
        res = resample(raw, num_points + 1) if n else torch.zeros(0, num_points + 1, 2, dtype=dtype, device=device)
        open_res = resample(raw, num_points) if n else res[:, :num_points]
        lines_l.append(torch.where(closed.to(device)[:, None, None], res[:, :num_points], open_res))
        labels_l.append(torch.randint(0, num_classes, (n,), generator=g).to(device))
        closed_l.append(closed.to(device))
    gt_lines = bh.combine_data(lines_l)
    gt_labels = bh.combine_data(labels_l, other_with_same_sample_sizes=gt_lines)
    gt_closed = bh.combine_data(closed_l, other_with_same_sample_sizes=gt_lines)
    pred_lines = torch.rand(batch, num_queries, num_points, 2, generator=g).to(dtype).to(device)
    # some queries near a lane, in one of its orders, so that the matching is not arbitrary
    for b in range(batch):
        n = int(gt_lines.sample_sizes[b])
        for i in range(min(n, num_queries)):
            t = gt_lines.tensor[b, i]
            t = t.flip(0) if i % 2 else t
            pred_lines[b, (3 * i + b) % num_queries] = t + 0.01 * torch.randn(num_points, 2, generator=g).to(dtype).to(device)
    pred_logits = (torch.randn(batch, num_queries, num_classes, generator=g) * 2).to(dtype).to(device)
    return pred_lines, pred_logits, gt_lines, gt_labels, gt_closed


def match(pred_lines, pred_logits, gt_lines, gt_labels, gt_closed, check=True):
    """-> (pred_ind, gt_ind): cost matrix and assignment on the device, two launches"""
    w = MATCH_WEIGHTS
    return polyline.batched_polyline_hungarian_match(pred_lines.detach(), gt_lines, pred_logits.detach(), gt_labels,
                                                     gt_closed=gt_closed, class_cost="focal", class_weight=w["cls"],
                                                     pts_weight=w["pts"], check=check)[:2]


def criterion_fused(pred_lines, pred_logits, gt_lines, gt_labels, gt_closed, matching=None):
    """the criterion per frame ``[B]``: five launches forward after the matching, two backward"""
    pred_ind, gt_ind = matching if matching is not None else match(pred_lines, pred_logits, gt_lines, gt_labels, gt_closed)
    loss_cls = bh.matched_focal_loss(pred_logits, gt_labels, pred_ind, gt_ind)
    loss_pts, loss_dir = polyline.matched_polyline_loss(pred_lines, gt_lines, pred_ind, gt_ind, gt_closed=gt_closed)
    return WEIGHTS["cls"] * loss_cls + WEIGHTS["pts"] * loss_pts + WEIGHTS["dir"] * loss_dir


def _orders(P, device):
    """index tensors of the orders: open [2, P], closed [2 P, P]"""
    p = torch.arange(P, device=device)
    s = p[:, None]
    return torch.stack([p, P - 1 - p]), torch.cat([(s + p) % P, (s - p) % P])


def line_losses_composed(pred_lines, gt_lines, pred_ind, gt_ind, gt_closed, dir_eps=1e-12):
    """``matched_polyline_loss`` as a torch composition: the [M, V, P, D] variants of the matched lanes, min over V"""
    B, Q, P, D = pred_lines.shape
    K = pred_ind.tensor.shape[1]
    dev = pred_lines.device
    valid = torch.arange(K, device=dev)[None] < pred_ind.sample_sizes[:, None]
    frame = torch.arange(B, device=dev)[:, None].expand(B, K)[valid]
    qs, gs = pred_ind.tensor[valid], gt_ind.tensor[valid]
    x, t, closed = pred_lines[frame, qs], gt_lines.tensor[frame, gs], gt_closed.tensor[frame, gs].bool()
    open_o, closed_o = _orders(P, dev)
    pad = open_o[:1].expand(2 * P - 2, P)                                   # open lines: their first order repeated
    order = torch.where(closed[:, None, None], closed_o[None], torch.cat([open_o, pad])[None])      # [M, 2P, P]
    variants = t[torch.arange(len(t), device=dev)[:, None, None], order]                            # [M, 2P, P, D]
    dist = (x[:, None] - variants).abs().sum((-1, -2))
    best = dist.min(1).indices
    ts = variants[torch.arange(len(t), device=dev), best]
    pts = (x - ts).abs().sum((-1, -2))
    a, b = x.roll(-1, 1) - x, ts.roll(-1, 1) - ts
    cos = (a * b).sum(-1) / torch.sqrt(((a * a).sum(-1) + dir_eps) * ((b * b).sum(-1) + dir_eps))
    seg = torch.arange(P, device=dev)[None] < torch.where(closed, P, P - 1)[:, None]
    dirs = ((1.0 - cos) * seg).sum(-1)
    factor = pred_ind.sample_sizes.sum().clamp(min=1)
    zero = torch.zeros(B, dtype=pts.dtype, device=dev)
    return zero.index_add(0, frame, pts) / factor, zero.index_add(0, frame, dirs) / factor


def class_loss_composed(pred_logits, gt_labels, pred_ind, gt_ind, alpha=0.25, gamma=2.0):
    B, Q, C = pred_logits.shape
    K = pred_ind.tensor.shape[1]
    dev = pred_logits.device
    valid = torch.arange(K, device=dev)[None] < pred_ind.sample_sizes[:, None]
    frame = torch.arange(B, device=dev)[:, None].expand(B, K)[valid]
    target = torch.zeros_like(pred_logits)
    target[frame, pred_ind.tensor[valid], gt_labels.tensor[frame, gt_ind.tensor[valid]]] = 1.0
    p = pred_logits.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(pred_logits, target, reduction="none")
    loss = ce * (1 - (p * target + (1 - p) * (1 - target))) ** gamma * (alpha * target + (1 - alpha) * (1 - target))
    return loss.sum((1, 2)) / pred_ind.sample_sizes.sum().clamp(min=1)


def criterion_composed(pred_lines, pred_logits, gt_lines, gt_labels, gt_closed, matching=None):
    pred_ind, gt_ind = matching if matching is not None else match(pred_lines, pred_logits, gt_lines, gt_labels, gt_closed)
    loss_cls = class_loss_composed(pred_logits, gt_labels, pred_ind, gt_ind)
    loss_pts, loss_dir = line_losses_composed(pred_lines, gt_lines, pred_ind, gt_ind, gt_closed)
    return WEIGHTS["cls"] * loss_cls + WEIGHTS["pts"] * loss_pts + WEIGHTS["dir"] * loss_dir


def main():
    device = "cuda" if torch.cuda.is_available() else "cpu"
    data = make_inputs(4, 50, 3, 12, 20, device, seed=1)
    lines, logits = data[0].clone().requires_grad_(True), data[1].clone().requires_grad_(True)
    loss = criterion_fused(lines, logits, *data[2:])
    loss.sum().backward()
    ref = criterion_composed(*data)
    print(f"device {device}: per-frame criterion {[round(float(v), 4) for v in loss.detach()]}")
    print(f"torch composition                  {[round(float(v), 4) for v in ref]}")
    print(f"gradient norms: lines {float(lines.grad.norm()):.4f}, logits {float(logits.grad.norm()):.4f}")


if __name__ == "__main__":
    main()
