"""Loss-side consumer of the ragged-batch operators: Hungarian matching + matched losses for a 2-D
detection head, written once in BATCHED form on top of ``accvlab.batching_helpers`` and once as the plain per-sample
loop it replaces.  It is the caller pattern of the reference's packages/batching_helpers/example/
{matcher.py, loss_computation.py} (cost matrices -> per-sample assignment -> matched gather -> masked sums -> existence
loss with weights written back through the match indices); this file is an independent formulation used by
tests/test_matched_loss_workflow.py (batched == per-sample, forward and gradients, CPU and GPU) and timed by
scripts/bench_secondary.py (config F3).

Shapes: ground truth ragged per frame — boxes ``[B, G*, 4]`` (x0,y0,x1,y1), labels ``[B, G*]`` int64, weights
``[B, G*]``; predictions dense — boxes ``[B, Q, 4]``, class scores ``[B, Q, C]``, existence ``[B, Q]``.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import torch
from scipy.optimize import linear_sum_assignment

import accvlab.batching_helpers as bh

EPS = 1e-6


# ------------------------------------------------------------------------------------------------ element-wise maths
def _iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """IoU of broadcastable boxes ``[..., 4]`` (union floored at EPS)."""
    wh_a = a[..., 2:] - a[..., :2]
    wh_b = b[..., 2:] - b[..., :2]
    inter_wh = (torch.minimum(a[..., 2:], b[..., 2:]) - torch.maximum(a[..., :2], b[..., :2])).clamp(min=0.0)
    inter = inter_wh[..., 0] * inter_wh[..., 1]
    union = (wh_a[..., 0] * wh_a[..., 1] + wh_b[..., 0] * wh_b[..., 1] - inter).clamp(min=EPS)
    return inter / union


def _one_hot(labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    return torch.nn.functional.one_hot(labels.clamp(0, num_classes - 1), num_classes).to(torch.float32)


# ------------------------------------------------------------------------------------------------ batched formulation
def match_batched(gt_boxes: bh.RaggedBatch, gt_labels: bh.RaggedBatch, pred_boxes, pred_scores):
    """-> (matched gt indices, matched prediction indices) as int64 RaggedBatches on the inputs' device."""
    num_classes = pred_scores.shape[-1]
    # padded cost matrices [B, Q, Gmax]: padded gt columns hold junk and are cut off by split() below
    cost = (1.0 - _iou(pred_boxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
           (1.0 - torch.einsum("bqc,bgc->bqg", pred_scores, _one_hot(gt_labels.tensor, num_classes)))
    cost = gt_labels.create_with_sample_sizes_like_self(cost.detach(), non_uniform_dim=2)
    per_frame = cost.to_device(torch.device("cpu")).split()
    gt_idx, pred_idx = [], []
    for m in per_frame:
        rows, cols = linear_sum_assignment(m.numpy())
        pred_idx.append(torch.as_tensor(rows, dtype=torch.int64))
        gt_idx.append(torch.as_tensor(cols, dtype=torch.int64))
    gt_rb = bh.combine_data(gt_idx)
    pred_rb = bh.combine_data(pred_idx, other_with_same_sample_sizes=gt_rb)
    dev = gt_boxes.tensor.device
    return gt_rb.to_device(dev), pred_rb.to_device(dev)


def match_batched_on_device(gt_boxes: bh.RaggedBatch, gt_labels: bh.RaggedBatch, pred_boxes, pred_scores, check=True):
    """``match_batched`` without the host round trip: the same padded cost matrices, solved per frame on their own device
    by ``bh.batched_linear_sum_assignment`` (padded gt columns are never read).  ``check=False`` skips the one status read
    (no host synchronisation; a frame without a complete matching then has no pairs instead of raising)."""
    num_classes = pred_scores.shape[-1]
    cost = (1.0 - _iou(pred_boxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
           (1.0 - torch.einsum("bqc,bgc->bqg", pred_scores, _one_hot(gt_labels.tensor, num_classes)))
    cost = gt_labels.create_with_sample_sizes_like_self(cost.detach(), non_uniform_dim=2)
    pred_rb, gt_rb = bh.batched_linear_sum_assignment(cost, check=check)[:2]
    return gt_rb, pred_rb


def match_batched_fused_cost(gt_boxes: bh.RaggedBatch, gt_labels: bh.RaggedBatch, pred_boxes, pred_scores, check=True):
    """``match_batched_on_device`` with the cost matrices built by ``bh.batched_matching_cost`` (one launch: the class
    term ``1 - p[q, l_g]`` plus ``1 - IoU``, the padded columns never computed) instead of the broadcast composition —
    cost and assignment are two launches, with no host synchronisation when ``check=False``."""
    pred_rb, gt_rb = bh.batched_hungarian_match(pred_scores, gt_labels, pred_boxes, gt_boxes, class_cost="one_minus_prob",
                                                iou_weight=1.0, iou_eps=EPS, check=check)[:2]
    return gt_rb, pred_rb


def loss_batched(gt_boxes, gt_labels, gt_weights, pred_boxes, pred_scores, pred_exist, match_gt, match_pred):
    """Per-frame loss ``[B]`` = class L1 + (1 - IoU) over matched pairs + existence L1 over all predictions."""
    num_q, num_classes = pred_scores.shape[1], pred_scores.shape[2]
    lab = bh.batched_indexing_access(gt_labels, match_gt)
    box_g = bh.batched_indexing_access(gt_boxes, match_gt)
    w = bh.batched_indexing_access(gt_weights, match_gt)
    sc = bh.batched_indexing_access(pred_scores, match_pred)
    box_p = bh.batched_indexing_access(pred_boxes, match_pred)

    cls_term = w.tensor * (sc.tensor - _one_hot(lab.tensor.to(torch.int64), num_classes)).abs().sum(-1)
    overlap = _iou(box_g.tensor, box_p.tensor)
    box_term = w.tensor * (1.0 - overlap)
    cls_loss = bh.sum_over_targets(lab.create_with_sample_sizes_like_self(cls_term, non_uniform_dim=1))
    box_loss = bh.sum_over_targets(lab.create_with_sample_sizes_like_self(box_term, non_uniform_dim=1))

    # existence: matched predictions should say 1 (weight = gt weight x overlap), the others 0 with the mean matched
    # weight rescaled by matched / unmatched counts
    matched = bh.get_mask_from_indices(num_q, match_pred)
    w_match = w.create_with_sample_sizes_like_self(w.tensor * (1.0 - box_term), non_uniform_dim=1)
    n = w_match.sample_sizes
    balance = torch.nan_to_num(n / (num_q - n), 0.0)
    background = (bh.average_over_targets(w_match) * balance).unsqueeze(-1).repeat(1, num_q)
    w_all = bh.batched_indexing_write(w_match, match_pred, background)
    exist_loss = (w_all * (pred_exist - matched.to(torch.float32)).abs()).sum(1)
    return cls_loss + box_loss + exist_loss


def loss_batched_fused(gt_boxes, gt_labels, gt_weights, pred_boxes, pred_scores, pred_exist, match_gt, match_pred):
    """The same loss with the class and box terms through ``bh.matched_pair_loss_sum`` (one launch each: the matched
    gathers, the per-object loss — L1 against one-hot labels / 1 - IoU, the two losses of the reference example — the
    weight look-up and the masked per-frame sum).  The existence term keeps the operator composition: it needs the
    PER-OBJECT overlaps, not their sum."""
    num_q = pred_scores.shape[1]
    cls_loss = bh.matched_pair_loss_sum(gt_labels, pred_scores, match_gt, match_pred, gt_weights, kind="onehot_l1")
    box_loss = bh.matched_pair_loss_sum(gt_boxes, pred_boxes, match_gt, match_pred, gt_weights, kind="iou_xyxy", eps=EPS)

    box_g = bh.batched_indexing_access(gt_boxes, match_gt)
    w = bh.batched_indexing_access(gt_weights, match_gt)
    box_p = bh.batched_indexing_access(pred_boxes, match_pred)
    box_term = w.tensor * (1.0 - _iou(box_g.tensor, box_p.tensor))
    matched = bh.get_mask_from_indices(num_q, match_pred)
    w_match = w.create_with_sample_sizes_like_self(w.tensor * (1.0 - box_term), non_uniform_dim=1)
    n = w_match.sample_sizes
    balance = torch.nan_to_num(n / (num_q - n), 0.0)
    background = (bh.average_over_targets(w_match) * balance).unsqueeze(-1).repeat(1, num_q)
    w_all = bh.batched_indexing_write(w_match, match_pred, background)
    exist_loss = (w_all * (pred_exist - matched.to(torch.float32)).abs()).sum(1)
    return cls_loss + box_loss + exist_loss


# ------------------------------------------------------------------------------------------------ per-sample loop
def loss_per_sample(gt_boxes_l, gt_labels_l, gt_weights_l, pred_boxes, pred_scores, pred_exist):
    """The same computation frame by frame with plain tensor indexing (what the batched form replaces)."""
    num_q, num_classes = pred_scores.shape[1], pred_scores.shape[2]
    out = []
    for b, (gb, gl, gw) in enumerate(zip(gt_boxes_l, gt_labels_l, gt_weights_l)):
        pb, ps, pe = pred_boxes[b], pred_scores[b], pred_exist[b]
        cost = (1.0 - _iou(pb.unsqueeze(1), gb.unsqueeze(0))) + (1.0 - ps @ _one_hot(gl, num_classes).T)
        rows, cols = linear_sum_assignment(cost.detach().cpu().numpy())
        rows = torch.as_tensor(rows, dtype=torch.int64, device=pb.device)
        cols = torch.as_tensor(cols, dtype=torch.int64, device=pb.device)
        w = gw[cols]
        cls_term = w * (ps[rows] - _one_hot(gl[cols], num_classes)).abs().sum(-1)
        box_term = w * (1.0 - _iou(gb[cols], pb[rows]))
        w_match = w * (1.0 - box_term)
        n = rows.numel()
        mean_w = w_match.sum() / n if n else w_match.sum() * 0.0
        balance = n / (num_q - n) if num_q != n else 0.0
        w_all = (mean_w * balance).expand(num_q).clone()
        w_all[rows] = w_match
        target = torch.zeros(num_q, device=pb.device)
        target[rows] = 1.0
        out.append(cls_term.sum() + box_term.sum() + (w_all * (pe - target).abs()).sum())
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ synthetic inputs
def make_inputs(batch, num_queries, num_classes, max_gt, device, seed=0, min_gt=0):
    g = torch.Generator().manual_seed(seed)
    gt_boxes_l, gt_labels_l, gt_weights_l = [], [], []
    for _ in range(batch):
        n = int(torch.randint(min_gt, max_gt + 1, (1,), generator=g))
        tl = torch.rand(n, 2, generator=g) * 80
        gt_boxes_l.append(torch.cat([tl, tl + 4 + torch.rand(n, 2, generator=g) * 30], 1).to(device))
        gt_labels_l.append(torch.randint(0, num_classes, (n,), generator=g).to(device))
        gt_weights_l.append((0.5 + torch.rand(n, generator=g)).to(device))
    tl = torch.rand(batch, num_queries, 2, generator=g) * 80
    pred_boxes = torch.cat([tl, tl + 4 + torch.rand(batch, num_queries, 2, generator=g) * 30], 2).to(device)
    pred_scores = torch.softmax(torch.randn(batch, num_queries, num_classes, generator=g), -1).to(device)
    pred_exist = torch.rand(batch, num_queries, generator=g).to(device)
    return gt_boxes_l, gt_labels_l, gt_weights_l, pred_boxes, pred_scores, pred_exist


def run_batched(gt_boxes_l, gt_labels_l, gt_weights_l, pred_boxes, pred_scores, pred_exist, fused=False):
    gt_boxes = bh.combine_data(gt_boxes_l)
    gt_labels = bh.combine_data(gt_labels_l, other_with_same_sample_sizes=gt_boxes)
    gt_weights = bh.combine_data(gt_weights_l, other_with_same_sample_sizes=gt_boxes)
    m_gt, m_pred = match_batched(gt_boxes, gt_labels, pred_boxes, pred_scores)
    fn = loss_batched_fused if fused else loss_batched          # the fused op is GPU-only
    return fn(gt_boxes, gt_labels, gt_weights, pred_boxes, pred_scores, pred_exist, m_gt, m_pred)


def run_batched_on_device(gt_boxes_l, gt_labels_l, gt_weights_l, pred_boxes, pred_scores, pred_exist, fused=False,
                          check=True):
    """``run_batched`` with the matching done by ``match_batched_on_device``."""
    gt_boxes = bh.combine_data(gt_boxes_l)
    gt_labels = bh.combine_data(gt_labels_l, other_with_same_sample_sizes=gt_boxes)
    gt_weights = bh.combine_data(gt_weights_l, other_with_same_sample_sizes=gt_boxes)
    m_gt, m_pred = match_batched_on_device(gt_boxes, gt_labels, pred_boxes, pred_scores, check=check)
    fn = loss_batched_fused if fused else loss_batched
    return fn(gt_boxes, gt_labels, gt_weights, pred_boxes, pred_scores, pred_exist, m_gt, m_pred)


def run_batched_fused_cost(gt_boxes_l, gt_labels_l, gt_weights_l, pred_boxes, pred_scores, pred_exist, fused=False,
                           check=True):
    """``run_batched`` with the matching done by ``match_batched_fused_cost``."""
    gt_boxes = bh.combine_data(gt_boxes_l)
    gt_labels = bh.combine_data(gt_labels_l, other_with_same_sample_sizes=gt_boxes)
    gt_weights = bh.combine_data(gt_weights_l, other_with_same_sample_sizes=gt_boxes)
    m_gt, m_pred = match_batched_fused_cost(gt_boxes, gt_labels, pred_boxes, pred_scores, check=check)
    fn = loss_batched_fused if fused else loss_batched
    return fn(gt_boxes, gt_labels, gt_weights, pred_boxes, pred_scores, pred_exist, m_gt, m_pred)


# ------------------------------------------------------------------------------------------------ focal class loss
def focal_class_loss_composed(pred_logits, gt_labels: bh.RaggedBatch, pred_ind: bh.RaggedBatch, gt_ind: bh.RaggedBatch,
                              alpha=0.25, gamma=2.0):
    """The classification loss a DETR-style head trains with, per frame ``[B]``, as the composition a user writes from
    the ragged operators and torch: the matched labels gathered through ``gt_ind`` and written through ``pred_ind`` into a
    ``[B, Q]`` label tensor filled with the background id ``C``, a one-hot target, torchvision's ``sigmoid_focal_loss``
    over all ``[B, Q, C]`` logits, divided by the number of matched pairs."""
    B, Q, C = pred_logits.shape
    matched_labels = bh.batched_indexing_access(gt_labels, gt_ind)
    background = torch.full((B, Q), C, dtype=matched_labels.tensor.dtype, device=pred_logits.device)
    query_labels = bh.batched_indexing_write(matched_labels, pred_ind, background)
    t = torch.nn.functional.one_hot(query_labels.to(torch.int64), C + 1)[..., :C].to(pred_logits.dtype)
    p = pred_logits.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(pred_logits, t, reduction="none")
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    num_pos = pred_ind.sample_sizes.sum().clamp(min=1)
    return loss.sum((1, 2)) / num_pos


def focal_class_loss_fused(pred_logits, gt_labels: bh.RaggedBatch, pred_ind: bh.RaggedBatch, gt_ind: bh.RaggedBatch,
                           alpha=0.25, gamma=2.0):
    """The same loss through ``bh.matched_focal_loss``: two launches forward, one backward, no one-hot target."""
    return bh.matched_focal_loss(pred_logits, gt_labels, pred_ind, gt_ind, alpha=alpha, gamma=gamma)


# ------------------------------------------------------------------------------------------------ box regression loss
def _to_xyxy(b: torch.Tensor, box_format: str) -> torch.Tensor:
    """mmdet's ``bbox_cxcywh_to_xyxy`` (or the identity)"""
    if box_format != "cxcywh":
        return b
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _aligned_overlaps(a: torch.Tensor, b: torch.Tensor, mode: str, eps: float = EPS) -> torch.Tensor:
    """mmdet's ``bbox_overlaps(a, b, mode, is_aligned=True, eps)`` of xyxy boxes ``[..., 4]``"""
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.max(area_a + area_b - overlap, overlap.new_tensor(eps))
    ious = overlap / union
    if mode == "iou":
        return ious
    enclose_wh = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    enclose = torch.max(enclose_wh[..., 0] * enclose_wh[..., 1], overlap.new_tensor(eps))
    return ious - (enclose - union) / enclose


def box_loss_composed(pred_boxes, gt_boxes: bh.RaggedBatch, pred_ind: bh.RaggedBatch, gt_ind: bh.RaggedBatch,
                      box_format="cxcywh", iou_kind="giou", code_weights=None):
    """The box regression loss a DETR-style head trains with, per frame ``(loss_l1 [B], loss_iou [B])``, as the composition
    a user writes from the ragged operators and torch: both sides gathered through the match indices, the format
    conversion, L1 on the raw coordinates, ``1 - GIoU`` as mmdet's aligned ``bbox_overlaps``, masked per-frame sums and
    the division by the number of matched pairs."""
    box_g = bh.batched_indexing_access(gt_boxes, gt_ind)
    box_p = bh.batched_indexing_access(pred_boxes, pred_ind)
    diff = (box_p.tensor - box_g.tensor).abs()
    if code_weights is not None:
        diff = diff * torch.as_tensor(code_weights, dtype=diff.dtype, device=diff.device)
    num_pos = pred_ind.sample_sizes.sum().clamp(min=1)
    loss_l1 = bh.sum_over_targets(box_g.create_with_sample_sizes_like_self(diff.sum(-1), non_uniform_dim=1)) / num_pos
    if iou_kind is None:
        return loss_l1, torch.zeros_like(loss_l1)
    term = 1.0 - _aligned_overlaps(_to_xyxy(box_p.tensor, box_format), _to_xyxy(box_g.tensor, box_format), iou_kind)
    loss_iou = bh.sum_over_targets(box_g.create_with_sample_sizes_like_self(term, non_uniform_dim=1)) / num_pos
    return loss_l1, loss_iou


def box_loss_fused(pred_boxes, gt_boxes: bh.RaggedBatch, pred_ind: bh.RaggedBatch, gt_ind: bh.RaggedBatch,
                   box_format="cxcywh", iou_kind="giou", code_weights=None):
    """The same two losses through ``bh.matched_box_loss``: two launches forward, one write-only launch backward."""
    return bh.matched_box_loss(pred_boxes, gt_boxes, pred_ind, gt_ind, box_format=box_format, iou_kind=iou_kind,
                               code_weights=code_weights, iou_eps=EPS)


# DETR's weights with the focal class term of Deformable-DETR: class 2, L1 5, GIoU 2 — in the matcher and in the loss
CRITERION_WEIGHTS = dict(cls=2.0, l1=5.0, giou=2.0)


def set_criterion_match(pred_logits, pred_boxes, gt_labels: bh.RaggedBatch, gt_boxes: bh.RaggedBatch, box_format="cxcywh"):
    """-> (pred_ind, gt_ind): cost matrices and assignment on the device, two launches, no host synchronisation"""
    w = CRITERION_WEIGHTS
    return bh.batched_hungarian_match(pred_logits.detach(), gt_labels, pred_boxes.detach(), gt_boxes, class_cost="focal",
                                      class_weight=w["cls"], l1_weight=w["l1"], giou_weight=w["giou"],
                                      box_format=box_format, iou_eps=EPS, check=False)[:2]


def set_criterion_fused(pred_logits, pred_boxes, gt_labels: bh.RaggedBatch, gt_boxes: bh.RaggedBatch, box_format="cxcywh",
                        matching=None):
    """The whole set-prediction criterion on the device, per frame ``[B]``: matching cost -> assignment ->
    ``matched_focal_loss`` + ``matched_box_loss`` with DETR's weights.  Both losses see the same pairs and divide by the
    same number of pairs; nothing synchronises with the host."""
    w = CRITERION_WEIGHTS
    pred_ind, gt_ind = matching or set_criterion_match(pred_logits, pred_boxes, gt_labels, gt_boxes, box_format)
    loss_cls = bh.matched_focal_loss(pred_logits, gt_labels, pred_ind, gt_ind)
    loss_l1, loss_giou = bh.matched_box_loss(pred_boxes, gt_boxes, pred_ind, gt_ind, box_format=box_format, iou_kind="giou",
                                             iou_eps=EPS)
    return w["cls"] * loss_cls + w["l1"] * loss_l1 + w["giou"] * loss_giou


def set_criterion_composed(pred_logits, pred_boxes, gt_labels: bh.RaggedBatch, gt_boxes: bh.RaggedBatch, box_format="cxcywh",
                           matching=None):
    """The same criterion from ``focal_class_loss_composed`` and ``box_loss_composed``."""
    w = CRITERION_WEIGHTS
    pred_ind, gt_ind = matching or set_criterion_match(pred_logits, pred_boxes, gt_labels, gt_boxes, box_format)
    loss_cls = focal_class_loss_composed(pred_logits, gt_labels, pred_ind, gt_ind)
    loss_l1, loss_giou = box_loss_composed(pred_boxes, gt_boxes, pred_ind, gt_ind, box_format=box_format, iou_kind="giou")
    return w["cls"] * loss_cls + w["l1"] * loss_l1 + w["giou"] * loss_giou
