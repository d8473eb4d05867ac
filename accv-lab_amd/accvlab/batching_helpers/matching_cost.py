"""(extension) Fused matching-cost matrices for ragged Hungarian matching — the ``[B, Q, G_max]`` costs that
``batched_linear_sum_assignment`` reads, in one launch instead of the broadcast chains of the reference's matcher
(packages/batching_helpers/example/matcher.py:22-31, 78-132: IoU through about ten element-wise ops, one-hot labels built
in a per-sample, per-object loop, an einsum).

GPU tensors run one HIP launch (``accv_matching_cost``); CPU tensors run the host implementation of the same operation
sequence (``accv_matching_cost_host``).  There is no CPU fallback for GPU tensors.
"""
from __future__ import annotations

import ctypes
import struct

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from .assignment import batched_linear_sum_assignment
from .ragged import RaggedBatch

__all__ = ["batched_matching_cost", "batched_hungarian_match"]

_DTYPES = _nat.FLOAT_DTYPE_CODES
_KINDS = {"one_minus_prob": _nat.MC_ONE_MINUS_PROB, "neg_prob": _nat.MC_NEG_PROB, "focal": _nat.MC_FOCAL}
_FORMATS = {"xyxy": 0, "cxcywh": _nat.MC_CXCYWH}
MAX_BOX_DIM = 16
_PARAMS = {}   # packed float parameters -> MatchingCostParams (a training loop uses one or two settings)


def _params(values):
    key = struct.pack("9d", *values)
    p = _PARAMS.get(key)
    if p is None:
        if len(_PARAMS) >= 64:
            _PARAMS.clear()
        p = _PARAMS[key] = _nat.MatchingCostParams(*values)
    return p


def _pred(name, t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"batched_matching_cost: {name} must be a tensor (needed by the {what} cost), got "
                        f"{type(t).__name__}")
    if t.dim() != 3:
        raise ValueError(f"batched_matching_cost: {name} must be [B, Q, {'C' if name == 'pred_scores' else 'D'}], got "
                         f"shape {tuple(t.shape)}")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"batched_matching_cost: the last dimension of {name} must have unit stride, got stride "
                         f"{t.stride(-1)}")
    return t.detach()


def _gt(name, rb, dim, what):
    if not isinstance(rb, RaggedBatch):
        raise TypeError(f"batched_matching_cost: {name} must be a RaggedBatch (needed by the {what} cost), got "
                        f"{type(rb).__name__}")
    if rb.num_batch_dims != 1 or rb.tensor.dim() != dim or rb.non_uniform_dim != 1:
        raise ValueError(f"batched_matching_cost: {name} must be a RaggedBatch [B, G*{', D' if dim == 3 else ''}] with "
                         f"non_uniform_dim 1, got shape {tuple(rb.tensor.shape)}, non_uniform_dim {rb.non_uniform_dim}")
    return rb.tensor.detach().contiguous()


def batched_matching_cost(pred_scores, gt_labels, pred_boxes=None, gt_boxes=None, *, class_cost: str = "one_minus_prob",
                          class_weight: float = 1.0, l1_weight: float = 0.0, iou_weight: float = 0.0,
                          giou_weight: float = 0.0, box_format: str = "xyxy", focal_alpha: float = 0.25,
                          focal_gamma: float = 2.0, focal_eps: float = 1e-12, iou_eps: float = 1e-6,
                          filler: float = 0.0) -> RaggedBatch:
    """Weighted matching costs of every (prediction, ground truth) pair of a batch, as the ragged ``[B, Q, G_max]``
    cost that ``batched_linear_sum_assignment`` consumes.

    Args:
        pred_scores: dense ``[B, Q, C]``: probabilities for ``class_cost`` ``"one_minus_prob"`` / ``"neg_prob"``, logits
            for ``"focal"``.
        gt_labels: RaggedBatch ``[B, G*]`` of int32 / int64 class labels.
        pred_boxes: dense ``[B, Q, D]``, ``D <= 16``.
        gt_boxes: RaggedBatch ``[B, G*, D]`` with the sample sizes of ``gt_labels``.
        class_cost, class_weight, l1_weight, iou_weight, giou_weight: the terms below and their weights.  A term whose
            weight is 0 is not evaluated; its inputs may be ``None``.
        box_format: ``"xyxy"`` or ``"cxcywh"`` — how the IoU / GIoU terms read the boxes (the L1 term reads the raw
            coordinates).
        focal_alpha, focal_gamma, focal_eps: parameters of the focal class cost.
        iou_eps: floor of the union (IoU, GIoU) and of the enclosing area (GIoU).
        filler: value of the padded columns ``[G_b, G_max)``.

    All float inputs share one dtype (float32, float16, bfloat16 or float64); the last dimension of ``pred_scores`` and
    ``pred_boxes`` must have unit stride, the batch and query strides are free (``bbox_pred[..., :8]`` of a
    ``[B, Q, 10]`` tensor needs no copy).  The sample sizes come from ``gt_labels`` (from ``gt_boxes`` when
    ``class_weight`` is 0); they are read on the device, clamped to ``[0, G_max]``, never copied to the host.

    Per pair ``(q, g)``, summed in the order cls, l1, iou, giou, each multiplied by its weight (the float64 evaluation
    of these formulas is the definition; float16 / bfloat16 are widened exactly to float32 and evaluated in float32):
        - ``one_minus_prob``: ``1 - p[q, l_g]`` (the reference example's ``_class_l1_cost_func_gt_labels``);
        - ``neg_prob``: ``-p[q, l_g]`` (DETR's ``HungarianMatcher``);
        - ``focal``: mmdet's ``FocalLossCost``, with ``s = sigmoid(x[q, l_g])`` and ``1 - s`` computed from
          ``exp(-|x|)``: ``alpha (1-s)^gamma (-log(s + eps)) - (1-alpha) s^gamma (-log(1 - s + eps))``;
        - ``l1``: ``sum_d |bp_d - bg_d|`` (``torch.cdist(p=1)``);
        - ``iou``: ``1 - inter / max(union, iou_eps)``, intersection sides clamped at 0, areas not clamped (the
          reference example's ``_iou_cost_func``);
        - ``giou``: ``-GIoU`` with mmdet's ``bbox_overlaps(mode="giou")`` floors ``max(union, eps)`` and
          ``max(enclose, eps)``; needs ``D == 4`` (as does ``iou``).
    NaN in an input of an evaluated term gives NaN for the pair; a label outside ``[0, C)`` gives a NaN class term (the
    solver then reports invalid entries); infinities behave as the float64 formula says.  No autograd.

    Returns:
        RaggedBatch ``[B, Q, G_max]``, contiguous, ``non_uniform_dim=2``, sharing the ground truth's sample sizes;
        float32 (float64 for float64 inputs); padded columns hold exactly ``filler``.
    """
    if class_cost not in _KINDS:
        raise ValueError(f"batched_matching_cost: class_cost must be one of {sorted(_KINDS)}, got {class_cost!r}")
    if box_format not in _FORMATS:
        raise ValueError(f"batched_matching_cost: box_format must be 'xyxy' or 'cxcywh', got {box_format!r}")
    values = tuple(float(v) for v in (class_weight, l1_weight, iou_weight, giou_weight, focal_alpha, focal_gamma,
                                      focal_eps, iou_eps, filler))
    use_cls = values[0] != 0.0
    use_box = any(v != 0.0 for v in values[1:4])
    use_iou = values[2] != 0.0 or values[3] != 0.0

    floats, labels, gboxes = [], None, None
    if use_cls:
        scores = _pred("pred_scores", pred_scores, "class")
        labels = _gt("gt_labels", gt_labels, 2, "class")
        if labels.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"batched_matching_cost: gt_labels must be int32 or int64, got {labels.dtype}")
        floats.append(("pred_scores", scores))
    if use_box:
        pboxes = _pred("pred_boxes", pred_boxes, "box")
        gboxes = _gt("gt_boxes", gt_boxes, 3, "box")
        floats += [("pred_boxes", pboxes), ("gt_boxes", gboxes)]
        D = int(pboxes.shape[-1])
        if int(gboxes.shape[-1]) != D:
            raise ValueError(f"batched_matching_cost: pred_boxes have {D} coordinates, gt_boxes {gboxes.shape[-1]}")
        if D > MAX_BOX_DIM:
            raise ValueError(f"batched_matching_cost: boxes of {D} coordinates exceed the limit of {MAX_BOX_DIM}")
        if use_iou and D != 4:
            raise ValueError(f"batched_matching_cost: the IoU / GIoU costs need boxes of 4 coordinates, got {D}")
    else:
        D = 0

    # the sample sizes (and G_max) come from the labels, or from the boxes when the class term is off
    sizes_rb = gt_labels if use_cls else (gt_boxes if use_box else (gt_labels if gt_labels is not None else gt_boxes))
    if not isinstance(sizes_rb, RaggedBatch) or sizes_rb.num_batch_dims != 1 or sizes_rb.non_uniform_dim != 1:
        raise TypeError("batched_matching_cost: gt_labels or gt_boxes must be a RaggedBatch [B, G*, ...] with "
                        "non_uniform_dim 1")
    ref = floats[0][1] if floats else None
    if ref is None:   # every weight is 0: shapes from whatever predictions were given
        ref = pred_scores if isinstance(pred_scores, torch.Tensor) else pred_boxes
        if not isinstance(ref, torch.Tensor) or ref.dim() != 3:
            raise ValueError("batched_matching_cost: pred_scores or pred_boxes [B, Q, *] is needed for the shape")
    dtype, dev = ref.dtype, ref.device
    if dtype not in _DTYPES:
        raise TypeError(f"batched_matching_cost: float32, float16, bfloat16 or float64 inputs expected, got {dtype}")
    for name, t in floats:
        if t.dtype != dtype:
            raise TypeError(f"batched_matching_cost: {name} is {t.dtype}, {floats[0][0]} {dtype}: all float inputs "
                            "must share one dtype")
    B, Q = int(ref.shape[0]), int(ref.shape[1])
    G = int(sizes_rb.tensor.shape[1])
    for name, t in [("gt_labels", labels), ("gt_boxes", gboxes), ("sample sizes", sizes_rb.tensor)] + floats:
        if t is None:
            continue
        if t.device != dev:
            raise ValueError(f"batched_matching_cost: {name} is on {t.device}, expected {dev}")
        if int(t.shape[0]) != B:
            raise ValueError(f"batched_matching_cost: {name} has batch size {t.shape[0]}, expected {B}")
    for name, t in floats:
        if name.startswith("pred") and int(t.shape[1]) != Q:
            raise ValueError(f"batched_matching_cost: {name} has {t.shape[1]} queries, expected {Q}")
    for name, t in (("gt_labels", labels), ("gt_boxes", gboxes)):
        if t is not None and int(t.shape[1]) != G:
            raise ValueError(f"batched_matching_cost: {name} has {t.shape[1]} objects per frame, expected {G}")

    out = torch.empty((B, Q, G), dtype=torch.float64 if dtype == torch.float64 else torch.float32, device=dev)
    if B * Q * G > 0:
        counts = sizes_rb.sample_sizes.to(device=dev, dtype=torch.int64).contiguous()
        C = int(scores.shape[2]) if use_cls else 0
        flags = (_nat.MC_LABELS_I64 if labels is not None and labels.dtype == torch.int64 else 0) | _FORMATS[box_format]
        p = _params(values)
        args = (scores.data_ptr() if use_cls else 0, pboxes.data_ptr() if use_box else 0,
                labels.data_ptr() if use_cls else 0, gboxes.data_ptr() if use_box else 0, counts.data_ptr(),
                _DTYPES[dtype], _KINDS[class_cost], flags, B, Q, C, G, D,
                scores.stride(0) if use_cls else 0, scores.stride(1) if use_cls else 0,
                pboxes.stride(0) if use_box else 0, pboxes.stride(1) if use_box else 0,
                ctypes.addressof(p), out.data_ptr())
        if dev.type not in ("cuda", "cpu"):
            raise RuntimeError(f"batched_matching_cost: unsupported device {dev}")
        _ops.run("accv_matching_cost", args, dev, "batched_matching_cost")
    return sizes_rb.create_with_sample_sizes_like_self(out, non_uniform_dim=2)


def batched_hungarian_match(pred_scores, gt_labels, pred_boxes=None, gt_boxes=None, *, class_cost: str = "one_minus_prob",
                            class_weight: float = 1.0, l1_weight: float = 0.0, iou_weight: float = 0.0,
                            giou_weight: float = 0.0, box_format: str = "xyxy", focal_alpha: float = 0.25,
                            focal_gamma: float = 2.0, focal_eps: float = 1e-12, iou_eps: float = 1e-6,
                            filler: float = 0.0, maximize: bool = False, check: bool = True):
    """``batched_linear_sum_assignment(batched_matching_cost(...), maximize=maximize, check=check)``: the Hungarian
    matching of a DETR-style head in two launches, with no host synchronisation when ``check=False``.

    Returns ``(pred_ind, gt_ind)`` (``check=True``) or ``(pred_ind, gt_ind, status)`` (``check=False``): the int64
    RaggedBatches ``[B, min(Q, G_max)]`` (and int32 status ``[B]``) of ``batched_linear_sum_assignment``, whose rows are
    the queries and columns the ground-truth objects.  See ``batched_matching_cost`` for the arguments.
    """
    cost = batched_matching_cost(pred_scores, gt_labels, pred_boxes, gt_boxes, class_cost=class_cost,
                                 class_weight=class_weight, l1_weight=l1_weight, iou_weight=iou_weight,
                                 giou_weight=giou_weight, box_format=box_format, focal_alpha=focal_alpha,
                                 focal_gamma=focal_gamma, focal_eps=focal_eps, iou_eps=iou_eps, filler=filler)
    return batched_linear_sum_assignment(cost, maximize=maximize, check=check)
