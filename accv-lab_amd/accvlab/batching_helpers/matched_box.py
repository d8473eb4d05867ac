"""(extension) Box regression loss of a set-prediction head (DETR / Deformable-DETR / StreamPETR) over the matched pairs:
the L1 term and the GIoU (or IoU) term in one operator — the link of the loss chain between
``batched_linear_sum_assignment`` and the criterion's weighted sum, next to ``matched_focal_loss``.

The torch composition gathers both sides through the match indices, converts the box format and runs about 25
element-wise launches forward and twice that backward on a few thousand numbers.  Here: two launches forward, one
write-only launch backward.

GPU tensors run the HIP kernels (``accv_matched_box_loss`` / ``_bwd``); CPU tensors run the host implementation of the
same operation sequence (``accv_matched_box_loss_host`` / ``_bwd_host``).  There is no CPU fallback for GPU tensors.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from .. import _amd_native as _nat
from . import _matched_pairs as _mp
from .ragged import RaggedBatch

__all__ = ["matched_box_loss"]

_WHO = "matched_box_loss"
_STEM = "accv_matched_box_loss"
_DTYPES = _mp.DTYPES
_IOU_KINDS = {None: _nat.MB_IOU_NONE, "iou": _nat.MB_IOU, "giou": _nat.MB_GIOU}
_FORMATS = {"xyxy": 0, "cxcywh": _nat.MB_CXCYWH}


class _Call:
    """the geometry and scalar parameters that the forward and the backward C-ABI calls of one invocation share; it holds
    no tensor a kernel reads (avg_dev is read by the forward alone)"""

    def __init__(self, boxes, gt, pind, flags, params, avg_dev):
        self.params, self.avg_dev = params, avg_dev
        self.dev = boxes.device
        self.B, self.Q, self.D = (int(v) for v in boxes.shape)
        self.G, self.K = int(gt.shape[1]), int(pind.shape[1])
        self.flags = flags
        self.out_dtype = _mp.out_dtype(boxes.dtype)

    def inputs(self, boxes, gt, pind, gind, counts, weights, cw_dev):
        """the pointer arguments; the optional operands go into the parameter struct"""
        self.params.query_weights = None if weights is None else weights.data_ptr()
        self.params.code_weights_dev = None if cw_dev is None else cw_dev.data_ptr()
        return (boxes.data_ptr(), gt.data_ptr(), pind.data_ptr(), gind.data_ptr(), counts.data_ptr())

    def shape(self, boxes):
        # a dimension of extent 1 may carry any stride
        sb = boxes.stride(0) if self.B > 1 else self.Q * max(boxes.stride(1), self.D)
        sq = boxes.stride(1) if self.Q > 1 else self.D
        return (_DTYPES[boxes.dtype], self.flags, self.B, self.Q, self.D, self.G, self.K, sb, sq,
                ctypes.addressof(self.params))


class _MatchedBoxLoss(torch.autograd.Function):
    """-> (L1 sums [B], IoU sums [B]), the two rows of one [2, B] tensor"""

    @staticmethod
    def forward(ctx, call, boxes, gt, pind, gind, counts, weights, cw_dev):
        tensors = (boxes, gt, pind, gind, counts, weights, cw_dev)
        run = call.B * call.Q * call.K > 0
        out, denom = _mp.run_forward(_WHO, _STEM, call, tensors, run, 2, (call.B, call.Q, call.D))
        ctx.call, ctx.run = call, run
        # everything the backward kernel reads: alive until then, and guarded by torch's version check
        ctx.save_for_backward(denom, *tensors)
        ctx.set_materialize_grads(False)   # an unused output arrives as None and goes down as a null pointer
        return out[0], out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_l1, grad_iou):
        call = ctx.call
        denom, *tensors = ctx.saved_tensors
        boxes = tensors[0]
        if not ctx.needs_input_grad[1]:
            return (None,) * 8
        if not ctx.run:   # no pair anywhere: nothing depends on the boxes
            return (None, torch.zeros(boxes.shape, dtype=boxes.dtype, device=call.dev)) + (None,) * 6
        return (None, _mp.run_backward(_WHO, _STEM, call, tensors, (grad_l1, grad_iou), denom)) + (None,) * 6


def matched_box_loss(pred_boxes: torch.Tensor, gt_boxes: RaggedBatch, pred_ind: RaggedBatch, gt_ind: RaggedBatch, *,
                     box_format: str = "xyxy", iou_kind: Optional[str] = "giou",
                     code_weights: Optional[Union[Sequence[float], torch.Tensor]] = None,
                     query_weights: Optional[torch.Tensor] = None, iou_eps: float = 1e-6,
                     avg_factor: Optional[Union[float, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-frame box regression losses ``(loss_l1 [B], loss_iou [B])`` over the matched pairs, both divided by the number
    of matched pairs and neither multiplied by a term weight: a criterion forms
    ``w_l1 * loss_l1 + w_giou * loss_iou + w_cls * matched_focal_loss(...)``.

    Args:
        pred_boxes: dense ``[B, Q, D]``, float32 / float16 / bfloat16 / float64, ``1 <= D <= 16``.  Unit stride in the
            last dimension; the batch and query strides are free (``code[..., :4]`` of a wider regression output needs
            no copy).
        gt_boxes: RaggedBatch ``[B, G*, D]`` of the same dtype.  Never differentiated.
        pred_ind, gt_ind: RaggedBatch ``[B, K]``, int32 / int64, one dtype — what ``batched_linear_sum_assignment`` /
            ``batched_hungarian_match`` return.  ONLY ``pred_ind.sample_sizes`` is read (on the device, clamped to
            ``[0, K]``); comparing the two would cost a synchronisation.
        box_format: ``"xyxy"`` or ``"cxcywh"`` (both sides; converted as mmdet's ``bbox_cxcywh_to_xyxy``, the L1 term is
            taken on the raw coordinates as DETR does).
        iou_kind: ``"giou"``, ``"iou"`` or ``None`` (L1 only: ``loss_iou`` is zeros and nothing is evaluated for it).  An
            IoU kind requires ``D == 4``.
        code_weights: optional ``[D]`` (mmdet3d's ``code_weights``), multiplies the L1 term per coordinate: a Python
            sequence (used in the arithmetic type, float32 or float64) or a tensor of the boxes' dtype on their device.
        query_weights: optional dense ``[B, Q]`` of the boxes' dtype; multiplies both terms of that query's pair.
        iou_eps: floor of the union and of the enclosing area (mmdet's ``eps``).
        avg_factor: ``None`` divides by ``max(M, 1)`` with ``M = sum_b clamp(n_b, 0, K)`` counted on the device — the
            number ``matched_focal_loss`` divides by; a Python number is used as given (``1.0`` gives raw sums); a 0-d
            float32 tensor on the boxes' device (an all-reduced count) is read on the device.
        No gradient flows to either weight or to ``avg_factor``.

    Definition (its float64 evaluation with autograd on the dtype-rounded inputs is what the tests pin)::

        for b, j < clamp(n_b, 0, K):                       # ascending j
            q, g = pred_ind[b, j], gt_ind[b, j]
            if 0 <= q < Q and 0 <= g < G_max and no lower j named q:      # a pair with both indices in range names q
                p, t = pred_boxes[b, q], gt_boxes[b, g]
                loss_l1[b]  += w[b, q] * sum_d cw[d] * |p[d] - t[d]|
                loss_iou[b] += w[b, q] * (1 - bbox_overlaps(xyxy(p), xyxy(t), mode=iou_kind, is_aligned=True, eps=iou_eps))
        loss_l1, loss_iou = loss_l1 / factor, loss_iou / factor

    The pair rule is ``matched_focal_loss``'s, so both losses always agree on which queries are matched: indices outside
    their range are skipped, not wrapped; a query named twice takes the pair in the lowest slot; slots at or past ``n_b``
    are never read.  A frame without pairs gives 0.  ``B``, ``Q`` or ``K`` of 0 give zeros and launch nothing.

    Returns two ``[B]`` tensors, float32 (float64 for float64 boxes).  Differentiable w.r.t. ``pred_boxes`` only, for
    either or both outputs (no double backward).  The tensors read by the backward (both box tensors, both index tensors,
    ``pred_ind.sample_sizes``, ``query_weights``, a tensor ``code_weights``) are saved; modifying them in place before
    ``backward()`` raises.  The gradient has the boxes' dtype, is contiguous and written completely,
    ``+0`` for unmatched queries.  It is the closed-form chain rule with float64 autograd's conventions where the
    definition is not smooth: an exact tie of a maximum / minimum splits the gradient evenly, a floor that fires passes
    none, ``|0|`` has gradient 0.  float16 / bfloat16 boxes are widened exactly and evaluated in float32, float64 in
    float64; sums are accumulated in float64 in a fixed order, so forward and backward are bitwise reproducible.  Two
    launches forward, one backward (no zero fill, no atomics), on torch's current stream, without host synchronisation or
    read-back: both directions can be captured into a graph.

    Special values: a NaN in a matched prediction makes its frame's sums and that query's gradient NaN (with an IoU kind
    all four components, otherwise the component of the NaN coordinate); rows of unmatched queries are never read.
    """
    _mp.dense(_WHO, "pred_boxes", pred_boxes, "[B, Q, D]")
    dev = pred_boxes.device
    B, Q, D = (int(v) for v in pred_boxes.shape)
    if not 1 <= D <= _nat.MB_MAX_D:
        raise ValueError(f"{_WHO}: needs 1 <= D <= {_nat.MB_MAX_D}, got D = {D}")
    _mp.not_overlapping(_WHO, "pred_boxes", pred_boxes, D)
    if box_format not in _FORMATS:
        raise ValueError(f"{_WHO}: box_format must be 'xyxy' or 'cxcywh', got {box_format!r}")
    if iou_kind not in _IOU_KINDS:
        raise ValueError(f"{_WHO}: iou_kind must be 'giou', 'iou' or None, got {iou_kind!r}")
    if iou_kind is not None and D != 4:
        raise ValueError(f"{_WHO}: iou_kind {iou_kind!r} needs D == 4, got D = {D}")
    iou_eps = float(iou_eps)
    if not iou_eps >= 0.0:
        raise ValueError(f"{_WHO}: iou_eps must be >= 0, got {iou_eps}")

    gt = _mp.ragged(_WHO, "gt_boxes", gt_boxes, "[B, G*, D]", 3)
    if gt.dtype != pred_boxes.dtype:
        raise TypeError(f"{_WHO}: gt_boxes is {gt.dtype}, pred_boxes {pred_boxes.dtype}")
    if int(gt.shape[2]) != D:
        raise ValueError(f"{_WHO}: gt_boxes has {gt.shape[2]} coordinates, pred_boxes {D}")
    pind, gind, counts = _mp.match_indices(_WHO, pred_ind, gt_ind)
    weights = _mp.query_weights(_WHO, query_weights, pred_boxes, "pred_boxes")
    cw_dev, cw_values = None, None
    if isinstance(code_weights, torch.Tensor):
        if tuple(code_weights.shape) != (D,):
            raise ValueError(f"{_WHO}: code_weights must have shape [{D}], got {tuple(code_weights.shape)}")
        if code_weights.dtype != pred_boxes.dtype:
            raise TypeError(f"{_WHO}: code_weights is {code_weights.dtype}, pred_boxes {pred_boxes.dtype}")
        if code_weights.device != dev:
            raise ValueError(f"{_WHO}: code_weights is on {code_weights.device}, pred_boxes on {dev}")
        cw_dev = code_weights.detach().contiguous()
    elif code_weights is not None:
        try:
            cw_values = [float(v) for v in code_weights]
        except TypeError:
            raise TypeError(f"{_WHO}: code_weights must be a sequence of numbers or a tensor, got "
                            f"{type(code_weights).__name__}") from None
        if len(cw_values) != D:
            raise ValueError(f"{_WHO}: code_weights must have shape [{D}], got {len(cw_values)} values")
    _mp.same_place(_WHO, dev, B, (("gt_boxes", gt), ("pred_ind", pind), ("gt_ind", gind), ("pred_ind.sample_sizes", counts),
                                  ("query_weights", weights)), ref="pred_boxes")

    mode, value, avg_dev = _nat.avg_factor_args(avg_factor, dev, _WHO, ValueError, "the boxes' device")
    params = _nat.MatchedBoxParams()
    params.iou_eps, params.avg_factor, params.avg_mode, params.iou_kind = iou_eps, value, mode, _IOU_KINDS[iou_kind]
    for d in range(D):
        params.code_weights[d] = 1.0 if cw_values is None else cw_values[d]
    params.avg_factor_dev = None if avg_dev is None else avg_dev.data_ptr()
    flags = (_nat.MB_IDX_I64 if pind.dtype == torch.int64 else 0) | _FORMATS[box_format]
    call = _Call(pred_boxes, gt, pind, flags, params, avg_dev)
    return _MatchedBoxLoss.apply(call, pred_boxes, gt, pind, gind, counts, weights, cw_dev)
