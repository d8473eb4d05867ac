"""(extension) Sigmoid focal classification loss of a set-prediction head (DETR / StreamPETR / Focal head) over ALL
queries against the labels of the matched ground truth — the last link of the loss chain after
``batched_matching_cost``, ``batched_linear_sum_assignment`` and ``matched_pair_loss_sum``.

The torch composition gathers the labels through ``gt_ind``, writes them into a ``[B, Q]`` label tensor filled with the
background id, builds a ``[B, Q, C]`` one-hot target and runs a dozen element-wise launches forward and about twice that
backward.  Here the target is derived in the kernel: two launches forward, one write-only launch backward.

GPU tensors run the HIP kernels (``accv_matched_focal_loss`` / ``_bwd``); CPU tensors run the host implementation of the
same operation sequence (``accv_matched_focal_loss_host`` / ``_bwd_host``).  There is no CPU fallback for GPU tensors.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Union

import torch
from torch.autograd.function import once_differentiable

from .. import _amd_native as _nat
from . import _matched_pairs as _mp
from .ragged import RaggedBatch

__all__ = ["matched_focal_loss"]

_WHO = "matched_focal_loss"
_STEM = "accv_matched_focal_loss"
_DTYPES = _mp.DTYPES
_PARAMS = {}   # (alpha, gamma, mode, value) -> MatchedFocalParams without a device pointer


def _params(alpha, gamma, mode, value, avg_dev):
    if avg_dev is not None:   # carries a pointer: not shared between calls
        return _nat.MatchedFocalParams(alpha, gamma, value, mode, avg_dev.data_ptr())
    key = (alpha, gamma, mode, value)
    p = _PARAMS.get(key)
    if p is None:
        if len(_PARAMS) >= 64:
            _PARAMS.clear()
        p = _PARAMS[key] = _nat.MatchedFocalParams(alpha, gamma, value, mode, None)
    return p


class _Call:
    """the geometry and scalar parameters that the forward and the backward C-ABI calls of one invocation share; it holds
    no tensor a kernel reads (avg_dev is read by the forward alone)"""

    def __init__(self, logits, labels, pind, params, avg_dev):
        self.params, self.avg_dev = params, avg_dev
        self.dev = logits.device
        self.B, self.Q, self.C = (int(v) for v in logits.shape)
        self.G, self.K = int(labels.shape[1]), int(pind.shape[1])
        self.flags = (_nat.MF_IDX_I64 if pind.dtype == torch.int64 else 0) | \
                     (_nat.MF_LABELS_I64 if labels.dtype == torch.int64 else 0)
        self.out_dtype = _mp.out_dtype(logits.dtype)

    @staticmethod
    def inputs(logits, labels, pind, gind, counts, weights):
        return (logits.data_ptr(), labels.data_ptr(), pind.data_ptr(), gind.data_ptr(), counts.data_ptr(),
                None if weights is None else weights.data_ptr())

    def shape(self, logits):
        # a dimension of extent 1 may carry any stride
        sb = logits.stride(0) if self.B > 1 else self.Q * max(logits.stride(1), self.C)
        sq = logits.stride(1) if self.Q > 1 else self.C
        return (_DTYPES[logits.dtype], self.flags, self.B, self.Q, self.C, self.G, self.K, sb, sq,
                ctypes.addressof(self.params))


class _MatchedFocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, logits, labels, pind, gind, counts, weights):
        tensors = (logits, labels, pind, gind, counts, weights)
        out, denom = _mp.run_forward(_WHO, _STEM, call, tensors, call.B * call.Q * call.C > 0, 1, (call.B, call.Q, call.C))
        ctx.call = call
        # everything the backward kernel reads: alive until then, and guarded by torch's version check
        ctx.save_for_backward(denom, *tensors)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        call = ctx.call
        denom, *tensors = ctx.saved_tensors
        logits = tensors[0]
        if not ctx.needs_input_grad[1]:
            return (None,) * 7
        if logits.numel() == 0:
            return (None, torch.empty(logits.shape, dtype=logits.dtype, device=call.dev)) + (None,) * 5
        return (None, _mp.run_backward(_WHO, _STEM, call, tensors, (grad_out,), denom)) + (None,) * 5


def matched_focal_loss(pred_logits: torch.Tensor, gt_labels: RaggedBatch, pred_ind: RaggedBatch, gt_ind: RaggedBatch, *,
                       alpha: float = 0.25, gamma: float = 2.0, query_weights: Optional[torch.Tensor] = None,
                       avg_factor: Optional[Union[float, torch.Tensor]] = None) -> torch.Tensor:
    """Per-frame sigmoid focal loss ``[B]`` of all ``Q x C`` logits of a frame, where a matched query's target is the
    one-hot of its ground-truth label and every other query is background, divided by the number of matched pairs.

    Args:
        pred_logits: dense ``[B, Q, C]``, float32 / float16 / bfloat16 / float64.  Unit stride in the last dimension; the
            batch and query strides are free (``cls_scores[..., :C]`` of a wider tensor needs no copy).
        gt_labels: RaggedBatch ``[B, G*]``, int32 / int64.
        pred_ind, gt_ind: RaggedBatch ``[B, K]``, int32 / int64, one dtype — what ``batched_linear_sum_assignment`` /
            ``batched_hungarian_match`` return.  ONLY ``pred_ind.sample_sizes`` is read (on the device, clamped to
            ``[0, K]``); comparing the two would cost a synchronisation.
        alpha: weight of the positives, ``1 - alpha`` of the negatives; ``alpha < 0`` switches the blend off
            (torchvision's convention).
        gamma: focusing exponent, ``>= 0``.  2 runs as multiplications, other values through ``pow`` with
            ``torch.pow``'s semantics (``gamma == 0`` included).
        query_weights: optional dense ``[B, Q]`` of the logits dtype (mmdet's ``label_weights``); multiplies all ``C``
            terms of a query.  No gradient flows to it.
        avg_factor: ``None`` divides by ``max(M, 1)`` with ``M`` the number of pairs, ``sum_b clamp(n_b, 0, K)``, counted
            on the device (DETR's ``num_boxes``); a Python number is used as given (``1.0`` gives raw sums); a 0-d float32
            tensor on the logits' device (an all-reduced count) is read on the device.  No gradient flows to it.

    Definition (torchvision's ``sigmoid_focal_loss`` / mmdet's ``py_sigmoid_focal_loss`` on one-hot targets; its float64
    evaluation on the dtype-rounded inputs is what the tests pin)::

        t = zeros(B, Q, C)
        for b, j < clamp(n_b, 0, K):                       # ascending j
            q, g = pred_ind[b, j], gt_ind[b, j]
            if 0 <= q < Q and 0 <= g < G_max and no lower j named q:      # a pair with both indices in range names q
                l = gt_labels[b, g]
                if 0 <= l < C: t[b, q, l] = 1              # any other label: the query's row stays all-background
        p = x.sigmoid(); ce = binary_cross_entropy_with_logits(x, t, reduction="none")
        loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
        if alpha >= 0: loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
        if query_weights is not None: loss = loss * query_weights[..., None]
        out = loss.sum((1, 2)) / factor

    Indices outside their range are skipped, not wrapped; a label outside ``[0, C)`` means background (mmdet's "label
    C"); a query named twice takes the pair in the lowest slot; slots at or past ``n_b`` are never read.  A frame without
    pairs is all background.  ``B``, ``Q`` or ``C`` of 0 give zeros and launch nothing.

    Returns ``[B]`` float32 (float64 for float64 logits), so that it adds to what ``matched_pair_loss_sum`` returns.
    Differentiable w.r.t. ``pred_logits`` only (no double backward); the gradient has the logits' dtype and is contiguous.
    The tensors read by the backward (logits, labels, both index tensors, ``pred_ind.sample_sizes``, ``query_weights``) are
    saved; modifying them in place before ``backward()`` raises.
    float16 / bfloat16 logits are widened exactly and evaluated in float32, float64 in float64; ``s``, ``1 - s`` and both
    softplus values come from ``exp(-|x|)`` without cancellation; sums are accumulated in float64 in a fixed order, so
    forward and backward are bitwise reproducible.  Two launches forward, one backward (every gradient element written
    exactly once: no zero fill, no atomics), on torch's current stream, without host synchronisation or read-back: both
    directions can be captured into a graph.

    Special values: a NaN logit makes its frame's sum and its own gradient NaN, all other gradients stay finite.  A
    logit of ``+inf`` gives ``+inf`` loss and gradient ``1 - alpha`` as a negative, 0 and -0 as a positive; ``-inf`` gives
    ``+inf`` and ``-alpha`` as a positive, 0 and 0 as a negative (the limits; the float64 composition has ``inf * 0``
    there).
    """
    _mp.dense(_WHO, "pred_logits", pred_logits, "[B, Q, C]")
    dev = pred_logits.device
    _mp.not_overlapping(_WHO, "pred_logits", pred_logits, int(pred_logits.shape[2]))
    alpha, gamma = float(alpha), float(gamma)
    if not gamma >= 0.0:
        raise ValueError(f"{_WHO}: gamma must be >= 0, got {gamma}")
    if alpha != alpha:
        raise ValueError(f"{_WHO}: alpha is NaN")

    labels = _mp.index(_WHO, "gt_labels", gt_labels, "[B, G*]")
    pind, gind, counts = _mp.match_indices(_WHO, pred_ind, gt_ind)
    weights = _mp.query_weights(_WHO, query_weights, pred_logits, "pred_logits")
    _mp.same_place(_WHO, dev, int(pred_logits.shape[0]), (("gt_labels", labels), ("pred_ind", pind), ("gt_ind", gind),
                                                            ("pred_ind.sample_sizes", counts), ("query_weights", weights)),
                   ref="pred_logits")

    mode, value, avg_dev = _nat.avg_factor_args(avg_factor, dev, _WHO, ValueError, "the logits' device")
    call = _Call(pred_logits, labels, pind, _params(alpha, gamma, mode, value, avg_dev), avg_dev)
    return _MatchedFocalLoss.apply(call, pred_logits, labels, pind, gind, counts, weights)
