"""(extension) Set prediction over polylines — what a MapTR-style vectorised map head or a lane-DETR head needs between
its decoder output and its criterion: the ``[B, Q, G_max]`` matching cost, the Hungarian matching on it and the loss over
the matched pairs.

A polyline is an ordered point list, but its identity is not ordered: an open line equals its reverse, a closed polygon
all of its cyclic shifts in both directions.  Cost and loss therefore take the minimum over the equivalent orders of the
point-wise L1 distance.  The torch composition materialises a ``[B, Q, G, V, P, D]`` tensor for that; here no order is ever
written to memory: one launch for the cost, two launches forward and one write-only launch backward for the loss.

GPU tensors run the HIP kernels (``accv_polyline_matching_cost``, ``accv_matched_polyline_loss`` / ``_bwd``); CPU tensors run
the host implementation of the same operation sequence (the ``_host`` entries).  There is no CPU fallback for GPU tensors.

Equivalent orders of a ground-truth line ``t`` of ``P`` points::

    open line      t^0[p] = t[p];               reversible: also t^1[p] = t[P - 1 - p]
    closed line    t^s[p] = t[(s + p) mod P];   reversible: also t^(P + s)[p] = t[(s - p) mod P]       (s < P)

``v*(x, t)`` is the lowest ``v`` that minimises ``sum_{p, d} |x[p, d] - t^v[p, d]|`` in the arithmetic type (float16 /
bfloat16 are widened exactly and evaluated in float32, float64 in float64).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from ... import _amd_native as _nat
from ..._amd_native import operands as _ops
from ...batching_helpers import _matched_pairs as _mp
from ...batching_helpers.assignment import batched_linear_sum_assignment
from ...batching_helpers.ragged import RaggedBatch

__all__ = ["batched_polyline_matching_cost", "batched_polyline_hungarian_match", "matched_polyline_loss"]

_DTYPES = _mp.DTYPES
_KINDS = {"one_minus_prob": _nat.MC_ONE_MINUS_PROB, "neg_prob": _nat.MC_NEG_PROB, "focal": _nat.MC_FOCAL}
_CLOSED_FLAGS = {torch.bool: 0, torch.uint8: 0, torch.int32: _nat.PM_CLOSED_I32, torch.int64: _nat.PM_CLOSED_I64}


def _lines(who, pred_lines, gt_lines):
    """-> (gt tensor, B, Q, G, P, D, stride_b, stride_q) of validated lines"""
    _mp.dense(who, "pred_lines", pred_lines, "[B, Q, P, D]", unit_stride=False)
    B, Q, P, D = (int(v) for v in pred_lines.shape)
    if not _nat.PM_MIN_P <= P <= _nat.PM_MAX_P:
        raise ValueError(f"{who}: needs {_nat.PM_MIN_P} <= P <= {_nat.PM_MAX_P}, got P = {P}")
    if D not in (2, 3):
        raise ValueError(f"{who}: needs D of 2 or 3, got D = {D}")
    if pred_lines.stride(3) != 1 or pred_lines.stride(2) != D:
        raise ValueError(f"{who}: the last two dimensions of pred_lines must be contiguous, got strides {pred_lines.stride()}")
    _mp.not_overlapping(who, "pred_lines", pred_lines, P * D)
    gt = _mp.ragged(who, "gt_lines", gt_lines, "[B, G*, P, D]", 4)
    if gt.dtype != pred_lines.dtype:
        raise TypeError(f"{who}: gt_lines is {gt.dtype}, pred_lines {pred_lines.dtype}")
    if tuple(gt.shape[2:]) != (P, D):
        raise ValueError(f"{who}: gt_lines has lines of shape {tuple(gt.shape[2:])}, pred_lines {(P, D)}")
    # a dimension of extent 1 may carry any stride
    sq = pred_lines.stride(1) if Q > 1 else P * D
    sb = pred_lines.stride(0) if B > 1 else Q * max(sq, P * D)
    return gt, B, Q, int(gt.shape[1]), P, D, sb, sq


def _closed(who, gt_closed, gt_lines, B, G, dev):
    """-> (tensor or None, flag)"""
    if gt_closed is None:
        return None, 0
    t = _mp.ragged(who, "gt_closed", gt_closed, "[B, G*]", 2)
    if t.dtype not in _CLOSED_FLAGS:
        raise TypeError(f"{who}: gt_closed must be bool, uint8, int32 or int64, got {t.dtype}")
    if tuple(t.shape) != (B, G):
        raise ValueError(f"{who}: gt_closed has shape {tuple(t.shape)}, gt_lines has [B, G_max] = {[B, G]}")
    if t.device != dev:
        raise ValueError(f"{who}: gt_closed is on {t.device}, pred_lines on {dev}")
    return t, _CLOSED_FLAGS[t.dtype]


def batched_polyline_matching_cost(pred_lines: Optional[torch.Tensor], gt_lines: Optional[RaggedBatch], pred_scores=None,
                                   gt_labels=None, *, gt_closed: Optional[RaggedBatch] = None, reversible: bool = True,
                                   pts_weight: float = 1.0, class_cost: str = "one_minus_prob", class_weight: float = 0.0,
                                   focal_alpha: float = 0.25, focal_gamma: float = 2.0, focal_eps: float = 1e-12,
                                   filler: float = 0.0) -> RaggedBatch:
    """Weighted matching costs of every (predicted line, ground-truth line) pair of a batch, as the ragged
    ``[B, Q, G_max]`` cost that ``batched_linear_sum_assignment`` consumes::

        cost[b, q, g] = class_weight * cls(q, l_g) + pts_weight * min_v sum_{p, d} |x_q[p, d] - t_g^v[p, d]|

    Args:
        pred_lines: dense ``[B, Q, P, D]``, float32 / float16 / bfloat16 / float64, ``2 <= P <= 128``, ``D`` 2 or 3.  The last
            two dimensions are contiguous; the batch and query strides are free (a slice of a wider decoder output needs no
            copy).
        gt_lines: RaggedBatch ``[B, G*, P, D]`` of the same dtype, each lane already resampled to ``P`` points
            (``interpolate``).
        pred_scores, gt_labels: dense ``[B, Q, C]`` and RaggedBatch ``[B, G*]`` (int32 / int64) of the class term, which is
            ``batched_matching_cost``'s: probabilities for ``"one_minus_prob"`` / ``"neg_prob"``, logits for ``"focal"``.
        gt_closed: optional RaggedBatch ``[B, G*]`` (bool / uint8 / int32 / int64) with the ground truth's sample sizes;
            non-zero marks a closed polygon of ``P`` distinct vertices (no repeated end point).  ``None``: every line is open.
        reversible: whether a line equals its reverse (see the module text for the equivalent orders).
        pts_weight, class_weight: a term whose weight is 0 is not evaluated; its inputs may be ``None``.
        class_cost, focal_alpha, focal_gamma, focal_eps: as in ``batched_matching_cost``.
        filler: value of the padded columns ``[G_b, G_max)``.

    The sample sizes come from ``gt_lines`` (from ``gt_labels`` when ``pts_weight`` is 0); they are read on the device,
    clamped to ``[0, G_max]``.  NaN in any coordinate of a pair gives NaN for that pair only; a label outside ``[0, C)``
    gives a NaN class term.  No autograd.  One launch on torch's current stream, no synchronisation.

    Returns:
        RaggedBatch ``[B, Q, G_max]``, contiguous, ``non_uniform_dim=2``, sharing the ground truth's sample sizes; float32
        (float64 for float64 inputs); padded columns hold exactly ``filler``.
    """
    who = "batched_polyline_matching_cost"
    if class_cost not in _KINDS:
        raise ValueError(f"{who}: class_cost must be one of {sorted(_KINDS)}, got {class_cost!r}")
    pts_weight, class_weight = float(pts_weight), float(class_weight)
    use_pts, use_cls = pts_weight != 0.0, class_weight != 0.0
    scores = labels = gt = closed = None
    closed_flag = 0
    if use_pts or pred_lines is not None:
        gt, B, Q, G, P, D, sb, sq = _lines(who, pred_lines, gt_lines)
        dev, dtype, sizes_rb = pred_lines.device, pred_lines.dtype, gt_lines
        closed, closed_flag = _closed(who, gt_closed, gt_lines, B, G, dev)
    if use_cls or gt is None:
        if not isinstance(pred_scores, torch.Tensor):
            raise TypeError(f"{who}: pred_scores must be a tensor (needed by the class cost), got {type(pred_scores).__name__}")
        if pred_scores.dim() != 3:
            raise ValueError(f"{who}: pred_scores must be [B, Q, C], got shape {tuple(pred_scores.shape)}")
        if pred_scores.shape[-1] > 1 and pred_scores.stride(-1) != 1:
            raise ValueError(f"{who}: the last dimension of pred_scores must have unit stride, got stride "
                             f"{pred_scores.stride(-1)}")
        scores = pred_scores.detach()
        labels = _mp.index(who, "gt_labels", gt_labels, "[B, G*]")
        if gt is None:
            B, Q, G, P, D, sb, sq = int(scores.shape[0]), int(scores.shape[1]), int(labels.shape[1]), 2, 2, 0, 4
            dev, dtype, sizes_rb = scores.device, scores.dtype, gt_labels
            if dtype not in _DTYPES:
                raise TypeError(f"{who}: pred_scores must be float32, float16, bfloat16 or float64, got {dtype}")
        if scores.dtype != dtype:
            raise TypeError(f"{who}: pred_scores is {scores.dtype}, pred_lines {dtype}: all float inputs must share one dtype")
        if tuple(scores.shape[:2]) != (B, Q):
            raise ValueError(f"{who}: pred_scores has shape {tuple(scores.shape)}, expected [{B}, {Q}, C]")
        if int(labels.shape[1]) != G:
            raise ValueError(f"{who}: gt_labels has {labels.shape[1]} objects per frame, expected {G}")
    _mp.same_place(who, dev, B, (("gt_lines", gt), ("pred_scores", scores), ("gt_labels", labels),
                                 ("sample sizes", sizes_rb.sample_sizes)))

    out = torch.empty((B, Q, G), dtype=torch.float64 if dtype == torch.float64 else torch.float32, device=dev)
    if B * Q * G > 0:
        counts = sizes_rb.sample_sizes.to(dtype=torch.int64).contiguous()
        p = _nat.PolylineMatchParams()
        p.class_weight, p.pts_weight, p.filler = class_weight, pts_weight, float(filler)
        p.focal_alpha, p.focal_gamma, p.focal_eps = float(focal_alpha), float(focal_gamma), float(focal_eps)
        p.pred_stride_b, p.pred_stride_q, p.class_kind = sb, sq, _KINDS[class_cost]
        p.gt_closed = _ops.ptr(closed)
        flags = ((_nat.PM_REVERSIBLE if reversible else 0) | closed_flag
                 | (_nat.PM_LABELS_I64 if labels is not None and labels.dtype == torch.int64 else 0))
        args = (pred_lines.data_ptr() if gt is not None else 0, gt.data_ptr() if gt is not None else 0,
                scores.data_ptr() if scores is not None else 0, labels.data_ptr() if labels is not None else 0,
                counts.data_ptr(), _DTYPES[dtype], flags, B, Q, G, P, D, int(scores.shape[2]) if scores is not None else 0,
                scores.stride(0) if scores is not None else 0, scores.stride(1) if scores is not None else 0,
                ctypes.addressof(p), out.data_ptr())
        _ops.run("accv_polyline_matching_cost", args, dev, who)
    return sizes_rb.create_with_sample_sizes_like_self(out, non_uniform_dim=2)


def batched_polyline_hungarian_match(pred_lines, gt_lines, pred_scores=None, gt_labels=None, *, gt_closed=None,
                                     reversible: bool = True, pts_weight: float = 1.0, class_cost: str = "one_minus_prob",
                                     class_weight: float = 0.0, focal_alpha: float = 0.25, focal_gamma: float = 2.0,
                                     focal_eps: float = 1e-12, filler: float = 0.0, maximize: bool = False,
                                     check: bool = True):
    """``batched_linear_sum_assignment(batched_polyline_matching_cost(...), maximize=maximize, check=check)``: the Hungarian
    matching of a polyline head in two launches, with no host synchronisation when ``check=False``.  Returns what
    ``batched_hungarian_match`` returns: ``(pred_ind, gt_ind)`` or, with ``check=False``, ``(pred_ind, gt_ind, status)``."""
    cost = batched_polyline_matching_cost(pred_lines, gt_lines, pred_scores, gt_labels, gt_closed=gt_closed,
                                          reversible=reversible, pts_weight=pts_weight, class_cost=class_cost,
                                          class_weight=class_weight, focal_alpha=focal_alpha, focal_gamma=focal_gamma,
                                          focal_eps=focal_eps, filler=filler)
    return batched_linear_sum_assignment(cost, maximize=maximize, check=check)


_WHO = "matched_polyline_loss"
_STEM = "accv_matched_polyline_loss"


class _Call:
    """the geometry and scalar parameters that the forward and the backward C-ABI calls of one invocation share; it holds
    no tensor a kernel reads (avg_dev is read by the forward alone)"""

    def __init__(self, lines, pind, flags, params, avg_dev, dims):
        self.params, self.avg_dev = params, avg_dev
        self.dev = lines.device
        self.B, self.Q, self.G, self.P, self.D = dims
        self.K = int(pind.shape[1])
        self.flags = flags
        self.out_dtype = _mp.out_dtype(lines.dtype)

    def inputs(self, lines, gt, pind, gind, counts, closed):
        """the pointer arguments; the optional operand goes into the parameter struct"""
        self.params.gt_closed = None if closed is None else closed.data_ptr()
        return (lines.data_ptr(), gt.data_ptr(), pind.data_ptr(), gind.data_ptr(), counts.data_ptr())

    def shape(self, lines):
        return (_DTYPES[lines.dtype], self.flags, self.B, self.Q, self.G, self.P, self.D, self.K,
                ctypes.addressof(self.params))


class _MatchedPolylineLoss(torch.autograd.Function):
    """-> (point sums [B], direction sums [B]), the two rows of one [2, B] tensor"""

    @staticmethod
    def forward(ctx, call, lines, gt, pind, gind, counts, closed):
        tensors = (lines, gt, pind, gind, counts, closed)
        run = call.B * call.Q * call.K > 0
        out, denom = _mp.run_forward(_WHO, _STEM, call, tensors, run, 2, (call.B, call.Q))
        ctx.call, ctx.run = call, run
        # everything the backward kernel reads: alive until then, and guarded by torch's version check
        ctx.save_for_backward(denom, *tensors)
        ctx.set_materialize_grads(False)   # an unused output arrives as None and goes down as a null pointer
        return out[0], out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_pts, grad_dir):
        call = ctx.call
        denom, *tensors = ctx.saved_tensors
        lines = tensors[0]
        if not ctx.needs_input_grad[1]:
            return (None,) * 7
        if not ctx.run:   # no pair anywhere: nothing depends on the lines
            return (None, torch.zeros(lines.shape, dtype=lines.dtype, device=call.dev)) + (None,) * 5
        return (None, _mp.run_backward(_WHO, _STEM, call, tensors, (grad_pts, grad_dir), denom)) + (None,) * 5


def matched_polyline_loss(pred_lines: torch.Tensor, gt_lines: RaggedBatch, pred_ind: RaggedBatch, gt_ind: RaggedBatch, *,
                          gt_closed: Optional[RaggedBatch] = None, reversible: bool = True, dir_loss: bool = True,
                          dir_eps: float = 1e-12,
                          avg_factor: Optional[Union[float, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-frame polyline losses ``(loss_pts [B], loss_dir [B])`` over the matched pairs, both divided by the number of
    matched pairs and neither multiplied by a term weight: a criterion forms
    ``w_cls * matched_focal_loss(...) + w_pts * loss_pts + w_dir * loss_dir``.

    Args:
        pred_lines, gt_lines, gt_closed, reversible: as in ``batched_polyline_matching_cost``.  ``gt_lines`` is never
            differentiated.
        pred_ind, gt_ind: RaggedBatch ``[B, K]``, int32 / int64, one dtype — what ``batched_polyline_hungarian_match``
            returns.  ONLY ``pred_ind.sample_sizes`` is read (on the device, clamped to ``[0, K]``).
        dir_loss: ``False`` evaluates nothing for the second output and returns zeros.
        dir_eps: added to both squared segment lengths under the root of the cosine.
        avg_factor: ``None`` divides by ``max(M, 1)`` with ``M = sum_b clamp(n_b, 0, K)`` counted on the device; a Python
            number is used as given; a 0-d float32 tensor on the lines' device is read on the device.

    Definition (its float64 evaluation with autograd on the dtype-rounded inputs is what the tests pin), with the pair rule
    of ``matched_box_loss`` (slots at or past ``n_b`` are never read, out-of-range indices are skipped, a query named twice
    takes the lowest slot) and ``t* = t_g^(v*)``::

        loss_pts[b] += sum_{p, d} |x[p, d] - t*[p, d]|
        loss_dir[b] += sum_s (1 - <a_s, b_s> / sqrt((|a_s|^2 + dir_eps) (|b_s|^2 + dir_eps)))
        a_s = x[s+1] - x[s],  b_s = t*[s+1] - t*[s];  s = 0 .. P-2 (open),  0 .. P-1 with s + 1 mod P (closed)

    A frame without pairs gives 0; ``B``, ``Q`` or ``K`` of 0 give zeros and launch nothing.

    Returns two ``[B]`` tensors, float32 (float64 for float64 lines).  Differentiable w.r.t. ``pred_lines`` only, for either
    or both outputs (no double backward).  The tensors read by the backward (both line tensors, both index tensors,
    ``pred_ind.sample_sizes``, ``gt_closed``) are saved; modifying them in place before ``backward()`` raises.  ``v*`` is a
    constant of the backward (what ``torch.min(dim)`` and a gather by order index do) and is searched again there; ``|0|``
    has gradient 0.  The gradient has the lines' dtype, is contiguous
    and written completely, ``+0`` for unmatched queries, without atomics or a zero fill.  Per-frame sums are accumulated in
    float64 in a fixed order: both directions are bitwise reproducible, run on torch's current stream without host
    synchronisation and can be captured into a graph.  Two launches forward, one backward.

    Special values: a NaN coordinate in a matched prediction makes its frame's sums and that query's gradient NaN; rows of
    unmatched queries are never read.
    """
    gt, B, Q, G, P, D, sb, sq = _lines(_WHO, pred_lines, gt_lines)
    dev = pred_lines.device
    closed, closed_flag = _closed(_WHO, gt_closed, gt_lines, B, G, dev)
    dir_eps = float(dir_eps)
    if not dir_eps >= 0.0:
        raise ValueError(f"{_WHO}: dir_eps must be >= 0, got {dir_eps}")
    pind, gind, counts = _mp.match_indices(_WHO, pred_ind, gt_ind)
    _mp.same_place(_WHO, dev, B, (("gt_lines", gt), ("pred_ind", pind), ("gt_ind", gind), ("pred_ind.sample_sizes", counts)))

    mode, value, avg_dev = _nat.avg_factor_args(avg_factor, dev, _WHO, ValueError, "the lines' device")
    params = _nat.PolylineMatchParams()
    params.dir_eps, params.avg_factor, params.avg_mode, params.dir_loss = dir_eps, value, mode, 1 if dir_loss else 0
    params.pred_stride_b, params.pred_stride_q = sb, sq
    params.avg_factor_dev = None if avg_dev is None else avg_dev.data_ptr()
    flags = ((_nat.PM_IDX_I64 if pind.dtype == torch.int64 else 0) | (_nat.PM_REVERSIBLE if reversible else 0) | closed_flag)
    call = _Call(pred_lines, pind, flags, params, avg_dev, (B, Q, G, P, D))
    return _MatchedPolylineLoss.apply(call, pred_lines, gt, pind, gind, counts, closed)
