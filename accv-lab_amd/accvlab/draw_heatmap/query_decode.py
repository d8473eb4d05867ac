"""(extension) The prediction side of a set-prediction head (DETR, Deformable DETR, DINO, PETR / StreamPETR, BEVFormer,
DETR3D), the inverse of ``batched_hungarian_match`` + ``matched_focal_loss`` / ``matched_box_loss``: from the raw class
logits ``[B, Q, C]`` and box rows ``[B, Q, D]`` of the last decoder layer to the top ``max_num`` (query, class) pairs of every
frame, decoded, filtered and compacted — in one launch, without a host round trip and in a defined order.

``query_box_decode_3d`` replaces mmdet3d's ``NMSFreeCoder.decode`` with ``denormalize_bbox``, ``query_box_decode_2d`` mmdet's
``DETRHead._predict_by_feat_single``: each a sigmoid over all ``B * Q * C`` logits, a ``topk`` over ``Q * C`` (whose order of
equal scores is undefined), a div and a mod, a gather, about a dozen element-wise launches, two masks and one boolean index
per frame with a host round trip.  They return the types ``rotated_nms_bev`` and ``nms_boxes`` take; no NMS lives here.
The float32 operation sequence is written out in ``csrc/query_decode_arith.h``.

Out of scope: softmax-with-background heads (take the softmax and drop the background column first, then pass
``scores_are_logits=False``); a ``D`` other than 8, 10 (3D) or 4 (2D); regression outputs wider than ``D`` (slice and make
contiguous what the head appends).
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch
from . import _detections as _det
from .box_decode import BoxDetections
from .center_decode import CenterPointDetections

MAX_K = _nat.QD_MAX_K
_DTYPES = _nat.FLOAT_DTYPE_CODES
_D3 = "query_box_decode_3d"
_D2 = "query_box_decode_2d"


def _check_head(who, cls_scores, bbox_preds, max_num, widths):
    """(B, Q, C, D) after every check of the two head outputs and max_num"""
    for name, x, what in (("cls_scores", cls_scores, "[B, Q, C]"), ("bbox_preds", bbox_preds, "[B, Q, D]")):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor")
        if x.dim() != 3:
            raise RuntimeError(f"{who}: {name} must be {what}, got {tuple(x.shape)}")
        if x.dtype not in _DTYPES or x.dtype == torch.float64:
            raise RuntimeError(f"{who}: {name} must be float32, float16 or bfloat16, got {x.dtype}")
    _ops.check_backend(who, "cls_scores", cls_scores.device)
    _ops.check_operands(who, (("cls_scores", cls_scores), ("bbox_preds", bbox_preds)), cls_scores, "scores'")
    B, Q, C = cls_scores.shape
    D = bbox_preds.shape[2]
    if tuple(bbox_preds.shape[:2]) != (B, Q):
        raise RuntimeError(f"{who}: bbox_preds must be [{B}, {Q}, D] like cls_scores, got {tuple(bbox_preds.shape)}")
    if D not in widths:
        raise RuntimeError(f"{who}: bbox_preds must hold {' or '.join(str(w) for w in widths)} values per query, got {D}")
    if isinstance(max_num, bool) or not isinstance(max_num, int) or not 1 <= max_num <= MAX_K:
        raise RuntimeError(f"{who}: max_num must be an integer in 1..{MAX_K}, got {max_num!r}")
    if Q * C >= 2 ** 32 - 1:
        raise RuntimeError(f"{who}: Q * C = {Q} * {C} must stay below 2^32 - 1")
    if max_num > Q * C:
        raise RuntimeError(f"{who}: max_num = {max_num} exceeds Q * C = {Q * C}")
    return B, Q, C, D


def query_box_decode_3d(cls_scores, bbox_preds, max_num, *, score_threshold=None, post_center_range=None,
                        scores_are_logits: bool = True, bottom_center: bool = False) -> CenterPointDetections:
    """The top ``max_num`` 3D detections of every frame from the raw outputs of a set-prediction head, in one launch.

    Args:
        cls_scores: ``[B, Q, C]``, contiguous, float32, float16 or bfloat16, on a GPU or the CPU; read in place, never copied
            or transposed.  ``all_cls_scores[-1]`` of a ``[L, B, Q, C]`` head output is such a view.
        bbox_preds: ``[B, Q, D]``, contiguous, the same dtype set, on the same device; ``D`` is 8 or 10, the mmdet3d box code
            ``(cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy])``.
        max_num: a Python int, ``1 <= max_num <= 1024`` and ``max_num <= Q * C``; ``Q * C < 2^32 - 1``.
        score_threshold: a number, or ``None`` for no score test.
        post_center_range: six numbers ``(x0, y0, z0, x1, y1, z1)``, or ``None`` for no range test.
        scores_are_logits: the score is ``sigmoid(cls_scores)``; ``False`` takes the values as scores.
        bottom_center: the written ``z`` becomes ``z - dz * 0.5``, as for ``center_point_decode``.

    Per frame ``b``, in float32, every operation rounded once:

    1. **Selection.**  The ``Q * C`` values ``cls_scores[b].view(-1)`` are ranked by descending value, equal values by
       ascending flat index ``q * C + c``; -0.0 ties with +0.0; every NaN ranks above +inf, NaNs among themselves by index.
       This is ``torch.sort(x, descending=True, stable=True)`` cut at ``max_num``, the order ``heatmap_peaks`` defines.  The
       ranking is on the RAW value: sigmoid is monotone, so this is a top-k of ``sigmoid(x)`` without a sigmoid pass over
       all logits.  **Where the float32 sigmoid saturates (logits above about 17), distinct logits give equal scores and
       ``torch.topk`` leaves their order unspecified; here the logit, then the index, decide.**  For rank ``r``:
       ``q = index // C``, ``label = index % C``.
    2. ``score = x``, or ``1 / (1 + exp(-x))`` with ``scores_are_logits``; float16 / bfloat16 values are widened exactly.
    3. The row ``bbox_preds[b, q]`` becomes ``(cx, cy, cz, exp(w), exp(l), exp(h), atan2(sin, cos)[, vx, vy])``: mmdet3d's
       ``denormalize_bbox`` column order, which is the ``(x, y, z, dx, dy, dz, yaw, ...)`` order ``rotated_nms_bev`` reads.
       The row is valid iff ``score > score_threshold`` and ``post_center_range[0:3] <= (cx, cy, cz) <=
       post_center_range[3:6]``, each where given; NaN fails every comparison it takes part in.  With ``bottom_center`` the
       written ``z`` is ``cz - exp(h) * 0.5``, applied after the range test.
    4. The valid rows go, in rank order, to slots ``0 .. kept - 1`` of ``[B, M, ...]``, ``M = max_num``.

    Returns: a :class:`CenterPointDetections` ``(boxes [B, M, D - 1] float32, scores [B, M] float32, labels [B, M] int64,
    source [B, M] int32)`` of RaggedBatch objects that share one int64 ``sample_sizes``; ``source`` holds the query index
    ``q``.  Padding slots are written too: +0 everywhere, ``source`` = -1.  ``rotated_nms_bev(result, thr)`` takes it as it is.

    Nothing takes a gradient.  To train through the selected rows, or to pick their query embeddings, gather them again::

        d = query_box_decode_3d(cls_scores, bbox_preds, 300)
        rows = bbox_preds.gather(1, d.source.tensor.clamp(min=0).long()[..., None].expand(-1, -1, bbox_preds.shape[2]))

    GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame, no atomics on global memory, no
    workspace, no host synchronisation, bitwise reproducible, graph-capturable); CPU tensors run the library's serial host
    entry over the same arithmetic.  The integer outputs, the centre, the velocity and raw scores of the two are bit-equal;
    ``exp``, ``atan2`` and the sigmoid agree to a few ulp.  ``B == 0`` gives empty outputs without a launch.

    Out of scope: softmax-with-background heads, a ``D`` other than 8 or 10, regression outputs wider than ``D``.
    """
    B, Q, C, D = _check_head(_D3, cls_scores, bbox_preds, max_num, (8, 10))
    thr = _det.threshold(_D3, "score_threshold", score_threshold)
    rng = None
    if post_center_range is not None:
        if not isinstance(post_center_range, (list, tuple)) or len(post_center_range) != 6:
            raise RuntimeError(f"{_D3}: post_center_range must be a sequence of 6 numbers, got {post_center_range!r}")
        rng = [_ops.number(_D3, f"post_center_range[{i}]", v) for i, v in enumerate(post_center_range)]
        if any(math.isnan(v) for v in rng):
            raise RuntimeError(f"{_D3}: post_center_range must not hold NaN, got {post_center_range!r}")
    dev = cls_scores.device
    M = max_num
    boxes, scores, labels, source = _det.empty_outputs((B, M), D - 1, dev)
    kept = _det.kept_sizes((B,), dev)
    if B:
        p = _nat.QueryDecode3dParams()
        p.cls_scores, p.bbox_preds = cls_scores.data_ptr(), bbox_preds.data_ptr()
        p.has_score_threshold, p.score_threshold = (0, 0.0) if thr is None else (1, thr)
        p.has_post_center_range = 0 if rng is None else 1
        for n, v in enumerate(rng or ()):
            p.post_center_range[n] = v
        p.score_dtype, p.box_dtype = _DTYPES[cls_scores.dtype], _DTYPES[bbox_preds.dtype]
        p.scores_are_logits, p.bottom_center = (1 if scores_are_logits else 0), (1 if bottom_center else 0)
        args = (ctypes.addressof(p), B, Q, C, D, M, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), source.data_ptr(),
                kept.data_ptr())
        _ops.run("accv_query_decode_3d", args, dev, _D3, host_entry=_nat.HOST_ENTRY_NAMES["accv_query_decode_3d"])
    return CenterPointDetections(*(RaggedBatch(x, sample_sizes=kept) for x in (boxes, scores, labels, source)))


def query_box_decode_2d(cls_scores, bbox_preds, max_num, *, image_hw, image_matrices=None, score_threshold=None,
                        scores_are_logits: bool = True, box_format: str = "cxcywh", normalized: bool = True, clip: bool = True,
                        order_corners: bool = True) -> BoxDetections:
    """The top ``max_num`` 2D detections of every frame from the raw outputs of a set-prediction head, in one launch.

    Args:
        cls_scores, max_num, score_threshold, scores_are_logits: as for :func:`query_box_decode_3d`.
        bbox_preds: ``[B, Q, 4]``, contiguous, float32, float16 or bfloat16, on the scores' device.
        image_hw: as for ``box_heatmap_decode``: ``(H, W)`` Python ints for every frame, or an int32 / int64 tensor ``[B, 2]``
            on the scores' device (read there); values are clamped to ``[0, 2^24]``.
        image_matrices: float32 ``[B, 2, 3]``, contiguous, on the scores' device: the forward matrix (source image to prepared
            image) of ``prepare_images``; the written boxes go back through its inverse.  ``None``: the boxes stay in the
            pixels of ``image_hw``.
        box_format: ``"cxcywh"`` (DETR) or ``"xyxy"``.
        normalized: the rows are fractions of the image: ``x *= W``, ``y *= H``.
        clip: clamp the corners to the image.
        order_corners: after ``image_matrices``, order the two corners per axis.

    Per frame ``b``: selection and score are steps 1 and 2 of :func:`query_box_decode_3d`; then, in float32, every operation
    rounded once:

    3. ``"cxcywh"`` becomes ``(cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h)``, ``"xyxy"`` is taken as it is; with
       ``normalized``, ``x *= f32(Wi)`` and ``y *= f32(Hi)``; with ``clip``, the clamp of step 4 of ``box_heatmap_decode``.
       The row is valid iff ``score > score_threshold`` (where given) and all four coordinates are finite.
    4. With ``image_matrices``: step 8 of ``box_heatmap_decode`` on the written boxes, including its rule for a matrix that
       is singular or not finite (boxes ``(0, 0, 0, 0)``, everything else of the frame kept) and ``order_corners``.
    5. The valid rows go, in rank order, to slots ``0 .. kept - 1`` of ``[B, M, ...]``, ``M = max_num``.

    Returns: a :class:`BoxDetections` whose ``extras`` is ``[B, M, 0]``; ``source`` holds the query index ``q``; the five
    RaggedBatch objects share one int64 ``sample_sizes``.  Padding slots are written too: +0 everywhere, ``source`` = -1.
    ``nms_boxes(result, thr)`` takes it as it is.

    Nothing takes a gradient; gather through ``source`` as shown for :func:`query_box_decode_3d`.  GPU tensors run one HIP
    kernel on torch's current stream, CPU tensors the library's serial host entry; all outputs of the two are bit-equal
    except the score under ``scores_are_logits``, which agrees to a few ulp.  ``B == 0`` gives empty outputs without a launch.

    Out of scope: softmax-with-background heads, a ``D`` other than 4, regression outputs wider than ``D``.
    """
    B, Q, C, _ = _check_head(_D2, cls_scores, bbox_preds, max_num, (4,))
    if box_format not in ("cxcywh", "xyxy"):
        raise RuntimeError(f"{_D2}: box_format must be 'cxcywh' or 'xyxy', got {box_format!r}")
    hw_t = image_hw if isinstance(image_hw, torch.Tensor) else None
    _ops.check_operands(_D2, (("image_hw", hw_t), ("image_matrices", image_matrices)), cls_scores, "scores'")
    Hi, Wi = _ops.image_hw_args(_D2, image_hw, hw_t, B, "B")
    if image_matrices is not None and (image_matrices.dtype != torch.float32 or tuple(image_matrices.shape) != (B, 2, 3)):
        raise RuntimeError(f"{_D2}: image_matrices must be float32 [{B}, 2, 3], got {image_matrices.dtype} "
                           f"{tuple(image_matrices.shape)}")
    thr = _det.threshold(_D2, "score_threshold", score_threshold)
    dev = cls_scores.device
    M = max_num
    boxes, scores, labels, source, extras = _det.empty_outputs((B, M), 4, dev, 0)
    kept = _det.kept_sizes((B,), dev)
    if B:
        p = _nat.QueryDecode2dParams()
        p.cls_scores, p.bbox_preds = cls_scores.data_ptr(), bbox_preds.data_ptr()
        p.image_hw, p.image_hw_i64 = _ops.ptr(hw_t), 1 if hw_t is not None and hw_t.dtype == torch.int64 else 0
        p.image_matrices = _ops.ptr(image_matrices)
        p.image_h, p.image_w = Hi, Wi
        p.has_score_threshold, p.score_threshold = (0, 0.0) if thr is None else (1, thr)
        p.score_dtype, p.box_dtype = _DTYPES[cls_scores.dtype], _DTYPES[bbox_preds.dtype]
        p.scores_are_logits, p.cxcywh, p.normalized, p.clip, p.order_corners = (
            1 if v else 0 for v in (scores_are_logits, box_format == "cxcywh", normalized, clip, order_corners))
        args = (ctypes.addressof(p), B, Q, C, M, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), source.data_ptr(),
                kept.data_ptr())
        _ops.run("accv_query_decode_2d", args, dev, _D2, host_entry=_nat.HOST_ENTRY_NAMES["accv_query_decode_2d"])
    return BoxDetections(*(RaggedBatch(x, sample_sizes=kept) for x in (boxes, scores, labels, source, extras)))
