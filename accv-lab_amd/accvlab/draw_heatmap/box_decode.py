"""(extension) The prediction side of a CenterNet / FCOS-style camera head, the inverse of ``boxes_to_heatmap``: from the
top-K peaks of the heat map and the regression maps a head trained on ``BoxHeatmapTargets`` produces (``center_offset``,
``height_width``, optional extra channels) to the filtered, NMS'd, compacted xyxy boxes in image pixels — or, with the
matrix the image was prepared with, in source-image pixels — in one launch, without a host round trip and in a defined
order; and the axis-aligned NMS it needs as an operator of its own, ``nms_boxes``.

It replaces mmdet's ``CenterNetHead._decode_heatmap`` (two gathers, the corner arithmetic, the rescale) and the
``batched_nms`` behind it, for which the ROCm build of torch has no ``torchvision.ops.nms``: a per-frame greedy loop with a
read-back.  The float32 operation sequence is written out in ``csrc/box_decode_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch
from . import _detections as _det

MAX_K = _nat.BD_MAX_K
MAX_MAPS = _nat.BD_MAX_MAPS
MAX_EXTRAS = _nat.BD_MAX_EXTRAS
_DTYPES = _nat.FLOAT_DTYPE_CODES
_DEC = "box_heatmap_decode"
_NMS = "nms_boxes"


class BoxDetections(NamedTuple):
    """2D detections: RaggedBatch objects ``[F, M, ...]`` that share one ``sample_sizes`` (int64 ``[F]``)."""
    boxes: object    # float32 [F, M, 4] as (x1, y1, x2, y2)
    scores: object   # float32 [F, M]
    labels: object   # int64 [F, M]
    source: object   # int32 [F, M], the peak rank k
    extras: object   # float32 [F, M, E]


def _detections(boxes, scores, labels, source, extras, sizes):
    return BoxDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in (boxes, scores, labels, source, extras)))


def box_heatmap_decode(peaks, feats, *, image_hw, image_matrices=None, score_threshold=None, scores_are_logits: bool = False,
                       min_size=None, clip: bool = True, order_corners: bool = True, iou_threshold=None,
                       class_agnostic: bool = False, post_max_size=None) -> BoxDetections:
    """Boxes, scores and labels from the heat-map peaks and regression maps of a 2D head, in one launch.

    Args:
        peaks: a ``HeatmapPeaks`` from ``heatmap_peaks(heat, K, per_class=False)``.  Only ``scores`` (float32, float16 or
            bfloat16), ``indices`` and ``classes`` (int64) are read, each ``[F, K]`` and contiguous, 1 <= K <= 1024.
        feats: one ``[F, c, Hm, Wm]`` tensor or a sequence of up to 8 of them: contiguous, float32, float16 or bfloat16
            (one dtype), read in place and never concatenated.  Their channels, concatenated, are
            ``(off_x, off_y, h, w, extra_0 .. extra_{E-1})`` with 0 <= E <= 4: the layout of
            ``BoxHeatmapTargets.center_offset`` and ``.height_width`` (map pixels, ``h`` before ``w``).  The map extent
            ``(Hm, Wm)`` comes from here; each at most 2^24.
        image_hw: as for ``boxes_to_heatmap``: ``(H, W)`` Python ints for every frame, or an int32 / int64 tensor ``[F, 2]``
            on the peaks' device (read there); values are clamped to ``[0, 2^24]``.
        image_matrices: float32 ``[F, 2, 3]``, contiguous, on the peaks' device: the forward matrix (source image to prepared
            image) that ``prepare_images`` and ``camera_augment_boxes`` take; the written boxes go back through its inverse.
            ``None``: the boxes stay in the pixels of ``image_hw``.
        score_threshold: a number, or ``None`` for no score test.
        scores_are_logits: the score is ``sigmoid(scores)``: ``heatmap_peaks`` can then run on the raw logits.
        min_size: a number or an ``(h, w)`` pair in image pixels, or ``None`` for no size test.
        clip: clamp the corners to the image.
        order_corners: after ``image_matrices``, order the two corners per axis (a flip leaves ``x1 > x2`` otherwise).
        iou_threshold: a number, or ``None`` for no NMS.
        class_agnostic: a kept box suppresses boxes of every class, not only of its own.
        post_max_size: an integer >= 1, or ``None``.

    Per frame ``f`` and peak rank ``k``, in float32, every operation rounded once, in the rank order the peaks arrive in:

    1. ``ys = index // Wm``, ``xs = index % Wm``; an index outside ``[0, Hm * Wm)`` or a negative class makes the peak
       invalid, and nothing is read from the maps for it; float16 / bfloat16 values are widened exactly;
    2. ``cx = xs + off_x``, ``cy = ys + off_y``; map-space corners ``(cx - 0.5 * w, cy - 0.5 * h)`` and
       ``(cx + 0.5 * w, cy + 0.5 * h)``;
    3. ``x = x_map * ux`` and ``y = y_map * uy`` with ``ux = f32(Wi) / f32(Wm)``, ``uy = f32(Hi) / f32(Hm)`` (the
       reciprocal of the scale ``boxes_to_heatmap`` applies);
    4. with ``clip``, ``v = 0 if v < 0 else (E if v > E else v)`` with ``E = Wi`` for x and ``Hi`` for y;
    5. ``score = scores[f, k]``, or ``1 / (1 + exp(-scores[f, k]))`` with ``scores_are_logits``; valid iff
       ``score > score_threshold``, ``y2 - y1 >= min_size[0]`` and ``x2 - x1 >= min_size[1]`` (each where given) and all
       four coordinates are finite; NaN fails every comparison it takes part in;
    6. greedy IoU NMS where ``iou_threshold`` is given: walking the valid peaks in rank order, a peak is kept iff no earlier
       kept peak of its class (of any class with ``class_agnostic``) has ``iou > iou_threshold`` with it — strictly greater;
       ``inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1))``, ``iou = inter / ((area_a + area_b) - inter)`` with
       ``area = (x2 - x1) * (y2 - y1)``; a NaN IoU (``0 / 0``: two boxes without area) suppresses nothing, and for a
       threshold >= 0 a box without area is kept and suppresses nothing.  This is mmdet's ``batched_nms`` rule without its
       coordinate-offset trick: classes are compared, not moved apart;
    7. the kept peaks go, in rank order, to slots ``0 .. kept - 1``; only the first ``post_max_size`` are written, and the
       walk stops there; ``source`` is the peak rank, ``labels`` the peak's class, ``extras`` the extra channels at its cell;
    8. with ``image_matrices``, the two corners of each written box go through the inverse of the frame's matrix
       ``[[a, b, tx], [c, d, ty]]``: ``x' = (d * (x - tx) - b * (y - ty)) / det``, ``y' = (a * (y - ty) - c * (x - tx)) / det``,
       ``det = a * d - b * c`` — the inverse ``prepare_images`` samples the image with.  This happens after the NMS and the
       size test, which see the prepared image (``nms_boxes`` on the result of a call with ``image_matrices`` sees the
       source image instead).  With ``order_corners`` the pairs ``(x1', x2')`` and ``(y1', y2')`` are
       ordered.  **A matrix that is singular or not finite gives boxes ``(0, 0, 0, 0)`` for its frame; the count, scores,
       labels, source and extras of the frame are kept.**

    Returns: a :class:`BoxDetections`.  ``M = min(K, post_max_size)`` is known on the host; the five RaggedBatch objects
    share one int64 ``sample_sizes``.  Padding slots are written too: +0 everywhere, ``source`` = -1.

    Nothing takes a gradient.  GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame, no
    atomics, no workspace, no host synchronisation, bitwise reproducible, graph-capturable); CPU tensors run the library's
    serial host entry over the same arithmetic.  All outputs of the two are bit-equal, except the score under
    ``scores_are_logits``, which depends on ``exp`` and agrees to a few ulp.  ``F == 0`` gives empty outputs without a launch.
    """
    scores, indices, classes = _det.check_peaks(_DEC, peaks, "F", MAX_K)
    maps = _det.check_feats(_DEC, feats, scores, "F", MAX_MAPS)
    C = sum(m.shape[1] for m in maps)
    if not 4 <= C <= 4 + MAX_EXTRAS:
        raise RuntimeError(f"{_DEC}: the maps must hold 4..{4 + MAX_EXTRAS} channels in total (off_x, off_y, h, w and up to "
                           f"{MAX_EXTRAS} extras), feats holds {C}")
    F, K = scores.shape
    Hm, Wm = maps[0].shape[2], maps[0].shape[3]
    if Hm < 1 or Wm < 1 or Hm > (1 << 24) or Wm > (1 << 24) or Hm * Wm >= 2 ** 31:
        raise RuntimeError(f"{_DEC}: the maps must have 1 <= H, W <= 2^24 and H * W < 2^31, got {Hm} x {Wm}")
    dev = scores.device
    hw_t = image_hw if isinstance(image_hw, torch.Tensor) else None
    _ops.check_operands(_DEC, (("image_hw", hw_t), ("image_matrices", image_matrices)), scores, "peaks'")
    Hi, Wi = _ops.image_hw_args(_DEC, image_hw, hw_t, F, "F")
    if image_matrices is not None and (image_matrices.dtype != torch.float32 or tuple(image_matrices.shape) != (F, 2, 3)):
        raise RuntimeError(f"{_DEC}: image_matrices must be float32 [{F}, 2, 3], got {image_matrices.dtype} "
                           f"{tuple(image_matrices.shape)}")
    thr = _det.threshold(_DEC, "score_threshold", score_threshold)
    iou = _det.threshold(_DEC, "iou_threshold", iou_threshold)
    if min_size is None or _ops.is_number(min_size):
        size = None if min_size is None else (min_size, min_size)
    elif isinstance(min_size, (list, tuple)) and len(min_size) == 2 and all(_ops.is_number(v) for v in min_size):
        size = tuple(min_size)
    else:
        raise RuntimeError(f"{_DEC}: min_size must be a Python number, an (h, w) pair of them or None, got {min_size!r}")
    if size is not None and any(math.isnan(v) for v in size):
        raise RuntimeError(f"{_DEC}: min_size must not hold NaN, got {min_size!r}")
    post = _det.cut(_DEC, "post_max_size", post_max_size)

    M = K if post is None else min(K, post)
    E = C - 4
    boxes, out_scores, labels, source, extras = _det.empty_outputs((F, M), 4, dev, E)
    kept = _det.kept_sizes((F,), dev)
    if F:
        p = _nat.BoxDecodeParams()
        p.scores, p.indices, p.classes = scores.data_ptr(), indices.data_ptr(), classes.data_ptr()
        p.num_maps = len(maps)
        for n, m in enumerate(maps):
            p.maps[n], p.channels[n] = m.data_ptr(), m.shape[1]
        p.image_hw, p.image_hw_i64 = _ops.ptr(hw_t), 1 if hw_t is not None and hw_t.dtype == torch.int64 else 0
        p.image_matrices = _ops.ptr(image_matrices)
        p.image_h, p.image_w = Hi, Wi
        p.has_score_threshold, p.score_threshold = (0, 0.0) if thr is None else (1, thr)
        p.has_iou_threshold, p.iou_threshold = (0, 0.0) if iou is None else (1, iou)
        p.has_min_size = 0 if size is None else 1
        if size is not None:
            p.min_size[0], p.min_size[1] = float(size[0]), float(size[1])
        p.score_dtype, p.map_dtype = _DTYPES[scores.dtype], _DTYPES[maps[0].dtype]
        p.scores_are_logits, p.clip, p.order_corners, p.class_agnostic = (1 if v else 0 for v in (scores_are_logits, clip, order_corners,
                                                                                                   class_agnostic))
        args = (ctypes.addressof(p), F, K, Hm, Wm, M, boxes.data_ptr(), out_scores.data_ptr(), labels.data_ptr(), source.data_ptr(),
                _ops.ptr(extras) if E else None, kept.data_ptr())
        _ops.run("accv_box_decode", args, dev, _DEC, host_entry=_nat.HOST_ENTRY_NAMES["accv_box_decode"])
    return _detections(boxes, out_scores, labels, source, extras, kept)


def _check_detections(det):
    """boxes, scores, labels, source, extras and the shared sample sizes after every check"""
    if not isinstance(det, (list, tuple)) or len(det) != 5:
        raise RuntimeError(f"{_NMS}: detections must be a BoxDetections (boxes, scores, labels, source, extras)")
    names = ("boxes", "scores", "labels", "source", "extras")
    dtypes = (torch.float32, torch.float32, torch.int64, torch.int32, torch.float32)
    whats = ("[F, N, 4]", "[F, N]", "[F, N]", "[F, N]", "[F, N, E]")
    tensors = []
    for name, x, dtype, what in zip(names, det, dtypes, whats):
        if not _ops.is_ragged(x):
            raise RuntimeError(f"{_NMS}: detections.{name} must be a RaggedBatch")
        tensors.append(_det.check_tensor(_NMS, f"detections.{name}", x.tensor, dtype, what.count(",") + 1, what))
    boxes, extras = tensors[0], tensors[4]
    F, N = boxes.shape[0], boxes.shape[1]
    if boxes.shape[2] != 4:
        raise RuntimeError(f"{_NMS}: detections.boxes must be [F, N, 4] as (x1, y1, x2, y2), got {tuple(boxes.shape)}")
    if not 1 <= N <= MAX_K:
        raise RuntimeError(f"{_NMS}: N must be in 1..{MAX_K}, got {N}")
    if extras.shape[2] > MAX_EXTRAS:
        raise RuntimeError(f"{_NMS}: E must be in 0..{MAX_EXTRAS}, got {extras.shape[2]}")
    for name, x in zip(names[1:], tensors[1:]):
        if tuple(x.shape[:2]) != (F, N) or x.device != boxes.device:
            raise RuntimeError(f"{_NMS}: detections.{name} must be {(F, N) + tuple(x.shape[2:])} on {boxes.device}, got "
                               f"{tuple(x.shape)} on {x.device}")
    return (*tensors, _det.shared_sample_sizes(_NMS, "detections", names, det, F, boxes.device, "the five members share one tensor"))


def nms_boxes(detections, iou_threshold, *, class_agnostic: bool = False, pre_max_size=None, post_max_size=None) -> BoxDetections:
    """Axis-aligned greedy IoU NMS of ragged xyxy boxes per frame, in one launch.

    It stands where ``torchvision.ops.nms`` / ``batched_nms`` (mmdet's ``batched_nms`` with its ``pre_max_size`` /
    ``post_max_size``-style cuts) would, per frame.

    Args:
        detections: a :class:`BoxDetections`: what ``box_heatmap_decode(..., iou_threshold=None)`` returns.  Any five
            RaggedBatch objects ``(boxes [F, N, 4] float32 xyxy, scores [F, N] float32, labels [F, N] int64, source [F, N]
            int32, extras [F, N, E] float32)``, contiguous, on one device and sharing one int64 ``sample_sizes``, are
            accepted too; 1 <= N <= 1024, 0 <= E <= 4.
        iou_threshold: a number, or ``None``: the detections are copied through with only the two cuts applied.
        class_agnostic: a kept box suppresses boxes of every label, not only of its own.
        pre_max_size, post_max_size: integers >= 1, or ``None``.

    **The slot order is the priority order.  Nothing is sorted**: the decode writes its detections in descending score
    order, and any other input is taken in the order it arrives in.  ``scores`` are only copied.

    Per frame ``f``:

    1. only the first ``min(sample_sizes[f], pre_max_size)`` slots exist;
    2. walking the slots in order, a box is kept iff no earlier kept box of its label (of any label with
       ``class_agnostic``) has ``iou > iou_threshold`` with it — strictly greater; the IoU is step 6 of
       :func:`box_heatmap_decode`, in float32;
    3. a box with a coordinate that is not finite is kept and suppresses nothing;
    4. the walk stops once ``post_max_size`` boxes are kept;
    5. the kept slots go, in slot order, to output slots ``0 .. kept - 1``: ``boxes``, ``scores``, ``labels``, ``source`` and
       ``extras`` pass through bit for bit.

    Returns: a :class:`BoxDetections`.  ``M = min(N, pre_max_size, post_max_size)`` is known on the host; the five
    RaggedBatch objects share one int64 ``sample_sizes``.  Padding slots are written too: +0 everywhere, ``source`` = -1.

    Nothing takes a gradient.  GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame, no
    atomics, no workspace, no host synchronisation, bitwise reproducible); CPU tensors run the library's serial host entry
    over the same arithmetic, bit-equal.  ``F == 0`` gives empty outputs without a launch.
    """
    if hasattr(detections, "_asdict"):
        detections = tuple(detections)
    bx, sc, lb, src, ex, sizes = _check_detections(detections)
    thr = _det.threshold(_NMS, "iou_threshold", iou_threshold)
    pre, post = _det.cut(_NMS, "pre_max_size", pre_max_size), _det.cut(_NMS, "post_max_size", post_max_size)
    F, N, E = bx.shape[0], bx.shape[1], ex.shape[2]
    dev = bx.device
    M = min(v for v in (N, pre, post) if v is not None)
    boxes, scores, labels, source, extras = _det.empty_outputs((F, M), 4, dev, E)
    kept = _det.kept_sizes((F,), dev)
    if F:
        p = _nat.BoxNmsParams()
        p.boxes, p.scores, p.labels, p.source, p.sizes = (x.data_ptr() for x in (bx, sc, lb, src, sizes))
        p.extras = ex.data_ptr() if E else None
        p.has_threshold, p.iou_threshold = (0, 0.0) if thr is None else (1, thr)
        p.class_agnostic = 1 if class_agnostic else 0
        args = (ctypes.addressof(p), F, N, E, N if pre is None else pre, M, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                source.data_ptr(), extras.data_ptr() if E else None, kept.data_ptr())
        _ops.run("accv_box_nms", args, dev, _NMS, host_entry=_nat.HOST_ENTRY_NAMES["accv_box_nms"])
    return _detections(boxes, scores, labels, source, extras, kept)
