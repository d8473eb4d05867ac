"""(extension) Rotated BEV IoU and rotated NMS for centre-point detections: the ``rotate`` branch of mmdet3d's
``CenterHead.get_bboxes`` — ``nms_bev`` over mmcv's ``nms_rotated`` — on what ``center_point_decode(..., nms_threshold=None)``
leaves on the device, for every task of the head in one launch and without a host round trip; and the IoU underneath it
(mmcv's ``box_iou_rotated`` for BEV boxes) as an operator of its own.  The float32 operation sequence is written out in
``csrc/rotated_iou_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import List

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch
from . import _detections as _det
from .center_decode import CenterPointDetections

MAX_TASKS = _nat.RN_MAX_TASKS
MAX_N = _nat.RN_MAX_N
MIN_D = _nat.RN_MIN_D
MAX_D = _nat.RN_MAX_D
_IOU = "rotated_iou_bev"
_NMS = "rotated_nms_bev"


def rotated_iou_bev(boxes_a, boxes_b):
    """Pairwise rotated IoU of two ragged sets of BEV boxes ``(x, y, dx, dy, yaw)`` per frame.

    Args:
        boxes_a, boxes_b: RaggedBatch objects ``[B, Na, 5]`` and ``[B, Nb, 5]``, float32 and contiguous, on one device
            (CUDA or CPU), each with int64 ``sample_sizes`` ``[B]``.

    Returns: a RaggedBatch ``[B, Na, Nb]`` float32 with ``boxes_a``'s sample sizes; ``out[b, i, j]`` is the IoU of
    ``boxes_a[b, i]`` against ``boxes_b[b, j]``, and +0 where ``i`` or ``j`` lies beyond its sample size.

    Per pair, in float32, every operation rounded once (``csrc/rotated_iou_arith.h``):

    1. a box whose five values are not all finite, or with ``dx <= 0`` or ``dy <= 0``, has IoU +0 with every box;
    2. if the squared centre distance exceeds ``(r_A + r_B)**2`` (``r`` the half diagonal) the IoU is +0 — exact;
    3. A is moved into B's frame (translate by ``-centre_B``, rotate by ``-yaw_B``); its corner polygon is clipped with
       Sutherland-Hodgman against ``|x| <= dx_B / 2`` and ``|y| <= dy_B / 2``; the area is the shoelace sum relative to the
       first vertex.  The relative angle is ``yaw_A - yaw_B`` with the rounding error of that float32 subtraction recovered
       exactly and applied to first order, so accumulated headings many turns from zero cost nothing;
    4. ``iou = inter / (dx_A * dy_A + dx_B * dy_B - inter)``.

    Identical boxes give exactly 1, boxes that share only an edge 0; against a float64 polygon clip the error stays below
    1e-5 for ``|yaw| <= 4096`` rad (about 650 turns), strips with an aspect of thousands that lie on each other included
    (measured: ``profiles/rotated_nms_accuracy.log``).  Beyond that domain the value is still a finite number in [0, 1],
    but the bar is not promised: wrap such yaws first.  One more term is outside the bar: the centre offset is rotated
    into B's frame with float32 products, which adds up to ``7e-7 * d / w`` (``d`` the centre distance, ``w`` the
    smallest side of the pair) — nothing for boxes of ordinary aspect, 2e-5 measured for 50 x 0.02 strips that overlap
    metres apart along their length.  Nothing takes a gradient.  GPU tensors run one HIP kernel on
    torch's current stream, CPU tensors the library's serial host entry over the same arithmetic.
    """
    ta, tb = [_det.check_tensor(_IOU, name, getattr(x, "tensor", None), torch.float32, 3, "[B, N, 5]", each=True)
              for name, x in (("boxes_a", boxes_a), ("boxes_b", boxes_b))]
    if ta.shape[2] != 5 or tb.shape[2] != 5:
        raise RuntimeError(f"{_IOU}: the boxes must be [B, N, 5] as (x, y, dx, dy, yaw), got {tuple(ta.shape)} and {tuple(tb.shape)}")
    if ta.shape[0] != tb.shape[0]:
        raise RuntimeError(f"{_IOU}: boxes_a holds {ta.shape[0]} frames, boxes_b {tb.shape[0]}")
    if ta.device != tb.device:
        raise RuntimeError(f"{_IOU}: boxes_a is on {ta.device}, boxes_b on {tb.device}")
    B, Na, Nb = ta.shape[0], ta.shape[1], tb.shape[1]
    dev = ta.device
    sa, sb = _det.sizes_of(_IOU, "boxes_a", boxes_a, B, dev), _det.sizes_of(_IOU, "boxes_b", boxes_b, B, dev)
    out = torch.empty((B, Na, Nb), dtype=torch.float32, device=dev)
    if out.numel():
        args = (ta.data_ptr(), sa.data_ptr(), tb.data_ptr(), sb.data_ptr(), B, Na, Nb, out.data_ptr())
        _ops.run("accv_rotated_iou_bev", args, dev, _IOU)
    return RaggedBatch(out, sample_sizes=sa)


def _check_task(t, det, ref):
    """boxes, scores, labels, source and the shared sample sizes of task t after every check; `ref` is task 0's boxes"""
    if not isinstance(det, (list, tuple)) or len(det) != 4:
        raise RuntimeError(f"{_NMS}: detections[{t}] must be a CenterPointDetections (boxes, scores, labels, source)")
    names = ("boxes", "scores", "labels", "source")
    dtypes = (torch.float32, torch.float32, torch.int64, torch.int32)
    tensors = []
    for name, x, dtype in zip(names, det, dtypes):
        if not _ops.is_ragged(x):
            raise RuntimeError(f"{_NMS}: detections[{t}].{name} must be a RaggedBatch")
        rank = 3 if name == "boxes" else 2
        tensors.append(_det.check_tensor(_NMS, f"detections[{t}].{name}", x.tensor, dtype, rank, "[B, N, D]" if rank == 3 else "[B, N]",
                                         each=True))
    boxes = tensors[0]
    ref = boxes if ref is None else ref
    B, N, D = boxes.shape
    if not 1 <= N <= MAX_N:
        raise RuntimeError(f"{_NMS}: N must be in 1..{MAX_N}, got {N}")
    if not MIN_D <= D <= MAX_D:
        raise RuntimeError(f"{_NMS}: D must be in {MIN_D}..{MAX_D} (x, y, z, dx, dy, dz, yaw, ...), got {D}")
    if boxes.shape != ref.shape or boxes.device != ref.device:
        raise RuntimeError(f"{_NMS}: detections[{t}].boxes is {tuple(boxes.shape)} on {boxes.device}, detections[0].boxes "
                           f"{tuple(ref.shape)} on {ref.device}: all tasks share B, N, D and device")
    for name, x in zip(names[1:], tensors[1:]):
        if tuple(x.shape) != (B, N) or x.device != boxes.device:
            raise RuntimeError(f"{_NMS}: detections[{t}].{name} must be {(B, N)} on {boxes.device}, got {tuple(x.shape)} on {x.device}")
    return (*tensors, _det.shared_sample_sizes(_NMS, f"detections[{t}]", names, det, B, boxes.device,
                                               "the four members of a task share one tensor"))


def rotated_nms_bev(detections, iou_threshold, *, pre_max_size=None, post_max_size=None) -> List[CenterPointDetections]:
    """Rotated BEV NMS of the detections of every task, in one launch.

    It replaces, in the ``rotate`` branch of mmdet3d's ``CenterHead.get_bboxes``, ``nms_bev`` and the mmcv operator
    ``nms_rotated`` under it, with their ``pre_max_size`` / ``post_max_size`` cuts, per frame and task.

    Args:
        detections: one :class:`CenterPointDetections` or a list of ``T`` of them (1 <= T <= 8): what
            ``center_point_decode(..., nms_threshold=None)`` returns.  Any four RaggedBatch objects ``(boxes [B, N, D]
            float32, scores [B, N] float32, labels [B, N] int64, source [B, N] int32)``, contiguous, on one device and
            sharing one int64 ``sample_sizes``, are accepted too; 1 <= N <= 1024, 7 <= D <= 16 with the box columns
            ``(x, y, z, dx, dy, dz, yaw, ...)``.  All tasks share ``B``, ``N``, ``D`` and device.
        iou_threshold: a number, a sequence of ``T`` numbers or ``None`` s, or ``None``.  A task without a threshold is
            copied through with only the two cuts applied.
        pre_max_size, post_max_size: integers >= 1, or ``None``.

    **The slot order is the priority order.  Nothing is sorted**: the decode writes its detections in descending score
    order, and any other input is taken in the order it arrives in.

    Per frame ``b`` and task ``t``:

    1. only the first ``min(sample_sizes[b], pre_max_size)`` slots exist;
    2. the BEV box of a slot is columns ``(0, 1, 3, 4, 6)`` of its row: ``(x, y, dx, dy, yaw)``;
    3. walking the slots in order, a box is kept iff no earlier kept box has ``iou > iou_threshold[t]`` with it — strictly
       greater, mmcv's rule; the IoU is that of :func:`rotated_iou_bev`, the later box against the kept one, within 1e-5
       of the float64 value for ``|yaw| <= 4096`` rad (about 650 turns);
    4. a box whose five BEV values are not all finite, or with ``dx <= 0`` or ``dy <= 0``, is kept and suppresses nothing;
    5. the walk stops once ``post_max_size`` boxes are kept;
    6. the kept slots go, in slot order, to output slots ``0 .. kept - 1``: all ``D`` box columns, ``scores``, ``labels``
       and ``source`` pass through bit for bit.

    Returns: a list with one :class:`CenterPointDetections` per task.  ``M = min(N, pre_max_size, post_max_size)`` is known
    on the host.  The ``T`` entries are views ``out[t]`` of single ``[T, B, M, ...]`` allocations, and the four RaggedBatch
    objects of a task share one int64 ``sample_sizes``.  Padding slots are written too: +0 everywhere, ``source`` = -1.
    ``source`` stays the peak rank the decode wrote, so ``gather_at_centers`` at
    ``peaks[t].indices.gather(1, d.source.tensor.clamp(min=0).long())`` still finds the cells of the kept detections.

    Nothing takes a gradient.  GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame and task,
    no atomics, no workspace, no host synchronisation, bitwise reproducible); CPU tensors run the library's serial host
    entry over the same arithmetic.  ``B == 0`` gives empty outputs without a launch.
    """
    if hasattr(detections, "boxes") or (isinstance(detections, (list, tuple)) and len(detections) == 4
                                        and all(hasattr(x, "sample_sizes") for x in detections)):
        detections = [detections]
    if not isinstance(detections, (list, tuple)) or not 1 <= len(detections) <= MAX_TASKS:
        raise RuntimeError(f"{_NMS}: detections must be a CenterPointDetections or a sequence of 1..{MAX_TASKS} of them")
    T = len(detections)
    per_task = []
    for t, det in enumerate(detections):
        per_task.append(_check_task(t, det, per_task[0][0] if per_task else None))
    if iou_threshold is None or (isinstance(iou_threshold, (int, float)) and not isinstance(iou_threshold, bool)):
        thr = [iou_threshold] * T
    elif isinstance(iou_threshold, (list, tuple)) and len(iou_threshold) == T:
        thr = list(iou_threshold)
    else:
        raise RuntimeError(f"{_NMS}: iou_threshold must be a number, a sequence of {T} numbers or Nones (one per task) or None, "
                           f"got {iou_threshold!r}")
    for t, v in enumerate(thr):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise RuntimeError(f"{_NMS}: iou_threshold[{t}] must be a Python number or None, got {v!r}")
        if math.isnan(v):
            raise RuntimeError(f"{_NMS}: iou_threshold[{t}] must not be NaN")
    pre, post = _det.cut(_NMS, "pre_max_size", pre_max_size, " or None"), _det.cut(_NMS, "post_max_size", post_max_size, " or None")

    boxes0 = per_task[0][0]
    B, N, D = boxes0.shape
    dev = boxes0.device
    M = min(v for v in (N, pre, post) if v is not None)
    boxes, scores, labels, source = _det.empty_outputs((T, B, M), D, dev)
    kept = _det.kept_sizes((T, B), dev)
    if B:
        p = _nat.RotatedNmsParams()
        for t, (bx, sc, lb, src, sizes) in enumerate(per_task):
            p.boxes[t], p.scores[t], p.labels[t], p.source[t], p.sizes[t] = (x.data_ptr() for x in (bx, sc, lb, src, sizes))
            p.has_threshold[t], p.iou_threshold[t] = (0, 0.0) if thr[t] is None else (1, float(thr[t]))
        p.num_tasks = T
        args = (ctypes.addressof(p), B, N, D, N if pre is None else pre, M, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                source.data_ptr(), kept.data_ptr())
        _ops.run("accv_rotated_nms_bev", args, dev, _NMS)
    out = []
    for t, sizes_t in enumerate(kept.unbind(0)):     # one sample_sizes tensor per task, shared by its four outputs
        out.append(CenterPointDetections(*(RaggedBatch(x[t], sample_sizes=sizes_t) for x in (boxes, scores, labels, source))))
    return out
