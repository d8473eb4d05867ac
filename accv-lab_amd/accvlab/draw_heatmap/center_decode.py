"""(extension) The prediction side of a centre-point head (CenterNet, CenterPoint and the BEV heads built on mmdet3d's
``CenterHead``), the inverse of ``center_point_targets``: from the top-K peaks of every task's heat map and its regression
maps to the filtered, circle-NMS'd, compacted detections — for every task of the head in one launch, without a host round
trip and in a defined order.

It replaces mmdet3d's ``CenterPointBBoxCoder.decode`` (five gathers, ``exp``, ``atan2``, the affine map back to metres, two
masks and a boolean index per frame) and the ``circle`` branch of ``CenterHead.get_bboxes`` (``circle_nms``, a numba loop
on the host, and the ``post_max_size`` cut); the float32 operation sequence is written out in
``csrc/center_decode_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Sequence

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch
from . import _detections as _det

MAX_TASKS = _nat.CD_MAX_TASKS
MAX_MAPS = _nat.CD_MAX_MAPS
MAX_CLASSES = _nat.CD_MAX_CLASSES
MAX_K = _nat.CD_MAX_K
_DTYPES = _nat.FLOAT_DTYPE_CODES
_WHO = "center_point_decode"


class CenterPointDetections(NamedTuple):
    """The detections of one task: RaggedBatch objects ``[B, M, ...]`` that share one ``sample_sizes`` (int64 ``[B]``)."""
    boxes: object    # float32 [B, M, C - 1] as (x, y, z, dx, dy, dz, yaw[, vx, vy])
    scores: object   # float32 [B, M]
    labels: object   # int64 [B, M], the global class id
    source: object   # int32 [B, M], the peak rank k


def _numbers(name, v, n, exact=False):
    if not isinstance(v, (list, tuple)) or (len(v) != n if exact else len(v) < n):
        raise RuntimeError(f"{_WHO}: {name} must be a sequence of {'' if exact else 'at least '}{n} numbers, got {v!r}")
    return [_ops.number(_WHO, f"{name}[{i}]", v[i]) for i in range(n)]


def _class_lists(tasks):
    """(T, first class slot of every task and the end, the global class ids in task order)"""
    if not isinstance(tasks, (list, tuple)) or not 1 <= len(tasks) <= MAX_TASKS:
        raise RuntimeError(f"{_WHO}: tasks must be a sequence of 1..{MAX_TASKS} sequences of class ids")
    first, ids = [0], []
    for t, task in enumerate(tasks):
        if not isinstance(task, (list, tuple)):
            raise RuntimeError(f"{_WHO}: tasks[{t}] must be a sequence of class ids")
        for c in task:
            if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < MAX_CLASSES:
                raise RuntimeError(f"{_WHO}: class ids must be integers in [0, {MAX_CLASSES}), got {c!r} in tasks[{t}]")
            if c in ids:
                raise RuntimeError(f"{_WHO}: class {c} is in more than one task (or twice in one)")
            ids.append(c)
        first.append(len(ids))
    return len(tasks), first, ids


def center_point_decode(peaks, feats, tasks: Sequence[Sequence[int]], *, pc_range, voxel_size, out_size_factor,
                        score_threshold=None, post_center_range=None, scores_are_logits: bool = False, norm_bbox: bool = True,
                        nms_threshold=None, post_max_size=None, bottom_center: bool = False) -> List[CenterPointDetections]:
    """Boxes, scores and labels of every task from its heat-map peaks and regression maps, in one launch.

    Args:
        peaks: one ``HeatmapPeaks`` per task, from ``heatmap_peaks(heat_t, K, per_class=False)``, or a single one for one
            task (then ``feats`` is that task's maps).  Only ``scores`` (float32, float16 or bfloat16), ``indices`` and
            ``classes`` (int64) are read, each ``[B, K]`` and contiguous, 1 <= K <= 1024; all tasks share ``B``, ``K``,
            dtype and device.
        feats: per task one ``[B, c, H, W]`` tensor or a sequence of up to 8 of them, as for ``gather_at_centers``:
            contiguous, float32, float16 or bfloat16, read in place and never concatenated.  Their channels, concatenated,
            are the target layout of ``center_point_targets``: ``(off_x, off_y, z, d0, d1, d2, sin, cos[, vx, vy])`` — 8 or
            10 channels, the same for every task.
        tasks: as for ``center_point_targets``: ``T`` sequences of class ids, 1 <= T <= 8, ids in [0, 64), each id in at
            most one task.  ``classes[b, k]`` is a position inside its task, the output label the global id
            ``tasks[t][position]``; a position outside its task makes the peak invalid.
        pc_range, voxel_size, out_size_factor, norm_bbox: as for ``center_point_targets``.
        score_threshold: a number, or ``None`` for no score test.
        post_center_range: six numbers ``(x0, y0, z0, x1, y1, z1)``, or ``None`` for no range test.
        scores_are_logits: the score is ``sigmoid(scores)``: ``heatmap_peaks`` can then run on the raw logits, and the
            sigmoid pass over the whole map disappears (sigmoid is monotone, so the rank order is the same).
        nms_threshold: a number, a sequence of ``T`` numbers (mmdet3d's per-task ``min_radius``, unchanged), or ``None``.
        post_max_size: an integer >= 1, or ``None``.
        bottom_center: ``z`` becomes ``z - dz / 2``, as mmdet3d's ``get_task_detections`` does it.

    Per frame ``b``, task ``t`` and peak rank ``k``, in float32, every operation rounded once, in the rank order the peaks
    arrive in:

    1. the ``C`` channels at in-plane index ``indices[b, k]`` (float16 / bfloat16 widened exactly), ``ys = index // W``,
       ``xs = index % W``; an index outside ``[0, H * W)`` makes the peak invalid, and nothing is read for it;
    2. ``x = ((xs + off_x) * out_size_factor) * voxel_size[0] + pc_range[0]``, ``y`` likewise; ``z`` as gathered;
       ``dims = exp(d)`` under ``norm_bbox``, else ``d``; ``yaw = atan2(sin, cos)``; the velocity passes through;
    3. ``score = scores[b, k]``, or ``1 / (1 + exp(-scores[b, k]))`` with ``scores_are_logits``;
    4. valid iff ``score > score_threshold`` and ``post_center_range[0:3] <= (x, y, z) <= post_center_range[3:6]`` (each
       where given) and index and class position are legal; NaN fails every comparison it takes part in;
    5. circle NMS where ``nms_threshold[t]`` is given, class-agnostic inside the task: walking the valid peaks in rank
       order, a peak is kept iff no earlier kept peak ``j`` has ``(x - x_j)**2 + (y - y_j)**2 <= nms_threshold[t]`` — the
       squared distance against the threshold as given, which is mmdet3d's rule; a NaN distance suppresses nothing;
    6. the kept peaks go, in rank order, to slots ``0 .. kept - 1``; only the first ``post_max_size`` are written;
    7. with ``bottom_center``, ``z - dz * 0.5`` in the written boxes (after the range test).

    Returns: a list with one :class:`CenterPointDetections` per task.  ``M = min(K, post_max_size)`` is known on the host.
    The ``T`` entries are views ``out[t]`` of single ``[T, B, M, ...]`` allocations, and the four RaggedBatch objects of a
    task share one int64 ``sample_sizes``.  Padding slots are written too: +0 everywhere, ``source`` = -1.

    Nothing takes a gradient.  To train through the selected values gather them again, one line per task::

        d = center_point_decode(peaks, feats, tasks, ...)[t]
        rows = gather_at_centers(feats[t], peaks[t].indices.gather(1, d.source.tensor.clamp(min=0).long()))

    GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame and task, no atomics, no workspace,
    no host synchronisation, bitwise reproducible); CPU tensors run the library's serial host entry over the same
    arithmetic.  The integer outputs and the exact channels of the two are equal; ``exp``, ``atan2`` and the sigmoid agree
    to a few ulp.  ``B == 0`` gives empty outputs without a launch.
    """
    T, first, ids = _class_lists(tasks)
    if hasattr(peaks, "scores"):
        peaks, feats = [peaks], [feats]
    if not isinstance(peaks, (list, tuple)) or len(peaks) != T:
        raise RuntimeError(f"{_WHO}: peaks must hold one HeatmapPeaks per task ({T}), or be a single one for one task")
    if not isinstance(feats, (list, tuple)) or len(feats) != T:
        raise RuntimeError(f"{_WHO}: feats must hold one entry per task ({T})")
    per_task, all_maps = [], []
    for t in range(T):
        per_task.append(_det.check_peaks(_WHO, peaks[t], "B", MAX_K, t, per_task[0][0] if per_task else None))
        all_maps.append(_det.check_feats(_WHO, feats[t], per_task[0][0], "B", MAX_MAPS, t, all_maps[0][0] if all_maps else None))
    scores0, map0 = per_task[0][0], all_maps[0][0]
    C = sum(m.shape[1] for m in all_maps[0])
    for t, maps in enumerate(all_maps):
        c = sum(m.shape[1] for m in maps)
        if c not in (8, 10) or c != C:
            raise RuntimeError(f"{_WHO}: the maps of a task must hold 8 or 10 channels in total, the same for every task; "
                               f"feats[{t}] holds {c}")
    B, K = scores0.shape
    H, W = map0.shape[2], map0.shape[3]
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise RuntimeError(f"{_WHO}: the maps must have H, W >= 1 and H * W < 2^31, got {H} x {W}")
    pc, vs = _numbers("pc_range", pc_range, 2), _numbers("voxel_size", voxel_size, 2)
    factor = _ops.number(_WHO, "out_size_factor", out_size_factor)
    if not (vs[0] > 0 and vs[1] > 0 and factor > 0 and all(math.isfinite(v) for v in (*vs, factor))):
        raise RuntimeError(f"{_WHO}: voxel_size and out_size_factor must be positive and finite, got {voxel_size!r}, "
                           f"{out_size_factor!r}")
    if not (math.isfinite(pc[0]) and math.isfinite(pc[1])):
        raise RuntimeError(f"{_WHO}: pc_range must be finite, got {pc_range!r}")
    thr = _det.threshold(_WHO, "score_threshold", score_threshold)
    rng = None if post_center_range is None else _numbers("post_center_range", post_center_range, 6, exact=True)
    if rng is not None and any(math.isnan(v) for v in rng):
        raise RuntimeError(f"{_WHO}: post_center_range must not hold NaN, got {post_center_range!r}")
    if nms_threshold is None or isinstance(nms_threshold, (int, float)):
        nms = [nms_threshold] * T
    elif isinstance(nms_threshold, (list, tuple)) and len(nms_threshold) == T:
        nms = list(nms_threshold)
    else:
        raise RuntimeError(f"{_WHO}: nms_threshold must be a number, a sequence of {T} numbers (one per task) or None, got "
                           f"{nms_threshold!r}")
    nms = [_det.threshold(_WHO, f"nms_threshold[{t}]", v) for t, v in enumerate(nms)]
    post_max_size = _det.cut(_WHO, "post_max_size", post_max_size)

    dev = scores0.device
    M = K if post_max_size is None else min(K, post_max_size)
    boxes, out_scores, labels, source = _det.empty_outputs((T, B, M), C - 1, dev)
    kept = _det.kept_sizes((T, B), dev)
    if B:
        p = _nat.CenterPointDecodeParams()
        for t, ((s, i, c), maps) in enumerate(zip(per_task, all_maps)):
            p.scores[t], p.indices[t], p.classes[t] = s.data_ptr(), i.data_ptr(), c.data_ptr()
            p.num_maps[t] = len(maps)
            for n, m in enumerate(maps):
                p.maps[t][n], p.channels[t][n] = m.data_ptr(), m.shape[1]
            p.has_nms[t], p.nms_threshold[t] = (0, 0.0) if nms[t] is None else (1, nms[t])
        p.pc_range[0], p.pc_range[1], p.voxel_size[0], p.voxel_size[1] = pc[0], pc[1], vs[0], vs[1]
        p.out_size_factor = float(factor)
        p.has_score_threshold, p.score_threshold = (0, 0.0) if thr is None else (1, thr)
        p.has_post_center_range = 0 if rng is None else 1
        for n, v in enumerate(rng or ()):
            p.post_center_range[n] = v
        p.score_dtype, p.map_dtype, p.num_tasks = _DTYPES[scores0.dtype], _DTYPES[map0.dtype], T
        p.scores_are_logits, p.norm_bbox, p.bottom_center = (1 if v else 0 for v in (scores_are_logits, norm_bbox, bottom_center))
        for t, v in enumerate(first):
            p.task_first[t] = v
        for n, v in enumerate(ids):
            p.class_ids[n] = v
        args = (ctypes.addressof(p), B, K, H, W, M, boxes.data_ptr(), out_scores.data_ptr(), labels.data_ptr(),
                source.data_ptr(), kept.data_ptr())
        _ops.run("accv_center_point_decode", args, dev, _WHO)
    out = []
    for t, sizes_t in enumerate(kept.unbind(0)):     # one sample_sizes tensor per task, shared by its four outputs
        out.append(CenterPointDetections(*(RaggedBatch(x[t], sample_sizes=sizes_t) for x in (boxes, out_scores, labels, source))))
    return out
