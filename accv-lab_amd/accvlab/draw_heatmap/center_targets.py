"""(extension) The target side of a centre-point head (CenterNet, CenterPoint and the BEV heads built on mmdet3d's
``CenterHead``): from raw ragged ground-truth 3D boxes to everything the rest of this package consumes — integer centres,
Gaussian radii and in-task labels for ``draw_heatmap_batched(labels=...)``, regression targets and centres for
``center_regression_loss``, in-plane indices for ``gather_at_centers`` — for every task of the head in one launch.

It replaces mmdet3d's ``CenterHead.get_targets_single``, a Python loop over frames, tasks and objects, and equals it where
that function is defined; the float32 operation sequence is written out in ``csrc/center_targets_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Sequence

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MAX_TASKS = _nat.CT_MAX_TASKS
MAX_CLASSES = _nat.CT_MAX_CLASSES
_WHO = "center_point_targets"


class CenterPointTargets(NamedTuple):
    """The targets of one task: RaggedBatch objects ``[B, M, ...]`` that share one ``sample_sizes`` (int64 ``[B]``)."""
    centers: object   # int32 [B, M, 2] as (x, y)
    radii: object     # int32 [B, M]
    labels: object    # int32 [B, M], the position of the class inside its task
    targets: object   # float32 [B, M, D + 1]
    indices: object   # int64 [B, M], y * W + x
    source: object    # int32 [B, M], the input slot


def _pair(name, v, integer=False):
    if not isinstance(v, (list, tuple)) or len(v) < 2:
        raise RuntimeError(f"{_WHO}: {name} must be a sequence of at least two numbers, got {v!r}")
    return _ops.number(_WHO, f"{name}[0]", v[0], integer), _ops.number(_WHO, f"{name}[1]", v[1], integer)


def _class_table(tasks):
    """(T, class -> task, class -> position in its task)"""
    if not isinstance(tasks, (list, tuple)) or not 1 <= len(tasks) <= MAX_TASKS:
        raise RuntimeError(f"{_WHO}: tasks must be a sequence of 1..{MAX_TASKS} sequences of class ids")
    task_of = [_nat.CT_NO_TASK] * MAX_CLASSES
    pos_of = [0] * MAX_CLASSES
    for t, ids in enumerate(tasks):
        if not isinstance(ids, (list, tuple)):
            raise RuntimeError(f"{_WHO}: tasks[{t}] must be a sequence of class ids")
        for pos, c in enumerate(ids):
            if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < MAX_CLASSES:
                raise RuntimeError(f"{_WHO}: class ids must be integers in [0, {MAX_CLASSES}), got {c!r} in tasks[{t}]")
            if task_of[c] != _nat.CT_NO_TASK:
                raise RuntimeError(f"{_WHO}: class {c} is in more than one task (or twice in one)")
            task_of[c], pos_of[c] = t, pos
    return len(tasks), task_of, pos_of


def center_point_targets(boxes, labels, tasks: Sequence[Sequence[int]], *, pc_range, voxel_size, out_size_factor, grid_size,
                         gaussian_overlap: float = 0.1, min_radius: int = 2, max_objs: int = 500,
                         norm_bbox: bool = True) -> List[CenterPointTargets]:
    """Centre-point targets of every task from a ragged batch of ground-truth 3D boxes, in one launch.

    Args:
        boxes: RaggedBatch float32 ``[B, Nmax, D]``, contiguous, ``D`` = 7 or 9 as ``(x, y, z, dx, dy, dz, yaw[, vx, vy])``.
            Only ``boxes.sample_sizes`` (int32 or int64) decides which slots are read.
        labels: RaggedBatch or tensor, int32 or int64 ``[B, Nmax]``, contiguous, on the boxes' device.
        tasks: ``T`` sequences of class ids, 1 <= T <= 8, ids in [0, 64), each id in at most one task.  A label in no task
            (negative ids included) belongs to no task.
        pc_range, voxel_size, out_size_factor, gaussian_overlap, min_radius, max_objs: Python numbers as in mmdet3d's
            ``train_cfg`` (of ``pc_range`` and ``voxel_size`` the x and y entries are used).
        grid_size: ``(W, H)`` of the feature map in cells.
        norm_bbox: the size channels are ``log(dx, dy, dz)`` instead of the raw values.

    Per frame ``b`` and task ``t``, in float32, every operation rounded once and in exactly this order:

    1. candidates: the slots ``n < sample_sizes[b]`` whose label is in task ``t``, ascending; only the first ``max_objs`` of
       them go on (mmdet3d's ``min(num_objs, max_objs)``, applied before the validity test);
    2. ``w = dx / voxel_size[0] / out_size_factor``, ``l = dy / voxel_size[1] / out_size_factor``,
       ``cx = (x - pc_range[0]) / voxel_size[0] / out_size_factor``, ``cy`` likewise;
    3. kept iff ``w > 0 and l > 0 and -1 < cx < W and -1 < cy < H`` (NaN fails); the cell is ``(int(cx), int(cy))``, truncated
       toward zero, so a centre in (-1, 0) lands in cell 0 as with mmdet3d's ``.to(torch.int32)``;
    4. ``radius = max(min_radius, int(gaussian_radius((l, w), gaussian_overlap)))``, CenterPoint's three-root rule; where
       Python's ``int`` would raise, the conversion is defined: NaN (a box of infinite extent) gives 0, hence
       ``min_radius``, and values beyond int32 saturate;
    5. target ``(cx - cell_x, cy - cell_y, z, dims, sin(yaw), cos(yaw)[, vx, vy])``, ``D + 1`` channels; non-finite ``z``,
       ``dz``, ``yaw`` or velocity pass through into the target row of their object and nowhere else;
    6. kept objects are compacted in ascending ``n`` to slots ``0 .. kept - 1``.

    Returns: a list with one :class:`CenterPointTargets` per task.  ``M = min(max_objs, Nmax)`` is known on the host.  The
    ``T`` entries are views ``out[t]`` of single ``[T, B, M, ...]`` allocations, so every per-task tensor is contiguous, and
    the six RaggedBatch objects of a task share one int64 ``sample_sizes`` = the kept count.  Padding slots
    ``kept .. M - 1`` are written too: 0 in every output, ``source`` = -1.  The result plugs into the consumers as is::

        for r, hm, maps in zip(center_point_targets(boxes, labels, tasks, ...), heatmaps, regression_maps):
            draw_heatmap_batched(hm, r.centers, r.radii, labels=r.labels, clear=True)
            loss = gaussian_focal_loss(logits, hm) + center_regression_loss(maps, r.centers, r.targets)
            attrs = batched_indexing_access(other_per_object_data, r.source)     # any further attribute

    GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame and task, no atomics, no host
    synchronisation, bitwise reproducible); CPU tensors run the library's serial host entry over the same arithmetic.  The
    integer outputs of the two are equal; the ``log`` / ``sin`` / ``cos`` channels agree to a few ulp.  Nothing takes a
    gradient.  ``B == 0`` or ``M == 0`` gives empty outputs without a launch.
    """
    if not _ops.is_ragged(boxes):
        raise RuntimeError(f"{_WHO}: boxes must be a RaggedBatch of float32 [B, Nmax, D]")
    b_t, sizes = boxes.tensor, boxes.sample_sizes
    l_t = _ops.tensor_of(labels)
    _ops.check_operands(_WHO, (("boxes", b_t), ("labels", l_t), ("sample_sizes", sizes)), b_t, "boxes'",
                        required=("boxes", "labels", "sample_sizes"))
    _ops.check_backend(_WHO, "boxes", b_t.device)
    if b_t.dtype != torch.float32 or b_t.dim() != 3 or b_t.shape[2] not in (7, 9):
        raise RuntimeError(f"{_WHO}: boxes must be float32 [B, Nmax, 7 or 9], got {b_t.dtype} {tuple(b_t.shape)}")
    B, N, D = b_t.shape
    if l_t.dtype not in (torch.int32, torch.int64) or tuple(l_t.shape) != (B, N):
        raise RuntimeError(f"{_WHO}: labels must be int32 or int64 [{B}, {N}], got {l_t.dtype} {tuple(l_t.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, B)
    T, task_of, pos_of = _class_table(tasks)
    pc, vs = _pair("pc_range", pc_range), _pair("voxel_size", voxel_size)
    W, H = _pair("grid_size", grid_size, integer=True)
    factor = _ops.number(_WHO, "out_size_factor", out_size_factor)
    overlap = _ops.number(_WHO, "gaussian_overlap", gaussian_overlap)
    min_radius, max_objs = _ops.number(_WHO, "min_radius", min_radius, True), _ops.number(_WHO, "max_objs", max_objs, True)
    if not (vs[0] > 0 and vs[1] > 0 and factor > 0 and math.isfinite(vs[0]) and math.isfinite(vs[1]) and math.isfinite(factor)):
        raise RuntimeError(f"{_WHO}: voxel_size and out_size_factor must be positive and finite, got {voxel_size!r}, "
                           f"{out_size_factor!r}")
    if not (math.isfinite(pc[0]) and math.isfinite(pc[1]) and math.isfinite(overlap)):
        raise RuntimeError(f"{_WHO}: pc_range and gaussian_overlap must be finite, got {pc_range!r}, {gaussian_overlap!r}")
    if W < 1 or H < 1 or W * H >= 2 ** 31:
        raise RuntimeError(f"{_WHO}: grid_size must be (W, H) with W, H >= 1 and W * H < 2^31, got {grid_size!r}")
    if max_objs < 0 or max_objs >= 2 ** 31 or abs(min_radius) >= 2 ** 31:
        raise RuntimeError(f"{_WHO}: max_objs must be in [0, 2^31) and min_radius an int32, got {max_objs}, {min_radius}")

    dev = b_t.device
    M = min(max_objs, N)
    shape = (T, B, M)
    centers = torch.empty(shape + (2,), dtype=torch.int32, device=dev)
    radii = torch.empty(shape, dtype=torch.int32, device=dev)
    out_labels = torch.empty(shape, dtype=torch.int32, device=dev)
    targets = torch.empty(shape + (D + 1,), dtype=torch.float32, device=dev)
    indices = torch.empty(shape, dtype=torch.int64, device=dev)
    source = torch.empty(shape, dtype=torch.int32, device=dev)
    if B == 0 or M == 0:
        kept = torch.zeros((T, B), dtype=torch.int64, device=dev)
    else:
        kept = torch.empty((T, B), dtype=torch.int64, device=dev)
        params = _nat.CenterPointTargetsParams((ctypes.c_double * 2)(*pc), (ctypes.c_double * 2)(*vs), float(factor),
                                               float(overlap), min_radius, max_objs, 1 if norm_bbox else 0, T,
                                               (ctypes.c_ubyte * MAX_CLASSES)(*task_of), (ctypes.c_ubyte * MAX_CLASSES)(*pos_of))
        flags = (_nat.CT_LABELS_I64 if l_t.dtype == torch.int64 else 0) | (_nat.CT_COUNTS_I64 if sizes.dtype == torch.int64 else 0)
        args = (b_t.data_ptr(), l_t.data_ptr(), sizes.data_ptr(), flags, B, N, D, W, H, M, ctypes.addressof(params),
                centers.data_ptr(), radii.data_ptr(), out_labels.data_ptr(), targets.data_ptr(), indices.data_ptr(),
                source.data_ptr(), kept.data_ptr())
        _ops.run("accv_center_point_targets", args, dev, _WHO)
    out = []
    for t, sizes_t in enumerate(kept.unbind(0)):     # one sample_sizes tensor per task, shared by its six outputs
        out.append(CenterPointTargets(*(RaggedBatch(x[t], sample_sizes=sizes_t)
                                        for x in (centers, radii, out_labels, targets, indices, source))))
    return out
