"""(extension) What the raw 3D boxes of a sample go through before ``center_point_targets``: the global BEV augmentation
(a rotation about z, then a uniform scaling, then a translation) of box centres, sizes, yaws and velocities and of every
matrix that maps to or from the augmented frame, the point-cloud-range test of the centres, and the compaction of every
per-object field over the resulting flag — for a ragged batch in one launch and without a host round trip.

It replaces three per-sample steps of the reference's DALI pipeline, ``BEVBBoxesTransformer3D``, ``PointsInRangeCheck`` and
``ConditionalElementRemover`` (``processing_steps/bev_bboxes_transformer_3d.py``, ``points_in_range_check.py``; wired at
``examples/pipeline_setup/stream_petr_pipeline.py:409-497``); the float32 operation sequence is written out in
``csrc/bev_augment_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MAX_POINT_TRANSFORMS = _nat.BA_MAX_POINT_TRANSFORMS
MAX_FRAME_TRANSFORMS = _nat.BA_MAX_FRAME_TRANSFORMS
_WHO = "bev_augment_boxes"


class BevAugmented(NamedTuple):
    """The augmented sample data.  ``boxes``, ``labels`` and ``source`` share one ``sample_sizes`` (int64 ``[B]``, the kept
    count); ``keep`` has the input's."""
    boxes: object               # RaggedBatch float32 [B, Nmax, D]: the kept boxes, augmented, compacted in slot order
    labels: object              # RaggedBatch [B, Nmax] of the labels' dtype, or None
    source: object              # RaggedBatch int32 [B, Nmax]: the input slot of each output slot, -1 in padding
    keep: object                # RaggedBatch bool [B, Nmax] over the INPUT slots
    point_transforms: tuple     # new tensors, M . A^-1
    frame_transforms: tuple     # new tensors, A . M


def _column(name, v, B, device, who):
    """`v` (a number or a tensor of B or 1 elements) as a float32 [B] tensor on `device`"""
    if isinstance(v, torch.Tensor):
        t = v.detach().to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() not in (1, B):
            raise RuntimeError(f"{who}: {name} must have 1 or {B} elements, got {tuple(v.shape)}")
        return t.expand(B)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise RuntimeError(f"{who}: {name} must be a number or a tensor, got {v!r}")
    return torch.full((B,), float(v), dtype=torch.float32, device=device)


def bev_augmentation_params(angle, scale=1.0, translation=(0.0, 0.0, 0.0), *, batch_size: Optional[int] = None,
                            device=None) -> torch.Tensor:
    """The ``[B, 7]`` float32 parameter rows ``(angle, cos, sin, scale, tx, ty, tz)`` of :func:`bev_augment_boxes`.

    ``angle`` (radians, about z) and ``scale`` are numbers or tensors of ``B`` elements, ``translation`` a sequence of three
    numbers or a ``[B, 3]`` tensor.  ``B`` is ``batch_size`` or the size of the first tensor among the arguments (1 if there
    is none); numbers are repeated.  The cosine and sine are evaluated in float64 from the float32 angle and then rounded,
    so they are the correctly rounded values of the angle the kernel adds to the yaws.  Runs on ``device`` (default: that
    of the first tensor, else the CPU) without a host synchronisation.
    """
    who = "bev_augmentation_params"
    tensors = [v for v in (angle, scale, translation) if isinstance(v, torch.Tensor)]
    if device is None:
        device = tensors[0].device if tensors else torch.device("cpu")
    device = torch.device(device)
    if batch_size is None:
        batch_size = 1
        if tensors:
            first = tensors[0]
            batch_size = first.shape[0] if first.dim() >= 1 else 1
    B = int(batch_size)
    a = _column("angle", angle, B, device, who)
    k = _column("scale", scale, B, device, who)
    if isinstance(translation, torch.Tensor):
        t = translation.detach().to(device=device, dtype=torch.float32)
        if t.dim() == 1 and t.shape[0] == 3:
            t = t[None]
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] not in (1, B):
            raise RuntimeError(f"{who}: translation must be [3] or [{B}, 3], got {tuple(translation.shape)}")
        t = t.expand(B, 3)
    else:
        if not isinstance(translation, (list, tuple)) or len(translation) != 3:
            raise RuntimeError(f"{who}: translation must be three numbers or a [B, 3] tensor, got {translation!r}")
        t = torch.stack([_column(f"translation[{i}]", v, B, device, who) for i, v in enumerate(translation)], 1)
    a64 = a.to(torch.float64)
    return torch.cat([a[:, None], a64.cos().to(torch.float32)[:, None], a64.sin().to(torch.float32)[:, None], k[:, None], t],
                     1).contiguous()


def _interval(name, v, who):
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise RuntimeError(f"{who}: {name} must be (min, max), got {v!r}")
    lo, hi = float(v[0]), float(v[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise RuntimeError(f"{who}: {name} must be finite with min <= max, got {v!r}")
    return lo, hi


def _uniform(lo, hi, shape, generator, device):
    """float32 draws in [lo, hi]; ``lo == hi`` is the value itself (the reference's _get_random_in_range)"""
    lo32 = torch.tensor(lo, dtype=torch.float32)
    hi32 = torch.tensor(hi, dtype=torch.float32)
    if lo == hi:
        return lo32.to(device).expand(shape)
    u = torch.rand(shape, generator=generator, dtype=torch.float32, device=device)
    return (lo32.to(device) + (hi32 - lo32).to(device) * u).clamp(lo32.item(), hi32.item())


def sample_bev_augmentation(batch_size: int, rotation_range=None, scaling_range=None, translation_max_abs=None, *,
                            generator: Optional[torch.Generator] = None, device=None) -> torch.Tensor:
    """The random decisions of the reference's ``BEVBBoxesTransformer3D`` as ``[B, 7]`` parameter rows: one uniform draw per
    sample of the angle in ``rotation_range`` (radians), of the scale in ``scaling_range`` and of each translation
    component in ``[-translation_max_abs[i], translation_max_abs[i]]``.  ``None`` disables a part (angle 0, scale 1,
    translation 0: the identity entries); ``min == max`` is the value itself, with no draw.  The draws are float32 from
    ``generator`` (its device is where they are made; default: torch's global generator of ``device``) and stay inside the
    float32 values of their borders.  The rows land on ``device`` (default: the generator's device, else the CPU).
    """
    who = "sample_bev_augmentation"
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 0:
        raise RuntimeError(f"{who}: batch_size must be a non-negative integer, got {batch_size!r}")
    B = batch_size
    draw_dev = generator.device if generator is not None else torch.device(device if device is not None else "cpu")
    out_dev = torch.device(device) if device is not None else draw_dev
    angle = torch.zeros((B,), dtype=torch.float32, device=draw_dev)
    scale = torch.ones((B,), dtype=torch.float32, device=draw_dev)
    trans = torch.zeros((B, 3), dtype=torch.float32, device=draw_dev)
    if rotation_range is not None:
        angle = _uniform(*_interval("rotation_range", rotation_range, who), (B,), generator, draw_dev)
    if scaling_range is not None:
        scale = _uniform(*_interval("scaling_range", scaling_range, who), (B,), generator, draw_dev)
    if translation_max_abs is not None:
        if not isinstance(translation_max_abs, (list, tuple)) or len(translation_max_abs) != 3:
            raise RuntimeError(f"{who}: translation_max_abs must be three numbers, got {translation_max_abs!r}")
        cols = []
        for i, m in enumerate(translation_max_abs):
            m = float(m)
            if not (math.isfinite(m) and m >= 0):
                raise RuntimeError(f"{who}: translation_max_abs[{i}] must be finite and non-negative, got {m!r}")
            cols.append(_uniform(-m, m, (B,), generator, draw_dev))
        trans = torch.stack(cols, 1)
    return bev_augmentation_params(angle.to(out_dev), scale.to(out_dev), trans.to(out_dev), batch_size=B, device=out_dev)


def _range(point_range):
    if point_range is None:
        return None
    if not isinstance(point_range, (list, tuple)) or len(point_range) != 2:
        raise RuntimeError(f"{_WHO}: point_range must be (min_xyz, max_xyz), got {point_range!r}")
    out = []
    for name, corner in zip(("min_xyz", "max_xyz"), point_range):
        if not isinstance(corner, (list, tuple)) or len(corner) != 3:
            raise RuntimeError(f"{_WHO}: point_range {name} must be three numbers, got {corner!r}")
        for v in corner:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise RuntimeError(f"{_WHO}: point_range {name} must be Python numbers (inf allowed, NaN not), got {v!r}")
        out.append([float(v) for v in corner])
    return out


def _matrices(name, tensors, limit, rows_allowed, B, device):
    if not isinstance(tensors, (list, tuple)):
        raise RuntimeError(f"{_WHO}: {name} must be a sequence of tensors")
    if len(tensors) > limit:
        raise RuntimeError(f"{_WHO}: at most {limit} {name} tensors, got {len(tensors)}")
    for i, t in enumerate(tensors):
        what = f"{name}[{i}]"
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{_WHO}: {what} must be a tensor")
        if t.device != device:
            raise RuntimeError(f"{_WHO}: {what} must be on the boxes' device {device}, got {t.device}")
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != B or t.shape[2] not in rows_allowed or t.shape[3] != 4:
            rows = " or ".join(str(r) for r in rows_allowed)
            raise RuntimeError(f"{_WHO}: {what} must be float32 [{B}, K, {rows}, 4], got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{_WHO}: {what} must be contiguous (it is not copied silently)")
    return tuple(tensors)


def bev_augment_boxes(boxes, params: torch.Tensor, *, labels=None, valid=None, point_range=None, range_check_on: str = "input",
                      point_transforms: Sequence[torch.Tensor] = (), frame_transforms: Sequence[torch.Tensor] = ()) -> BevAugmented:
    """Global BEV augmentation, range filter and compaction of a ragged batch of 3D boxes, in one launch.

    Args:
        boxes: RaggedBatch float32 ``[B, Nmax, D]``, contiguous, ``D`` = 7 or 9 as ``(x, y, z, dx, dy, dz, yaw[, vx, vy])``,
            the layout ``center_point_targets`` takes.  ``boxes.sample_sizes`` (int32 or int64) is read on the device and
            clamped to ``[0, Nmax]``; slots from it on are never read into a decision.  ``Nmax`` is not limited.
        params: float32 ``[B, 7]`` on the boxes' device, rows ``(angle, cos, sin, scale, tx, ty, tz)``, see
            :func:`bev_augmentation_params` and :func:`sample_bev_augmentation`.  The cosine and sine are read from the row
            and never computed, so for given rows every output is bit-equal between the device, the host entry and a
            float32 restatement of the definition.  ``scale == 0`` and non-finite rows are computed as written.
        labels: optional RaggedBatch or tensor, int32 or int64 ``[B, Nmax]``, compacted along with the boxes.
        valid: optional bool or uint8 ``[B, Nmax]`` (tensor or RaggedBatch): the rest of the keep condition, e.g. the
            reference's ``num_lidar_points >= 1 and category >= 0``.
        point_range: ``None`` or ``(min_xyz, max_xyz)``, Python numbers (inf for "no border").  A box is inside iff
            ``min <= c <= max`` on all three coordinates of its centre ``c``: both borders inclusive, NaN fails, the
            float32 centre compared with the number as given (the reference's ``check_points_in_box``).
        range_check_on: ``"input"`` tests the raw centre (the reference's step order), ``"output"`` the augmented one
            (mmdet3d's ``ObjectRangeFilter`` after ``GlobalRotScaleTrans``).
        point_transforms: up to 4 float32 tensors ``[B, K, R, 4]``, ``R`` = 3 or 4, ``K >= 0``: matrices applied to points
            of the augmented frame (``lidar2img``, extrinsics, ``ego_to_world``); the result holds ``M . A^-1``.
        frame_transforms: up to 2 float32 tensors ``[B, K, 4, 4]``: matrices whose results are points of that frame
            (``world_to_ego``); the result holds ``A . M``.  ``A = T . S . R`` is the augmentation of a point.

    Per frame, with its row ``(θ, c, s, k, tx, ty, tz)``, in float32, every operation rounded once and in this order:
    centre ``((c*x - s*y)*k + tx, (s*x + c*y)*k + ty, z*k + tz)``; sizes ``d*k``; velocity ``((c*vx - s*vy)*k,
    (s*vx + c*vy)*k)``; yaw ``yaw + θ`` wrapped into ``[-π, π]`` by whole turns as the reference's ``ensure_range`` does
    (NaN stays NaN, ±inf gives NaN).  A slot is kept iff ``valid`` and inside ``point_range``; kept boxes are compacted in
    ascending slot order.

    Returns: :class:`BevAugmented`.  The compacted outputs share one new int64 ``sample_sizes`` written on the device;
    their padding is written too (0, ``source`` -1), ``keep`` is False from ``sample_sizes`` on, and every output element is
    written exactly once.  ``source`` serves ``batched_indexing_access`` for any further per-object field.  The result
    plugs into ``center_point_targets(out.boxes, out.labels, ...)`` as is.

    GPU tensors run one HIP kernel on torch's current stream (one workgroup per frame, no atomics, no workspace, no host
    synchronisation, bitwise reproducible); CPU tensors run the library's serial host entry over the same arithmetic, with
    bit-equal results.  Nothing takes a gradient and no input is modified.  ``B == 0`` gives empty outputs without a launch.
    """
    if not _ops.is_ragged(boxes):
        raise RuntimeError(f"{_WHO}: boxes must be a RaggedBatch of float32 [B, Nmax, D]")
    b_t, sizes = boxes.tensor, boxes.sample_sizes
    l_t, v_t = _ops.tensor_of(labels), _ops.tensor_of(valid)
    _ops.check_operands(_WHO, (("boxes", b_t), ("params", params), ("labels", l_t), ("valid", v_t), ("sample_sizes", sizes)),
                        b_t, "boxes'", required=("boxes", "params", "sample_sizes"))
    dev = b_t.device
    _ops.check_backend(_WHO, "boxes", dev)
    if b_t.dtype != torch.float32 or b_t.dim() != 3 or b_t.shape[2] not in (7, 9):
        raise RuntimeError(f"{_WHO}: boxes must be float32 [B, Nmax, 7 or 9], got {b_t.dtype} {tuple(b_t.shape)}")
    B, N, D = b_t.shape
    if params.dtype != torch.float32 or tuple(params.shape) != (B, 7):
        raise RuntimeError(f"{_WHO}: params must be float32 [{B}, 7], got {params.dtype} {tuple(params.shape)}")
    if l_t is not None and (l_t.dtype not in (torch.int32, torch.int64) or tuple(l_t.shape) != (B, N)):
        raise RuntimeError(f"{_WHO}: labels must be int32 or int64 [{B}, {N}], got {l_t.dtype} {tuple(l_t.shape)}")
    if v_t is not None and (v_t.dtype not in (torch.bool, torch.uint8) or tuple(v_t.shape) != (B, N)):
        raise RuntimeError(f"{_WHO}: valid must be bool or uint8 [{B}, {N}], got {v_t.dtype} {tuple(v_t.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, B)
    if range_check_on not in ("input", "output"):
        raise RuntimeError(f"{_WHO}: range_check_on must be 'input' or 'output', got {range_check_on!r}")
    rng = _range(point_range)
    p_in = _matrices("point_transforms", point_transforms, MAX_POINT_TRANSFORMS, (3, 4), B, dev)
    f_in = _matrices("frame_transforms", frame_transforms, MAX_FRAME_TRANSFORMS, (4,), B, dev)

    out_boxes = torch.empty_like(b_t)
    out_labels = torch.empty_like(l_t) if l_t is not None else None
    source = torch.empty((B, N), dtype=torch.int32, device=dev)
    keep = torch.empty((B, N), dtype=torch.bool, device=dev)
    kept = torch.empty((B,), dtype=torch.int64, device=dev)
    p_out = tuple(torch.empty_like(t) for t in p_in)
    f_out = tuple(torch.empty_like(t) for t in f_in)
    if B > 0:
        prm = _nat.BevAugmentParams()
        if rng is not None:
            prm.range_min, prm.range_max = (ctypes.c_double * 3)(*rng[0]), (ctypes.c_double * 3)(*rng[1])
            prm.has_range = 1
        for i, (src, dst) in enumerate(zip(p_in, p_out)):
            prm.point_in[i], prm.point_out[i] = src.data_ptr(), dst.data_ptr()
            prm.point_count[i], prm.point_rows[i] = src.shape[1], src.shape[2]
        for i, (src, dst) in enumerate(zip(f_in, f_out)):
            prm.frame_in[i], prm.frame_out[i], prm.frame_count[i] = src.data_ptr(), dst.data_ptr(), src.shape[1]
        prm.num_point_transforms, prm.num_frame_transforms = len(p_in), len(f_in)
        flags = ((_nat.BA_LABELS_I64 if l_t is not None and l_t.dtype == torch.int64 else 0)
                 | (_nat.BA_COUNTS_I64 if sizes.dtype == torch.int64 else 0)
                 | (_nat.BA_RANGE_ON_OUTPUT if range_check_on == "output" else 0))
        args = (b_t.data_ptr(), params.data_ptr(), _ops.ptr(l_t), _ops.ptr(v_t), sizes.data_ptr(), flags, B, N, D,
                ctypes.addressof(prm), out_boxes.data_ptr(), _ops.ptr(out_labels), source.data_ptr(), keep.data_ptr(),
                kept.data_ptr())
        _ops.run("accv_bev_augment", args, dev, _WHO)
    return BevAugmented(RaggedBatch(out_boxes, sample_sizes=kept),
                        RaggedBatch(out_labels, sample_sizes=kept) if out_labels is not None else None,
                        RaggedBatch(source, sample_sizes=kept), RaggedBatch(keep, sample_sizes=sizes), p_out, f_out)
