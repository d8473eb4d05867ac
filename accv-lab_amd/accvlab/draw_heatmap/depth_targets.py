"""(extension) The depth supervision of an LSS head (BEVDepth, BEVDet4D-Depth, BEVStereo): from the lidar points of a frame
to the nearest depth, and its bin, per cell of every camera's downsampled feature map — in one launch.

It replaces two passes of those code bases: the loader's per-camera CPU pass (``map_pointcloud_to_image`` /
``depth_transform``: a numpy matmul, the masks, a scatter into a full-resolution ``H x W`` map) and the head's device pass
over ``[B, N, H, W]`` (``get_downsampled_gt_depth``: reshape, ``min`` over the stride blocks, bins, one-hot).  The matrices
are the ones the other operators hand out: ``camera_augment_boxes(...).projection_matrices`` is ``lidar2img`` with the
image matrix folded in, or pass the raw ``lidar2img`` with ``image_transforms``.  The float32 operation sequence is written
out in ``csrc/depth_targets_arith.h``.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops

MAX_CAMERAS = _nat.DT_MAX_CAMERAS
DT_BAND_CELLS = _nat.DT_BAND_CELLS
MAX_BINS = _nat.DT_MAX_BINS
_MAX_EXTENT = 1 << 24
_WHO = "lidar_depth_targets"


class DepthTargets(NamedTuple):
    """The depth targets of every camera."""
    depth: torch.Tensor             # float32 [B, C, h, w]: the nearest depth of the cell, 0.0 where no point fell
    bins: object                    # int32 [B, C, h, w]: the bin of that depth, -1 where there is none; None without depth_bins


def _pair(name, v, what):
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise RuntimeError(f"{_WHO}: {name} must be {what}, got {v!r}")
    return v


def lidar_depth_targets(points, projection: torch.Tensor, *, image_hw, downsample: int = 16, depth_range, depth_bins=None,
                        image_transforms=None, _band_rows: int = 0) -> DepthTargets:
    """Per-camera depth and depth-bin maps from the lidar points of a ragged batch of frames, in one launch.

    Args:
        points: RaggedBatch float32 ``[B, P, D]``, ``D >= 3``, contiguous, ``non_uniform_dim`` 1.  Channels 0..2 are x, y, z,
            read in place; further channels (intensity, time) are ignored.  ``points.sample_sizes`` (int32 or int64) is read
            on the device and clamped to ``[0, P]``; slots from it on are never read.  There is no limit on ``P``.  Other
            float dtypes raise ``TypeError``.
        projection: float32 ``[B, C, R, 4]``, ``R`` in {3, 4}, ``1 <= C <= 16``, contiguous, on the points' device: lidar to
            image pixels, ``lidar2img`` as the other operators hand it out.  Row 3 is never read.
        image_hw: ``(H, W)`` Python ints in ``1 .. 2^24``, the extent of the image the projection (after
            ``image_transforms``) maps into.  The output shape depends on it, so a tensor is not accepted.
        downsample: a Python int ``>= 1``; the maps are ``h = ceil(H / downsample)`` by ``w = ceil(W / downsample)``;
            ``w`` may not exceed ``DT_BAND_CELLS`` = 8192.
        depth_range: ``(d_min, d_max)`` Python numbers, ``0 < d_min < d_max``, both finite (as float32).  ``d_min > 0`` is
            required: the kernel orders depths by their bit pattern.
        depth_bins: ``None``, or ``(lo, step, count)`` with ``step > 0`` and ``1 <= count <= 2^15``.
        image_transforms: optional float32 ``[B, C, 2, 3]``, the forward matrix ``prepare_images`` takes.  It is folded into
            rows 0 and 1 of ``projection`` with exactly the arithmetic of step 2 of :func:`camera_augment_boxes`, so the
            result equals the call with the matrices ``camera_augment_boxes`` returns, bit for bit.

    Per ``(b, c)`` and real point, in float32, every operation rounded once and in the written order, nothing contracted
    (``d_min``, ``d_max``, ``lo`` and ``step`` are rounded to float32 once):

    1. ``p_k = ((m_k0*x + m_k1*y) + m_k2*z) + m_k3`` for ``k`` = 0, 1, 2; ``d = p_2``, ``u = p_0 / d``, ``v = p_1 / d``
       (IEEE division).
    2. The point counts iff ``d >= d_min and d < d_max and u >= 0 and u < W and v >= 0 and v < H``: float compares, so NaN
       fails and ``d <= 0`` (behind the camera) fails.  **BEVDepth casts the coordinates to int16 before its test and so
       lets ``u`` in (-1, 0) through as pixel 0; this operator does not.**
    3. Its cell is ``(int(v) // downsample, int(u) // downsample)``.
    4. ``depth[b, c, cy, cx]`` is the minimum ``d`` over the points of the cell, ``0.0`` where there is none.  A minimum
       needs no tie rule: equal depths are equal values.
    5. With ``depth_bins``: ``t = (depth - lo) / step``; ``bins[b, c, cy, cx] = int(t)`` if the cell has a point,
       ``t >= 0`` and ``int(t) < count``, else ``-1``.

    BEVDepth's one-hot target is ``F.one_hot(bins.long() + 1, count + 1)[..., 1:]`` with ``lo = d_min``.  BEVDepth itself
    evaluates ``(d - (d_min - step)) / step`` and floors; the subtraction there and the one here round differently, so for a
    depth within a few ulp of a bin edge ``lo + n * step`` the two may land in neighbouring bins.

    Returns: :class:`DepthTargets` ``(depth float32 [B, C, h, w], bins int32 [B, C, h, w] or None)``.  Every output element
    is written exactly once.  Nothing takes a gradient and no input is modified.

    GPU tensors run one HIP kernel on torch's current stream (output-stationary: a workgroup keeps a band of whole map rows
    in LDS, streams the frame's points and takes an LDS atomic minimum on the bit pattern of ``d``; no atomics on global
    memory, no workspace, no clear, no host synchronisation, bitwise reproducible); CPU tensors run the library's serial
    host entry over the same arithmetic, with bit-equal results.  ``B == 0`` gives empty outputs without a launch;
    ``P == 0`` still takes the launch that writes zeros and -1.  ``B`` is limited to 65535 frames.
    """
    if not _ops.is_ragged(points) or not isinstance(points.tensor, torch.Tensor):
        raise RuntimeError(f"{_WHO}: points must be a RaggedBatch of float32 [B, P, D]")
    p_t, sizes = points.tensor, points.sample_sizes
    if isinstance(image_hw, torch.Tensor):
        raise RuntimeError(f"{_WHO}: image_hw must be (H, W) Python ints (the output shape depends on it), got a tensor")
    _ops.check_operands(_WHO, (("points", p_t), ("projection", projection), ("image_transforms", image_transforms),
                               ("sample_sizes", sizes)), p_t, "points'", required=("points", "projection", "sample_sizes"))
    dev = p_t.device
    _ops.check_backend(_WHO, "points", dev)
    for name, t in (("points", p_t), ("projection", projection), ("image_transforms", image_transforms)):
        if t is not None:
            _ops.check_float32(_WHO, name, t)
    if (p_t.dtype != torch.float32 or p_t.dim() != 3 or p_t.shape[2] < 3 or getattr(points, "num_batch_dims", 1) != 1
            or getattr(points, "non_uniform_dim", 1) != 1):
        raise RuntimeError(f"{_WHO}: points must be float32 [B, P, D] with D >= 3, one batch dimension and non_uniform_dim 1, "
                           f"got {p_t.dtype} {tuple(p_t.shape)}")
    B, P, D = (int(v) for v in p_t.shape)
    if (projection.dtype != torch.float32 or projection.dim() != 4 or projection.shape[0] != B
            or projection.shape[2] not in (3, 4) or projection.shape[3] != 4):
        raise RuntimeError(f"{_WHO}: projection must be float32 [{B}, C, R, 4] with R in (3, 4), got {projection.dtype} "
                           f"{tuple(projection.shape)}")
    C, R = int(projection.shape[1]), int(projection.shape[2])
    if not 1 <= C <= MAX_CAMERAS:
        raise RuntimeError(f"{_WHO}: {C} cameras per frame, 1..MAX_CAMERAS = {MAX_CAMERAS} are supported")
    if image_transforms is not None and (image_transforms.dtype != torch.float32 or tuple(image_transforms.shape) != (B, C, 2, 3)):
        raise RuntimeError(f"{_WHO}: image_transforms must be float32 [{B}, {C}, 2, 3], got {image_transforms.dtype} "
                           f"{tuple(image_transforms.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, B)
    H, W = _pair("image_hw", image_hw, "(H, W) Python ints")
    if not (_ops.is_int(H) and _ops.is_int(W)) or not (1 <= H <= _MAX_EXTENT and 1 <= W <= _MAX_EXTENT):
        raise RuntimeError(f"{_WHO}: image_hw must be (H, W) Python ints in 1..2^24, got {image_hw!r}")
    if not _ops.is_int(downsample) or not 1 <= downsample <= _MAX_EXTENT:
        raise RuntimeError(f"{_WHO}: downsample must be a Python int >= 1, got {downsample!r}")
    d_min, d_max = (_ops.number(_WHO, f"depth_range[{i}]", v) for i, v in enumerate(_pair("depth_range", depth_range, "(d_min, d_max)")))
    if not (0 < d_min < d_max and math.isfinite(d_max)):
        raise RuntimeError(f"{_WHO}: depth_range needs 0 < d_min < d_max, both finite, got {depth_range!r}")
    lo, step, count = 0.0, 1.0, 0
    if depth_bins is not None:
        if not isinstance(depth_bins, (list, tuple)) or len(depth_bins) != 3:
            raise RuntimeError(f"{_WHO}: depth_bins must be None or (lo, step, count), got {depth_bins!r}")
        lo, step = _ops.number(_WHO, "depth_bins[0]", depth_bins[0]), _ops.number(_WHO, "depth_bins[1]", depth_bins[1])
        count = _ops.number(_WHO, "depth_bins[2]", depth_bins[2], integer=True)
        if not (math.isfinite(lo) and 0 < step and math.isfinite(step) and 1 <= count <= MAX_BINS):
            raise RuntimeError(f"{_WHO}: depth_bins needs a finite lo, a finite step > 0 and 1 <= count <= {MAX_BINS}, got {depth_bins!r}")
    h, w = -(-H // downsample), -(-W // downsample)
    if w > DT_BAND_CELLS:
        raise RuntimeError(f"{_WHO}: map rows of {w} cells, at most DT_BAND_CELLS = {DT_BAND_CELLS} are supported")
    if not _ops.is_int(_band_rows) or _band_rows < 0 or _band_rows * w > DT_BAND_CELLS:
        raise RuntimeError(f"{_WHO}: _band_rows = {_band_rows!r} rows of {w} cells exceed DT_BAND_CELLS = {DT_BAND_CELLS}")
    if B > 65535:
        raise RuntimeError(f"{_WHO}: {B} frames, at most 65535 are supported")

    depth = torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    bins = torch.empty((B, C, h, w), dtype=torch.int32, device=dev) if count else None
    if B:
        prm = _nat.DepthTargetsParams()
        prm.points, prm.sample_sizes, prm.projection = _ops.ptr(p_t), sizes.data_ptr(), projection.data_ptr()
        prm.image_transforms = _ops.ptr(image_transforms)
        prm.image_h, prm.image_w = H, W
        prm.depth_min, prm.depth_max, prm.bin_lo, prm.bin_step = float(d_min), float(d_max), float(lo), float(step)
        prm.downsample, prm.bin_count = downsample, count
        prm.sizes_i64, prm.band_rows = (1 if sizes.dtype == torch.int64 else 0), _band_rows
        args = (ctypes.addressof(prm), B, P, D, C, R, depth.data_ptr(), _ops.ptr(bins))
        _ops.run("accv_depth_targets", args, dev, _WHO, host_entry=_nat.HOST_ENTRY_NAMES["accv_depth_targets"])
    return DepthTargets(depth, bins)
