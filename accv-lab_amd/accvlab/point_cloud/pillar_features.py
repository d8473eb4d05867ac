"""(extension) Pillar decoration and the voxel mean: from the voxels of :func:`voxelize_points` to the rows a pillar feature
net's first linear layer reads, and to the per-voxel mean of ``HardSimpleVFE``, one launch each.

``pillar_features`` replaces the part of mmdet3d's non-legacy ``PillarFeatureNet.forward`` in front of its PFN layers: a sum,
a divide, three strided slice assignments into a ``zeros_like``, a norm, a ``cat``, a mask build and a multiply, about a
dozen launches and several passes over the largest tensor of the lidar branch.  mmdet3d is not a dependency: the docstring
below is the definition, and the float32 operation sequence is written out in ``csrc/pillar_features_arith.h``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from .voxelize import MAX_D, MAX_POINTS, MIN_D, Voxels


def _unpack(who, voxels, num_points, coors, need_coors):
    """the three tensors of a call, from a Voxels tuple or as given"""
    if isinstance(voxels, Voxels):
        if num_points is not None or coors is not None:
            raise RuntimeError(f"{who}: a Voxels tuple stands for voxels, num_points and coors; pass nothing else")
        voxels, num_points, coors = voxels.voxels, voxels.num_points, voxels.coors
    _ops.check_operands(who, (("voxels", voxels), ("num_points", num_points), ("coors", coors if need_coors else None)), voxels,
                        "voxels'", required=("voxels", "num_points") + (("coors",) if need_coors else ()))
    _ops.check_backend(who, "voxels", voxels.device)
    _ops.check_float32(who, "voxels", voxels)
    if (voxels.dtype != torch.float32 or voxels.dim() not in (3, 4) or not MIN_D <= voxels.shape[-1] <= MAX_D
            or not 1 <= voxels.shape[-2] <= MAX_POINTS):
        raise RuntimeError(f"{who}: voxels must be float32 [M, T, D] or [B, V, T, D] with {MIN_D} <= D <= {MAX_D} and "
                           f"1 <= T <= {MAX_POINTS}, got {voxels.dtype} {tuple(voxels.shape)}")
    lead = tuple(voxels.shape[:-2])
    if num_points.dtype != torch.int32 or tuple(num_points.shape) != lead:
        raise RuntimeError(f"{who}: num_points must be int32 {list(lead)}, got {num_points.dtype} {tuple(num_points.shape)}")
    if need_coors and (coors.dtype != torch.int32 or tuple(coors.shape[:-1]) != lead or coors.dim() != len(lead) + 1
                       or coors.shape[-1] not in (3, 4)):
        raise RuntimeError(f"{who}: coors must be int32 {list(lead)} + [3] as (z, y, x) or + [4] as (b, z, y, x), got "
                           f"{coors.dtype} {tuple(coors.shape)}")
    return voxels, num_points, coors, lead


def _numbers(who, name, v, n, what):
    if not isinstance(v, (list, tuple)) or len(v) != n:
        raise RuntimeError(f"{who}: {name} must be {what}, got {v!r}")
    return [float(_ops.number(who, f"{name}[{i}]", x)) for i, x in enumerate(v)]


def pillar_features(voxels, num_points: Optional[torch.Tensor] = None, coors: Optional[torch.Tensor] = None, *, voxel_size,
                    point_cloud_range, with_cluster_center: bool = True, with_voxel_center: bool = True,
                    with_distance: bool = False) -> torch.Tensor:
    """The decorated rows of every voxel: mmdet3d's non-legacy ``PillarFeatureNet`` up to its first linear layer.

    Args:
        voxels: float32 ``[M, T, D]`` or ``[B, V, T, D]``, contiguous, ``3 <= D <= 16``, ``1 <= T <= 128``; channels 0..2 are
            x, y, z.  Or the :class:`Voxels` of :func:`voxelize_points`, in place of the three tensors.
        num_points: int32 ``[M]`` or ``[B, V]``, clamped to ``[0, T]`` on the device.
        coors: int32 ``[..., 3]`` as ``(z, y, x)`` or ``[..., 4]`` as ``(b, z, y, x)``; the last three columns are read.
        voxel_size: ``(vx, vy, vz)`` Python numbers, positive and finite as float32.
        point_cloud_range: ``(x0, y0, z0, x1, y1, z1)`` Python numbers; the lower corner is read, finite as float32.
        with_cluster_center, with_voxel_center, with_distance: the channel groups to append.

    Per voxel, in float32, every operation rounded once, nothing contracted, ``/`` and ``sqrt`` correctly rounded:

    * ``n = clamp(num_points, 0, T)``.
    * ``s_k = ((p_0k + p_1k) + p_2k) + ...`` over the rows ``j < n`` in row order, ``k`` in x, y, z (torch's ``sum`` has no
      defined order; this one is the library's), and ``mean_k = s_k / float(n)``.
    * ``centre_k = float(c_k) * v_k + (v_k * 0.5f + lo_k)`` with ``c`` = (x, y, z) from ``coors`` columns (-1, -2, -3);
      ``coors`` of -1 is computed like any other value.
    * A row ``j < n`` is ``[the D input channels bit for bit | p_jk - mean_k | p_jk - centre_k |
      sqrt((x * x + y * y) + z * z)]`` with the groups that were asked for.
    * A row ``j >= n`` is ``+0.0`` in every channel, whatever the input holds there (mmdet3d's mask multiply, except that a
      NaN in padding does not survive); a voxel with ``n == 0`` is all ``+0.0`` and divides nothing.

    Returns float32 ``[..., T, F]``, ``F = D + 3 * with_cluster_center + 3 * with_voxel_center + with_distance``, every
    element written exactly once.  Nothing takes a gradient (the inputs are raw points) and no input is modified.

    GPU tensors take **one kernel launch** on torch's current stream, no workspace, no host synchronisation,
    hipGraph-capturable: a workgroup stages as many consecutive voxels as fit its LDS budget, sums from LDS and all its lanes
    write the rows.  CPU tensors run the library's host entry over the same arithmetic, with bit-equal results.  ``M == 0``
    gives an empty output without a launch.
    """
    who = "pillar_features"
    voxels, num_points, coors, lead = _unpack(who, voxels, num_points, coors, True)
    vs = _numbers(who, "voxel_size", voxel_size, 3, "(vx, vy, vz) Python numbers")
    rng = _numbers(who, "point_cloud_range", point_cloud_range, 6, "(x0, y0, z0, x1, y1, z1) Python numbers")
    with np.errstate(all="ignore"):
        if not all(np.float32(v) > 0 and np.isfinite(np.float32(v)) for v in vs):
            raise RuntimeError(f"{who}: voxel_size must be positive and finite in float32, got {tuple(voxel_size)!r}")
        if not all(np.isfinite(np.float32(v)) for v in rng[:3]):
            raise RuntimeError(f"{who}: point_cloud_range needs a lower corner that is finite in float32, got "
                               f"{tuple(point_cloud_range)!r}")
    for name, flag in (("with_cluster_center", with_cluster_center), ("with_voxel_center", with_voxel_center),
                       ("with_distance", with_distance)):
        if not isinstance(flag, bool):
            raise RuntimeError(f"{who}: {name} must be a bool, got {flag!r}")
    T, D = int(voxels.shape[-2]), int(voxels.shape[-1])
    flags = ((_nat.PF_CLUSTER if with_cluster_center else 0) | (_nat.PF_CENTER if with_voxel_center else 0)
             | (_nat.PF_DISTANCE if with_distance else 0))
    F = D + 3 * with_cluster_center + 3 * with_voxel_center + int(with_distance)
    out = torch.empty(lead + (T, F), dtype=torch.float32, device=voxels.device)
    M = num_points.numel()
    if M:
        prm = _nat.PillarFeaturesParams()
        prm.voxels, prm.num_points, prm.coors = voxels.data_ptr(), num_points.data_ptr(), coors.data_ptr()
        prm.voxel_size[:], prm.range_min[:] = vs, rng[:3]
        prm.coor_width, prm.flags = int(coors.shape[-1]), flags
        _ops.run("accv_pillar_features", (ctypes.addressof(prm), M, T, D, out.data_ptr()), voxels.device, who,
                 host_entry=_nat.HOST_ENTRY_NAMES["accv_pillar_features"])
    return out


def voxel_mean(voxels, num_points: Optional[torch.Tensor] = None, *, num_features: Optional[int] = None) -> torch.Tensor:
    """The mean of the points of every voxel: mmdet3d's ``HardSimpleVFE``.

    Args:
        voxels, num_points: as in :func:`pillar_features`; a :class:`Voxels` tuple stands for both.
        num_features: the leading channels to average, ``1 <= num_features <= D``; all ``D`` by default.

    Per voxel and channel ``k < num_features``: ``s_k / float(n)`` with ``n`` and the row-order sum ``s_k`` of
    :func:`pillar_features`, and ``+0.0`` where ``n == 0`` (mmdet3d divides by zero there).  Returns float32
    ``[..., num_features]``.  One kernel launch on torch's current stream for GPU tensors, the host entry for CPU tensors,
    bit-equal results; nothing takes a gradient.
    """
    who = "voxel_mean"
    voxels, num_points, _, lead = _unpack(who, voxels, num_points, None, False)
    T, D = int(voxels.shape[-2]), int(voxels.shape[-1])
    nf = D if num_features is None else num_features
    if not _ops.is_int(nf) or not 1 <= nf <= D:
        raise RuntimeError(f"{who}: num_features must be a Python int in 1..D = {D}, got {num_features!r}")
    out = torch.empty(lead + (nf,), dtype=torch.float32, device=voxels.device)
    M = num_points.numel()
    if M:
        _ops.run("accv_voxel_mean", (voxels.data_ptr(), num_points.data_ptr(), M, T, D, nf, out.data_ptr()), voxels.device, who,
                 host_entry=_nat.HOST_ENTRY_NAMES["accv_voxel_mean"])
    return out
