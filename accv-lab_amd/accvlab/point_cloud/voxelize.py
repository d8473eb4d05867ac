"""(extension) Hard voxelization of a ragged batch of lidar point clouds: the pass from the points to the voxels or pillars
that the network reads, for the whole batch, with the result of the sequential loop whatever the order the GPU runs in.

It replaces mmcv's ``Voxelization`` (``hard_voxelize_forward``; spconv's ``points_to_voxel`` is the same rule), which
mmdet3d calls once per frame in a Python loop (``Base3DDetector.voxelize``) and whose GPU kernel hands out voxel numbers
with an atomic counter: voxel order, the voxels that survive ``max_voxels`` and the points that survive ``max_points``
differ from run to run there.  The definition here is mmcv's ``hard_voxelize_forward_cpu``; the float32 operation sequence
is written out in ``csrc/voxelize_arith.h``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MIN_D = _nat.VX_MIN_D
MAX_D = _nat.VX_MAX_D
MAX_POINTS = _nat.VX_MAX_POINTS
MAX_VOXELS = _nat.VX_MAX_VOXELS
_MAX_FRAMES = 65535
_MAX_SLOTS = 1 << 31
_WHO = "voxelize_points"
_f32 = np.float32


class Voxels(NamedTuple):
    """The voxels of every frame, padded to ``max_voxels`` per frame."""
    voxels: torch.Tensor            # float32 [B, V, T, D]: the points of each voxel, +0.0 rows from num_points on
    coors: torch.Tensor             # int32 [B, V, 3]: (z, y, x) of each voxel, -1 from voxel_counts on
    num_points: torch.Tensor        # int32 [B, V]: points stored per voxel, 0 from voxel_counts on
    voxel_counts: torch.Tensor      # int32 [B]: voxels per frame
    point_voxel: Optional[torch.Tensor]   # int32 [B, P]: the voxel number of each point or -1; None unless asked for

    def ragged(self):
        """``(voxels, coors, num_points)`` as RaggedBatches over ``voxel_counts`` (views, no copy, no synchronisation)"""
        return tuple(RaggedBatch(t, sample_sizes=self.voxel_counts) for t in (self.voxels, self.coors, self.num_points))


def _triple(name, v, n, what):
    if not isinstance(v, (list, tuple)) or len(v) != n:
        raise RuntimeError(f"{_WHO}: {name} must be {what}, got {v!r}")
    return [_ops.number(_WHO, f"{name}[{i}]", x) for i, x in enumerate(v)]


def _grid(voxel_size, point_cloud_range):
    """``(g_x, g_y, g_z)`` as mmcv's wrapper computes it, in float32: ``round((hi - lo) / v)``, ties to even"""
    with np.errstate(all="ignore"):
        v = [_f32(x) for x in voxel_size]
        lo, hi = [_f32(x) for x in point_cloud_range[:3]], [_f32(x) for x in point_cloud_range[3:]]
        for k in range(3):
            if not (v[k] > 0 and np.isfinite(v[k])):
                raise RuntimeError(f"{_WHO}: voxel_size must be positive and finite in float32, got {tuple(voxel_size)!r}")
            if not (np.isfinite(lo[k]) and np.isfinite(hi[k]) and hi[k] > lo[k]):
                raise RuntimeError(f"{_WHO}: point_cloud_range needs finite lo < hi in float32 along every axis, got "
                                   f"{tuple(point_cloud_range)!r}")
        g = [float(np.rint((hi[k] - lo[k]) / v[k])) for k in range(3)]
    if not all(1 <= x < 2 ** 31 for x in g):
        raise RuntimeError(f"{_WHO}: the grid needs 1 .. 2^31 - 1 cells along every axis, got {g!r}")
    if g[0] * g[1] * g[2] >= 2 ** 31:
        raise RuntimeError(f"{_WHO}: the grid has {g[0] * g[1] * g[2]:.0f} cells, fewer than 2^31 are supported")
    return tuple(int(x) for x in g)


def voxelize_points(points, *, voxel_size, point_cloud_range, max_points: int, max_voxels: int, augmentation=None,
                    return_point_voxel: bool = False, _table_slots: int = 0) -> Voxels:
    """Hard voxelization of the lidar points of a ragged batch of frames, bitwise reproducible.

    Args:
        points: RaggedBatch float32 ``[B, P, D]``, ``3 <= D <= 16``, contiguous, ``non_uniform_dim`` 1.  Channels 0..2 are
            x, y, z; the others pass through.  ``points.sample_sizes`` (int32 or int64) is read on the device and clamped
            to ``[0, P]``; slots from it on are never read.  ``B <= 65535``, ``P < 2^31 - 1``.  Other float dtypes raise
            ``TypeError``.
        voxel_size: ``(vx, vy, vz)`` Python numbers, positive and finite as float32.
        point_cloud_range: ``(x0, y0, z0, x1, y1, z1)`` Python numbers, ``lo < hi``, finite as float32.  The grid is
            ``g_k = round((hi_k - lo_k) / v_k)`` in float32, as mmcv's Python wrapper computes it; each ``g_k >= 1`` and
            ``g_x * g_y * g_z < 2^31``.
        max_points: ``T``, ``1 <= T <= 128``: the points a voxel keeps.
        max_voxels: ``V``, ``1 <= V <= 2^20``: the voxels a frame keeps.
        augmentation: optional float32 ``[B, 7]`` on the points' device: the rows ``(θ, c, s, k, tx, ty, tz)`` of
            :func:`accvlab.draw_heatmap.bev_augment_boxes`.  x, y, z go through its ``augment_center``
            (``csrc/bev_augment_arith.h``) before the voxel test and are stored augmented, so the augmented cloud never
            has to exist as a tensor.  (An identity row stores ``-0.0`` coordinates as ``+0.0``; everything else keeps its
            bits.)
        return_point_voxel: also return the voxel number of every point.

    Per frame, points in slot order, in float32, every operation rounded once, nothing contracted, ``/`` correctly rounded:

    1. With ``augmentation``, ``(x, y, z) = augment_center(row, x, y, z)``.
    2. ``t_k = floor((p_k - lo_k) / v_k)``; the point is in range iff ``t_k >= 0 and t_k < float(g_k)`` for all three
       ``k``.  **These are float compares, so NaN, +inf and -inf are out of range; mmcv casts to int first, which is
       undefined for them.**  ``c_k = int(t_k)``, ``key = (c_z * g_y + c_y) * g_x + c_x``.
    3. If the key has no voxel yet: if ``V`` voxels already exist **the point is skipped and the loop goes on** (mmcv's
       ``continue``; older mmcv versions stop at this point, spconv goes on as well); otherwise the voxel takes the next
       number and ``coors`` is written.
    4. If the voxel holds fewer than ``T`` points, the point's ``D`` channels are stored in the voxel's next row: x, y, z as
       augmented, the other channels bit for bit, NaN payloads included.

    Returns: :class:`Voxels` ``(voxels float32 [B, V, T, D], coors int32 [B, V, 3] as (z, y, x), num_points int32 [B, V],
    voxel_counts int32 [B], point_voxel int32 [B, P] or None)``.  Padding is written too and every element exactly once:
    rows of a voxel from ``num_points`` on are ``+0.0``; voxels from ``voxel_counts[b]`` on have zero rows, ``coors`` of -1
    and ``num_points`` of 0.  ``point_voxel`` is -1 for a point out of range, for a slot beyond ``sample_sizes`` and where
    the voxel was refused by ``max_voxels``; a point beyond ``max_points`` still reports its voxel (what a dynamic scatter
    needs).  Nothing takes a gradient and no input is modified.

    GPU tensors take **one ``hipMemsetAsync`` and five kernel launches** on torch's current stream (three without points), no
    host synchronisation, hipGraph-capturable; the workspace comes from torch's caching allocator.  No atomic decides an
    order: a per-frame hash table keeps the lowest point index of every key (compare-and-swap claim, ``atomicMin``), a prefix
    sum over the points in order (a count launch and a numbering launch) numbers the voxels, a bounded ``atomicMin`` cascade sorts each voxel's first ``T`` point
    indices, and a gather writes the outputs.  CPU tensors run the sequential loop of the library's host entry over the
    same arithmetic, with bit-equal results.  ``B == 0`` gives empty outputs without a launch; ``P == 0`` still writes all
    padding.  ``_table_slots`` (tests) overrides the hash-table size per frame: 0, or a power of two above ``P``.
    """
    if not _ops.is_ragged(points) or not isinstance(points.tensor, torch.Tensor):
        raise RuntimeError(f"{_WHO}: points must be a RaggedBatch of float32 [B, P, D]")
    p_t, sizes = points.tensor, points.sample_sizes
    _ops.check_operands(_WHO, (("points", p_t), ("augmentation", augmentation), ("sample_sizes", sizes)), p_t, "points'",
                        required=("points", "sample_sizes"))
    dev = p_t.device
    _ops.check_backend(_WHO, "points", dev)
    for name, t in (("points", p_t), ("augmentation", augmentation)):
        if t is not None:
            _ops.check_float32(_WHO, name, t)
    if (p_t.dtype != torch.float32 or p_t.dim() != 3 or not MIN_D <= p_t.shape[2] <= MAX_D
            or getattr(points, "num_batch_dims", 1) != 1 or getattr(points, "non_uniform_dim", 1) != 1):
        raise RuntimeError(f"{_WHO}: points must be float32 [B, P, D] with {MIN_D} <= D <= {MAX_D}, one batch dimension and "
                           f"non_uniform_dim 1, got {p_t.dtype} {tuple(p_t.shape)}")
    B, P, D = (int(v) for v in p_t.shape)
    if B > _MAX_FRAMES or P >= 2 ** 31 - 1:
        raise RuntimeError(f"{_WHO}: {B} frames of {P} point slots; at most {_MAX_FRAMES} frames and fewer than 2^31 - 1 slots "
                           "are supported")
    _ops.check_sample_sizes(_WHO, sizes, B)
    if augmentation is not None and (augmentation.dtype != torch.float32 or tuple(augmentation.shape) != (B, 7)):
        raise RuntimeError(f"{_WHO}: augmentation must be float32 [{B}, 7], got {augmentation.dtype} {tuple(augmentation.shape)}")
    vs = _triple("voxel_size", voxel_size, 3, "(vx, vy, vz) Python numbers")
    rng = _triple("point_cloud_range", point_cloud_range, 6, "(x0, y0, z0, x1, y1, z1) Python numbers")
    _grid(vs, rng)
    if not _ops.is_int(max_points) or not 1 <= max_points <= MAX_POINTS:
        raise RuntimeError(f"{_WHO}: max_points must be a Python int in 1..{MAX_POINTS}, got {max_points!r}")
    if not _ops.is_int(max_voxels) or not 1 <= max_voxels <= MAX_VOXELS:
        raise RuntimeError(f"{_WHO}: max_voxels must be a Python int in 1..{MAX_VOXELS}, got {max_voxels!r}")
    if not _ops.is_int(_table_slots) or (_table_slots != 0 and not (P < _table_slots <= _MAX_SLOTS
                                                                    and _table_slots & (_table_slots - 1) == 0)):
        raise RuntimeError(f"{_WHO}: _table_slots must be 0 or a power of two above P = {P} and at most 2^31, got {_table_slots!r}")
    T, V = max_points, max_voxels

    voxels = torch.empty((B, V, T, D), dtype=torch.float32, device=dev)
    coors = torch.empty((B, V, 3), dtype=torch.int32, device=dev)
    num_points = torch.empty((B, V), dtype=torch.int32, device=dev)
    voxel_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    point_voxel = torch.empty((B, P), dtype=torch.int32, device=dev) if return_point_voxel else None
    if B:
        prm = _nat.VoxelizeParams()
        prm.points, prm.sample_sizes, prm.augmentation = _ops.ptr(p_t), sizes.data_ptr(), _ops.ptr(augmentation)
        prm.voxel_size[:] = [float(v) for v in vs]
        prm.range_min[:], prm.range_max[:] = [float(v) for v in rng[:3]], [float(v) for v in rng[3:]]
        prm.table_slots, prm.max_points, prm.max_voxels = _table_slots, T, V
        prm.sizes_i64 = 1 if sizes.dtype == torch.int64 else 0
        args = (ctypes.addressof(prm), B, P, D, voxels.data_ptr(), coors.data_ptr(), num_points.data_ptr(),
                voxel_counts.data_ptr(), _ops.ptr(point_voxel))
        if dev.type == "cuda":
            nbytes = _nat.lib().accv_voxelize_workspace_bytes(B, P, V, T, _table_slots)
            if nbytes == 0:
                raise RuntimeError(f"{_WHO}: no workspace size for B {B}, P {P}, V {V}, T {T}, table_slots {_table_slots}")
            ws = _nat.workspace(nbytes, dev)
            args = args + (ws.data_ptr(), nbytes)
        _ops.run("accv_voxelize", args, dev, _WHO, host_entry=_nat.HOST_ENTRY_NAMES["accv_voxelize"])
    return Voxels(voxels, coors, num_points, voxel_counts, point_voxel)


def concatenate_voxels(vox: Voxels):
    """mmdet3d's form of the voxels of a batch: ``(voxels [M, T, D], coors [M, 4] as (b, z, y, x), num_points [M])``, the
    frames' voxels one after the other, ``M = voxel_counts.sum()``.

    **The read of ``M`` is a host synchronisation, the only one**; the three outputs are then written by the ragged pack
    operator (``accv_ragged_pack``, one launch each) on GPU tensors, by one masked selection each on CPU tensors.
    """
    if not isinstance(vox, Voxels):
        raise RuntimeError("concatenate_voxels: expected the Voxels of voxelize_points")
    B, V, T, D = (int(v) for v in vox.voxels.shape)
    dev = vox.voxels.device
    batch = torch.arange(B, dtype=torch.int32, device=dev).view(B, 1, 1).expand(B, V, 1)
    coors4 = torch.cat([batch, vox.coors], dim=2)
    sizes = vox.voxel_counts.to(torch.int64)
    if dev.type != "cuda":
        keep = torch.arange(V, device=dev).view(1, V) < sizes.view(B, 1)
        return vox.voxels[keep], coors4[keep], vox.num_points[keep]
    ends = torch.cumsum(sizes, 0)
    offsets = ends - sizes
    M = int(ends[-1].item()) if B else 0
    out = (torch.empty((M, T, D), dtype=torch.float32, device=dev), torch.empty((M, 4), dtype=torch.int32, device=dev),
           torch.empty((M,), dtype=torch.int32, device=dev))
    if M:
        with _nat.device_guard(dev):
            for flat, padded in zip(out, (vox.voxels, coors4, vox.num_points)):
                row_bytes = (flat.numel() // M) * 4
                _nat.check(_nat.lib().accv_ragged_pack(flat.data_ptr(), padded.data_ptr(), offsets.data_ptr(), sizes.data_ptr(), B, V,
                                                       row_bytes, 1, _nat.stream_ptr(dev)), "concatenate_voxels")
    return out
