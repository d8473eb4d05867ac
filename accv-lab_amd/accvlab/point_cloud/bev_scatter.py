"""(extension) BEV scatter: from the per-pillar features of a pillar feature net to the dense map a 2D backbone convolves,
for the whole batch, and the backward of that.

It replaces mmdet3d's ``PointPillarsScatter``, a Python loop over frames (a ``zeros`` canvas, a boolean mask, an index
assignment of a transposed tensor, then ``torch.stack``), which moves every frame's canvas about three times and has an
autograd backward of the same shape.  Here the canvas is written once, zeros included.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .. import _amd_native as _nat
from .._amd_native import operands as _ops

MAX_CHANNELS = _nat.BS_MAX_C
_WHO = "scatter_to_bev"
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


class _ScatterToBev(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, coors, geom):
        rows, V, B, C, ny, nx = geom
        dev = features.device
        canvas = torch.empty((B, C, ny, nx), dtype=features.dtype, device=dev)
        index = torch.empty((B, ny, nx), dtype=torch.int32, device=dev)
        if canvas.numel():
            _ops.run("accv_bev_scatter", (_ops.ptr(features), _ops.ptr(coors), rows, V, B, C, ny, nx, int(coors.shape[-1]),
                                          features.element_size(), canvas.data_ptr(), index.data_ptr()), dev, _WHO,
                     host_entry=_nat.HOST_ENTRY_NAMES["accv_bev_scatter"])
        ctx.geom, ctx.shape = geom, tuple(features.shape)
        # the backward reads the coors and the index, never the features: those are neither kept alive nor guarded
        ctx.save_for_backward(coors, index)
        ctx.mark_non_differentiable(index)
        return canvas, index

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_canvas, _grad_index):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        coors, index = ctx.saved_tensors
        rows, V, B, C, ny, nx = ctx.geom
        grad_canvas = grad_canvas.contiguous()
        grad = torch.empty(ctx.shape, dtype=grad_canvas.dtype, device=grad_canvas.device)
        if grad.numel():
            _ops.run("accv_bev_scatter_bwd", (_ops.ptr(grad_canvas), _ops.ptr(coors), _ops.ptr(index), rows, V, B, C, ny, nx,
                                              int(coors.shape[-1]), grad.element_size(), grad.data_ptr()), grad.device,
                     _WHO + " backward", host_entry=_nat.HOST_ENTRY_NAMES["accv_bev_scatter_bwd"])
        return grad, None, None


def scatter_to_bev(features: torch.Tensor, coors: torch.Tensor, *, grid_hw, batch_size: Optional[int] = None,
                   return_index: bool = False):
    """The dense BEV map of per-pillar features: mmdet3d's ``PointPillarsScatter`` for the whole batch, differentiable.

    Args:
        features: float32, float16 or bfloat16, contiguous.  Either ``[M, C]`` with ``coors`` int32 ``[M, 4]`` as
            ``(b, z, y, x)`` and ``batch_size`` given (mmdet3d's call), or ``[B, V, C]`` with ``coors`` int32 ``[B, V, 3]``
            as ``(z, y, x)``, the padded form of :class:`Voxels`, where the frame of row ``r`` is ``r // V``.
            ``1 <= C <= 1024``, fewer than 2^31 rows.
        coors: int32 (other integer dtypes raise ``TypeError``), contiguous, on the features' device.
        grid_hw: ``(ny, nx)`` Python ints; ``B * ny * nx < 2^31``.
        batch_size: ``B`` of the flat form; the padded form takes it from the shape.
        return_index: also return ``index``.

    With ``r`` the flat row number: a row is *placed* iff ``0 <= b < B``, ``0 <= y < ny`` and ``0 <= x < nx``; ``z`` is
    ignored, as ``PointPillarsScatter`` ignores it, so the padding rows of :func:`voxelize_points` (``coors = -1``) are
    skipped without ``voxel_counts``.

    * ``index[b, y, x]`` is the highest placed ``r`` of the cell, or ``-1``: the last write of the sequential loop.
    * ``canvas[b, c, y, x] = features[index[b, y, x], c]``, or ``+0`` where the index is ``-1``.  The copy moves bits, NaN
      payloads included.
    * ``grad_features[r, c] = grad_canvas[b, c, y, x]`` if ``index[cell(r)] == r``, else ``+0``: rows that lose a cell to a
      higher row, unplaced rows and padding get a zero gradient.

    Returns ``canvas [B, C, ny, nx]`` of the features' dtype, and ``index`` int32 ``[B, ny, nx]`` (not differentiable) with
    ``return_index``.  Every element of both is written exactly once; no input is modified.

    GPU tensors take **one ``hipMemsetAsync`` and two kernel launches** in the forward and **one launch** in the backward,
    on torch's current stream, without a host synchronisation, hipGraph-capturable: the memset clears ``index``, a lane per
    row marks its cell with ``atomicMax`` (order-independent, so the result is a pure function of the inputs), and a
    workgroup per 64 cells x 64 channels writes the canvas from the occupied cells' feature rows through LDS in 16-byte
    stores, or zeros only where its cells hold no row; no atomic touches the canvas and it is never read or cleared.  Where
    ``features``, the canvas, ``C`` or ``nx`` is not 16-byte aligned an element-wise path does the same.  The backward reads
    ``coors``, ``index`` and ``grad_canvas``, never ``features``, which are not saved.  CPU tensors run the sequential loop
    of the library's host entries, with bit-equal results.
    """
    _ops.check_operands(_WHO, (("features", features), ("coors", coors)), features, "features'", required=("features", "coors"))
    dev = features.device
    _ops.check_backend(_WHO, "features", dev)
    if features.dtype not in _DTYPES:
        raise TypeError(f"{_WHO}: features must be float32, float16 or bfloat16, got {features.dtype}")
    if coors.dtype != torch.int32:
        if not coors.is_floating_point() and coors.dtype != torch.bool:
            raise TypeError(f"{_WHO}: coors must be int32, got {coors.dtype}")
        raise RuntimeError(f"{_WHO}: coors must be int32, got {coors.dtype}")
    if (not isinstance(grid_hw, (list, tuple)) or len(grid_hw) != 2 or not all(_ops.is_int(v) and v >= 0 for v in grid_hw)):
        raise RuntimeError(f"{_WHO}: grid_hw must be (ny, nx) non-negative Python ints, got {grid_hw!r}")
    ny, nx = int(grid_hw[0]), int(grid_hw[1])
    if features.dim() == 2:
        if coors.dim() != 2 or tuple(coors.shape) != (features.shape[0], 4):
            raise RuntimeError(f"{_WHO}: features [M, C] need coors int32 [M, 4] as (b, z, y, x), got {tuple(features.shape)} and "
                               f"{tuple(coors.shape)}")
        if not _ops.is_int(batch_size) or batch_size < 0:
            raise RuntimeError(f"{_WHO}: features [M, C] need batch_size, a non-negative Python int, got {batch_size!r}")
        B, V = batch_size, 0
    elif features.dim() == 3:
        if tuple(coors.shape) != tuple(features.shape[:2]) + (3,):
            raise RuntimeError(f"{_WHO}: features [B, V, C] need coors int32 [B, V, 3] as (z, y, x), got {tuple(features.shape)} "
                               f"and {tuple(coors.shape)}")
        B, V = int(features.shape[0]), int(features.shape[1])
        if batch_size is not None and batch_size != B:
            raise RuntimeError(f"{_WHO}: batch_size {batch_size!r} contradicts features [B, V, C] with B = {B}")
    else:
        raise RuntimeError(f"{_WHO}: features must be [M, C] or [B, V, C], got {tuple(features.shape)}")
    C = int(features.shape[-1])
    rows = features.numel() // C if C else 0
    if not 1 <= C <= MAX_CHANNELS:
        raise RuntimeError(f"{_WHO}: features need 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    if rows >= 2 ** 31 or B * ny * nx >= 2 ** 31:
        raise RuntimeError(f"{_WHO}: {rows} rows and B * ny * nx = {B * ny * nx} cells; fewer than 2^31 of each are supported")
    canvas, index = _ScatterToBev.apply(features, coors, (rows, V, B, C, ny, nx))
    return (canvas, index) if return_index else canvas
