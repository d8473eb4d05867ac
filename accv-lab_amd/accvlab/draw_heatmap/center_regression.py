"""(extension) The regression branch of a centre-point head (CenterNet, CenterPoint: offset, size, height, rot, vel at the
object centres) next to the heat-map branch this package already covers: mmdet's ``transpose_and_gather_feat``
(models/utils/gaussian_target.py) and the L1 term of mmdet3d's ``CenterHead.loss`` without the ``torch.cat`` of the heads,
the ``permute(0, 2, 3, 1).contiguous()`` of the whole ``[B, C, H, W]`` tensor, the gather, and in the backward the scatter
into a zero-filled tensor, the permute back and the split of the cat.

``gather_at_centers`` and ``center_regression_loss`` equal this composition (what the tests pin)::

    f = torch.cat(feats, 1)                                              # [B, C, H, W]
    rows = f.permute(0, 2, 3, 1).reshape(B, H * W, C)
    ind = (y * W + x).clamp(0, H * W - 1)                                # int64 [B, Nmax]
    valid = (slot < sample_sizes[:, None]) & (0 <= x) & (x < W) & (0 <= y) & (y < H)
    g = torch.where(valid[..., None], rows.gather(1, ind[..., None].expand(-1, -1, C)), 0)      # gather_at_centers
    per = loss(g - targets, reduction="none") * weights                  # l1_loss / smooth_l1_loss
    loss = torch.where(valid[..., None], per, 0).sum() / denom           # denom = valid.sum().clamp(min=1) by default

with ``N * C`` scattered reads forward and one write-only pass over the gradient maps backward.  GPU only.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Union

import torch
from torch.autograd.function import once_differentiable

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch
from . import _detections as _det

_DTYPES = _nat.FLOAT_DTYPE_CODES
_KINDS = {"l1": _nat.CR_L1, "smooth_l1": _nat.CR_SMOOTH_L1}
MAX_MAPS = _nat.CR_MAX_MAPS
MAX_CHANNELS = _nat.CR_MAX_CHANNELS


def _check_feats(who, feats):
    """the maps as a tuple, after every check that needs no device"""
    maps = _det.maps_of(who, "feats", feats)
    if len(maps) > MAX_MAPS:
        raise RuntimeError(f"{who}: at most {MAX_MAPS} maps are supported, got {len(maps)}")
    for i, m in enumerate(maps):
        if not isinstance(m, torch.Tensor):
            raise RuntimeError(f"{who}: feats[{i}] must be a tensor")
        if not m.is_cuda:
            raise RuntimeError(f"{who}: feats[{i}] must be a CUDA tensor (there is no CPU path)")
        if m.dim() != 4:
            raise RuntimeError(f"{who}: feats[{i}] must be [B, C, H, W], got {m.dim()} dimensions")
        if not m.is_contiguous():
            raise RuntimeError(f"{who}: feats[{i}] must be contiguous (a map is not copied silently)")
    first = maps[0]
    if first.dtype not in _DTYPES or first.dtype == torch.float64:
        raise RuntimeError(f"{who}: feats must be float32, float16 or bfloat16, got {first.dtype}")
    for i, m in enumerate(maps[1:], 1):
        if m.dtype != first.dtype:
            raise RuntimeError(f"{who}: feats[{i}] has dtype {m.dtype}, feats[0] {first.dtype}")
        if m.device != first.device:
            raise RuntimeError(f"{who}: feats[{i}] is on {m.device}, feats[0] on {first.device}")
        if (m.shape[0], m.shape[2], m.shape[3]) != (first.shape[0], first.shape[2], first.shape[3]):
            raise RuntimeError(f"{who}: feats[{i}] has shape {tuple(m.shape)}, feats[0] {tuple(first.shape)}: B, H and W "
                               "must agree")
    channels = sum(m.shape[1] for m in maps)
    if channels > MAX_CHANNELS:
        raise RuntimeError(f"{who}: at most {MAX_CHANNELS} channels in total are supported, got {channels}")
    if first.shape[2] * first.shape[3] >= 2 ** 31:
        raise RuntimeError(f"{who}: a plane of {first.shape[2]} x {first.shape[3]} exceeds 2^31 - 1 cells")
    return maps


def _check_ragged_centers(who, centers, first):
    if not _ops.is_ragged(centers):
        raise RuntimeError(f"{who}: centers must be a RaggedBatch of int32 [B, Nmax, 2] (x, y)")
    c_t, sizes = centers.tensor, centers.sample_sizes
    for name, t in (("centers", c_t), ("sample_sizes", sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor")
        if t.device != first.device:
            raise RuntimeError(f"{who}: {name} must be on the maps' device {first.device}, got {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous")
    if c_t.dtype != torch.int32 or c_t.dim() != 3 or c_t.shape[2] != 2 or c_t.shape[0] != first.shape[0]:
        raise RuntimeError(f"{who}: centers must be int32 [B, Nmax, 2] with B = {first.shape[0]}, got {c_t.dtype} "
                           f"{tuple(c_t.shape)}")
    if sizes.dtype not in (torch.int32, torch.int64) or sizes.shape != (first.shape[0],):
        raise RuntimeError(f"{who}: sample_sizes must be int32 or int64 [B], got {sizes.dtype} {tuple(sizes.shape)}")
    return c_t, sizes


class _Call:
    """the geometry that every C-ABI call of one operator invocation shares: the host array of the channel counts, the
    shapes of the maps and of the centres; it holds no tensor a kernel reads"""

    def __init__(self, maps, where, sizes, index_form):
        self.n = len(maps)
        self.dev = maps[0].device
        self.dtype = _DTYPES[maps[0].dtype]
        self.B, _, self.H, self.W = maps[0].shape
        self.channels = (ctypes.c_int * self.n)(*[m.shape[1] for m in maps])
        self.C = sum(self.channels)
        self.map_dtype = maps[0].dtype
        self.shapes = [tuple(m.shape) for m in maps]
        self.N = where.shape[1]
        self.flags = _nat.CR_INDEX_FORM if index_form else (_nat.CR_COUNTS_I64 if sizes.dtype == torch.int64 else 0)

    def pointers(self, tensors):
        return (ctypes.c_void_p * self.n)(*[t.data_ptr() for t in tensors])

    def geometry(self, where, sizes):
        return (ctypes.addressof(self.channels), self.n, self.dtype, self.B, self.H, self.W, where.data_ptr(),
                _ops.ptr(sizes), self.N)

    def empty_maps(self, needed):
        """uninitialised gradient maps (contiguous, as the maps are) where `needed`, None elsewhere"""
        return [torch.empty(shape, dtype=self.map_dtype, device=self.dev) if need else None
                for shape, need in zip(self.shapes, needed)]


class _GatherAtCenters(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, where, sizes, *maps):
        out = torch.empty((call.B, call.N, call.C), dtype=maps[0].dtype, device=call.dev)
        if out.numel() > 0:
            ptrs = call.pointers(maps)
            with _nat.device_guard(call.dev):
                _nat.check(_nat.lib().accv_gather_at_centers(ctypes.addressof(ptrs), *call.geometry(where, sizes),
                                                             call.flags, out.data_ptr(), _nat.stream_ptr(call.dev)),
                           "gather_at_centers")
        ctx.call = call
        # the scatter reads the centres and the sample sizes, never the maps: those are neither kept alive nor guarded
        ctx.save_for_backward(where, sizes)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        call = ctx.call
        where, sizes = ctx.saved_tensors
        grads = call.empty_maps(ctx.needs_input_grad[3:])
        if any(g is not None and g.numel() > 0 for g in grads):
            # the kernel writes every map of the call; one that needs no gradient still gets a buffer
            spare = call.empty_maps([g is None for g in grads])
            bufs = [s if g is None else g for s, g in zip(spare, grads)]
            grad = grad.contiguous()
            ptrs = call.pointers(bufs)
            with _nat.device_guard(call.dev):
                _nat.check(_nat.lib().accv_scatter_at_centers(ctypes.addressof(ptrs), *call.geometry(where, sizes),
                                                              call.flags, grad.data_ptr(), _nat.stream_ptr(call.dev)),
                           "gather_at_centers backward")
        return (None, None, None, *grads)


class _CenterRegressionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, where, sizes, targets, weights, params, avg_factor, *maps):
        dev = call.dev
        loss = torch.zeros((), dtype=torch.float32, device=dev) if call.B == 0 else torch.empty((), dtype=torch.float32, device=dev)
        denom = torch.empty((), dtype=torch.float32, device=dev)
        flags = call.flags | (_nat.CR_WEIGHTS_PER_CHANNEL if weights is not None and weights.dim() == 3 else 0)
        if call.B > 0:
            lib = _nat.lib()
            ws = _nat.workspace(lib.accv_center_regression_loss_workspace_bytes(call.B), dev)
            ptrs = call.pointers(maps)
            with _nat.device_guard(dev):
                _nat.check(lib.accv_center_regression_loss(
                    ctypes.addressof(ptrs), *call.geometry(where, sizes), flags, targets.data_ptr(),
                    _ops.ptr(weights), ctypes.addressof(params),
                    avg_factor.data_ptr() if isinstance(avg_factor, torch.Tensor) else None, loss.data_ptr(),
                    denom.data_ptr(), ws.data_ptr(), ws.numel(), _nat.stream_ptr(dev)), "center_regression_loss")
        ctx.call, ctx.flags, ctx.params = call, flags, params
        ctx.has_weights = weights is not None
        # everything the backward kernel reads: alive until then, and guarded by torch's version check
        ctx.save_for_backward(where, sizes, targets, denom, *(() if weights is None else (weights,)), *maps)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        call = ctx.call
        where, sizes, targets, denom, *rest = ctx.saved_tensors
        weights, maps = (rest[0], rest[1:]) if ctx.has_weights else (None, rest)
        grads = [torch.empty_like(m) if need else None for m, need in zip(maps, ctx.needs_input_grad[7:])]
        if any(g is not None and g.numel() > 0 for g in grads):
            bufs = [torch.empty_like(m) if g is None else g for m, g in zip(maps, grads)]
            grad = grad.contiguous().to(torch.float32)
            feat_ptrs, grad_ptrs = call.pointers(maps), call.pointers(bufs)
            with _nat.device_guard(call.dev):
                _nat.check(_nat.lib().accv_center_regression_loss_bwd(
                    ctypes.addressof(feat_ptrs), ctypes.addressof(grad_ptrs), *call.geometry(where, sizes), ctx.flags,
                    targets.data_ptr(), _ops.ptr(weights), ctypes.addressof(ctx.params),
                    grad.data_ptr(), denom.data_ptr(), _nat.stream_ptr(call.dev)), "center_regression_loss backward")
        return (None, None, None, None, None, None, None, *grads)


def gather_at_centers(feats: Union[torch.Tensor, Sequence[torch.Tensor]], where):
    """The values of regression maps at object centres: mmdet's ``transpose_and_gather_feat`` without the transpose.

    Args:
        feats: one ``[B, C, H, W]`` tensor or a sequence of up to 8 of them with equal ``B, H, W``, dtype and device (the
            separate heads of a CenterPoint task: reg, height, dim, rot, vel); contiguous, on a GPU; float32, float16 or
            bfloat16.  They are read in place, never concatenated or copied.  Their channels are concatenated in the order
            given, ``C = sum(C_i)``, at most 64 in total.
        where: either a RaggedBatch (anything with ``.tensor`` and ``.sample_sizes``) of int32 centres ``[B, Nmax, 2]`` as
            ``(x, y)`` — the object ``draw_heatmap_batched`` takes; only ``sample_sizes`` (int32 or int64) decides which
            slots are read — or an int64 tensor ``[B, K]`` of in-plane indices ``y * W + x``, what
            ``heatmap_peaks(..., per_class=False).indices`` returns.

    Returns: a RaggedBatch ``[B, Nmax, C]`` with the same sample sizes, or a tensor ``[B, K, C]``, in the dtype of
    ``feats``.  A slot is valid when it lies below its frame's sample size and its cell inside the map; valid rows are
    bit-exact copies of ``feats[i][b, :, y, x]``, every other row (padding, centres outside the map) is exactly 0, and
    nothing outside the maps is ever read.

    Differentiable w.r.t. every tensor in ``feats`` (gradient in their dtype; no double backward).  The tensors read by
    the backward (the centres and their sample sizes, or the indices) are saved; modifying them in place before
    ``backward()`` raises.  The maps are not read again: they are not kept alive and may change.  The backward is one
    kernel that writes the gradient maps completely — zeros, and at each valid cell the sum of the rows that name it, in
    ascending slot order, accumulated in float32 and rounded once — without atomics, so it is bitwise reproducible.  One
    launch per direction on torch's current stream; no host synchronisation.

    Read-back of a CenterNet head, from the peaks to boxes::

        peaks = heatmap_peaks(heat.sigmoid(), k)                       # [B, k] scores, indices, classes, ys, xs
        off, wh = gather_at_centers([offset_map, wh_map], peaks.indices).split(2, -1)
        cx, cy = peaks.xs + off[..., 0], peaks.ys + off[..., 1]
        boxes = torch.stack([cx - wh[..., 0] / 2, cy - wh[..., 1] / 2, cx + wh[..., 0] / 2, cy + wh[..., 1] / 2], -1)
        keep = peaks.scores > score_thr
    """
    who = "gather_at_centers"
    maps = _check_feats(who, feats)
    first = maps[0]
    if _ops.is_ragged(where):
        call_where, call_sizes = _check_ragged_centers(who, where, first)
        call = _Call(maps, call_where, call_sizes, False)
    else:
        if not isinstance(where, torch.Tensor):
            raise RuntimeError(f"{who}: where must be a RaggedBatch of int32 centres or an int64 tensor [B, K] of indices")
        if where.device != first.device:
            raise RuntimeError(f"{who}: where must be on the maps' device {first.device}, got {where.device}")
        if where.dtype != torch.int64 or where.dim() != 2 or where.shape[0] != first.shape[0]:
            raise RuntimeError(f"{who}: indices must be int64 [B, K] with B = {first.shape[0]}, got {where.dtype} "
                               f"{tuple(where.shape)}")
        if not where.is_contiguous():
            raise RuntimeError(f"{who}: indices must be contiguous")
        call_where, call_sizes = where, None
        call = _Call(maps, where, None, True)
    out = _GatherAtCenters.apply(call, call_where, call_sizes, *maps)
    return RaggedBatch(out, sample_sizes=where.sample_sizes) if _ops.is_ragged(where) else out


def center_regression_loss(feats: Union[torch.Tensor, Sequence[torch.Tensor]], centers, targets, weights=None, *,
                           kind: str = "l1", beta: float = 1.0,
                           avg_factor: Optional[Union[float, torch.Tensor]] = None) -> torch.Tensor:
    """The regression term of a centre-point head as one 0-d float32 tensor::

        loss = sum over valid (b, n) and c of  w[b, n(, c)] * l(feats[b, c, y_bn, x_bn] - targets[b, n, c])  /  denom

    Args:
        feats, centers: as for :func:`gather_at_centers` (ragged int32 centres only).
        targets: float32 ``[B, Nmax, C]``, tensor or RaggedBatch, contiguous.
        weights: optional float32 ``[B, Nmax]`` (an object mask or weight) or ``[B, Nmax, C]`` (mask x code weights, as
            CenterPoint's ``bbox_weights``), tensor or RaggedBatch.  Rows of invalid slots of ``targets`` and ``weights``
            are never read.  Neither takes a gradient; one that requires grad is refused.
        kind: ``"l1"`` or ``"smooth_l1"`` (with ``beta`` > 0): torch's ``l1_loss`` / ``smooth_l1_loss``.
        avg_factor: ``None`` divides by ``max(number of valid objects, 1)`` counted on the device; a Python number is used
            as given; a 0-d float32 tensor on the same device (a count shared with the heat-map loss, or all-reduced) is
            read on the device.  No gradient flows to it.

    Arithmetic in float32 with float16 / bfloat16 maps widened exactly; one float64 partial sum per frame, added in a
    fixed order, so the same inputs give the same bits on every run.  Differentiable w.r.t. every tensor in ``feats``
    (gradient in their dtype; no double backward) through the complete-write kernel of :func:`gather_at_centers`'s
    backward: the contribution of a slot is ``(w * l'(d)) * (grad / denom)`` in float32, several objects on one cell add
    up in ascending slot order.  The tensors read by the backward (maps, centres, sample sizes, targets, weights) are
    saved; modifying them in place before ``backward()`` raises.  Two launches forward, one backward, on torch's current
    stream; no host synchronisation.

    Special values follow float64 autograd of the definition: NaN / inf in a read cell, target or weight reach the loss
    and that cell's gradient; whatever invalid slots, unread cells or unread target rows hold reaches nothing.
    """
    who = "center_regression_loss"
    maps = _check_feats(who, feats)
    first = maps[0]
    c_t, sizes = _check_ragged_centers(who, centers, first)
    if kind not in _KINDS:
        raise RuntimeError(f"{who}: kind must be 'l1' or 'smooth_l1', got {kind!r}")
    if kind == "smooth_l1" and not (float(beta) > 0.0):
        raise RuntimeError(f"{who}: smooth_l1 needs beta > 0, got {beta}")
    B, N, C = first.shape[0], c_t.shape[1], sum(m.shape[1] for m in maps)
    targets, weights = _ops.tensor_of(targets), _ops.tensor_of(weights)
    for name, t, shapes in (("targets", targets, ((B, N, C),)), ("weights", weights, ((B, N), (B, N, C)))):
        if t is None and name == "weights":
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor or a RaggedBatch")
        if t.device != first.device:
            raise RuntimeError(f"{who}: {name} must be on the maps' device {first.device}, got {t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
        if tuple(t.shape) not in shapes:
            raise RuntimeError(f"{who}: {name} must have shape {' or '.join(str(list(s)) for s in shapes)}, got "
                               f"{list(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous")
        if t.requires_grad:
            raise RuntimeError(f"{who}: no gradient flows to {name}; detach it")
    mode, value, avg_factor = _nat.avg_factor_args(avg_factor, first.device, who, RuntimeError, "the maps' device")
    params = _nat.CenterRegressionParams(_KINDS[kind], mode, float(beta), value)
    call = _Call(maps, c_t, sizes, False)
    return _CenterRegressionLoss.apply(call, c_t, sizes, targets, weights, params, avg_factor, *maps)
