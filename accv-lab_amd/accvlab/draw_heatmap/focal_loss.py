"""(extension) The consumer of the drawn heat maps: the Gaussian focal loss of CenterNet / CenterPoint-style heads
(packages/draw_heatmap/docs/intro.rst:7-25 introduces the operator as the target of its centerness term), fused into ONE
streaming pass forward and one backward.

``gaussian_focal_loss(logits, target)`` equals this composition (what the tests pin)::

    p = logits.float().sigmoid()
    if clamp_eps > 0:
        p = p.clamp(clamp_eps, 1 - clamp_eps)      # CenterPoint's clamp_sigmoid; 0 = CenterNet (no clamp)
    pos = target.eq(1)
    pos_loss = -(p + 1e-12).log() * (1 - p).pow(alpha) * pos
    neg_loss = -(1 - p + 1e-12).log() * p.pow(alpha) * (1 - target).pow(gamma)
    total = (pos_weight * pos_loss + neg_weight * neg_loss).sum()
    loss = total / (pos.sum().clamp(min=1) if avg_factor is None else avg_factor)

without the ~ten full passes over the map that composition makes, and without the host synchronisation of a
``num_pos.item()``: the positive count is taken exactly in the same pass and stays on the device.  GPU only.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch.autograd.function import once_differentiable

from .. import _amd_native as _nat

_DTYPES = _nat.FLOAT_DTYPE_CODES


def _check(logits, target, alpha, gamma):
    for name, t in (("logits", logits), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"gaussian_focal_loss: {name} must be a tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"gaussian_focal_loss: {name} must be contiguous (a heat map is not copied silently)")
        if not t.is_cuda:
            raise RuntimeError(f"gaussian_focal_loss: {name} must be a CUDA tensor (there is no CPU path)")
    if logits.dtype not in _DTYPES or logits.dtype == torch.float64:
        raise RuntimeError(f"gaussian_focal_loss: logits must be float32, float16 or bfloat16, got {logits.dtype}")
    if target.dtype != torch.float32:
        raise RuntimeError(f"gaussian_focal_loss: target must be float32, got {target.dtype}")
    if target.shape != logits.shape:
        raise RuntimeError(f"gaussian_focal_loss: target shape {tuple(target.shape)} differs from logits "
                           f"{tuple(logits.shape)}")
    if target.device != logits.device:
        raise RuntimeError("gaussian_focal_loss: logits and target must be on the same device")
    if target.requires_grad:
        raise RuntimeError("gaussian_focal_loss: no gradient flows to target; detach it")
    if not (alpha >= 1.0 and gamma >= 0.0):
        raise RuntimeError(f"gaussian_focal_loss: needs alpha >= 1 and gamma >= 0, got alpha={alpha}, gamma={gamma}")


class _GaussianFocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, alpha, gamma, pos_weight, neg_weight, clamp_eps, avg):
        dev = logits.device
        n = logits.numel()
        loss = torch.zeros((), dtype=torch.float32, device=dev) if n == 0 else torch.empty((), dtype=torch.float32, device=dev)
        denom = torch.empty((), dtype=torch.float32, device=dev)
        params = (float(alpha), float(gamma), float(pos_weight), float(neg_weight), float(clamp_eps))
        mode, value, avg_dev = avg
        dev_ptr = avg_dev.data_ptr() if avg_dev is not None else None
        if n > 0:
            lib = _nat.lib()
            ws = _nat.workspace(lib.accv_gaussian_focal_loss_workspace_bytes(n), dev)
            with _nat.device_guard(dev):
                _nat.check(lib.accv_gaussian_focal_loss(
                    logits.data_ptr(), target.data_ptr(), n, _DTYPES[logits.dtype], *params, mode, value, dev_ptr,
                    loss.data_ptr(), denom.data_ptr(), ws.data_ptr(), ws.numel(), _nat.stream_ptr(dev)),
                    "gaussian_focal_loss")
        ctx.save_for_backward(logits, target, denom)
        ctx.params = params
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        logits, target, denom = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        g = torch.empty_like(logits)
        if logits.numel() > 0:
            grad = grad.contiguous().to(torch.float32)
            with _nat.device_guard(logits.device):
                _nat.check(_nat.lib().accv_gaussian_focal_loss_bwd(
                    logits.data_ptr(), target.data_ptr(), logits.numel(), _DTYPES[logits.dtype], *ctx.params,
                    grad.data_ptr(), denom.data_ptr(), g.data_ptr(), _nat.stream_ptr(logits.device)),
                    "gaussian_focal_loss backward")
        return g, None, None, None, None, None, None, None


def gaussian_focal_loss(logits: torch.Tensor, target: torch.Tensor, *, alpha: float = 2.0, gamma: float = 4.0,
                        pos_weight: float = 1.0, neg_weight: float = 1.0, clamp_eps: float = 1e-4,
                        avg_factor: Optional[Union[float, torch.Tensor]] = None) -> torch.Tensor:
    """Gaussian focal loss of raw head outputs against a drawn heat-map target, as a 0-d float32 tensor.

    Args:
        logits: the head output before the sigmoid — any shape, contiguous, on a GPU; float32, float16 or bfloat16.
        target: float32 of the same shape and device, contiguous: what ``draw_heatmap*`` writes (``[B, H, W]``,
            ``[B, C, H, W]`` or any other layout — the op is shape-agnostic).  Elements equal to 1 are the positives.
        alpha, gamma: focal exponent of the prediction (>= 1) and of the Gaussian penalty reduction (>= 0).
            ``alpha=2, gamma=4`` run as multiplications; other values through ``powf``.
        pos_weight, neg_weight: weights of the positive and the negative term.
        clamp_eps: the sigmoid is clamped to ``[clamp_eps, 1 - clamp_eps]`` (CenterPoint's ``clamp_sigmoid``);
            0 disables the clamp (CenterNet).  Must be below 0.5.
        avg_factor: ``None`` divides by ``max(num_pos, 1)`` with ``num_pos`` counted exactly on the device; a Python
            number is used as given; a 0-d float32 tensor on the same device (e.g. an all-reduced count) is read on the
            device.  No gradient flows to it.

    Returns: the loss, 0-d float32 (0 for empty inputs).  Differentiable w.r.t. ``logits`` only (the gradient has the
    dtype of ``logits``; double backward is not supported); a ``target`` that requires grad is refused.  Neither
    direction synchronises with the host: one streaming kernel plus a one-block finishing kernel forward, one streaming
    kernel backward, all on torch's current stream.  The forward is bitwise reproducible (no atomics).

    Special values follow float64 autograd of the definition: a NaN logit makes the loss NaN and its own gradient NaN
    (so AMP's ``GradScaler`` skips the step), the clamp still gives exactly 0 gradient to finite logits outside
    ``[eps, 1 - eps]``, and ±inf logits give a finite loss and a zero gradient.
    """
    _check(logits, target, alpha, gamma)
    avg = _nat.avg_factor_args(avg_factor, logits.device, "gaussian_focal_loss", RuntimeError, "the logits' device")
    return _GaussianFocalLoss.apply(logits, target, alpha, gamma, pos_weight, neg_weight, clamp_eps, avg)
