"""(private) What the losses over matched pairs — ``matched_focal_loss``, ``matched_box_loss``, ``matched_polyline_loss`` —
share on the host side: the validation of the match indices and of the dense prediction, and the two calls through the
C ABI.  Every function takes the operator's name ``who`` for its messages; the pair rule itself is ``csrc/matched_pairs.h``.
"""
from __future__ import annotations

import torch

from .. import _amd_native as _nat
from .ragged import RaggedBatch

DTYPES = _nat.FLOAT_DTYPE_CODES


def ragged(who, name, rb, what, dims):
    """the padded tensor of a RaggedBatch ``what`` (``"[B, G*, D]"``) of ``dims`` dimensions, detached and contiguous"""
    if not isinstance(rb, RaggedBatch):
        raise TypeError(f"{who}: {name} must be a RaggedBatch {what}, got {type(rb).__name__}")
    t = rb.tensor
    if rb.num_batch_dims != 1 or t.dim() != dims or rb.non_uniform_dim != 1:
        raise ValueError(f"{who}: {name} must be a RaggedBatch {what} with non_uniform_dim 1, got shape {tuple(t.shape)}, "
                         f"non_uniform_dim {rb.non_uniform_dim}")
    return t.detach().contiguous()


def index(who, name, rb, what="[B, K]"):
    t = ragged(who, name, rb, what, 2)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{who}: {name} must be int32 or int64, got {t.dtype}")
    return t


def match_indices(who, pred_ind, gt_ind):
    """-> (pind, gind, counts): both ``[B, K]`` index tensors and ``pred_ind.sample_sizes`` as int64 ``[B]``"""
    pind = index(who, "pred_ind", pred_ind)
    gind = index(who, "gt_ind", gt_ind)
    if pind.dtype != gind.dtype:
        raise TypeError(f"{who}: pred_ind is {pind.dtype}, gt_ind {gind.dtype}: one index dtype expected")
    if pind.shape != gind.shape:
        raise ValueError(f"{who}: pred_ind has shape {tuple(pind.shape)}, gt_ind {tuple(gind.shape)}")
    sizes = pred_ind.sample_sizes
    if sizes.dim() != 1 or sizes.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{who}: pred_ind.sample_sizes must be int32 or int64 [B]")
    return pind, gind, sizes.detach().to(torch.int64).contiguous()


def same_place(who, dev, B, named, ref=None):
    """every tensor of ``named`` (pairs of name and tensor or None) is on ``dev`` and has batch size ``B``; ``ref`` names
    the tensor that ``dev`` and ``B`` come from in the messages"""
    for name, t in named:
        if t is None:
            continue
        if t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, {f'{ref} on' if ref else 'expected'} {dev}")
        if int(t.shape[0]) != B:
            raise ValueError(f"{who}: {name} has batch size {t.shape[0]}, {ref or 'expected'} {B}")


def query_weights(who, weights, pred, pred_name):
    """``query_weights`` ``[B, Q]`` of the dtype of ``pred`` ``[B, Q, ...]``, detached and contiguous, or None"""
    if weights is None:
        return None
    B, Q = int(pred.shape[0]), int(pred.shape[1])
    if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (B, Q):
        raise ValueError(f"{who}: query_weights must be a tensor [B, Q] = [{B}, {Q}], got "
                         f"{tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights).__name__}")
    if weights.dtype != pred.dtype:
        raise TypeError(f"{who}: query_weights is {weights.dtype}, {pred_name} {pred.dtype}")
    return weights.detach().contiguous()


def dense(who, name, t, dims, unit_stride=True):
    """the dense prediction ``name`` of dimensions ``dims`` (``"[B, Q, C]"``): a float tensor of that rank on a supported
    device, with unit stride in its last dimension where ``unit_stride`` asks for it"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if t.dim() != dims.count(",") + 1:
        raise ValueError(f"{who}: {name} must be {dims}, got shape {tuple(t.shape)}")
    if t.dtype not in DTYPES:
        raise TypeError(f"{who}: {name} must be float32, float16, bfloat16 or float64, got {t.dtype}")
    if unit_stride and t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{who}: the last dimension of {name} must have unit stride, got stride {t.stride(-1)}")
    if t.device.type not in ("cuda", "cpu"):
        raise RuntimeError(f"{who}: unsupported device {t.device}")


def not_overlapping(who, name, t, row):
    """the rows of ``row`` elements of ``t`` ``[B, Q, ...]`` neither overlap nor run backwards"""
    if t.shape[1] > 1 and row > 0 and t.stride(1) < row or t.shape[0] > 1 and t.stride(0) < 0:
        raise ValueError(f"{who}: overlapping or reversed {name} (strides {t.stride()}) are not supported")


def out_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def run_forward(who, stem, call, tensors, run, n_out, workspace_dims):
    """-> (out, denom).  ``out`` is ``[B]`` for one output and ``[n_out, B]`` otherwise: written by the entry point ``stem``
    (its ``_host`` twin for CPU tensors) when ``run``, zeros when nothing runs.  ``call`` gives the pointer and shape
    arguments, ``workspace_dims`` is what ``<stem>_workspace_bytes`` takes."""
    dev = call.dev
    out = (torch.empty if run else torch.zeros)((call.B,) if n_out == 1 else (n_out, call.B), dtype=call.out_dtype, device=dev)
    denom = torch.empty((), dtype=torch.float64, device=dev)
    if run:
        lib = _nat.lib()
        args = (*call.inputs(*tensors), *call.shape(tensors[0]), out.data_ptr(), denom.data_ptr())
        if dev.type == "cuda":
            nbytes = getattr(lib, stem + "_workspace_bytes")(*workspace_dims)
            ws = _nat.workspace(nbytes, dev)
            with _nat.device_guard(dev):
                _nat.check(getattr(lib, stem)(*args, ws.data_ptr(), nbytes, _nat.stream_ptr(dev)), who)
        else:
            _nat.check(getattr(lib, stem + "_host")(*args), who)
    return out, denom


def run_backward(who, stem, call, tensors, grads, denom):
    """-> the gradient of ``tensors[0]`` in its dtype, contiguous and written completely by ``<stem>_bwd`` (``_bwd_host``
    for CPU tensors); a gradient of ``grads`` that is None goes down as a null pointer"""
    dev, pred = call.dev, tensors[0]
    grad = torch.empty(pred.shape, dtype=pred.dtype, device=dev)
    grads = [None if g is None else g.to(call.out_dtype).contiguous() for g in grads]
    args = (*call.inputs(*tensors), *(None if g is None else g.data_ptr() for g in grads), denom.data_ptr(),
            *call.shape(pred), grad.data_ptr())
    lib = _nat.lib()
    if dev.type == "cuda":
        with _nat.device_guard(dev):
            _nat.check(getattr(lib, stem + "_bwd")(*args, _nat.stream_ptr(dev)), who + " backward")
    else:
        _nat.check(getattr(lib, stem + "_bwd_host")(*args), who + " backward")
    return grad
