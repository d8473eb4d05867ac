"""How a Python operator hands its operands to the C-ABI: what counts as a ragged operand, that the operands of a call
share one device, are contiguous and are never copied silently, the argument checks that read the same in every operator,
and which entry runs — ``accv_X`` on the device's current stream or its host entry (``accv_X_host``, or the name the
operator gives).

Every check takes the operator's name ``who`` for its message.  Checks that one operator words differently stay with that
operator.  torch is imported on the first check that needs it, so importing this module needs none.
"""
from __future__ import annotations

from . import OK, SIGNATURES, check, device_guard, lib, stream_ptr

_torch = None
# accv_X -> accv_X_host; the names are the interned keys of SIGNATURES, which keeps the attribute look-up on lib() cheap
_HOST_ENTRY = {name[:-len("_host")]: name for name in SIGNATURES if name.endswith("_host")}


def _import_torch():
    global _torch
    import torch as _torch
    return _torch


def is_ragged(x) -> bool:
    return hasattr(x, "tensor") and hasattr(x, "sample_sizes")


def tensor_of(x):
    """the tensor of a RaggedBatch; a tensor (or None) as it is"""
    return x.tensor if x is not None and is_ragged(x) else x


def ptr(t):
    return None if t is None else t.data_ptr()


def is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def number(who, name, v, integer=False):
    if not (is_int(v) if integer else is_number(v)):
        raise RuntimeError(f"{who}: {name} must be a Python {'integer' if integer else 'number'}, got {v!r}")
    return v


def run(entry, args, device, who, host_extra=(), host_entry=None):
    """One native call: ``entry`` with torch's current stream of ``device`` behind ``args`` for a CUDA device, else its
    ``_host`` twin with the tuple ``host_extra`` behind them (what only the host entry takes).  ``host_entry`` names the
    host entry of an operator whose host entry is not ``entry + "_host"``."""
    if device.type == "cuda":
        with device_guard(device):
            status = getattr(lib(), entry)(*args, stream_ptr(device))
    else:
        status = getattr(lib(), host_entry or _HOST_ENTRY[entry])(*(args + host_extra))
    if status != OK:   # check() raises with the library's message; a launch that went well does not pay for the call
        check(status, who)


def check_operands(who, operands, ref, owner, required=()):
    """Every operand of ``operands`` (pairs of name and value) is a tensor, on the device of ``ref`` and contiguous.
    None is skipped unless the name is in ``required``; ``owner`` names ``ref`` in the message ("boxes'")."""
    tensor = (_torch or _import_torch()).Tensor
    device = None
    for name, t in operands:
        if t is None and name not in required:
            continue
        if not isinstance(t, tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor")
        if device is None:   # read once a tensor has been seen: ref is usually the first operand
            device = ref.device
        if t.device != device:
            raise RuntimeError(f"{who}: {name} must be on the {owner} device {device}, got {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous (it is not copied silently)")


def check_backend(who, name, device):
    if device.type not in ("cuda", "cpu"):
        raise RuntimeError(f"{who}: {name} must be CUDA or CPU tensors, got {device}")


def check_float32(who, name, t):
    """another float dtype is a TypeError; what is no float at all is left to the operand's own dtype and shape check"""
    torch = _torch or _import_torch()
    if t.is_floating_point() and t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32 (the definition is float32), got {t.dtype}")


def check_sample_sizes(who, sizes, B):
    torch = _torch or _import_torch()
    if sizes.dtype not in (torch.int32, torch.int64) or tuple(sizes.shape) != (B,):
        raise RuntimeError(f"{who}: sample_sizes must be int32 or int64 [{B}], got {sizes.dtype} {tuple(sizes.shape)}")


def check_bboxes(who, bboxes, b_t, dims):
    """``(B, G)`` of the ragged 2D boxes ``bboxes`` with the tensor ``b_t``; ``dims`` is how the operator writes the shape"""
    torch = _torch or _import_torch()
    if (b_t.dtype != torch.float32 or b_t.dim() != 3 or b_t.shape[2] != 4 or getattr(bboxes, "num_batch_dims", 1) != 1
            or getattr(bboxes, "non_uniform_dim", 1) != 1):
        raise RuntimeError(f"{who}: bboxes must be float32 {dims} with one batch dimension and non_uniform_dim 1, "
                           f"got {b_t.dtype} {tuple(b_t.shape)}")
    return int(b_t.shape[0]), int(b_t.shape[1])


def check_box_count(who, G, limit):
    if G > limit:
        raise RuntimeError(f"{who}: {G} box slots per frame, at most MAX_BOXES = {limit} are supported")


def image_hw_args(who, image_hw, hw_t, B, batch):
    """``(H, W)`` of the C-ABI: Python ints clamped to ``[0, 2^24]``, or ``(0, 0)`` next to a checked tensor ``hw_t``
    (``image_hw`` itself when it is a tensor, else None); ``batch`` is the operator's letter for ``B``"""
    torch = _torch or _import_torch()
    if hw_t is not None:
        if hw_t.dtype not in (torch.int32, torch.int64) or tuple(hw_t.shape) != (B, 2):
            raise RuntimeError(f"{who}: an image_hw tensor must be int32 or int64 [{B}, 2], got {hw_t.dtype} {tuple(hw_t.shape)}")
        return 0, 0
    if not isinstance(image_hw, (list, tuple)) or len(image_hw) != 2 or not (is_int(image_hw[0]) and is_int(image_hw[1])):
        raise RuntimeError(f"{who}: image_hw must be (H, W) Python ints or an integer tensor [{batch}, 2], got {image_hw!r}")
    return max(0, min(int(image_hw[0]), 1 << 24)), max(0, min(int(image_hw[1]), 1 << 24))
