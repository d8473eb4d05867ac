"""(private) What the detection decoders share on the Python side: the checks of the operands they take in (heat-map peaks,
regression maps read in place, ragged detections that share one ``sample_sizes``), of their thresholds and cuts, and the
rows they hand out.  As in ``_amd_native/operands.py``: every check takes the operator's name ``who``, a check that reads
the same in every operator lives here once, and what one operator words differently stays with that operator or is an
argument.  Every message and the order of the checks are pinned by ``tests/test_detection_intake_cpu.py``.
"""
from __future__ import annotations

import math

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops

_DTYPES = _nat.FLOAT_DTYPE_CODES


# ---------------------------------------------------------------------------------------------------------------- intake
def check_peaks(who, p, batch, max_k, t=None, ref=None):
    """scores, indices, classes of a HeatmapPeaks after every check.  ``batch`` is the operator's letter for the first
    axis; ``t`` the task of an operator that takes one HeatmapPeaks per task, ``ref`` then task 0's scores."""
    pre = "peaks" if t is None else f"peaks[{t}]"
    if not all(hasattr(p, n) for n in ("scores", "indices", "classes")):
        raise RuntimeError(f"{who}: {pre} must be a HeatmapPeaks (scores, indices, classes)")
    s, i, c = p.scores, p.indices, p.classes
    for name, x in (("scores", s), ("indices", i), ("classes", c)):
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"{who}: {pre}.{name} must be a tensor")
        if x.dim() != 2:
            raise RuntimeError(f"{who}: {pre}.{name} must be [{batch}, K] (heatmap_peaks with per_class=False), got "
                               f"{tuple(x.shape)}")
        if not x.is_contiguous():
            raise RuntimeError(f"{who}: {pre}.{name} must be contiguous (it is not copied silently)")
    _ops.check_backend(who, "peaks", s.device)
    if s.dtype not in _DTYPES or s.dtype == torch.float64:
        raise RuntimeError(f"{who}: {pre}.scores must be float32, float16 or bfloat16, got {s.dtype}")
    if not 1 <= s.shape[1] <= max_k:
        raise RuntimeError(f"{who}: K must be in 1..{max_k}, got {s.shape[1]}")
    if ref is None:
        ref = s
    elif s.dtype != ref.dtype or s.shape != ref.shape or s.device != ref.device:
        raise RuntimeError(f"{who}: {pre}.scores is {s.dtype} {tuple(s.shape)} on {s.device}, peaks[0].scores "
                           f"{ref.dtype} {tuple(ref.shape)} on {ref.device}: all tasks share B, K, dtype and device")
    for name, x in (("indices", i), ("classes", c)):
        if x.dtype != torch.int64 or x.shape != ref.shape or x.device != ref.device:
            raise RuntimeError(f"{who}: {pre}.{name} must be int64 {tuple(ref.shape)} on {ref.device}, got {x.dtype} "
                               f"{tuple(x.shape)} on {x.device}")
    return s, i, c


def maps_of(who, name, feats):
    """one map or a sequence of them as a tuple: the form every "up to 8 maps read in place" operand arrives in"""
    maps = (feats,) if isinstance(feats, torch.Tensor) else tuple(feats) if isinstance(feats, (list, tuple)) else None
    if not maps:
        raise RuntimeError(f"{who}: {name} must be a tensor or a non-empty sequence of tensors")
    return maps


def check_feats(who, feats, scores, batch, max_maps, t=None, ref=None):
    """the regression maps next to the peaks whose scores are ``scores``, as a tuple after every check.  ``t`` is the task
    of an operator that takes the maps per task, ``ref`` then task 0's first map."""
    pre, per, first = ("feats", "", "feats[0]") if t is None else (f"feats[{t}]", " per task", "feats[0][0]")
    maps = maps_of(who, pre, feats)
    if len(maps) > max_maps:
        raise RuntimeError(f"{who}: at most {max_maps} maps{per} are supported, {pre} has {len(maps)}")
    r = maps[0] if ref is None else ref
    for i, m in enumerate(maps):
        if not isinstance(m, torch.Tensor):
            raise RuntimeError(f"{who}: {pre}[{i}] must be a tensor")
        if m.dim() != 4:
            raise RuntimeError(f"{who}: {pre}[{i}] must be [{batch}, C, H, W], got {m.dim()} dimensions")
        if not m.is_contiguous():
            raise RuntimeError(f"{who}: {pre}[{i}] must be contiguous (a map is not copied silently)")
        if m.device != scores.device:
            raise RuntimeError(f"{who}: {pre}[{i}] is on {m.device}, the peaks on {scores.device}")
        if m.dtype not in _DTYPES or m.dtype == torch.float64:
            raise RuntimeError(f"{who}: feats must be float32, float16 or bfloat16, got {m.dtype}")
        if m.dtype != r.dtype:
            raise RuntimeError(f"{who}: {pre}[{i}] has dtype {m.dtype}, {first} {r.dtype}")
        if (m.shape[0], m.shape[2], m.shape[3]) != (scores.shape[0], r.shape[2], r.shape[3]):
            raise RuntimeError(f"{who}: {pre}[{i}] has shape {tuple(m.shape)}: {batch} = {scores.shape[0]}, H = {r.shape[2]} "
                               f"and W = {r.shape[3]} must agree")
    return maps


def check_tensor(who, name, x, dtype, rank, what, each=False):
    """the tensor of one member of a detections tuple; ``each`` words the backend check for a single tensor"""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{who}: {name} must hold a tensor")
    if x.dim() != rank:
        raise RuntimeError(f"{who}: {name} must be {what}, got {tuple(x.shape)}")
    if x.dtype != dtype:
        raise RuntimeError(f"{who}: {name} must be {str(dtype).replace('torch.', '')}, got {x.dtype}")
    if not each:
        _ops.check_backend(who, name, x.device)
    elif x.device.type not in ("cuda", "cpu"):
        raise RuntimeError(f"{who}: {name} must be a CUDA or CPU tensor, got {x.device}")
    if not x.is_contiguous():
        raise RuntimeError(f"{who}: {name} must be contiguous (it is not copied silently)")
    return x


def sizes_of(who, name, ragged, B, device):
    """the sample sizes of the RaggedBatch ``name``: an int64 tensor [B] on ``device``, contiguous"""
    sizes = ragged.sample_sizes
    if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int64 or tuple(sizes.shape) != (B,) or sizes.device != device:
        raise RuntimeError(f"{who}: the sample_sizes of {name} must be an int64 tensor ({B},) on {device}")
    if not sizes.is_contiguous():
        raise RuntimeError(f"{who}: the sample_sizes of {name} must be contiguous")
    return sizes


def shared_sample_sizes(who, pre, names, members, B, device, rule):
    """the sample sizes of ``members[0]``, which every other member shares: the same object, or a tensor of the same
    dtype and shape at the same data pointer.  ``rule`` closes the message."""
    sizes = sizes_of(who, f"{pre}.{names[0]}", members[0], B, device)
    for name, x in zip(names[1:], members[1:]):
        other = x.sample_sizes
        if other is not sizes and not (isinstance(other, torch.Tensor) and other.data_ptr() == sizes.data_ptr()
                                       and other.dtype == sizes.dtype and other.shape == sizes.shape):
            raise RuntimeError(f"{who}: {pre}.{name} does not share the sample_sizes of {pre}.{names[0]} ({rule})")
    return sizes


def threshold(who, name, v):
    """a threshold as a float, or None: a Python number that is not NaN"""
    if v is None:
        return None
    if math.isnan(_ops.number(who, name, v)):
        raise RuntimeError(f"{who}: {name} must not be NaN")
    return float(v)


def cut(who, name, v, or_none=""):
    """pre_max_size / post_max_size: a Python integer >= 1, or None; ``or_none`` is what an operator adds to the type
    message (" or None")"""
    if v is None:
        return None
    if not _ops.is_int(v):
        raise RuntimeError(f"{who}: {name} must be a Python integer{or_none}, got {v!r}")
    if v < 1:
        raise RuntimeError(f"{who}: {name} must be at least 1, got {v}")
    return v


# ---------------------------------------------------------------------------------------------------------------- output
def empty_outputs(shape, width, dev, extras=None):
    """uninitialised boxes ``shape + (width,)``, scores, labels and source ``shape`` and, with ``extras`` (their count, 0
    included), extras ``shape + (extras,)``: the kernel writes every element, padding too"""
    out = (torch.empty(shape + (width,), dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
           torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.int32, device=dev))
    return out if extras is None else out + (torch.empty(shape + (extras,), dtype=torch.float32, device=dev),)


def kept_sizes(shape, dev):
    """the int64 counts the kernel writes, batch axis last: zeros for an empty batch, which launches nothing"""
    return (torch.zeros if shape[-1] == 0 else torch.empty)(shape, dtype=torch.int64, device=dev)
