"""(extension) The read-back half of the drawn heat maps: mmdet's ``get_local_maximum`` + ``get_topk_from_heatmap``
(models/utils/gaussian_target.py, which packages/draw_heatmap/docs/intro.rst names as what the drawing operator replaces),
fused into two HIP launches that read the map once.

``heatmap_peaks(heat, k)`` equals this composition (what the tests pin)::

    hmax = F.max_pool2d(heat, kernel, stride=1, padding=(kernel - 1) // 2)
    s = heat * (hmax == heat)                                         # get_local_maximum
    scores, order = torch.sort(s.view(B, -1), dim=1, descending=True, stable=True)
    scores, inds = scores[:, :k], order[:, :k]                        # get_topk_from_heatmap, with a defined tie order
    classes, inds = inds // (H * W), inds % (H * W)
    ys, xs = inds // W, inds % W

without the ~five full passes of the composition and without ``torch.topk``'s unspecified order of equal scores.  GPU only.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import _amd_native as _nat

_DTYPES = _nat.FLOAT_DTYPE_CODES
_MAX_K = 1024


class HeatmapPeaks(NamedTuple):
    scores: torch.Tensor
    indices: torch.Tensor
    classes: torch.Tensor
    ys: torch.Tensor
    xs: torch.Tensor


def _check(heatmap, k, kernel):
    if not isinstance(heatmap, torch.Tensor):
        raise RuntimeError("heatmap_peaks: heatmap must be a tensor")
    if not heatmap.is_cuda:
        raise RuntimeError("heatmap_peaks: heatmap must be a CUDA tensor (there is no CPU path)")
    if not heatmap.is_contiguous():
        raise RuntimeError("heatmap_peaks: heatmap must be contiguous (a heat map is not copied silently)")
    if heatmap.dtype not in _DTYPES or heatmap.dtype == torch.float64:
        raise RuntimeError(f"heatmap_peaks: heatmap must be float32, float16 or bfloat16, got {heatmap.dtype}")
    if heatmap.dim() not in (3, 4):
        raise RuntimeError(f"heatmap_peaks: heatmap must be [B, H, W] or [B, C, H, W], got {heatmap.dim()} dimensions")
    if isinstance(kernel, bool) or not isinstance(kernel, int) or not (1 <= kernel <= 7) or kernel % 2 == 0:
        raise RuntimeError(f"heatmap_peaks: kernel must be odd and in 1..7, got {kernel!r}")
    if isinstance(k, bool) or not isinstance(k, int) or not (1 <= k <= _MAX_K):
        raise RuntimeError(f"heatmap_peaks: k must be an integer in 1..{_MAX_K}, got {k!r}")


def heatmap_peaks(heatmap: torch.Tensor, k: int, *, kernel: int = 3, per_class: bool = False) -> HeatmapPeaks:
    """The ``k`` strongest local maxima of a heat map, per frame or per class plane, in a defined order.

    Args:
        heatmap: ``[B, H, W]`` (one class) or ``[B, C, H, W]``; contiguous, on a GPU; float32, float16 or bfloat16.
            It is read, never modified or copied.
        k: peaks per group, 1..1024 and at most the group size.
        kernel: odd window size in 1..7 of the local-maximum test (mmdet's ``get_local_maximum`` kernel).
        per_class: ``False`` ranks each frame's C·H·W elements together (mmdet's ``get_topk_from_heatmap``);
            ``True`` ranks each ``(b, c)`` plane on its own.

    Definition: ``s = x * (x == max over the kernel x kernel window)``, the window clipped at the map border (as
    ``max_pool2d`` with padding ``kernel // 2``); every member of a plateau survives, suppressed elements score 0.  Per
    group the ``k`` largest ``s`` in descending order; equal scores come in ascending flat index of the group
    (class-major when ``per_class=False``) — exactly ``torch.sort(s, descending=True, stable=True)`` cut at ``k``, so a map
    with fewer than ``k`` peaks is filled up deterministically with its first suppressed elements.  NaN and infinities
    follow the same composition: the window maximum carries NaN through (as ``max_pool2d``), so a NaN scores NaN, its
    finite neighbours score 0 and a suppressed ±inf scores NaN (``inf * 0``); every NaN, whatever its sign or payload,
    ranks above +inf, NaNs among themselves by ascending index, and reads back as NaN.  -0.0 ties with +0.0.

    Returns: ``HeatmapPeaks(scores, indices, classes, ys, xs)``, each ``[B, k]`` (``[B, C, k]`` with ``per_class=True``).
    ``scores`` has the input dtype and holds the map's values exactly; ``indices`` (in-plane ``y * W + x``), ``classes``
    (0 for a 3-D map), ``ys`` and ``xs`` are int64.  Differences from mmdet: there ``xs`` is float, here int64; and the
    order of equal scores is defined here, unspecified there (``torch.topk``).

    The outputs carry no gradient.  To train through the selected scores gather them from the map::

        peaks = heatmap_peaks(heat.detach(), k)
        scores = heat.flatten(-2).gather(-1, peaks.indices)                       # per_class=True: [B, C, k]
        scores = heat.flatten(1).gather(1, peaks.classes * H * W + peaks.indices)  # per_class=False: [B, k]

    and a score threshold is one line on the sorted result: ``keep = peaks.scores > thr``.

    Two launches on torch's current stream; no host synchronisation; allocates only the outputs and one workspace.
    Results are bitwise reproducible.
    """
    _check(heatmap, k, kernel)
    if heatmap.dim() == 3:
        B, H, W = heatmap.shape
        C = 1
    else:
        B, C, H, W = heatmap.shape
    group = H * W if per_class else C * H * W
    if k > group:
        raise RuntimeError(f"heatmap_peaks: k = {k} exceeds the group size {group}")
    dev = heatmap.device
    shape = (B, C, k) if per_class else (B, k)
    scores = torch.empty(shape, dtype=heatmap.dtype, device=dev)
    indices, classes, ys, xs = (torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(4))
    if B > 0 and C > 0:
        lib = _nat.lib()
        ws_bytes = lib.accv_heatmap_peaks_workspace_bytes(B, C, H, W, k)
        if ws_bytes == 0:
            raise RuntimeError(f"heatmap_peaks: map {B} x {C} x {H} x {W} is too large (groups below 2^32 - 1 elements)")
        ws = _nat.workspace(ws_bytes, dev)
        with _nat.device_guard(dev):
            _nat.check(lib.accv_heatmap_peaks(
                heatmap.data_ptr(), _DTYPES[heatmap.dtype], B, C, H, W, kernel, k, 1 if per_class else 0,
                scores.data_ptr(), indices.data_ptr(), classes.data_ptr(), ys.data_ptr(), xs.data_ptr(),
                ws.data_ptr(), ws.numel(), _nat.stream_ptr(dev)), "heatmap_peaks")
    return HeatmapPeaks(scores, indices, classes, ys, xs)
