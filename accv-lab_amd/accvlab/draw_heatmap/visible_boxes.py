"""(extension) Which 2D boxes of a camera image become heat-map targets at all: the reference's ``VisibleBboxSelector``
step (packages/dali_pipeline_framework, processing_steps/visible_bbox_selector.py; the operators ``check_bbox_visibiity``
and ``check_minimum_bbox_size``, operators_impl/numba_operators/numba_operators.py:240-403) for a ragged batch in one
launch.  A box is dropped when nearer boxes cover it completely, or when it is smaller than a minimum size after clipping
to the image.

The reference paints an ``H x W`` int32 canvas per sample on the CPU and calls ``np.unique`` on it.  Here nothing is
proportional to the image: after clipping all edges are integers, so a box is visible exactly if it is the top-most box at
one of the points (x edge, y edge) of its frame (``csrc/visible_boxes.hip``).
"""
from __future__ import annotations

import ctypes

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MAX_BOXES = _nat.VB_MAX_BOXES
_WHO = "visible_bbox_mask"


def visible_bbox_mask(bboxes, depths=None, *, image_hw, check_occlusion: bool = True, minimum_size=None,
                      shrink_to_int: bool = False):
    """The mask of the boxes that stay, bool ``[B, G_max]``, as a RaggedBatch that shares ``bboxes``' sample sizes.

    Args:
        bboxes: RaggedBatch float32 ``[B, G_max, 4]``, contiguous, one batch dimension, ``non_uniform_dim`` 1; rows
            ``(x1, y1, x2, y2)`` with the corners in either order.  ``G_max`` is limited to ``MAX_BOXES`` = 256 per frame;
            more raise ``RuntimeError`` before any launch.  Only ``bboxes.sample_sizes`` (int32 or int64, read on the device
            and clamped to ``[0, G_max]``) decides which slots are boxes.  Other float dtypes raise ``TypeError``.
        depths: RaggedBatch or tensor float32 ``[B, G_max]``, smaller is nearer; required with ``check_occlusion``.
        image_hw: ``(H, W)`` Python ints for every frame, or an int32 / int64 tensor ``[B, 2]`` on the boxes' device (read
            there); values are clamped to ``[0, 2^24]``, where every comparison below is exact in float32.
        check_occlusion, minimum_size: at least one check must be requested; with both the result is their AND, and a box
            that fails the size test still occludes.
        shrink_to_int: round the corners inwards instead of outwards.

    Per frame, in float32 until the conversion to integers:

    1. ``min_x = b0 if b0 < b2 else b2``, ``max_x`` the other one, y likewise; a box with a NaN coordinate is never visible
       and paints nothing;
    2. lower edges ``floor``, upper edges ``ceil`` (``ceil`` and ``floor`` with ``shrink_to_int``); each rounded edge is
       clamped to ``[-1, W + 1]`` (``[-1, H + 1]``), which changes no decision for a finite value and defines inf and 1e30;
    3. a box with ``min_x > W or max_x < 0 or min_y > H or max_y < 0`` is outside: never visible, paints nothing;
    4. the rest paints its clip to the image, the half-open ``[min_x, max_x) x [min_y, max_y)``; an empty one paints nothing;
    5. paint order ``np.argsort(-depth, kind="stable")``, last on top: ``j`` lies above ``i`` iff ``depth_j < depth_i``, or
       they are equal and ``j > i`` (the reference's unstable sort leaves ties open); ``-0.0 == 0.0``; a NaN depth lies
       above every number and two NaNs tie;
    6. occlusion: true iff some pixel of the painted rectangle is in the painted rectangle of no box above it;
    7. size: raw coordinates clipped to ``[0, W]`` / ``[0, H]``, then ``|x2 - x1| >= float32(minimum_size)`` and
       ``|y2 - y1| >= float32(minimum_size)``; NaN gives false.

    Padding slots are never read as boxes and come out ``False``; every output element is written.  GPU tensors run one HIP
    kernel on torch's current stream (a workgroup per frame, no memory proportional to ``H * W``, no host synchronisation,
    bitwise reproducible); CPU tensors run the library's host entry over the same integer algorithm, with equal results.
    Nothing takes a gradient.
    """
    if not _ops.is_ragged(bboxes):
        raise RuntimeError(f"{_WHO}: bboxes must be a RaggedBatch of float32 [B, G_max, 4]")
    b_t, sizes = bboxes.tensor, bboxes.sample_sizes
    if not check_occlusion and minimum_size is None:
        raise RuntimeError(f"{_WHO}: at least one of check_occlusion and minimum_size must be requested")
    if check_occlusion and depths is None:
        raise RuntimeError(f"{_WHO}: check_occlusion needs depths")
    d_t = _ops.tensor_of(depths) if check_occlusion else None
    hw_t = image_hw if isinstance(image_hw, torch.Tensor) else None
    _ops.check_operands(_WHO, (("bboxes", b_t), ("depths", d_t), ("sample_sizes", sizes), ("image_hw", hw_t)), b_t, "boxes'")
    _ops.check_backend(_WHO, "bboxes", b_t.device)
    _ops.check_float32(_WHO, "bboxes", b_t)
    B, G = _ops.check_bboxes(_WHO, bboxes, b_t, "[B, G_max, 4]")
    if d_t is not None:
        _ops.check_float32(_WHO, "depths", d_t)
        if d_t.dtype != torch.float32 or tuple(d_t.shape) != (B, G):
            raise RuntimeError(f"{_WHO}: depths must be float32 [{B}, {G}], got {d_t.dtype} {tuple(d_t.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, B)
    H, W = _ops.image_hw_args(_WHO, image_hw, hw_t, B, "B")
    if minimum_size is not None and not _ops.is_number(minimum_size):
        raise RuntimeError(f"{_WHO}: minimum_size must be a Python number or None, got {minimum_size!r}")
    _ops.check_box_count(_WHO, G, MAX_BOXES)

    dev = b_t.device
    out = torch.empty((B, G), dtype=torch.bool, device=dev)
    if B > 0 and G > 0:
        params = _nat.VisibleBoxesParams(float(minimum_size) if minimum_size is not None else 0.0, H, W,
                                         1 if check_occlusion else 0, 0 if minimum_size is None else 1, 1 if shrink_to_int else 0)
        flags = ((_nat.VB_COUNTS_I64 if sizes.dtype == torch.int64 else 0)
                 | (_nat.VB_HW_I64 if hw_t is not None and hw_t.dtype == torch.int64 else 0))
        args = (b_t.data_ptr(), _ops.ptr(d_t), sizes.data_ptr(), _ops.ptr(hw_t), flags, B, G, ctypes.addressof(params),
                out.data_ptr())
        _ops.run("accv_visible_boxes", args, dev, _WHO)
    return RaggedBatch(out, sample_sizes=sizes)


def select_visible_bboxes(bboxes, depths, *others, image_hw, check_occlusion: bool = True, minimum_size=None,
                          shrink_to_int: bool = False):
    """The reference's ``VisibleBboxSelector`` followed by its ``ConditionalElementRemover``: the mask of
    :func:`visible_bbox_mask` (same arguments) and every given RaggedBatch compacted by it.

    Returns ``(mask, bboxes', depths', *others')``; ``depths`` may be ``None`` without the occlusion check and then stays
    ``None``.  The compaction is ``batched_bool_indexing`` (no new kernel; its read-back of the largest kept count is the
    one host synchronisation), so the results share the layout of every other RaggedBatch of the package and go straight
    into ``get_centers_and_radii``::

        mask, boxes, depths, centers = select_visible_bboxes(boxes, depths, centers, image_hw=(900, 1600), minimum_size=2)
        c, r = get_centers_and_radii(centers, boxes, 4.0)
        draw_heatmap_batched(heatmap, c, r, clear=True)
    """
    from ..batching_helpers import batched_bool_indexing

    mask = visible_bbox_mask(bboxes, depths, image_hw=image_hw, check_occlusion=check_occlusion, minimum_size=minimum_size,
                             shrink_to_int=shrink_to_int)
    return (mask,) + tuple(None if x is None else batched_bool_indexing(x, mask) for x in (bboxes, depths) + others)
