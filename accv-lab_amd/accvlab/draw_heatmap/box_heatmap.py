"""(extension) 2D boxes of a camera batch -> Gaussian heat maps and the per-object targets of a CenterNet-style head: the
reference's ``BoundingBoxToHeatmapConverter`` step (packages/dali_pipeline_framework, processing_steps/
bounding_box_to_heatmap_converter.py; helpers ``apply_clipping_and_get_with_clipping_info`` / ``get_is_active``,
operators_impl/python_operator_functions/python_operator_functions.py:103-252, ``get_center_from_bboxes`` /
``get_radii_from_bboxes``, operators_impl/numba_operators/numba_operators.py:788-905, and the native rasteriser
ext_impl/DrawGaussians.cc:32-76) for a ragged batch in one launch.  It follows ``select_visible_bboxes`` in the 2D target
chain, as the reference's step follows its ``VisibleBboxSelector``.

The reference runs this step per sample on DALI's CPU threads.  Here one HIP kernel scales, clips, decides, writes the side
outputs and draws the maps (``csrc/box_heatmap.hip``; the per-object arithmetic is ``csrc/box_heatmap_arith.h``).
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MAX_BOXES = _nat.BH_MAX_BOXES
MAX_CATEGORIES = _nat.BH_MAX_CATEGORIES
_WHO = "boxes_to_heatmap"


class BoxHeatmapTargets(NamedTuple):
    """Result of :func:`boxes_to_heatmap`; the per-object fields are RaggedBatches that share ``bboxes.sample_sizes``."""
    heatmap: torch.Tensor          # float32 [B, C, H, W], or [B, H, W] with use_per_category_heatmap=False
    is_active: object              # bool [B, G]
    center: object                 # int32 [B, G, 2], (x, y)
    center_offset: object          # float32 [B, G, 2], (x, y)
    height_width: object           # float32 [B, G, 2], (h, w)
    bboxes_heatmap: object         # float32 [B, G, 4]
    radii: object                  # float32 [B, G]


def _pair(name, v):
    if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(_ops.is_number(x) for x in v):
        raise RuntimeError(f"{_WHO}: {name} must be a (height, width) pair of Python numbers, got {v!r}")
    return float(v[0]), float(v[1])


def boxes_to_heatmap(bboxes, *, image_hw, heatmap_hw, centers=None, categories=None, num_categories=None, is_valid=None,
                     min_object_size=None, per_category_min_object_sizes=None, use_per_category_heatmap: bool = True,
                     min_fraction_area_clipping: float = 0.25, min_radius: float = 0.5, max_radius: float = 10.0,
                     radius_scaling_factor: float = 0.8, radius_to_sigma_factor: float = 1.0 / 3.0, k_for_classes=None,
                     out=None) -> BoxHeatmapTargets:
    """Gaussian heat maps and per-object targets from image-space boxes, as a :class:`BoxHeatmapTargets`.

    Args:
        bboxes: RaggedBatch float32 ``[B, G_max, 4]``, contiguous, one batch dimension, ``non_uniform_dim`` 1; rows
            ``(x1, y1, x2, y2)`` in image pixels, the two corners in either order and on either diagonal.  ``G_max`` is
            limited to ``MAX_BOXES`` = 256 per frame; more raise ``RuntimeError`` before any launch.  Only
            ``bboxes.sample_sizes`` (int32 or int64, read on the device and clamped to ``[0, G_max]``) decides which slots
            are objects.  Other float dtypes raise ``TypeError``.
        image_hw: ``(H, W)`` Python ints for every frame, or an int32 / int64 tensor ``[B, 2]`` on the boxes' device (read
            there); values are clamped to ``[0, 2^24]``.
        heatmap_hw: ``(H, W)`` of the map, Python ints in ``[1, 2^24]``.
        centers: RaggedBatch or tensor float32 ``[B, G_max, 2]`` rows ``(x, y)`` in image pixels, e.g. the projection of a 3D
            centre; default: the box centre ``((b0 + b2) / 2, (b1 + b3) / 2)``.
        categories: RaggedBatch or tensor int32 / int64 ``[B, G_max]``.  Required, together with ``num_categories`` > 0
            (at most ``MAX_CATEGORIES`` = 128), when ``use_per_category_heatmap`` is true, ``num_categories`` is given or
            ``per_category_min_object_sizes`` is given (the reference constructor's rule); must be ``None`` otherwise.
        is_valid: RaggedBatch or tensor bool ``[B, G_max]``, ANDed into ``is_active``.
        min_object_size: ``(h, w)`` minimum clipped size in map pixels for every object; excludes
            ``per_category_min_object_sizes``, ``num_categories`` pairs ``(h, w)`` indexed by the object's category.
        use_per_category_heatmap: a plane per category (``C = num_categories``), else one map without the plane dimension.
        min_fraction_area_clipping, min_radius, max_radius, radius_scaling_factor, radius_to_sigma_factor: finite Python
            numbers, each rounded once to float32; ``0 < max_radius <= 16384``, ``radius_to_sigma_factor > 0``.
        k_for_classes: the peak value per plane, ``C`` finite Python numbers (one without per-category maps); default 1.0.
            The two per-class tables travel to the kernel by value: no allocation, copy or launch of their own.
        out: an existing float32 map ``[B, C, H, W]`` (``[B, H, W]`` without per-category maps) on the boxes' device,
            contiguous, to write into; default: a new one.

    Per object, in float32 with one rounded operation per step (``Wi, Hi`` the frame's image extent, ``Wm, Hm`` the map's):

    1. ``sx = f32(Wm) / f32(Wi)``, ``sy = f32(Hm) / f32(Hi)``; scaled coordinates are ``sx * x`` and ``sy * y`` for the
       four box coordinates and the centre.
    2. An object with a scaled coordinate that is not finite (NaN, inf, an overflow, or any value in a frame with a
       non-positive image extent, where ``sx`` or ``sy`` is inf) is inactive and ALL its outputs are 0.  From here on every
       value is finite, except where noted.
    3. ``clip(v, m) = 0 if v < 0 else (m if v > m else v)``; ``bboxes_heatmap`` is ``(clip(X1, Wm - 1), clip(Y1, Hm - 1),
       clip(X2, Wm - 1), clip(Y2, Hm - 1))``, in input corner order.
    4. ``height_width = (|y2c - y1c|, |x2c - x1c|)`` of the clipped box.
    5. ``fraction = (hc * wc) / (ho * wo)`` with ``ho = |Y2 - Y1|``, ``wo = |X2 - X1|`` of the scaled, unclipped box.  A box
       of zero area gives ``0 / 0`` = NaN, a product that overflows gives ``x / inf`` = 0.
    6. The scaled centre is clipped to the same ranges; ``center = floor(clipped)`` as ``(x, y)`` and
       ``center_offset = clipped - floor(clipped)``.
    7. ``radii``: with ``l, r`` the smaller and larger of ``x1c, x2c`` (``l = x1c if x1c <= x2c else x2c``) and ``t, b`` of
       ``y1c, y2c``, ``d = min(cx - l, cy - t, r - cx, b - cy)`` over the clipped centre, ``d = 0 if d < 0``;
       ``q = d * f32(radius_scaling_factor)``; ``q = lo if q < lo`` with ``lo = max(0.5, f32(min_radius))`` (the reference
       documents 0.5 as the enforced lower bound); ``radius = f32(max_radius) if q > f32(max_radius) else q``.  A centre
       outside its box gives the minimum radius and the object stays active.
    8. ``is_active`` is the AND of: the finite test of step 2; ``fraction >= f32(min_fraction_area_clipping)`` (a NaN
       fraction compares false: a zero-area box is inactive); the size test ``hc >= min_h and wc >= min_w`` with the global
       pair or the pair of the object's category, when one is given; ``0 <= category < num_categories`` whenever categories
       are used (a negative id is inactive here; in the reference it indexes out of bounds); ``is_valid``.  Inactive objects
       with finite coordinates keep their other outputs.
    9. Drawing: ``R = int(ceil(radius))``, ``sigma = radius * f32(radius_to_sigma_factor)``.  Each active object writes
       ``k[plane] * exp(-(dx^2 + dy^2) / (2 sigma^2))`` to the pixels of ``[cx - R, cx + R] x [cy - R, cy + R]`` inside the
       map, on plane ``category`` (plane 0 without per-category maps), combined by ``max`` with 0 and with the other objects.
       That is DrawGaussians.cc:35-74 on a zero map.  The exponential is float32 (``__expf`` on the device, ``std::exp`` on
       the host): map values agree with the exact value to 1e-5 x max(1, max k), not bit for bit.

    Every element of the map and every slot of the per-object outputs is written, padding slots as ``False`` / 0; nothing is
    cleared beforehand and nothing is read from the map.  The per-object outputs are bitwise equal between device and host.
    GPU tensors run one HIP kernel on torch's current stream and current device (a workgroup per frame, plane and 64 x 16
    tile; every workgroup recomputes its frame's records, so there is no pre-pass, no workspace, no atomics and no host
    synchronisation); CPU tensors run the library's host entry over the same per-object functions.  Nothing takes a gradient.
    """
    if not _ops.is_ragged(bboxes):
        raise RuntimeError(f"{_WHO}: bboxes must be a RaggedBatch of float32 [B, G_max, 4]")
    b_t, sizes = bboxes.tensor, bboxes.sample_sizes

    # which arguments need and exclude each other (the reference constructor, :170-212)
    uses_categories = bool(use_per_category_heatmap) or num_categories is not None or per_category_min_object_sizes is not None
    if uses_categories:
        if categories is None:
            raise RuntimeError(f"{_WHO}: categories must be given when use_per_category_heatmap is true, or num_categories or "
                               "per_category_min_object_sizes is given")
        if isinstance(num_categories, bool) or not isinstance(num_categories, int) or num_categories <= 0:
            raise RuntimeError(f"{_WHO}: num_categories must be a positive Python int when categories are used, "
                               f"got {num_categories!r}")
        if num_categories > MAX_CATEGORIES:
            raise RuntimeError(f"{_WHO}: {num_categories} categories, at most MAX_CATEGORIES = {MAX_CATEGORIES} are supported")
    elif categories is not None:
        raise RuntimeError(f"{_WHO}: categories are given but nothing uses them (set num_categories)")
    if min_object_size is not None and per_category_min_object_sizes is not None:
        raise RuntimeError(f"{_WHO}: min_object_size and per_category_min_object_sizes exclude each other")
    if per_category_min_object_sizes is not None:
        if (not isinstance(per_category_min_object_sizes, (list, tuple))
                or len(per_category_min_object_sizes) != num_categories):
            raise RuntimeError(f"{_WHO}: per_category_min_object_sizes must hold num_categories = {num_categories} pairs")
        cat_sizes = [_pair("an entry of per_category_min_object_sizes", v) for v in per_category_min_object_sizes]
    glob_size = _pair("min_object_size", min_object_size) if min_object_size is not None else (0.0, 0.0)
    if (not isinstance(heatmap_hw, (list, tuple)) or len(heatmap_hw) != 2
            or not all(_ops.is_int(v) for v in heatmap_hw)
            or not all(1 <= v <= (1 << 24) for v in heatmap_hw)):
        raise RuntimeError(f"{_WHO}: heatmap_hw must be (H, W) Python ints in [1, 2^24], got {heatmap_hw!r}")
    Hm, Wm = heatmap_hw
    scalars = dict(min_fraction_area_clipping=min_fraction_area_clipping, min_radius=min_radius, max_radius=max_radius,
                   radius_scaling_factor=radius_scaling_factor, radius_to_sigma_factor=radius_to_sigma_factor)
    for name, v in scalars.items():
        if not _ops.is_number(v) or not math.isfinite(v):
            raise RuntimeError(f"{_WHO}: {name} must be a finite Python number, got {v!r}")
    if not 0 < max_radius <= 16384:
        raise RuntimeError(f"{_WHO}: max_radius must be in (0, 16384], got {max_radius!r}")
    if not radius_to_sigma_factor > 0:
        raise RuntimeError(f"{_WHO}: radius_to_sigma_factor must be positive, got {radius_to_sigma_factor!r}")
    planes = num_categories if use_per_category_heatmap else 1
    if k_for_classes is not None:
        if (not isinstance(k_for_classes, (list, tuple)) or len(k_for_classes) != planes
                or not all(_ops.is_number(v) and math.isfinite(v) for v in k_for_classes)):
            raise RuntimeError(f"{_WHO}: k_for_classes must hold {planes} finite Python numbers (one per plane), "
                               f"got {k_for_classes!r}")

    c_t, cat_t, v_t = _ops.tensor_of(centers), _ops.tensor_of(categories), _ops.tensor_of(is_valid)
    hw_t = image_hw if isinstance(image_hw, torch.Tensor) else None
    _ops.check_operands(_WHO, (("bboxes", b_t), ("centers", c_t), ("categories", cat_t), ("is_valid", v_t),
                               ("sample_sizes", sizes), ("image_hw", hw_t), ("out", out)), b_t, "boxes'")
    _ops.check_backend(_WHO, "bboxes", b_t.device)
    _ops.check_float32(_WHO, "bboxes", b_t)
    B, G = _ops.check_bboxes(_WHO, bboxes, b_t, "[B, G_max, 4]")
    if c_t is not None:
        _ops.check_float32(_WHO, "centers", c_t)
        if c_t.dtype != torch.float32 or tuple(c_t.shape) != (B, G, 2):
            raise RuntimeError(f"{_WHO}: centers must be float32 [{B}, {G}, 2], got {c_t.dtype} {tuple(c_t.shape)}")
    if cat_t is not None and (cat_t.dtype not in (torch.int32, torch.int64) or tuple(cat_t.shape) != (B, G)):
        raise RuntimeError(f"{_WHO}: categories must be int32 or int64 [{B}, {G}], got {cat_t.dtype} {tuple(cat_t.shape)}")
    if v_t is not None and (v_t.dtype != torch.bool or tuple(v_t.shape) != (B, G)):
        raise RuntimeError(f"{_WHO}: is_valid must be bool [{B}, {G}], got {v_t.dtype} {tuple(v_t.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, B)
    Hi, Wi = _ops.image_hw_args(_WHO, image_hw, hw_t, B, "B")
    _ops.check_box_count(_WHO, G, MAX_BOXES)
    map_shape = (B, planes, Hm, Wm) if use_per_category_heatmap else (B, Hm, Wm)
    dev = b_t.device
    if out is not None:
        if out.is_floating_point() and out.dtype != torch.float32:
            raise TypeError(f"{_WHO}: out must be float32, got {out.dtype}")
        if out.dtype != torch.float32 or tuple(out.shape) != map_shape:
            raise RuntimeError(f"{_WHO}: out must be float32 {list(map_shape)}, got {out.dtype} {tuple(out.shape)}")
        heatmap = out
    else:
        heatmap = torch.empty(map_shape, dtype=torch.float32, device=dev)

    active = torch.empty((B, G), dtype=torch.bool, device=dev)
    center = torch.empty((B, G, 2), dtype=torch.int32, device=dev)
    offset = torch.empty((B, G, 2), dtype=torch.float32, device=dev)
    hw_out = torch.empty((B, G, 2), dtype=torch.float32, device=dev)
    boxes_out = torch.empty((B, G, 4), dtype=torch.float32, device=dev)
    radii = torch.empty((B, G), dtype=torch.float32, device=dev)
    if B > 0:
        params = _nat.BoxHeatmapParams()
        params.image_h, params.image_w, params.map_h, params.map_w = Hi, Wi, Hm, Wm
        params.min_fraction_area_clipping = float(min_fraction_area_clipping)
        params.min_radius, params.max_radius = float(min_radius), float(max_radius)
        params.radius_scaling_factor = float(radius_scaling_factor)
        params.radius_to_sigma_factor = float(radius_to_sigma_factor)
        params.min_object_size[0], params.min_object_size[1] = glob_size
        params.num_categories = num_categories if uses_categories else 0
        params.per_category_heatmap = 1 if use_per_category_heatmap else 0
        params.has_min_object_size = 0 if min_object_size is None else 1
        params.has_per_category_min_object_sizes = 0 if per_category_min_object_sizes is None else 1
        if per_category_min_object_sizes is not None:
            for c, (h, w) in enumerate(cat_sizes):
                params.per_category_min_object_sizes[c][0], params.per_category_min_object_sizes[c][1] = h, w
        for c in range(planes):
            params.k_for_classes[c] = 1.0 if k_for_classes is None else float(k_for_classes[c])
        flags = ((_nat.BH_COUNTS_I64 if sizes.dtype == torch.int64 else 0)
                 | (_nat.BH_HW_I64 if hw_t is not None and hw_t.dtype == torch.int64 else 0)
                 | (_nat.BH_CATEGORIES_I64 if cat_t is not None and cat_t.dtype == torch.int64 else 0))
        ptr = _ops.ptr
        args = (ptr(b_t), ptr(c_t), ptr(cat_t), ptr(v_t), ptr(sizes), ptr(hw_t), flags, B, G, ctypes.addressof(params),
                ptr(heatmap), ptr(active), ptr(center), ptr(offset), ptr(hw_out), ptr(boxes_out), ptr(radii))
        _ops.run("accv_box_heatmap", args, dev, _WHO)
    ragged = lambda t: RaggedBatch(t, sample_sizes=sizes)
    return BoxHeatmapTargets(heatmap, ragged(active), ragged(center), ragged(offset), ragged(hw_out), ragged(boxes_out),
                             ragged(radii))
