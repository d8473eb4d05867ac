"""(extension) What the 2D annotations of a camera image go through while the image is warped: the annotation side of the
reference's ``AffineTransformer`` (its 2 x 3 matrix applied to the point fields ``centers`` and ``bboxes`` and to the
projection matrices ``lidar2img`` / ``intr_lidar2img``), then ``VisibleBboxSelector`` on the warped boxes, the condition
``is_active = categories >= 0 and is_visible``, the ``ConditionalElementRemover`` over ``bboxes, centers, depths,
categories`` and the two ``CoordinateCropper`` steps — for a ragged batch in one launch and without a host round trip.

The steps are wired in the reference's ``examples/pipeline_setup/stream_petr_pipeline.py`` (``pre_processing_steps``); the
float32 operation sequence is written out in ``csrc/camera_boxes_arith.h``, the visibility decision is that of
:func:`visible_bbox_mask` (``csrc/visible_boxes_arith.h``), and both kernels run one visibility walk
(``csrc/visible_boxes_block.h``).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from ..batching_helpers import RaggedBatch

MAX_BOXES = _nat.CB_MAX_BOXES
MAX_MATRICES = _nat.CB_MAX_MATRICES
_WHO = "camera_augment_boxes"


class CameraBoxes(NamedTuple):
    """The augmented annotations.  ``bboxes``, ``centers``, ``depths``, ``categories`` and ``source`` share one
    ``sample_sizes`` (int64 ``[F]``, the kept count); ``keep`` and ``visible`` have the input's."""
    bboxes: object                  # RaggedBatch float32 [F, G, 4]: the kept boxes, warped, compacted, cropped
    centers: object                 # RaggedBatch float32 [F, G, 2], or None
    depths: object                  # RaggedBatch float32 [F, G], or None
    categories: object              # RaggedBatch [F, G] of the categories' dtype, or None
    source: object                  # RaggedBatch int32 [F, G]: the input slot of each output slot, -1 in padding
    keep: object                    # RaggedBatch bool [F, G] over the INPUT slots
    visible: object                 # RaggedBatch bool [F, G] over the INPUT slots
    projection_matrices: tuple      # new tensors, [[A], [0 0 1]] . M


def _matrices(tensors, F, device):
    if not isinstance(tensors, (list, tuple)):
        raise RuntimeError(f"{_WHO}: projection_matrices must be a sequence of tensors")
    if len(tensors) > MAX_MATRICES:
        raise RuntimeError(f"{_WHO}: at most {MAX_MATRICES} projection_matrices tensors, got {len(tensors)}")
    for i, t in enumerate(tensors):
        what = f"projection_matrices[{i}]"
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{_WHO}: {what} must be a tensor")
        if t.device != device:
            raise RuntimeError(f"{_WHO}: {what} must be on the boxes' device {device}, got {t.device}")
        if (t.dtype != torch.float32 or t.dim() not in (3, 4) or t.shape[0] != F or t.shape[-2] not in (3, 4)
                or t.shape[-1] not in (3, 4)):
            raise RuntimeError(f"{_WHO}: {what} must be float32 [{F}, R, C] or [{F}, K, R, C] with R, C in (3, 4), got "
                               f"{t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{_WHO}: {what} must be contiguous (it is not copied silently)")
    return tuple(tensors)


def camera_augment_boxes(bboxes, transforms: torch.Tensor, *, image_hw, centers=None, depths=None, categories=None, valid=None,
                         check_occlusion: bool = True, minimum_size=None, shrink_to_int: bool = False, crop: bool = True,
                         order_corners: bool = False, projection_matrices: Sequence[torch.Tensor] = ()) -> CameraBoxes:
    """Warp, visibility test, compaction and crop of the 2D annotations of a ragged batch of camera images, in one launch.
    A frame is one camera image.

    Args:
        bboxes: RaggedBatch float32 ``[F, G, 4]``, contiguous, one batch dimension, ``non_uniform_dim`` 1; rows
            ``(x1, y1, x2, y2)`` with the corners in either order.  ``G`` is limited to ``MAX_BOXES`` = 256 per frame, as
            for :func:`visible_bbox_mask`; more raise ``RuntimeError`` before any launch.  ``bboxes.sample_sizes`` (int32 or
            int64) is read on the device and clamped to ``[0, G]``; slots from it on are never read.  Other float dtypes
            raise ``TypeError``.
        transforms: float32 ``[F, 2, 3]`` on the boxes' device, the forward matrix ``[[a, b, tx], [c, d, ty]]`` from source
            to output pixels: the tensor ``prepare_images(transforms=...)`` takes, see
            ``accvlab.image_prep.sample_image_transforms``.  Non-finite entries are computed as written.
        image_hw: ``(H, W)`` Python ints for every frame, or an int32 / int64 tensor ``[F, 2]`` on the boxes' device (read
            there): the extent of the output image AFTER tile padding (``padded_hw``), which is what the reference's
            selector and croppers use.  Values are clamped to ``[0, 2^24]``.
        centers: optional float32 ``[F, G, 2]``, warped, compacted and cropped with the boxes.
        depths: optional float32 ``[F, G]``, smaller is nearer; required with ``check_occlusion``; compacted.
        categories: optional int32 or int64 ``[F, G]``; a negative category is not kept; compacted.
        valid: optional bool or uint8 ``[F, G]``: the rest of the keep condition.
            ``centers``, ``depths``, ``categories`` and ``valid`` may each be a tensor or a RaggedBatch.
        check_occlusion, minimum_size, shrink_to_int: as for :func:`visible_bbox_mask`; unlike there, neither check may be
            requested, and then every real slot is visible.
        crop: clamp the kept coordinates to the image (the reference's two ``CoordinateCropper`` steps).
        order_corners: rewrite each warped box as ``(min_x, min_y, max_x, max_y)``.  The reference does not: a flip leaves
            ``x1 > x2``.
        projection_matrices: up to 4 float32 tensors ``[F, R, C]`` or ``[F, K, R, C]`` with ``R``, ``C`` in {3, 4}
            (``lidar2img`` as 3 x 4 or 4 x 4, intrinsics as 3 x 3), ``K >= 0``.

    Per frame with its matrix, in float32, every operation rounded once and in the written order, nothing contracted:

    1. warp: each corner and the centre become ``((a*x + b*y) + tx, (c*x + d*y) + ty)``.  With ``order_corners`` the box
       is then ordered by the ``<`` selection of step 1 of :func:`visible_bbox_mask` (a pair with a NaN stays as it is);
    2. projection matrices: row 0 becomes ``(a*m0j + b*m1j) + tx*m2j``, row 1 ``(c*m0j + d*m1j) + ty*m2j``; row 2, and
       row 3 if present, are copied bit for bit (the reference multiplies by ``[[A], [0 0 1]]`` from the left);
    3. ``visible``: exactly the decision of :func:`visible_bbox_mask` on the warped boxes, before any crop, with every
       corner case defined there (NaN, inf, ties, flipped corners, empty rectangles).  A box that is dropped for its
       category or its ``valid`` flag still occludes: the reference evaluates visibility before the condition;
    4. ``keep = visible and categories >= 0 and valid`` (each where given);
    5. kept slots are compacted in ascending slot order;
    6. with ``crop`` every kept coordinate becomes ``0 if v < 0 else E if v > E else v``, ``E = W`` for x and ``H`` for y:
       NaN stays NaN (the reference's ``crop_coordinates``).

    Returns: :class:`CameraBoxes`.  The compacted outputs share one new int64 ``sample_sizes`` written on the device; their
    padding is written too (0, ``source`` -1); ``keep`` and ``visible`` are False from the input count on; every output
    element is written exactly once.  ``source`` serves ``batched_indexing_access`` for any further per-object field.  The
    result plugs into ``boxes_to_heatmap(out.bboxes, centers=out.centers, categories=out.categories, ...)`` as is.

    GPU tensors run one HIP kernel on torch's current stream (a workgroup per frame, no atomics, no workspace, no host
    synchronisation, bitwise reproducible); CPU tensors run the library's serial host entry over the same arithmetic, with
    bit-equal results.  Nothing takes a gradient and no input is modified.  ``F == 0`` or ``G == 0`` gives empty
    compacted outputs without a launch (with ``G == 0`` the projection matrices, if any, still take one).
    """
    if not _ops.is_ragged(bboxes):
        raise RuntimeError(f"{_WHO}: bboxes must be a RaggedBatch of float32 [F, G, 4]")
    b_t, sizes = bboxes.tensor, bboxes.sample_sizes
    if check_occlusion and depths is None:
        raise RuntimeError(f"{_WHO}: check_occlusion needs depths")
    c_t, d_t = _ops.tensor_of(centers), _ops.tensor_of(depths)
    k_t, v_t = _ops.tensor_of(categories), _ops.tensor_of(valid)
    hw_t = image_hw if isinstance(image_hw, torch.Tensor) else None
    if not isinstance(b_t, torch.Tensor):
        raise RuntimeError(f"{_WHO}: bboxes must be a RaggedBatch of float32 [F, G, 4]")
    _ops.check_operands(_WHO, (("bboxes", b_t), ("transforms", transforms), ("centers", c_t), ("depths", d_t), ("categories", k_t),
                               ("valid", v_t), ("sample_sizes", sizes), ("image_hw", hw_t)), b_t, "boxes'",
                        required=("bboxes", "transforms", "sample_sizes"))
    dev = b_t.device
    _ops.check_backend(_WHO, "bboxes", dev)
    for name, t in (("bboxes", b_t), ("transforms", transforms), ("centers", c_t), ("depths", d_t)):
        if t is not None and t.is_floating_point() and t.dtype != torch.float32:
            raise TypeError(f"{_WHO}: {name} must be float32 (the definition is float32), got {t.dtype}")
    F, G = _ops.check_bboxes(_WHO, bboxes, b_t, "[F, G, 4]")
    if transforms.dtype != torch.float32 or tuple(transforms.shape) != (F, 2, 3):
        raise RuntimeError(f"{_WHO}: transforms must be float32 [{F}, 2, 3], got {transforms.dtype} {tuple(transforms.shape)}")
    if c_t is not None and (c_t.dtype != torch.float32 or tuple(c_t.shape) != (F, G, 2)):
        raise RuntimeError(f"{_WHO}: centers must be float32 [{F}, {G}, 2], got {c_t.dtype} {tuple(c_t.shape)}")
    if d_t is not None and (d_t.dtype != torch.float32 or tuple(d_t.shape) != (F, G)):
        raise RuntimeError(f"{_WHO}: depths must be float32 [{F}, {G}], got {d_t.dtype} {tuple(d_t.shape)}")
    if k_t is not None and (k_t.dtype not in (torch.int32, torch.int64) or tuple(k_t.shape) != (F, G)):
        raise RuntimeError(f"{_WHO}: categories must be int32 or int64 [{F}, {G}], got {k_t.dtype} {tuple(k_t.shape)}")
    if v_t is not None and (v_t.dtype not in (torch.bool, torch.uint8) or tuple(v_t.shape) != (F, G)):
        raise RuntimeError(f"{_WHO}: valid must be bool or uint8 [{F}, {G}], got {v_t.dtype} {tuple(v_t.shape)}")
    _ops.check_sample_sizes(_WHO, sizes, F)
    H, W = _ops.image_hw_args(_WHO, image_hw, hw_t, F, "F")
    if minimum_size is not None and not _ops.is_number(minimum_size):
        raise RuntimeError(f"{_WHO}: minimum_size must be a Python number or None, got {minimum_size!r}")
    _ops.check_box_count(_WHO, G, MAX_BOXES)
    m_in = _matrices(projection_matrices, F, dev)

    out_boxes = torch.empty_like(b_t)
    out_centers = torch.empty_like(c_t) if c_t is not None else None
    out_depths = torch.empty_like(d_t) if d_t is not None else None
    out_cats = torch.empty_like(k_t) if k_t is not None else None
    source = torch.empty((F, G), dtype=torch.int32, device=dev)
    keep = torch.empty((F, G), dtype=torch.bool, device=dev)
    visible = torch.empty((F, G), dtype=torch.bool, device=dev)
    kept = (torch.empty if G > 0 else torch.zeros)((F,), dtype=torch.int64, device=dev)
    m_out = tuple(torch.empty_like(t) for t in m_in)
    if F > 0 and (G > 0 or any(t.numel() for t in m_in)):
        prm = _nat.CameraBoxesParams()
        prm.minimum_size = float(minimum_size) if minimum_size is not None else 0.0
        prm.image_h, prm.image_w = H, W
        ptr = _ops.ptr
        prm.image_hw = ptr(hw_t)
        for i, (src, dst) in enumerate(zip(m_in, m_out)):
            prm.mat_in[i], prm.mat_out[i] = src.data_ptr(), dst.data_ptr()
            prm.mat_count[i] = src.shape[1] if src.dim() == 4 else 1
            prm.mat_rows[i], prm.mat_cols[i] = src.shape[-2], src.shape[-1]
        prm.num_matrices = len(m_in)
        prm.check_occlusion, prm.check_size = 1 if check_occlusion else 0, 0 if minimum_size is None else 1
        prm.shrink_to_int, prm.crop, prm.order_corners = 1 if shrink_to_int else 0, 1 if crop else 0, 1 if order_corners else 0
        flags = ((_nat.CB_COUNTS_I64 if sizes.dtype == torch.int64 else 0)
                 | (_nat.CB_HW_I64 if hw_t is not None and hw_t.dtype == torch.int64 else 0)
                 | (_nat.CB_CATEGORIES_I64 if k_t is not None and k_t.dtype == torch.int64 else 0))
        args = (b_t.data_ptr(), transforms.data_ptr(), ptr(c_t), ptr(d_t), ptr(k_t), ptr(v_t), sizes.data_ptr(), flags, F, G,
                ctypes.addressof(prm), out_boxes.data_ptr(), ptr(out_centers), ptr(out_depths), ptr(out_cats), source.data_ptr(),
                keep.data_ptr(), visible.data_ptr(), kept.data_ptr())
        _ops.run("accv_camera_boxes", args, dev, _WHO)
    rag = lambda t: RaggedBatch(t, sample_sizes=kept) if t is not None else None   # noqa: E731
    return CameraBoxes(rag(out_boxes), rag(out_centers), rag(out_depths), rag(out_cats), rag(source),
                       RaggedBatch(keep, sample_sizes=sizes), RaggedBatch(visible, sample_sizes=sizes), m_out)
