"""accvlab.draw_heatmap — MI355X-native drop-in for the reference package of the same name.

Public API (same names, argument meaning and error behaviour as
packages/draw_heatmap/accvlab/draw_heatmap/__init__.py:22-24 of the reference):
``draw_heatmap`` (flat / "concatenated" input) and ``draw_heatmap_batched`` (RaggedBatch input, optional
class-wise planes).  Both accept one extra keyword, ``clear=False``: with ``clear=True`` the map is
overwritten with max(0, splats) in a single write-only pass (fused zero-fill + draw).
Extensions next to them: ``get_centers_and_radii`` (bbox -> centre/radius front end) and ``draw_polylines_batched`` /
``sample_lane_targets`` (lane raster = polyline sampler + splat), ``draw_heatmap_multiscale`` (all strides of a batch in one
launch), ``draw_targets_multiscale`` (box maps + lane maps of a step in two launches), the maps' consumer
``gaussian_focal_loss`` (the fused GaussianFocalLoss centerness term, forward and backward), and their read-back
``heatmap_peaks`` (local-maximum suppression + top-k in two launches, with a defined tie order), and the regression branch
of the same heads: ``gather_at_centers`` (the maps' values at the object centres or at the peaks' indices) and
``center_regression_loss`` (their L1 / smooth-L1 loss; the backward of both writes the gradient maps in one pass), and the
front of that path: ``center_point_targets`` (raw ragged 3D boxes -> centres, radii, in-task labels, regression targets and
indices of every task of a CenterPoint head in one launch), and its inverse at the end of the path:
``center_point_decode`` (the peaks and regression maps of every task -> filtered, circle-NMS'd, compacted boxes, scores
and labels in one launch), and the other NMS of those heads after it: ``rotated_nms_bev`` (rotated BEV-IoU NMS of every
task's detections in one launch) over ``rotated_iou_bev`` (the pairwise rotated IoU of two ragged BEV box sets).  Ahead of
the 2D target chain: ``visible_bbox_mask`` / ``select_visible_bboxes`` (which boxes of a camera image are drawn at all: the
occlusion and minimum-size test of the reference's VisibleBboxSelector in one launch, without a canvas), and the step after
it: ``boxes_to_heatmap`` (the reference's BoundingBoxToHeatmapConverter: image-space boxes -> scaled and clipped boxes, the
active decision, integer centres, offsets, sizes, float radii and the per-category Gaussian maps, ``BoxHeatmapTargets``, in
one launch), and the step in front of both: ``camera_augment_boxes`` (the annotation side of the reference's AffineTransformer,
its VisibleBboxSelector, the ``categories >= 0 and is_visible`` condition, the ConditionalElementRemover and the two
CoordinateCroppers: raw ragged 2D boxes, centres, depths and categories and the image matrix of their frame -> warped,
visibility-filtered, compacted and cropped annotations and updated projection matrices, ``CameraBoxes``, in one launch).
Ahead of the 3D target chain: ``bev_augment_boxes`` (the reference's BEVBBoxesTransformer3D, PointsInRangeCheck
and ConditionalElementRemover: raw ragged 3D boxes and the matrices of their frame -> rotated, scaled and translated boxes,
range-filtered and compacted, ``BevAugmented``, in one launch; ``bev_augmentation_params`` / ``sample_bev_augmentation``
build its parameter rows).  At the end of the 2D path, the inverse of ``boxes_to_heatmap``: ``box_heatmap_decode`` (the peaks of
the heat map and the offset / size maps of a CenterNet-style camera head -> filtered, IoU-NMS'd, compacted xyxy boxes,
``BoxDetections``, back in source-image pixels through the matrix of ``prepare_images``, in one launch) and the NMS under it
as an operator of its own: ``nms_boxes`` (axis-aligned greedy IoU NMS of ragged boxes per frame, class-aware or agnostic).
For set-prediction heads (DETR, PETR / StreamPETR, BEVFormer), whose loss side lives in ``accvlab.batching_helpers``:
``query_box_decode_3d`` / ``query_box_decode_2d`` (raw class logits and box rows -> the top ``max_num`` (query, class) pairs
of every frame in a defined order, decoded, filtered and compacted in one launch, as the ``CenterPointDetections`` /
``BoxDetections`` that ``rotated_nms_bev`` / ``nms_boxes`` take).

For the depth supervision of LSS heads (BEVDepth, BEVDet4D-Depth, BEVStereo): ``lidar_depth_targets`` (the lidar points of
a frame -> the nearest depth and its bin per cell of every camera's downsampled feature map, through the image matrix
``prepare_images`` warped the image with, in one launch).
"""
from .bev_augment import BevAugmented, bev_augment_boxes, bev_augmentation_params, sample_bev_augmentation
from .box_decode import BoxDetections, box_heatmap_decode, nms_boxes
from .box_heatmap import BoxHeatmapTargets, boxes_to_heatmap
from .camera_boxes import CameraBoxes, camera_augment_boxes
from .center_decode import CenterPointDetections, center_point_decode
from .center_regression import center_regression_loss, gather_at_centers
from .center_targets import CenterPointTargets, center_point_targets
from .depth_targets import DepthTargets, lidar_depth_targets
from .focal_loss import gaussian_focal_loss
from .lanes import (draw_polylines_batched, draw_polylines_multiscale, draw_targets_multiscale, sample_lane_targets,
                    sample_lanes)
from .ops import draw_heatmap, draw_heatmap_batched, draw_heatmap_multiscale, get_centers_and_radii
from .peaks import HeatmapPeaks, heatmap_peaks
from .query_decode import query_box_decode_2d, query_box_decode_3d
from .rotated_nms import rotated_iou_bev, rotated_nms_bev
from .visible_boxes import select_visible_bboxes, visible_bbox_mask

__version__ = "0.1.0"
__all__ = ["__version__", "draw_heatmap", "draw_heatmap_batched", "get_centers_and_radii", "draw_polylines_batched",
           "draw_heatmap_multiscale", "draw_polylines_multiscale", "draw_targets_multiscale", "sample_lane_targets", "sample_lanes",
           "gaussian_focal_loss", "heatmap_peaks", "HeatmapPeaks", "gather_at_centers", "center_regression_loss",
           "center_point_targets", "CenterPointTargets", "center_point_decode", "CenterPointDetections", "rotated_iou_bev",
           "rotated_nms_bev", "visible_bbox_mask", "select_visible_bboxes", "boxes_to_heatmap", "BoxHeatmapTargets",
           "bev_augment_boxes", "BevAugmented", "bev_augmentation_params", "sample_bev_augmentation",
           "camera_augment_boxes", "CameraBoxes", "box_heatmap_decode", "nms_boxes", "BoxDetections",
           "query_box_decode_3d", "query_box_decode_2d", "lidar_depth_targets", "DepthTargets"]
