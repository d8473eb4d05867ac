"""ctypes binding of libaccv_hip.so (the gfx950 C-ABI declared in include/accv_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, an exception is
raised — the product path never routes through a CPU or eager-PyTorch substitute.
Build the library with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C accv-lab_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACCV_HIP_LIB points experiments at another build of the library, e.g. one made by scripts/build_prev_lib.sh or
# scripts/build_variant_lib.sh
# ACCV_NO_HOST_FASTPATH=1: the operators keep to their python formulation (the C++ host fast paths of draw_heatmap_batched,
# the ragged gather / scatter and the lane sampler decline everything) — used to run the test-suite over both
NO_HOST_FASTPATH = os.environ.get("ACCV_NO_HOST_FASTPATH", "") not in ("", "0")
LIB_PATH = os.environ.get("ACCV_HIP_LIB") or os.path.join(_HERE, "libaccv_hip.so")

OK = 0
HM_CLEAR = 1
HM_COUNTS_I64 = 2
HM_SMALL_RADII = 4
HM_WRITE_THROUGH = 8
HM_GROUP_BOXES_GIVEN = 16
HM_TILE_ROWS_16 = 32
HM_TILE_ROWS_8 = 64
HM_CALLER_SCALE_ORDER = 256
HM_PLAIN_STORES = 128
HM_POINT_COUNTS_I64 = 512
MP_IDX_I64 = 1
MP_COUNTS_I64 = 2
MP_LABELS_I64 = 4
FL_AVG_NUM_POS = 0
FL_AVG_VALUE = 1
FL_AVG_DEVICE = 2
LSA_MAXIMIZE = 1
LSA_THREADS_64 = 2
LSA_THREADS_1024 = 4
MC_ONE_MINUS_PROB = 0
MC_NEG_PROB = 1
MC_FOCAL = 2
MC_LABELS_I64 = 1
MC_CXCYWH = 2
CR_MAX_MAPS = 8
CR_MAX_CHANNELS = 64
CR_COUNTS_I64 = 1
CR_INDEX_FORM = 2
CR_WEIGHTS_PER_CHANNEL = 4
CR_L1 = 0
CR_SMOOTH_L1 = 2
MF_IDX_I64 = 1
MF_LABELS_I64 = 2
MB_IDX_I64 = 1
MB_CXCYWH = 2
MB_IOU_NONE = 0
MB_IOU = 1
MB_GIOU = 2
MB_MAX_D = 16
PM_IDX_I64 = 1
PM_REVERSIBLE = 2
PM_LABELS_I64 = 4
PM_CLOSED_I32 = 8
PM_CLOSED_I64 = 16
PM_MIN_P = 2
PM_MAX_P = 128
CT_MAX_TASKS = 8
CT_MAX_CLASSES = 64
CT_NO_TASK = 255
CT_LABELS_I64 = 1
CT_COUNTS_I64 = 2
BA_MAX_POINT_TRANSFORMS = 4
BA_MAX_FRAME_TRANSFORMS = 2
BA_COUNTS_I64 = 1
BA_LABELS_I64 = 2
BA_RANGE_ON_OUTPUT = 4
CD_MAX_TASKS = 8
CD_MAX_MAPS = 8
CD_MAX_CLASSES = 64
CD_MAX_K = 1024
RN_MAX_TASKS = 8
RN_MAX_N = 1024
RN_MIN_D = 7
RN_MAX_D = 16
BD_MAX_K = 1024
BD_MAX_MAPS = 8
BD_MAX_EXTRAS = 4
QD_MAX_K = 1024
DT_MAX_CAMERAS = 16
DT_BAND_CELLS = 8192
DT_MAX_BINS = 32768
VX_MIN_D = 3
VX_MAX_D = 16
VX_MAX_POINTS = 128
VX_MAX_VOXELS = 1 << 20
PF_CLUSTER = 1
PF_CENTER = 2
PF_DISTANCE = 4
BS_MAX_C = 1024
VB_MAX_BOXES = 256
VB_COUNTS_I64 = 1
VB_HW_I64 = 2
CB_MAX_BOXES = 256
CB_MAX_MATRICES = 4
CB_COUNTS_I64 = 1
CB_HW_I64 = 2
CB_CATEGORIES_I64 = 4
BH_MAX_BOXES = 256
BH_MAX_CATEGORIES = 128
BH_TILE_W = 64
BH_TILE_H = 16
BH_COUNTS_I64 = 1
BH_HW_I64 = 2
BH_CATEGORIES_I64 = 4
IP_MAX_EXTENT = 16384
IP_TILE_W = 64
IP_TILE_H = 16
IP_LAYOUT_CHW = 0
IP_LAYOUT_HWC = 1

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_u = ctypes.c_uint
_sz = ctypes.c_size_t
_i64 = ctypes.c_int64
_ll = ctypes.c_longlong
_u64 = ctypes.c_uint64

# name -> (restype, argtypes); must list every symbol include/accv_hip.h declares (tests check this)
SIGNATURES = {
    "accv_last_error": (ctypes.c_char_p, []),
    "accv_version": (_i, []),
    "accv_draw_heatmap_last_dispatch": (ctypes.c_char_p, []),
    "accv_draw_heatmap_time_next_launch": (_i, [_vp, _vp]),
    "accv_draw_heatmap_flat_workspace_bytes": (_sz, [_i, _i]),
    "accv_draw_heatmap_flat_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _u, _vp, _sz, _vp]),
    "accv_draw_heatmap_batched_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _u, _vp]),
    "accv_fill_f32": (_i, [_vp, _sz, _f, _vp]),
    "accv_draw_heatmap_multiscale_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _f, _u, _vp]),
    "accv_draw_heatmap_multiscale_sample_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _f, _u,
                                                      _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "accv_draw_points_workspace_bytes": (_sz, [_i, _i]),
    "accv_draw_points_multiscale_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _f, _f, _u, _vp, _sz, _vp]),
    "accv_draw_polylines_fused_applicable": (_i, [_vp, _vp, _i, _i, _i, _i, _i]),
    "accv_draw_polylines_multiscale_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _f, _f, _u, _vp]),
    "accv_heatmap_targets_from_boxes_f32": (_i, [_vp, _vp, _ll, _f, _vp, _vp, _vp]),
    "accv_heatmap_targets_from_points_f32": (_i, [_vp, _ll, _f, _i, _vp, _vp, _vp]),
    # H2 ragged kernels
    "accv_ragged_gather": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp]),
    "accv_ragged_gather_fill": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _u64, _i, _i, _i, _vp, _vp]),
    "accv_ragged_scatter": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp]),
    "accv_ragged_map_pairs": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp]),
    "accv_ragged_insert_const": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _u64, _i, _i, _i, _vp, _vp]),
    "accv_ragged_pad_fill": (_i, [_vp, _vp, _ll, _ll, _ll, _u64, _i, _i, _vp]),
    "accv_ragged_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _i, _vp, _vp]),
    "accv_ragged_mask_to_indices": (_i, [_vp, _vp, _i, _ll, _ll, _vp, _vp, _vp]),
    "accv_ragged_mask_to_indices_workspace_bytes": (_sz, [_ll, _ll]),
    "accv_ragged_mask_to_indices_ws": (_i, [_vp, _vp, _i, _ll, _ll, _vp, _vp, _vp, _sz, _vp]),
    "accv_ragged_pack": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _i, _vp]),
    "accv_matched_pair_reduce_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _f, _i, _i, _vp, _vp]),
    "accv_matched_pair_reduce_bwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _f, _i, _i,
                                              _vp, _vp, _vp, _vp]),
    "accv_matched_pair_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _f, _f, _u, _vp, _vp]),
    "accv_matched_pair_reduce_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _f, _f, _u,
                                          _vp, _vp, _vp, _vp]),
    # Gaussian focal loss on a heat-map target
    "accv_gaussian_focal_loss_workspace_bytes": (_sz, [_ll]),
    "accv_gaussian_focal_loss": (_i, [_vp, _vp, _ll, _i, _f, _f, _f, _f, _f, _i, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "accv_gaussian_focal_loss_bwd": (_i, [_vp, _vp, _ll, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    # heat-map peak extraction (local-maximum suppression + top-k)
    "accv_heatmap_peaks_workspace_bytes": (_sz, [_ll, _ll, _ll, _ll, _i]),
    "accv_heatmap_peaks": (_i, [_vp, _i, _ll, _ll, _ll, _ll, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # batched linear sum assignment (Hungarian matching)
    "accv_linear_assignment_workspace_bytes": (_sz, [_ll, _ll, _ll, _i]),
    "accv_linear_assignment": (_i, [_vp, _i, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _u, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "accv_linear_assignment_host": (_i, [_vp, _i, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _u, _vp, _vp, _vp, _vp]),
    # matching-cost matrices (params: a MatchingCostParams by address)
    "accv_matching_cost": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp,
                                _vp]),
    "accv_matching_cost_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp,
                                     _vp]),
    # matched sigmoid focal loss (params: a MatchedFocalParams by address)
    "accv_matched_focal_loss_workspace_bytes": (_sz, [_ll, _ll, _ll]),
    "accv_matched_focal_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp,
                                     _vp, _sz, _vp]),
    "accv_matched_focal_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll,
                                         _vp, _vp, _vp]),
    "accv_matched_focal_loss_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp,
                                          _vp]),
    "accv_matched_focal_loss_bwd_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll,
                                              _ll, _vp, _vp]),
    # matched box loss (params: a MatchedBoxParams by address; out is [2, B])
    "accv_matched_box_loss_workspace_bytes": (_sz, [_ll, _ll, _ll]),
    "accv_matched_box_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _sz,
                                   _vp]),
    "accv_matched_box_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp,
                                       _vp]),
    "accv_matched_box_loss_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp]),
    "accv_matched_box_loss_bwd_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp,
                                            _vp]),
    # polyline matching cost and matched polyline loss (params: a PolylineMatchParams by address; out of the loss is [2, B])
    "accv_polyline_matching_cost": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp]),
    "accv_polyline_matching_cost_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp]),
    "accv_matched_polyline_loss_workspace_bytes": (_sz, [_ll, _ll]),
    "accv_matched_polyline_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _sz,
                                        _vp]),
    "accv_matched_polyline_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _vp,
                                            _vp, _vp]),
    "accv_matched_polyline_loss_host": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp]),
    "accv_matched_polyline_loss_bwd_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u, _ll, _ll, _ll, _ll, _ll, _ll,
                                                 _vp, _vp]),
    # centre-point regression (maps: host arrays of pointers and channel counts; params: a CenterRegressionParams by address)
    "accv_gather_at_centers": (_i, [_vp, _vp, _i, _i, _ll, _ll, _ll, _vp, _vp, _ll, _u, _vp, _vp]),
    "accv_scatter_at_centers": (_i, [_vp, _vp, _i, _i, _ll, _ll, _ll, _vp, _vp, _ll, _u, _vp, _vp]),
    "accv_center_regression_loss_workspace_bytes": (_sz, [_ll]),
    "accv_center_regression_loss": (_i, [_vp, _vp, _i, _i, _ll, _ll, _ll, _vp, _vp, _ll, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _sz, _vp]),
    "accv_center_regression_loss_bwd": (_i, [_vp, _vp, _vp, _i, _i, _ll, _ll, _ll, _vp, _vp, _ll, _u, _vp, _vp, _vp, _vp, _vp,
                                             _vp]),
    # centre-point targets from ragged 3D boxes (params: a CenterPointTargetsParams by address; outputs [T, B, M, ...])
    "accv_center_point_targets": (_i, [_vp, _vp, _vp, _u, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp]),
    "accv_center_point_targets_host": (_i, [_vp, _vp, _vp, _u, _ll, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp]),
    # BEV box augmentation + range filter (params: a BevAugmentParams by address; outputs [B, N, ...])
    "accv_bev_augment": (_i, [_vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_bev_augment_host": (_i, [_vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    # visible-box selection (params: a VisibleBoxesParams by address; out is bool bytes [B, G])
    "accv_visible_boxes": (_i, [_vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp, _vp]),
    "accv_visible_boxes_host": (_i, [_vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp]),
    # camera-box augmentation (params: a CameraBoxesParams by address; outputs [F, G, ...])
    "accv_camera_boxes": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_camera_boxes_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # box-to-heat-map targets (params: a BoxHeatmapParams by address; the map and six per-object outputs)
    "accv_box_heatmap": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_box_heatmap_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # camera-image preparation (params: a PrepareImagesParams by address; the host entry also takes the coords output)
    "accv_prepare_images": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_prepare_images_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # NV12 surfaces: the conversion (params: an Nv12Params by address) and prepare_images reading the planes (params: a
    # PrepareImagesNv12Params by address)
    "accv_nv12_to_rgb": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "accv_nv12_to_rgb_host": (_i, [_vp, _vp, _vp, _vp]),
    "accv_prepare_images_nv12": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_prepare_images_nv12_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # centre-point decoding with circle NMS (params: a CenterPointDecodeParams by address; outputs [T, B, M, ...])
    "accv_center_point_decode": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_center_point_decode_host": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    # rotated BEV IoU and rotated NMS (params: a RotatedNmsParams by address; NMS outputs [T, B, M, ...])
    "accv_rotated_iou_bev": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp, _vp]),
    "accv_rotated_iou_bev_host": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _vp]),
    "accv_rotated_nms_bev": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_rotated_nms_bev_host": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    # 2D box decoding and axis-aligned NMS (params: a BoxDecodeParams / BoxNmsParams by address; outputs [F, M, ...]); their
    # host entries end in _cpu
    "accv_box_decode": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_box_decode_cpu": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_box_nms": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_box_nms_cpu": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    # top-k box decoding for set-prediction heads (params: a QueryDecode3dParams / QueryDecode2dParams by address; outputs
    # [B, M, ...]); their host entries end in _cpu
    "accv_query_decode_3d": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_query_decode_3d_cpu": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    "accv_query_decode_2d": (_i, [_vp, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp]),
    "accv_query_decode_2d_cpu": (_i, [_vp, _ll, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    # lidar depth targets (params: a DepthTargetsParams by address; outputs [B, C, h, w]); the host entry ends in _cpu
    "accv_depth_targets": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp, _vp]),
    "accv_depth_targets_cpu": (_i, [_vp, _ll, _ll, _ll, _ll, _ll, _vp, _vp]),
    # hard voxelization (params: a VoxelizeParams by address; outputs [B, V, ...] and point_voxel [B, P]); the host entry ends
    # in _cpu and takes no workspace
    "accv_voxelize_workspace_bytes": (_sz, [_ll, _ll, _ll, _ll, _ll]),
    "accv_voxelize": (_i, [_vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "accv_voxelize_cpu": (_i, [_vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp]),
    # pillar decoration (params: a PillarFeaturesParams by address; out [M, T, F]) and the voxel mean (out [M, num_features]);
    # the host entries end in _cpu
    "accv_pillar_features": (_i, [_vp, _ll, _ll, _ll, _vp, _vp]),
    "accv_pillar_features_cpu": (_i, [_vp, _ll, _ll, _ll, _vp]),
    "accv_voxel_mean": (_i, [_vp, _vp, _ll, _ll, _ll, _ll, _vp, _vp]),
    "accv_voxel_mean_cpu": (_i, [_vp, _vp, _ll, _ll, _ll, _ll, _vp]),
    # BEV scatter (canvas [B, C, ny, nx], index [B, ny, nx]) and its backward (grad_features [rows, C]); the host entries
    # end in _cpu
    "accv_bev_scatter": (_i, [_vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp, _vp]),
    "accv_bev_scatter_cpu": (_i, [_vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp]),
    "accv_bev_scatter_bwd": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp, _vp]),
    "accv_bev_scatter_bwd_cpu": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp]),
    # H3 multi-tensor copier
    "accv_mtc_plan": (_i, [_ll, _vp, _vp, _vp, _ll, _ll, _vp, _vp, _vp, _vp]),
    "accv_pinned_acquire": (_vp, [_sz]),
    "accv_pinned_release": (None, [_vp]),
    "accv_pinned_trim": (None, []),
    "accv_pinned_total_bytes": (_sz, []),
    "accv_mtc_worker_count": (_i, []),
    "accv_mtc_pack_host": (_i, [_ll, _vp, _vp, _vp, _vp, _ll]),
    "accv_mtc_stage_h2d": (_i, [_ll, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _i]),
    "accv_mtc_stage_h2d_async": (_i, [_ll, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "accv_mtc_async_wait": (_i, [_ll]),
    "accv_mtc_async_poll": (_i, [_ll]),
    "accv_mtc_shutdown": (None, []),
    "accv_mtc_async_tickets_held": (_ll, []),
    "accv_mtc_coalesce": (_i, [_vp, _ll, _vp, _i, _vp]),
    "accv_memcpy_async": (_i, [_vp, _vp, _sz, _i, _vp]),
    # lane_helpers
    "accv_polyline_scratch_bytes": (_sz, [_ll, _i, _i]),
    "accv_polyline_sample": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "accv_polyline_sample_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i]),
    "accv_polyline_sample_boxes": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "accv_polyline_grad_workspace_bytes": (_sz, [_ll, _i, _i, _i, _i]),
    "accv_polyline_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "accv_polyline_grad_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i]),
}



class MatchingCostParams(ctypes.Structure):
    """accv_matching_cost_params of include/accv_hip.h"""
    _fields_ = [(n, ctypes.c_double) for n in ("class_weight", "l1_weight", "iou_weight", "giou_weight", "focal_alpha",
                                                "focal_gamma", "focal_eps", "iou_eps", "filler")]


class MatchedFocalParams(ctypes.Structure):
    """accv_matched_focal_params of include/accv_hip.h"""
    _fields_ = [("alpha", ctypes.c_double), ("gamma", ctypes.c_double), ("avg_factor", ctypes.c_double),
                ("avg_mode", ctypes.c_int), ("avg_factor_dev", ctypes.c_void_p)]


class MatchedBoxParams(ctypes.Structure):
    """accv_matched_box_params of include/accv_hip.h"""
    _fields_ = [("iou_eps", ctypes.c_double), ("avg_factor", ctypes.c_double), ("code_weights", ctypes.c_double * 16),
                ("avg_mode", ctypes.c_int), ("iou_kind", ctypes.c_int), ("avg_factor_dev", ctypes.c_void_p),
                ("code_weights_dev", ctypes.c_void_p), ("query_weights", ctypes.c_void_p)]


class PolylineMatchParams(ctypes.Structure):
    """accv_polyline_match_params of include/accv_hip.h"""
    _fields_ = ([(n, ctypes.c_double) for n in ("class_weight", "pts_weight", "focal_alpha", "focal_gamma", "focal_eps",
                                                "filler", "dir_eps", "avg_factor")]
                + [("pred_stride_b", ctypes.c_longlong), ("pred_stride_q", ctypes.c_longlong), ("class_kind", ctypes.c_int),
                   ("avg_mode", ctypes.c_int), ("dir_loss", ctypes.c_int), ("avg_factor_dev", ctypes.c_void_p),
                   ("gt_closed", ctypes.c_void_p)])


class CenterRegressionParams(ctypes.Structure):
    """accv_center_regression_params of include/accv_hip.h"""
    _fields_ = [("kind", ctypes.c_int), ("avg_mode", ctypes.c_int), ("beta", ctypes.c_float), ("avg_factor", ctypes.c_float)]


class CenterPointTargetsParams(ctypes.Structure):
    """accv_center_point_targets_params of include/accv_hip.h"""
    _fields_ = [("pc_range", ctypes.c_double * 2), ("voxel_size", ctypes.c_double * 2), ("out_size_factor", ctypes.c_double),
                ("gaussian_overlap", ctypes.c_double), ("min_radius", ctypes.c_int), ("max_objs", ctypes.c_int),
                ("norm_bbox", ctypes.c_int), ("num_tasks", ctypes.c_int), ("class_task", ctypes.c_ubyte * 64),
                ("class_pos", ctypes.c_ubyte * 64)]


class BevAugmentParams(ctypes.Structure):
    """accv_bev_augment_params of include/accv_hip.h"""
    _fields_ = [("range_min", ctypes.c_double * 3), ("range_max", ctypes.c_double * 3), ("point_in", ctypes.c_void_p * 4),
                ("point_out", ctypes.c_void_p * 4), ("point_count", ctypes.c_longlong * 4), ("frame_in", ctypes.c_void_p * 2),
                ("frame_out", ctypes.c_void_p * 2), ("frame_count", ctypes.c_longlong * 2), ("point_rows", ctypes.c_int * 4),
                ("num_point_transforms", ctypes.c_int), ("num_frame_transforms", ctypes.c_int), ("has_range", ctypes.c_int)]


class VisibleBoxesParams(ctypes.Structure):
    """accv_visible_boxes_params of include/accv_hip.h"""
    _fields_ = [("minimum_size", ctypes.c_double), ("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong),
                ("check_occlusion", ctypes.c_int), ("check_size", ctypes.c_int), ("shrink_to_int", ctypes.c_int)]


class CameraBoxesParams(ctypes.Structure):
    """accv_camera_boxes_params of include/accv_hip.h"""
    _fields_ = [("minimum_size", ctypes.c_double), ("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong),
                ("image_hw", ctypes.c_void_p), ("mat_in", ctypes.c_void_p * 4), ("mat_out", ctypes.c_void_p * 4),
                ("mat_count", ctypes.c_longlong * 4), ("mat_rows", ctypes.c_int * 4), ("mat_cols", ctypes.c_int * 4),
                ("num_matrices", ctypes.c_int), ("check_occlusion", ctypes.c_int), ("check_size", ctypes.c_int),
                ("shrink_to_int", ctypes.c_int), ("crop", ctypes.c_int), ("order_corners", ctypes.c_int)]


class BoxHeatmapParams(ctypes.Structure):
    """accv_box_heatmap_params of include/accv_hip.h"""
    _fields_ = [("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong), ("map_h", ctypes.c_longlong),
                ("map_w", ctypes.c_longlong), ("min_fraction_area_clipping", ctypes.c_double), ("min_radius", ctypes.c_double),
                ("max_radius", ctypes.c_double), ("radius_scaling_factor", ctypes.c_double),
                ("radius_to_sigma_factor", ctypes.c_double), ("min_object_size", ctypes.c_double * 2),
                ("num_categories", ctypes.c_int), ("per_category_heatmap", ctypes.c_int), ("has_min_object_size", ctypes.c_int),
                ("has_per_category_min_object_sizes", ctypes.c_int),
                ("per_category_min_object_sizes", (ctypes.c_float * 2) * 128), ("k_for_classes", ctypes.c_float * 128)]


class PrepareImagesParams(ctypes.Structure):
    """accv_prepare_images_params of include/accv_hip.h"""
    _fields_ = [("batch", ctypes.c_longlong), ("source_h", ctypes.c_longlong), ("source_w", ctypes.c_longlong),
                ("output_h", ctypes.c_longlong), ("output_w", ctypes.c_longlong), ("tile_h", ctypes.c_longlong),
                ("tile_w", ctypes.c_longlong), ("mean", ctypes.c_double * 3), ("std", ctypes.c_double * 3),
                ("pad_before_normalize", ctypes.c_int), ("is_bgr", ctypes.c_int), ("layout", ctypes.c_int),
                ("dtype", ctypes.c_int), ("source_hw_i64", ctypes.c_int)]


class Nv12Params(ctypes.Structure):
    """accv_nv12_params of include/accv_hip.h"""
    _fields_ = [("batch", ctypes.c_longlong), ("height", ctypes.c_longlong), ("width", ctypes.c_longlong),
                ("y_stride_batch", ctypes.c_longlong), ("y_stride_row", ctypes.c_longlong),
                ("uv_stride_batch", ctypes.c_longlong), ("uv_stride_row", ctypes.c_longlong),
                ("full_range", ctypes.c_int), ("as_bgr", ctypes.c_int), ("chroma_vu", ctypes.c_int)]


class PrepareImagesNv12Params(ctypes.Structure):
    """accv_prepare_images_nv12_params of include/accv_hip.h"""
    _fields_ = [("prepare", PrepareImagesParams), ("planes", Nv12Params)]


class CenterPointDecodeParams(ctypes.Structure):
    """accv_center_point_decode_params of include/accv_hip.h"""
    _fields_ = [("scores", ctypes.c_void_p * 8), ("indices", ctypes.c_void_p * 8), ("classes", ctypes.c_void_p * 8),
                ("maps", (ctypes.c_void_p * 8) * 8), ("channels", (ctypes.c_int * 8) * 8), ("num_maps", ctypes.c_int * 8),
                ("has_nms", ctypes.c_int * 8), ("nms_threshold", ctypes.c_double * 8), ("pc_range", ctypes.c_double * 2),
                ("voxel_size", ctypes.c_double * 2), ("out_size_factor", ctypes.c_double), ("score_threshold", ctypes.c_double),
                ("post_center_range", ctypes.c_double * 6), ("score_dtype", ctypes.c_int), ("map_dtype", ctypes.c_int),
                ("num_tasks", ctypes.c_int), ("has_score_threshold", ctypes.c_int), ("has_post_center_range", ctypes.c_int),
                ("scores_are_logits", ctypes.c_int), ("norm_bbox", ctypes.c_int), ("bottom_center", ctypes.c_int),
                ("task_first", ctypes.c_ubyte * 9), ("class_ids", ctypes.c_ubyte * 64)]


class RotatedNmsParams(ctypes.Structure):
    """accv_rotated_nms_params of include/accv_hip.h"""
    _fields_ = [("boxes", ctypes.c_void_p * 8), ("scores", ctypes.c_void_p * 8), ("labels", ctypes.c_void_p * 8),
                ("source", ctypes.c_void_p * 8), ("sizes", ctypes.c_void_p * 8), ("iou_threshold", ctypes.c_double * 8),
                ("has_threshold", ctypes.c_int * 8), ("num_tasks", ctypes.c_int)]


class BoxDecodeParams(ctypes.Structure):
    """accv_box_decode_params of include/accv_hip.h"""
    _fields_ = [("scores", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("classes", ctypes.c_void_p),
                ("maps", ctypes.c_void_p * 8), ("channels", ctypes.c_int * 8), ("num_maps", ctypes.c_int),
                ("image_hw_i64", ctypes.c_int), ("image_hw", ctypes.c_void_p), ("image_matrices", ctypes.c_void_p),
                ("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong), ("score_threshold", ctypes.c_double),
                ("min_size", ctypes.c_double * 2), ("iou_threshold", ctypes.c_double), ("score_dtype", ctypes.c_int),
                ("map_dtype", ctypes.c_int), ("has_score_threshold", ctypes.c_int), ("has_min_size", ctypes.c_int),
                ("has_iou_threshold", ctypes.c_int), ("scores_are_logits", ctypes.c_int), ("clip", ctypes.c_int),
                ("order_corners", ctypes.c_int), ("class_agnostic", ctypes.c_int)]


class BoxNmsParams(ctypes.Structure):
    """accv_box_nms_params of include/accv_hip.h"""
    _fields_ = [("boxes", ctypes.c_void_p), ("scores", ctypes.c_void_p), ("labels", ctypes.c_void_p),
                ("source", ctypes.c_void_p), ("extras", ctypes.c_void_p), ("sizes", ctypes.c_void_p),
                ("iou_threshold", ctypes.c_double), ("has_threshold", ctypes.c_int), ("class_agnostic", ctypes.c_int)]


class QueryDecode3dParams(ctypes.Structure):
    """accv_query_decode_3d_params of include/accv_hip.h"""
    _fields_ = [("cls_scores", ctypes.c_void_p), ("bbox_preds", ctypes.c_void_p), ("score_threshold", ctypes.c_double),
                ("post_center_range", ctypes.c_double * 6), ("score_dtype", ctypes.c_int), ("box_dtype", ctypes.c_int),
                ("has_score_threshold", ctypes.c_int), ("has_post_center_range", ctypes.c_int),
                ("scores_are_logits", ctypes.c_int), ("bottom_center", ctypes.c_int)]


class QueryDecode2dParams(ctypes.Structure):
    """accv_query_decode_2d_params of include/accv_hip.h"""
    _fields_ = [("cls_scores", ctypes.c_void_p), ("bbox_preds", ctypes.c_void_p), ("image_hw", ctypes.c_void_p),
                ("image_matrices", ctypes.c_void_p), ("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong),
                ("score_threshold", ctypes.c_double), ("score_dtype", ctypes.c_int), ("box_dtype", ctypes.c_int),
                ("image_hw_i64", ctypes.c_int), ("has_score_threshold", ctypes.c_int), ("scores_are_logits", ctypes.c_int),
                ("cxcywh", ctypes.c_int), ("normalized", ctypes.c_int), ("clip", ctypes.c_int), ("order_corners", ctypes.c_int)]


class DepthTargetsParams(ctypes.Structure):
    """accv_depth_targets_params of include/accv_hip.h"""
    _fields_ = [("points", ctypes.c_void_p), ("sample_sizes", ctypes.c_void_p), ("projection", ctypes.c_void_p),
                ("image_transforms", ctypes.c_void_p), ("image_h", ctypes.c_longlong), ("image_w", ctypes.c_longlong),
                ("depth_min", ctypes.c_double), ("depth_max", ctypes.c_double), ("bin_lo", ctypes.c_double),
                ("bin_step", ctypes.c_double), ("downsample", ctypes.c_int), ("bin_count", ctypes.c_int),
                ("sizes_i64", ctypes.c_int), ("band_rows", ctypes.c_int)]


class VoxelizeParams(ctypes.Structure):
    """accv_voxelize_params of include/accv_hip.h"""
    _fields_ = [("points", ctypes.c_void_p), ("sample_sizes", ctypes.c_void_p), ("augmentation", ctypes.c_void_p),
                ("voxel_size", ctypes.c_double * 3), ("range_min", ctypes.c_double * 3), ("range_max", ctypes.c_double * 3),
                ("table_slots", ctypes.c_longlong), ("max_points", ctypes.c_int), ("max_voxels", ctypes.c_int),
                ("sizes_i64", ctypes.c_int)]


class PillarFeaturesParams(ctypes.Structure):
    """accv_pillar_features_params of include/accv_hip.h"""
    _fields_ = [("voxels", ctypes.c_void_p), ("num_points", ctypes.c_void_p), ("coors", ctypes.c_void_p),
                ("voxel_size", ctypes.c_double * 3), ("range_min", ctypes.c_double * 3), ("coor_width", ctypes.c_int),
                ("flags", ctypes.c_uint)]


_lib = None
_handle = None

try:  # METH_FASTCALL trampoline (csrc_host/fastcall.cpp): same exported functions, ~0.3 us per call instead of ~4 us
    from . import _fastcall
except ImportError:  # pragma: no cover - the ctypes path is complete on its own
    _fastcall = None
if os.environ.get("ACCV_NO_FASTCALL") == "1":
    _fastcall = None

_INT_CLASS = (_vp, _i, _u, _sz, _i64, _ll, _u64)
# entry points that BLOCK (wait for a native job, run a long host memcpy): they stay on ctypes, which drops the
# interpreter lock for the duration of the call — the trampoline keeps it
# every host entry runs its whole operator inside the call
_BLOCKING = {name for name in SIGNATURES if name.endswith("_host")} | {"accv_mtc_async_wait", "accv_mtc_stage_h2d"}
# accv_X -> its host entry where that is not accv_X_host; these run their whole operator inside the call as well, so they
# stay on ctypes too
HOST_ENTRY_NAMES = {"accv_box_decode": "accv_box_decode_cpu", "accv_box_nms": "accv_box_nms_cpu",
                    "accv_query_decode_3d": "accv_query_decode_3d_cpu", "accv_query_decode_2d": "accv_query_decode_2d_cpu",
                    "accv_depth_targets": "accv_depth_targets_cpu", "accv_voxelize": "accv_voxelize_cpu",
                    "accv_pillar_features": "accv_pillar_features_cpu", "accv_voxel_mean": "accv_voxel_mean_cpu",
                    "accv_bev_scatter": "accv_bev_scatter_cpu", "accv_bev_scatter_bwd": "accv_bev_scatter_bwd_cpu"}
_CTYPES_ONLY = _BLOCKING | set(HOST_ENTRY_NAMES.values())


def _fast_entry(fn, res, args):
    """A callable with the C argument order that goes through the trampoline, or None when the signature is not
    eligible (non-int result, string arguments, a float count other than 0 or 2)."""
    if _fastcall is None or res is not _i or len(args) > 22:
        return None
    floats = [k for k, a in enumerate(args) if a is _f]
    if any(a is not _f and a not in _INT_CLASS for a in args):
        return None
    addr = ctypes.cast(fn, ctypes.c_void_p).value
    if not floats and len(args) <= 20:
        import functools
        return functools.partial(_fastcall.call_ints, addr)
    if len(floats) == 2 and floats[1] == floats[0] + 1 and len(args) - 2 <= 20:
        f0, call = floats[0], _fastcall.call_f2
        return lambda *a: call(addr, a[f0], a[f0 + 1], *a[:f0], *a[f0 + 2:])
    return None


class _Lib:
    """Attribute access by exported name; hot entry points resolve to the trampoline, everything else to ctypes."""

    def __init__(self, handle):
        self._ctypes = handle

    def __getattr__(self, name):
        fn = getattr(self._ctypes, name)
        sig = SIGNATURES.get(name)
        fast = _fast_entry(fn, *sig) if sig and name not in _CTYPES_ONLY else None
        fn = fast or fn
        setattr(self, name, fn)       # cached: __getattr__ is not consulted again
        return fn


class AccvNativeError(RuntimeError):
    """Raised when a libaccv_hip.so entry point reports a failure (mirrors the reference's TORCH_CHECK ->
    RuntimeError behaviour)."""


def lib() -> "_Lib":
    global _lib, _handle
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `make -C accv-lab_amd/csrc` or __graft_entry__.build()). There is no CPU fallback."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _handle = handle
        _lib = _Lib(handle)
    return _lib


def ctypes_lib() -> ctypes.CDLL:
    """The plain ctypes handle (symbol-table checks, tests)."""
    lib()
    return _handle


def check(status: int, what: str = "") -> None:
    if status != OK:
        msg = lib().accv_last_error()
        raise AccvNativeError(f"{what}: {msg.decode() if msg else 'error'} (status {status})")


def __getattr__(name):
    # FLOAT_DTYPE_CODES: torch dtype -> dtype code of the loss-side entry points (accv::DType in csrc/accv_numeric.h).  An
    # operator that does not take float64 refuses it itself.  Built on first use, so importing this module needs no torch.
    if name == "FLOAT_DTYPE_CODES":
        import torch

        codes = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}
        globals()[name] = codes
        return codes
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def avg_factor_args(avg_factor, device, who: str, exc, where: str):
    """`avg_factor` of a mean-reduced loss as (mode, value, device tensor or None): None counts on the device, a number is
    passed by value, a 0-d float32 tensor on `device` is read on the device.  A wrong tensor raises `exc`; `where` names
    the device in the message ("the logits' device")."""
    import torch

    if avg_factor is None:
        return FL_AVG_NUM_POS, 0.0, None
    if isinstance(avg_factor, torch.Tensor):
        if not (avg_factor.dim() == 0 and avg_factor.dtype == torch.float32 and avg_factor.device == device):
            raise exc(f"{who}: a tensor avg_factor must be a 0-d float32 tensor on {where}")
        return FL_AVG_DEVICE, 0.0, avg_factor.detach()
    return FL_AVG_VALUE, float(avg_factor), None


def workspace(nbytes: int, device):
    """Uninitialised scratch memory for one native call (torch's allocator aligns it to more than the 16 bytes needed)."""
    import torch

    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def last_dispatch() -> str:
    """Kernel instantiation + launch geometry of the last draw_heatmap call on this thread."""
    s = ctypes_lib().accv_draw_heatmap_last_dispatch()
    return s.decode() if s else ""


def stream_ptr(device) -> int:
    """hipStream_t of torch's CURRENT stream on `device` (the reference launches on
    at::cuda::getCurrentCUDAStream(), draw_heatmap_cuda.cu:65)."""
    import torch

    idx = device.index
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the accessor torch's own generated code uses
    if raw is None:  # pragma: no cover - other torch builds
        return torch.cuda.current_stream(device).cuda_stream
    return raw(torch.cuda.current_device() if idx is None else idx)


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(device):
    """Context manager that makes `device` current for a launch (the reference's at::DeviceGuard,
    draw_heatmap_cuda.cu:64) — free when it already is, which is the case in one-process-per-GPU training."""
    import torch

    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(idx)
