"""One table of malformed inputs through every detection operator that takes the operand, on CPU tensors at the smallest
legal shapes (one frame, K or N = 2, maps [1, c, 2, 2]): the full message text, the exception type and, where an input breaks
two rules at once, which one is reported.  The strings are written out: a shared check that rewords one fails here."""
import math
from types import SimpleNamespace as NS

import pytest
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import (BoxDetections, CenterPointDetections, box_heatmap_decode, center_point_decode,
                                  center_regression_loss, gather_at_centers, nms_boxes, query_box_decode_2d,
                                  query_box_decode_3d, rotated_iou_bev, rotated_nms_bev)

CPD, BHD, RNB, NB = "center_point_decode", "box_heatmap_decode", "rotated_nms_bev", "nms_boxes"
Q3, Q2, IOU = "query_box_decode_3d", "query_box_decode_2d", "rotated_iou_bev"
NAN = float("nan")
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def strided(shape, dtype=F32):
    """a non-contiguous tensor of `shape`: every second element of the last axis of a tensor twice as wide"""
    t = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype)[..., ::2]
    assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------------ well-formed calls
def peaks(K=2, **over):
    p = dict(scores=torch.zeros((1, K)), indices=torch.zeros((1, K), dtype=I64), classes=torch.zeros((1, K), dtype=I64))
    p.update(over)
    return NS(**p)


def cpd(p=None, feats=None, tasks=((0,),), **kw):
    p = peaks() if p is None else p
    feats = torch.zeros((1, 8, 2, 2)) if feats is None else feats
    if len(tasks) > 1:
        return center_point_decode(p, feats, [list(t) for t in tasks], pc_range=(0.0, 0.0), voxel_size=(1.0, 1.0),
                                   out_size_factor=1, **kw)
    return center_point_decode([p], [feats], [list(t) for t in tasks], pc_range=(0.0, 0.0), voxel_size=(1.0, 1.0),
                               out_size_factor=1, **kw)


def bhd(p=None, feats=None, **kw):
    return box_heatmap_decode(peaks() if p is None else p, torch.zeros((1, 4, 2, 2)) if feats is None else feats,
                              image_hw=(2, 2), **kw)


def det3(N=2, D=7, sizes=None, B=1, **over):
    """the four members of a CenterPointDetections; `over` replaces a member's tensor (or, as name_sizes, its sample sizes)"""
    sizes = torch.full((B,), N, dtype=I64) if sizes is None else sizes
    t = dict(boxes=torch.zeros((B, N, D)), scores=torch.zeros((B, N)), labels=torch.zeros((B, N), dtype=I64),
             source=torch.zeros((B, N), dtype=I32))
    return CenterPointDetections(*(NS(tensor=over.get(n, x), sample_sizes=over.get(n + "_sizes", sizes)) for n, x in t.items()))


def det2(N=2, E=0, sizes=None, B=1, **over):
    sizes = torch.full((B,), N, dtype=I64) if sizes is None else sizes
    t = dict(boxes=torch.zeros((B, N, 4)), scores=torch.zeros((B, N)), labels=torch.zeros((B, N), dtype=I64),
             source=torch.zeros((B, N), dtype=I32), extras=torch.zeros((B, N, E)))
    return BoxDetections(*(NS(tensor=over.get(n, x), sample_sizes=over.get(n + "_sizes", sizes)) for n, x in t.items()))


def rnb(det=None, thr=0.5, **kw):
    return rotated_nms_bev(det3() if det is None else det, thr, **kw)


def nb(det=None, thr=0.5, **kw):
    return nms_boxes(det2() if det is None else det, thr, **kw)


def iou(a=None, b=None):
    box = lambda t: NS(tensor=t, sample_sizes=torch.ones((1,), dtype=I64))   # noqa: E731
    return rotated_iou_bev(box(torch.zeros((1, 2, 5)) if a is None else a), box(torch.zeros((1, 2, 5)) if b is None else b))


def q3(cls=None, rows=None, max_num=1, **kw):
    return query_box_decode_3d(torch.zeros((1, 2, 1)) if cls is None else cls, torch.zeros((1, 2, 8)) if rows is None else rows,
                               max_num, **kw)


def q2(cls=None, rows=None, max_num=1, **kw):
    return query_box_decode_2d(torch.zeros((1, 2, 1)) if cls is None else cls, torch.zeros((1, 2, 4)) if rows is None else rows,
                               max_num, image_hw=(2, 2), **kw)


def maps9(c=1):
    return [torch.zeros((1, c, 2, 2))] * 9


ROWS = [
    # --------------------------------------------------------------------------------------------- peaks: not a tensor
    ("cpd-peaks-no-fields", lambda: cpd(NS(scores=torch.zeros((1, 2)))), f"{CPD}: peaks[0] must be a HeatmapPeaks (scores, indices, classes)"),
    ("bhd-peaks-no-fields", lambda: bhd(NS(scores=torch.zeros((1, 2)))), f"{BHD}: peaks must be a HeatmapPeaks (scores, indices, classes)"),
    ("cpd-scores-not-tensor", lambda: cpd(peaks(scores=[[0.0, 0.0]])), f"{CPD}: peaks[0].scores must be a tensor"),
    ("bhd-scores-not-tensor", lambda: bhd(peaks(scores=[[0.0, 0.0]])), f"{BHD}: peaks.scores must be a tensor"),
    ("cpd-classes-not-tensor", lambda: cpd(peaks(classes=None)), f"{CPD}: peaks[0].classes must be a tensor"),
    ("bhd-classes-not-tensor", lambda: bhd(peaks(classes=None)), f"{BHD}: peaks.classes must be a tensor"),
    # wrong rank
    ("cpd-scores-rank", lambda: cpd(peaks(scores=torch.zeros((1, 2, 1)))),
     f"{CPD}: peaks[0].scores must be [B, K] (heatmap_peaks with per_class=False), got (1, 2, 1)"),
    ("bhd-scores-rank", lambda: bhd(peaks(scores=torch.zeros((1, 2, 1)))),
     f"{BHD}: peaks.scores must be [F, K] (heatmap_peaks with per_class=False), got (1, 2, 1)"),
    ("cpd-indices-rank", lambda: cpd(peaks(indices=torch.zeros((2,), dtype=I64))),
     f"{CPD}: peaks[0].indices must be [B, K] (heatmap_peaks with per_class=False), got (2,)"),
    ("bhd-indices-rank", lambda: bhd(peaks(indices=torch.zeros((2,), dtype=I64))),
     f"{BHD}: peaks.indices must be [F, K] (heatmap_peaks with per_class=False), got (2,)"),
    # non-contiguous
    ("cpd-scores-strided", lambda: cpd(peaks(scores=strided((1, 2)))), f"{CPD}: peaks[0].scores must be contiguous (it is not copied silently)"),
    ("bhd-scores-strided", lambda: bhd(peaks(scores=strided((1, 2)))), f"{BHD}: peaks.scores must be contiguous (it is not copied silently)"),
    ("cpd-classes-strided", lambda: cpd(peaks(classes=strided((1, 2), I64))), f"{CPD}: peaks[0].classes must be contiguous (it is not copied silently)"),
    ("bhd-classes-strided", lambda: bhd(peaks(classes=strided((1, 2), I64))), f"{BHD}: peaks.classes must be contiguous (it is not copied silently)"),
    # a device that is neither
    ("cpd-scores-meta", lambda: cpd(peaks(scores=torch.zeros((1, 2), device="meta"))), f"{CPD}: peaks must be CUDA or CPU tensors, got meta"),
    ("bhd-scores-meta", lambda: bhd(peaks(scores=torch.zeros((1, 2), device="meta"))), f"{BHD}: peaks must be CUDA or CPU tensors, got meta"),
    # float64
    ("cpd-scores-f64", lambda: cpd(peaks(scores=torch.zeros((1, 2), dtype=F64))),
     f"{CPD}: peaks[0].scores must be float32, float16 or bfloat16, got torch.float64"),
    ("bhd-scores-f64", lambda: bhd(peaks(scores=torch.zeros((1, 2), dtype=F64))),
     f"{BHD}: peaks.scores must be float32, float16 or bfloat16, got torch.float64"),
    ("cpd-scores-int", lambda: cpd(peaks(scores=torch.zeros((1, 2), dtype=I64))),
     f"{CPD}: peaks[0].scores must be float32, float16 or bfloat16, got torch.int64"),
    # K = 0 and K = 1025
    ("cpd-K0", lambda: cpd(peaks(0)), f"{CPD}: K must be in 1..1024, got 0"),
    ("bhd-K0", lambda: bhd(peaks(0)), f"{BHD}: K must be in 1..1024, got 0"),
    ("cpd-K1025", lambda: cpd(peaks(1025)), f"{CPD}: K must be in 1..1024, got 1025"),
    ("bhd-K1025", lambda: bhd(peaks(1025)), f"{BHD}: K must be in 1..1024, got 1025"),
    # int32 indices, a shape of their own
    ("cpd-indices-i32", lambda: cpd(peaks(indices=torch.zeros((1, 2), dtype=I32))),
     f"{CPD}: peaks[0].indices must be int64 (1, 2) on cpu, got torch.int32 (1, 2) on cpu"),
    ("bhd-indices-i32", lambda: bhd(peaks(indices=torch.zeros((1, 2), dtype=I32))),
     f"{BHD}: peaks.indices must be int64 (1, 2) on cpu, got torch.int32 (1, 2) on cpu"),
    ("cpd-classes-shape", lambda: cpd(peaks(classes=torch.zeros((1, 3), dtype=I64))),
     f"{CPD}: peaks[0].classes must be int64 (1, 2) on cpu, got torch.int64 (1, 3) on cpu"),
    ("bhd-classes-shape", lambda: bhd(peaks(classes=torch.zeros((1, 3), dtype=I64))),
     f"{BHD}: peaks.classes must be int64 (1, 2) on cpu, got torch.int64 (1, 3) on cpu"),
    # the cross-task reference, which only the centre-point decoder has
    ("cpd-task1-K", lambda: cpd([peaks(2), peaks(1)], [torch.zeros((1, 8, 2, 2))] * 2, tasks=((0,), (1,))),
     f"{CPD}: peaks[1].scores is torch.float32 (1, 1) on cpu, peaks[0].scores torch.float32 (1, 2) on cpu: all tasks share B, K, dtype "
     "and device"),
    ("cpd-task1-dtype", lambda: cpd([peaks(2), peaks(scores=torch.zeros((1, 2), dtype=torch.float16))], [torch.zeros((1, 8, 2, 2))] * 2,
                                    tasks=((0,), (1,))),
     f"{CPD}: peaks[1].scores is torch.float16 (1, 2) on cpu, peaks[0].scores torch.float32 (1, 2) on cpu: all tasks share B, K, dtype "
     "and device"),
    ("cpd-task1-indices", lambda: cpd([peaks(2), peaks(indices=torch.zeros((1, 2), dtype=I32))], [torch.zeros((1, 8, 2, 2))] * 2,
                                      tasks=((0,), (1,))),
     f"{CPD}: peaks[1].indices must be int64 (1, 2) on cpu, got torch.int32 (1, 2) on cpu"),
    # order: rank before contiguity, dtype before K, K before the indices, the peaks before the maps
    ("cpd-order-rank-strided", lambda: cpd(peaks(scores=strided((1, 2, 2)))),
     f"{CPD}: peaks[0].scores must be [B, K] (heatmap_peaks with per_class=False), got (1, 2, 2)"),
    ("bhd-order-rank-strided", lambda: bhd(peaks(scores=strided((1, 2, 2)))),
     f"{BHD}: peaks.scores must be [F, K] (heatmap_peaks with per_class=False), got (1, 2, 2)"),
    ("cpd-order-f64-K0", lambda: cpd(peaks(0, scores=torch.zeros((1, 0), dtype=F64))),
     f"{CPD}: peaks[0].scores must be float32, float16 or bfloat16, got torch.float64"),
    ("bhd-order-f64-K0", lambda: bhd(peaks(0, scores=torch.zeros((1, 0), dtype=F64))),
     f"{BHD}: peaks.scores must be float32, float16 or bfloat16, got torch.float64"),
    ("cpd-order-K-indices", lambda: cpd(peaks(1025, indices=torch.zeros((1, 2), dtype=I32))), f"{CPD}: K must be in 1..1024, got 1025"),
    ("bhd-order-K-indices", lambda: bhd(peaks(1025, indices=torch.zeros((1, 2), dtype=I32))), f"{BHD}: K must be in 1..1024, got 1025"),
    ("cpd-order-peaks-feats", lambda: cpd(peaks(0), maps9()), f"{CPD}: K must be in 1..1024, got 0"),
    ("bhd-order-peaks-feats", lambda: bhd(peaks(0), maps9()), f"{BHD}: K must be in 1..1024, got 0"),
    # ---------------------------------------------------------------------------------------------- feats: not a tensor
    ("cpd-feats-none", lambda: center_point_decode([peaks()], [None], [[0]], pc_range=(0, 0), voxel_size=(1, 1), out_size_factor=1),
     f"{CPD}: feats[0] must be a tensor or a non-empty sequence of tensors"),
    ("cpd-feats-empty", lambda: cpd(feats=[]), f"{CPD}: feats[0] must be a tensor or a non-empty sequence of tensors"),
    ("bhd-feats-empty", lambda: bhd(feats=[]), f"{BHD}: feats must be a tensor or a non-empty sequence of tensors"),
    ("bhd-feats-number", lambda: bhd(feats=3.0), f"{BHD}: feats must be a tensor or a non-empty sequence of tensors"),
    ("gac-feats-empty", lambda: gather_at_centers([], torch.zeros((1, 1), dtype=I64)),
     "gather_at_centers: feats must be a tensor or a non-empty sequence of tensors"),
    ("crl-feats-none", lambda: center_regression_loss(None, None, None), "center_regression_loss: feats must be a tensor or a non-empty sequence of tensors"),
    ("cpd-map-not-tensor", lambda: cpd(feats=[torch.zeros((1, 8, 2, 2)), 3.0]), f"{CPD}: feats[0][1] must be a tensor"),
    ("bhd-map-not-tensor", lambda: bhd(feats=[torch.zeros((1, 4, 2, 2)), 3.0]), f"{BHD}: feats[1] must be a tensor"),
    ("gac-map-not-tensor", lambda: gather_at_centers([3.0], torch.zeros((1, 1), dtype=I64)), "gather_at_centers: feats[0] must be a tensor"),
    ("crl-map-not-tensor", lambda: center_regression_loss([3.0], None, None), "center_regression_loss: feats[0] must be a tensor"),
    # a ninth map
    ("cpd-nine-maps", lambda: cpd(feats=maps9()), f"{CPD}: at most 8 maps per task are supported, feats[0] has 9"),
    ("bhd-nine-maps", lambda: bhd(feats=maps9()), f"{BHD}: at most 8 maps are supported, feats has 9"),
    ("gac-nine-maps", lambda: gather_at_centers(maps9(), torch.zeros((1, 1), dtype=I64)), "gather_at_centers: at most 8 maps are supported, got 9"),
    ("crl-nine-maps", lambda: center_regression_loss(maps9(), None, None), "center_regression_loss: at most 8 maps are supported, got 9"),
    # there is no CPU path behind the regression operators: what they say of a CPU map
    ("gac-cpu-map", lambda: gather_at_centers(torch.zeros((1, 1, 2, 2)), torch.zeros((1, 1), dtype=I64)),
     "gather_at_centers: feats[0] must be a CUDA tensor (there is no CPU path)"),
    ("crl-cpu-map", lambda: center_regression_loss(torch.zeros((1, 1, 2, 2)), None, None),
     "center_regression_loss: feats[0] must be a CUDA tensor (there is no CPU path)"),
    # wrong rank
    ("cpd-map-rank", lambda: cpd(feats=torch.zeros((8, 2, 2))), f"{CPD}: feats[0][0] must be [B, C, H, W], got 3 dimensions"),
    ("bhd-map-rank", lambda: bhd(feats=torch.zeros((4, 2, 2))), f"{BHD}: feats[0] must be [F, C, H, W], got 3 dimensions"),
    # non-contiguous
    ("cpd-map-strided", lambda: cpd(feats=strided((1, 8, 2, 2))), f"{CPD}: feats[0][0] must be contiguous (a map is not copied silently)"),
    ("bhd-map-strided", lambda: bhd(feats=strided((1, 4, 2, 2))), f"{BHD}: feats[0] must be contiguous (a map is not copied silently)"),
    # another device than the peaks
    ("cpd-map-meta", lambda: cpd(feats=torch.zeros((1, 8, 2, 2), device="meta")), f"{CPD}: feats[0][0] is on meta, the peaks on cpu"),
    ("bhd-map-meta", lambda: bhd(feats=torch.zeros((1, 4, 2, 2), device="meta")), f"{BHD}: feats[0] is on meta, the peaks on cpu"),
    # float64, two dtypes
    ("cpd-map-f64", lambda: cpd(feats=torch.zeros((1, 8, 2, 2), dtype=F64)), f"{CPD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    ("bhd-map-f64", lambda: bhd(feats=torch.zeros((1, 4, 2, 2), dtype=F64)), f"{BHD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    ("cpd-map-dtypes", lambda: cpd(feats=[torch.zeros((1, 4, 2, 2)), torch.zeros((1, 4, 2, 2), dtype=torch.float16)]),
     f"{CPD}: feats[0][1] has dtype torch.float16, feats[0][0] torch.float32"),
    ("bhd-map-dtypes", lambda: bhd(feats=[torch.zeros((1, 2, 2, 2)), torch.zeros((1, 2, 2, 2), dtype=torch.float16)]),
     f"{BHD}: feats[1] has dtype torch.float16, feats[0] torch.float32"),
    ("cpd-task1-map-dtype", lambda: cpd([peaks(), peaks()], [torch.zeros((1, 8, 2, 2)), torch.zeros((1, 8, 2, 2), dtype=torch.bfloat16)],
                                        tasks=((0,), (1,))),
     f"{CPD}: feats[1][0] has dtype torch.bfloat16, feats[0][0] torch.float32"),
    # maps that disagree in H, in B with the peaks
    ("cpd-map-H", lambda: cpd(feats=[torch.zeros((1, 4, 2, 2)), torch.zeros((1, 4, 3, 2))]),
     f"{CPD}: feats[0][1] has shape (1, 4, 3, 2): B = 1, H = 2 and W = 2 must agree"),
    ("bhd-map-H", lambda: bhd(feats=[torch.zeros((1, 2, 2, 2)), torch.zeros((1, 2, 3, 2))]),
     f"{BHD}: feats[1] has shape (1, 2, 3, 2): F = 1, H = 2 and W = 2 must agree"),
    ("cpd-map-B", lambda: cpd(feats=torch.zeros((2, 8, 2, 2))), f"{CPD}: feats[0][0] has shape (2, 8, 2, 2): B = 1, H = 2 and W = 2 must agree"),
    ("bhd-map-B", lambda: bhd(feats=torch.zeros((2, 4, 2, 2))), f"{BHD}: feats[0] has shape (2, 4, 2, 2): F = 1, H = 2 and W = 2 must agree"),
    ("cpd-task1-map-W", lambda: cpd([peaks(), peaks()], [torch.zeros((1, 8, 2, 2)), torch.zeros((1, 8, 2, 3))], tasks=((0,), (1,))),
     f"{CPD}: feats[1][0] has shape (1, 8, 2, 3): B = 1, H = 2 and W = 2 must agree"),
    # the channel sums stay with their operators
    ("cpd-channels", lambda: cpd(feats=torch.zeros((1, 9, 2, 2))),
     f"{CPD}: the maps of a task must hold 8 or 10 channels in total, the same for every task; feats[0] holds 9"),
    ("bhd-channels", lambda: bhd(feats=torch.zeros((1, 3, 2, 2))),
     f"{BHD}: the maps must hold 4..8 channels in total (off_x, off_y, h, w and up to 4 extras), feats holds 3"),
    # order: the count before the members, rank before contiguity, dtype before shape
    ("cpd-order-nine-not-tensor", lambda: cpd(feats=[3.0] * 9), f"{CPD}: at most 8 maps per task are supported, feats[0] has 9"),
    ("bhd-order-nine-not-tensor", lambda: bhd(feats=[3.0] * 9), f"{BHD}: at most 8 maps are supported, feats has 9"),
    ("gac-order-nine-not-tensor", lambda: gather_at_centers([3.0] * 9, None), "gather_at_centers: at most 8 maps are supported, got 9"),
    ("gac-order-not-tensor-cpu", lambda: gather_at_centers([torch.zeros((1, 1, 2, 2)), 3.0], None),
     "gather_at_centers: feats[0] must be a CUDA tensor (there is no CPU path)"),
    ("cpd-order-rank-strided-map", lambda: cpd(feats=strided((8, 2, 2))), f"{CPD}: feats[0][0] must be [B, C, H, W], got 3 dimensions"),
    ("bhd-order-rank-strided-map", lambda: bhd(feats=strided((4, 2, 2))), f"{BHD}: feats[0] must be [F, C, H, W], got 3 dimensions"),
    ("cpd-order-f64-H", lambda: cpd(feats=[torch.zeros((1, 4, 2, 2)), torch.zeros((1, 4, 3, 2), dtype=F64)]),
     f"{CPD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    ("bhd-order-f64-H", lambda: bhd(feats=[torch.zeros((1, 2, 2, 2)), torch.zeros((1, 2, 3, 2), dtype=F64)]),
     f"{BHD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    ("cpd-order-map0-then-map1", lambda: cpd(feats=[torch.zeros((1, 4, 2, 2), dtype=F64), 3.0]),
     f"{CPD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    ("bhd-order-map0-then-map1", lambda: bhd(feats=[torch.zeros((1, 2, 2, 2), dtype=F64), 3.0]),
     f"{BHD}: feats must be float32, float16 or bfloat16, got torch.float64"),
    # ------------------------------------------------------------------------------------- detections: not a tensor, rank
    ("rnb-not-ragged", lambda: rnb([(torch.zeros((1, 2, 7)),) * 4]), f"{RNB}: detections[0].boxes must be a RaggedBatch"),
    ("nb-not-ragged", lambda: nb((torch.zeros((1, 2, 4)),) * 5), f"{NB}: detections.boxes must be a RaggedBatch"),
    ("rnb-boxes-not-tensor", lambda: rnb(det3(boxes=[1.0])), f"{RNB}: detections[0].boxes must hold a tensor"),
    ("nb-boxes-not-tensor", lambda: nb(det2(boxes=[1.0])), f"{NB}: detections.boxes must hold a tensor"),
    ("iou-not-tensor", lambda: rotated_iou_bev(torch.zeros((1, 2, 5)), torch.zeros((1, 2, 5))), f"{IOU}: boxes_a must hold a tensor"),
    ("rnb-boxes-rank", lambda: rnb(det3(boxes=torch.zeros((1, 2)))), f"{RNB}: detections[0].boxes must be [B, N, D], got (1, 2)"),
    ("nb-boxes-rank", lambda: nb(det2(boxes=torch.zeros((1, 2)))), f"{NB}: detections.boxes must be [F, N, 4], got (1, 2)"),
    ("rnb-scores-rank", lambda: rnb(det3(scores=torch.zeros((1, 2, 1)))), f"{RNB}: detections[0].scores must be [B, N], got (1, 2, 1)"),
    ("nb-extras-rank", lambda: nb(det2(extras=torch.zeros((1, 2)))), f"{NB}: detections.extras must be [F, N, E], got (1, 2)"),
    ("iou-rank", lambda: iou(b=torch.zeros((2, 5))), f"{IOU}: boxes_b must be [B, N, 5], got (2, 5)"),
    # float64 boxes, int32 labels
    ("rnb-boxes-f64", lambda: rnb(det3(boxes=torch.zeros((1, 2, 7), dtype=F64))), f"{RNB}: detections[0].boxes must be float32, got torch.float64"),
    ("nb-boxes-f64", lambda: nb(det2(boxes=torch.zeros((1, 2, 4), dtype=F64))), f"{NB}: detections.boxes must be float32, got torch.float64"),
    ("iou-f64", lambda: iou(torch.zeros((1, 2, 5), dtype=F64)), f"{IOU}: boxes_a must be float32, got torch.float64"),
    ("rnb-labels-i32", lambda: rnb(det3(labels=torch.zeros((1, 2), dtype=I32))), f"{RNB}: detections[0].labels must be int64, got torch.int32"),
    ("nb-labels-i32", lambda: nb(det2(labels=torch.zeros((1, 2), dtype=I32))), f"{NB}: detections.labels must be int64, got torch.int32"),
    ("rnb-source-i64", lambda: rnb(det3(source=torch.zeros((1, 2), dtype=I64))), f"{RNB}: detections[0].source must be int32, got torch.int64"),
    ("nb-source-i64", lambda: nb(det2(source=torch.zeros((1, 2), dtype=I64))), f"{NB}: detections.source must be int32, got torch.int64"),
    # a device that is neither: the two NMS operators word it differently
    ("rnb-boxes-meta", lambda: rnb(det3(boxes=torch.zeros((1, 2, 7), device="meta"))), f"{RNB}: detections[0].boxes must be a CUDA or CPU tensor, got meta"),
    ("iou-meta", lambda: iou(torch.zeros((1, 2, 5), device="meta")), f"{IOU}: boxes_a must be a CUDA or CPU tensor, got meta"),
    ("nb-boxes-meta", lambda: nb(det2(boxes=torch.zeros((1, 2, 4), device="meta"))), f"{NB}: detections.boxes must be CUDA or CPU tensors, got meta"),
    # non-contiguous
    ("rnb-boxes-strided", lambda: rnb(det3(boxes=strided((1, 2, 7)))), f"{RNB}: detections[0].boxes must be contiguous (it is not copied silently)"),
    ("nb-boxes-strided", lambda: nb(det2(boxes=strided((1, 2, 4)))), f"{NB}: detections.boxes must be contiguous (it is not copied silently)"),
    ("nb-scores-strided", lambda: nb(det2(scores=strided((1, 2)))), f"{NB}: detections.scores must be contiguous (it is not copied silently)"),
    ("iou-strided", lambda: iou(b=strided((1, 2, 5))), f"{IOU}: boxes_b must be contiguous (it is not copied silently)"),
    # N = 0 and N = 1025
    ("rnb-N0", lambda: rnb(det3(0)), f"{RNB}: N must be in 1..1024, got 0"),
    ("nb-N0", lambda: nb(det2(0)), f"{NB}: N must be in 1..1024, got 0"),
    ("rnb-N1025", lambda: rnb(det3(1025)), f"{RNB}: N must be in 1..1024, got 1025"),
    ("nb-N1025", lambda: nb(det2(1025)), f"{NB}: N must be in 1..1024, got 1025"),
    # the members' shapes
    ("rnb-scores-shape", lambda: rnb(det3(scores=torch.zeros((1, 3)))), f"{RNB}: detections[0].scores must be (1, 2) on cpu, got (1, 3) on cpu"),
    ("nb-scores-shape", lambda: nb(det2(scores=torch.zeros((1, 3)))), f"{NB}: detections.scores must be (1, 2) on cpu, got (1, 3) on cpu"),
    ("nb-extras-shape", lambda: nb(det2(extras=torch.zeros((1, 3, 1)))), f"{NB}: detections.extras must be (1, 2, 1) on cpu, got (1, 3, 1) on cpu"),
    # sample sizes: int32, strided, and a member that does not share them
    ("rnb-sizes-i32", lambda: rnb(det3(sizes=torch.full((1,), 2, dtype=I32))),
     f"{RNB}: the sample_sizes of detections[0].boxes must be an int64 tensor (1,) on cpu"),
    ("nb-sizes-i32", lambda: nb(det2(sizes=torch.full((1,), 2, dtype=I32))), f"{NB}: the sample_sizes of detections.boxes must be an int64 tensor (1,) on cpu"),
    ("iou-sizes-shape", lambda: rotated_iou_bev(NS(tensor=torch.zeros((1, 2, 5)), sample_sizes=torch.ones((2,), dtype=I64)),
                                                NS(tensor=torch.zeros((1, 2, 5)), sample_sizes=torch.ones((1,), dtype=I64))),
     f"{IOU}: the sample_sizes of boxes_a must be an int64 tensor (1,) on cpu"),
    ("rnb-sizes-not-tensor", lambda: rnb(det3(boxes_sizes=[2])), f"{RNB}: the sample_sizes of detections[0].boxes must be an int64 tensor (1,) on cpu"),
    ("nb-sizes-not-tensor", lambda: nb(det2(boxes_sizes=[2])), f"{NB}: the sample_sizes of detections.boxes must be an int64 tensor (1,) on cpu"),
    ("rnb-sizes-strided", lambda: rnb(det3(B=2, sizes=strided((2,), I64))), f"{RNB}: the sample_sizes of detections[0].boxes must be contiguous"),
    ("nb-sizes-strided", lambda: nb(det2(B=2, sizes=strided((2,), I64))), f"{NB}: the sample_sizes of detections.boxes must be contiguous"),
    ("rnb-not-shared", lambda: rnb(det3(scores_sizes=torch.full((1,), 2, dtype=I64))),
     f"{RNB}: detections[0].scores does not share the sample_sizes of detections[0].boxes (the four members of a task share one tensor)"),
    ("nb-not-shared", lambda: nb(det2(scores_sizes=torch.full((1,), 2, dtype=I64))),
     f"{NB}: detections.scores does not share the sample_sizes of detections.boxes (the five members share one tensor)"),
    ("rnb-source-not-shared", lambda: rnb(det3(source_sizes=None)),
     f"{RNB}: detections[0].source does not share the sample_sizes of detections[0].boxes (the four members of a task share one tensor)"),
    ("nb-extras-not-shared", lambda: nb(det2(extras_sizes=torch.full((1,), 2, dtype=I32))),
     f"{NB}: detections.extras does not share the sample_sizes of detections.boxes (the five members share one tensor)"),
    # order: rank before dtype, dtype before contiguity, N before the members, the members before the sharing
    ("rnb-order-rank-f64", lambda: rnb(det3(boxes=torch.zeros((1, 2), dtype=F64))), f"{RNB}: detections[0].boxes must be [B, N, D], got (1, 2)"),
    ("nb-order-rank-f64", lambda: nb(det2(boxes=torch.zeros((1, 2), dtype=F64))), f"{NB}: detections.boxes must be [F, N, 4], got (1, 2)"),
    ("rnb-order-f64-strided", lambda: rnb(det3(boxes=strided((1, 2, 7), F64))), f"{RNB}: detections[0].boxes must be float32, got torch.float64"),
    ("nb-order-f64-strided", lambda: nb(det2(boxes=strided((1, 2, 4), F64))), f"{NB}: detections.boxes must be float32, got torch.float64"),
    ("rnb-order-N-shared", lambda: rnb(det3(0, scores_sizes=torch.zeros((1,), dtype=I64))), f"{RNB}: N must be in 1..1024, got 0"),
    ("nb-order-N-shared", lambda: nb(det2(0, scores_sizes=torch.zeros((1,), dtype=I64))), f"{NB}: N must be in 1..1024, got 0"),
    ("rnb-order-shape-shared", lambda: rnb(det3(scores=torch.zeros((1, 3)), scores_sizes=torch.zeros((1,), dtype=I64))),
     f"{RNB}: detections[0].scores must be (1, 2) on cpu, got (1, 3) on cpu"),
    ("nb-order-shape-shared", lambda: nb(det2(scores=torch.zeros((1, 3)), scores_sizes=torch.zeros((1,), dtype=I64))),
     f"{NB}: detections.scores must be (1, 2) on cpu, got (1, 3) on cpu"),
    ("rnb-order-sizes-shared", lambda: rnb(det3(sizes=torch.full((1,), 2, dtype=I32), scores_sizes=torch.zeros((1,), dtype=I64))),
     f"{RNB}: the sample_sizes of detections[0].boxes must be an int64 tensor (1,) on cpu"),
    ("nb-order-sizes-shared", lambda: nb(det2(sizes=torch.full((1,), 2, dtype=I32), scores_sizes=torch.zeros((1,), dtype=I64))),
     f"{NB}: the sample_sizes of detections.boxes must be an int64 tensor (1,) on cpu"),
    ("rnb-order-detections-threshold", lambda: rnb(det3(0), NAN), f"{RNB}: N must be in 1..1024, got 0"),
    ("nb-order-detections-threshold", lambda: nb(det2(0), NAN), f"{NB}: N must be in 1..1024, got 0"),
    # ------------------------------------------------------------------------------------------------- the head outputs
    ("q3-cls-not-tensor", lambda: q3(cls=[[[0.0]]]), f"{Q3}: cls_scores must be a tensor"),
    ("q2-rows-not-tensor", lambda: q2(rows=[[[0.0] * 4] * 2]), f"{Q2}: bbox_preds must be a tensor"),
    ("q3-cls-rank", lambda: q3(cls=torch.zeros((1, 2))), f"{Q3}: cls_scores must be [B, Q, C], got (1, 2)"),
    ("q2-rows-rank", lambda: q2(rows=torch.zeros((2, 4))), f"{Q2}: bbox_preds must be [B, Q, D], got (2, 4)"),
    ("q3-cls-f64", lambda: q3(cls=torch.zeros((1, 2, 1), dtype=F64)), f"{Q3}: cls_scores must be float32, float16 or bfloat16, got torch.float64"),
    ("q2-rows-f64", lambda: q2(rows=torch.zeros((1, 2, 4), dtype=F64)), f"{Q2}: bbox_preds must be float32, float16 or bfloat16, got torch.float64"),
    ("q3-cls-strided", lambda: q3(cls=strided((1, 2, 1))), f"{Q3}: cls_scores must be contiguous (it is not copied silently)"),
    ("q2-rows-strided", lambda: q2(rows=strided((1, 2, 4))), f"{Q2}: bbox_preds must be contiguous (it is not copied silently)"),
    ("q3-max-num-0", lambda: q3(max_num=0), f"{Q3}: max_num must be an integer in 1..1024, got 0"),
    ("q2-max-num-1025", lambda: q2(max_num=1025), f"{Q2}: max_num must be an integer in 1..1024, got 1025"),
    ("q3-max-num-true", lambda: q3(max_num=True), f"{Q3}: max_num must be an integer in 1..1024, got True"),
    ("q2-max-num-float", lambda: q2(max_num=1.5), f"{Q2}: max_num must be an integer in 1..1024, got 1.5"),
    # ------------------------------------------------------------------------------------------------------ thresholds
    ("cpd-score-nan", lambda: cpd(score_threshold=NAN), f"{CPD}: score_threshold must not be NaN"),
    ("bhd-score-nan", lambda: bhd(score_threshold=NAN), f"{BHD}: score_threshold must not be NaN"),
    ("q3-score-nan", lambda: q3(score_threshold=NAN), f"{Q3}: score_threshold must not be NaN"),
    ("q2-score-nan", lambda: q2(score_threshold=NAN), f"{Q2}: score_threshold must not be NaN"),
    ("cpd-nms-nan", lambda: cpd(nms_threshold=NAN), f"{CPD}: nms_threshold[0] must not be NaN"),
    ("bhd-iou-nan", lambda: bhd(iou_threshold=NAN), f"{BHD}: iou_threshold must not be NaN"),
    ("nb-iou-nan", lambda: nb(thr=NAN), f"{NB}: iou_threshold must not be NaN"),
    ("rnb-iou-nan", lambda: rnb(thr=NAN), f"{RNB}: iou_threshold[0] must not be NaN"),
    ("rnb-iou-list-nan", lambda: rnb(thr=[NAN]), f"{RNB}: iou_threshold[0] must not be NaN"),
    ("cpd-score-true", lambda: cpd(score_threshold=True), f"{CPD}: score_threshold must be a Python number, got True"),
    ("bhd-score-text", lambda: bhd(score_threshold="0.5"), f"{BHD}: score_threshold must be a Python number, got '0.5'"),
    ("q3-score-tensor", lambda: q3(score_threshold=[0.5]), f"{Q3}: score_threshold must be a Python number, got [0.5]"),
    ("q2-score-true", lambda: q2(score_threshold=True), f"{Q2}: score_threshold must be a Python number, got True"),
    ("bhd-iou-true", lambda: bhd(iou_threshold=True), f"{BHD}: iou_threshold must be a Python number, got True"),
    ("nb-iou-text", lambda: nb(thr="0.5"), f"{NB}: iou_threshold must be a Python number, got '0.5'"),
    ("cpd-nms-text", lambda: cpd(nms_threshold=["0.5"]), f"{CPD}: nms_threshold[0] must be a Python number, got '0.5'"),
    ("rnb-iou-text", lambda: rnb(thr=["0.5"]), f"{RNB}: iou_threshold[0] must be a Python number or None, got '0.5'"),
    ("rnb-iou-true", lambda: rnb(thr=True),
     f"{RNB}: iou_threshold must be a number, a sequence of 1 numbers or Nones (one per task) or None, got True"),
    # --------------------------------------------------------------------------------------------------------- the cuts
    ("cpd-post-0", lambda: cpd(post_max_size=0), f"{CPD}: post_max_size must be at least 1, got 0"),
    ("bhd-post-0", lambda: bhd(post_max_size=0), f"{BHD}: post_max_size must be at least 1, got 0"),
    ("nb-post-0", lambda: nb(post_max_size=0), f"{NB}: post_max_size must be at least 1, got 0"),
    ("rnb-post-0", lambda: rnb(post_max_size=0), f"{RNB}: post_max_size must be at least 1, got 0"),
    ("nb-pre-0", lambda: nb(pre_max_size=0), f"{NB}: pre_max_size must be at least 1, got 0"),
    ("rnb-pre-minus", lambda: rnb(pre_max_size=-3), f"{RNB}: pre_max_size must be at least 1, got -3"),
    ("cpd-post-true", lambda: cpd(post_max_size=True), f"{CPD}: post_max_size must be a Python integer, got True"),
    ("bhd-post-true", lambda: bhd(post_max_size=True), f"{BHD}: post_max_size must be a Python integer, got True"),
    ("nb-post-true", lambda: nb(post_max_size=True), f"{NB}: post_max_size must be a Python integer, got True"),
    ("rnb-post-true", lambda: rnb(post_max_size=True), f"{RNB}: post_max_size must be a Python integer or None, got True"),
    ("cpd-post-float", lambda: cpd(post_max_size=1.5), f"{CPD}: post_max_size must be a Python integer, got 1.5"),
    ("bhd-post-float", lambda: bhd(post_max_size=1.5), f"{BHD}: post_max_size must be a Python integer, got 1.5"),
    ("nb-post-float", lambda: nb(post_max_size=1.5), f"{NB}: post_max_size must be a Python integer, got 1.5"),
    ("rnb-post-float", lambda: rnb(post_max_size=1.5), f"{RNB}: post_max_size must be a Python integer or None, got 1.5"),
    ("nb-pre-float", lambda: nb(pre_max_size=1.5), f"{NB}: pre_max_size must be a Python integer, got 1.5"),
    ("rnb-pre-true", lambda: rnb(pre_max_size=True), f"{RNB}: pre_max_size must be a Python integer or None, got True"),
    # order: the thresholds before the cuts, pre before post, the operands before both
    ("cpd-order-score-post", lambda: cpd(score_threshold=NAN, post_max_size=0), f"{CPD}: score_threshold must not be NaN"),
    ("cpd-order-nms-post", lambda: cpd(nms_threshold=NAN, post_max_size=0), f"{CPD}: nms_threshold[0] must not be NaN"),
    ("bhd-order-score-iou", lambda: bhd(score_threshold=NAN, iou_threshold=NAN), f"{BHD}: score_threshold must not be NaN"),
    ("bhd-order-iou-post", lambda: bhd(iou_threshold=NAN, post_max_size=0), f"{BHD}: iou_threshold must not be NaN"),
    ("nb-order-iou-pre", lambda: nb(thr=NAN, pre_max_size=0), f"{NB}: iou_threshold must not be NaN"),
    ("rnb-order-iou-pre", lambda: rnb(thr=NAN, pre_max_size=0), f"{RNB}: iou_threshold[0] must not be NaN"),
    ("nb-order-pre-post", lambda: nb(pre_max_size=0, post_max_size=True), f"{NB}: pre_max_size must be at least 1, got 0"),
    ("rnb-order-pre-post", lambda: rnb(pre_max_size=0, post_max_size=True), f"{RNB}: pre_max_size must be at least 1, got 0"),
    ("cpd-order-feats-post", lambda: cpd(feats=maps9(), post_max_size=0), f"{CPD}: at most 8 maps per task are supported, feats[0] has 9"),
    ("bhd-order-feats-score", lambda: bhd(feats=maps9(), score_threshold=NAN), f"{BHD}: at most 8 maps are supported, feats has 9"),
    ("q3-order-head-score", lambda: q3(max_num=0, score_threshold=NAN), f"{Q3}: max_num must be an integer in 1..1024, got 0"),
]


@pytest.mark.parametrize("call,message", [pytest.param(c, m, id=i) for i, c, m in ROWS])
def test_malformed_input_is_refused_with_this_message(call, message):
    with pytest.raises(RuntimeError) as e:
        call()
    assert type(e.value) is RuntimeError
    assert str(e.value) == message


def test_every_row_has_its_own_id_and_every_operator_its_rows():
    ids = [i for i, _, _ in ROWS]
    assert len(set(ids)) == len(ids)
    for prefix in ("cpd", "bhd", "rnb", "nb", "iou", "q3", "q2", "gac", "crl"):
        assert any(i.startswith(prefix + "-") for i in ids), prefix


def test_the_well_formed_calls_of_the_table_pass():
    """what every row above departs from by one or two operands: smallest shapes, padding and counts as documented"""
    (d,) = cpd(score_threshold=0.5, nms_threshold=0.1, post_max_size=1)
    assert tuple(d.boxes.tensor.shape) == (1, 1, 7) and d.boxes.sample_sizes is d.source.sample_sizes
    assert d.boxes.sample_sizes.tolist() == [0] and d.source.tensor.tolist() == [[-1]]
    (d,) = cpd()
    assert d.boxes.sample_sizes.tolist() == [2] and d.source.tensor.tolist() == [[0, 1]]
    b = bhd(score_threshold=-1.0, iou_threshold=0.5, post_max_size=2)
    assert tuple(b.boxes.tensor.shape) == (1, 2, 4) and tuple(b.extras.tensor.shape) == (1, 2, 0)
    assert b.boxes.sample_sizes.tolist() == [2] and b.extras.sample_sizes is b.boxes.sample_sizes
    (r,) = rnb(pre_max_size=2, post_max_size=1)
    assert tuple(r.boxes.tensor.shape) == (1, 1, 7) and r.boxes.sample_sizes.tolist() == [1]
    n = nb(pre_max_size=1)
    assert tuple(n.boxes.tensor.shape) == (1, 1, 4) and n.boxes.sample_sizes.tolist() == [1]
    assert tuple(iou().tensor.shape) == (1, 2, 2)
    assert q3(score_threshold=0.25).boxes.sample_sizes.tolist() == [1]
    assert q2(score_threshold=0.75).boxes.sample_sizes.tolist() == [0]
    # members that share their sample sizes through a view of one tensor, not one object: the data pointer decides
    sizes = torch.full((1,), 2, dtype=I64)
    assert rnb(det3(sizes=sizes, scores_sizes=sizes.view(1)))[0].boxes.sample_sizes.tolist() == [2]
    assert nb(det2(sizes=sizes, extras_sizes=sizes.view(1))).boxes.sample_sizes.tolist() == [2]


@pytest.mark.parametrize("B", [0, 1])
def test_empty_batches_have_zeroed_sizes_and_the_shapes_of_full_ones(B):
    p = NS(scores=torch.zeros((B, 2)), indices=torch.zeros((B, 2), dtype=I64), classes=torch.zeros((B, 2), dtype=I64))
    (d,) = center_point_decode(p, torch.zeros((B, 8, 2, 2)), [[0]], pc_range=(0.0, 0.0), voxel_size=(1.0, 1.0), out_size_factor=1)
    b = box_heatmap_decode(p, torch.zeros((B, 5, 2, 2)), image_hw=(2, 2))
    sizes = torch.full((B,), 2, dtype=I64)
    d3 = CenterPointDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in
                                 (torch.zeros((B, 2, 7)), torch.zeros((B, 2)), torch.zeros((B, 2), dtype=I64), torch.zeros((B, 2), dtype=I32))))
    d2 = BoxDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in
                         (torch.zeros((B, 2, 4)), torch.zeros((B, 2)), torch.zeros((B, 2), dtype=I64), torch.zeros((B, 2), dtype=I32),
                          torch.zeros((B, 2, 1)))))
    (r,) = rotated_nms_bev(d3, None)
    n = nms_boxes(d2, None)
    q = query_box_decode_3d(torch.zeros((B, 2, 1)), torch.zeros((B, 2, 8)), 2)
    w = query_box_decode_2d(torch.zeros((B, 2, 1)), torch.zeros((B, 2, 4)), 2, image_hw=(2, 2))
    for out, width in ((d, 7), (b, 4), (r, 7), (n, 4), (q, 7), (w, 4)):
        assert tuple(out.boxes.tensor.shape) == (B, 2, width) and out.boxes.tensor.dtype == F32
        assert tuple(out.scores.tensor.shape) == (B, 2) and out.scores.tensor.dtype == F32
        assert out.labels.tensor.dtype == I64 and out.source.tensor.dtype == I32
        s = out.boxes.sample_sizes
        assert s.dtype == I64 and s.tolist() == [2] * B and all(m.sample_sizes is s for m in out)
    assert tuple(b.extras.tensor.shape) == (B, 2, 1) and tuple(n.extras.tensor.shape) == (B, 2, 1) and tuple(w.extras.tensor.shape) == (B, 2, 0)
    assert not math.isnan(float(b.extras.tensor.sum()))
