"""Bad-argument calls of the operators that have a device entry and a host entry, for the table
tests/golden/operand_errors.json: golden/make_operand_errors.py records (exception type, message) of every case,
test_operand_errors_cpu.py replays them and compares both exactly.

Every case is a valid CPU call (B = 2, G = 3) with one or two operands spoilt, so it is refused before any native call.
A tensor on the meta device is "another device"; `Rag` stands in for a RaggedBatch where a real one would not hold the
spoilt tensor (the wrappers ask for `.tensor` and `.sample_sizes` only).
"""
import torch

from accvlab.batching_helpers import RaggedBatch, batched_linear_sum_assignment, batched_matching_cost
from accvlab.draw_heatmap import (bev_augment_boxes, boxes_to_heatmap, camera_augment_boxes, center_point_decode,
                                  center_point_targets, center_regression_loss, gather_at_centers, rotated_iou_bev,
                                  rotated_nms_bev, visible_bbox_mask)
from accvlab.draw_heatmap.peaks import HeatmapPeaks
from accvlab.image_prep import nv12_to_rgb, prepare_images, prepare_images_nv12
from accvlab.lane_helpers.polyline import batched_polyline_matching_cost

B, G = 2, 3


class Rag:
    def __init__(self, tensor, sample_sizes):
        self.tensor, self.sample_sizes = tensor, sample_sizes


def _f(*shape):
    return torch.arange(1, 1 + int(torch.Size(shape).numel()), dtype=torch.float32).reshape(shape) / 8


def _i(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype)


def _noncontig(t):
    """the same shape, dtype and values behind a `[:, ::2]` slice (`[::2]` for one dimension)"""
    if t.dim() == 1:
        return t.repeat_interleave(2)[::2]
    return t.repeat_interleave(2, dim=1)[:, ::2]


def _other_int(t):
    return t.to(torch.int16)


FAULTS = {
    "not_tensor": lambda t: t.tolist(),
    "meta": lambda t: t.to("meta"),
    "noncontig": _noncontig,
    "float64": lambda t: t.double(),
    "int16": _other_int,
    "float32": lambda t: t.float(),
    "rank": lambda t: t[..., None].contiguous(),
    "shape": lambda t: torch.cat([t, t], dim=-1).contiguous(),
}
_FLOAT = ("not_tensor", "meta", "noncontig", "float64", "shape", "int16")
_INT = ("not_tensor", "meta", "noncontig", "float32", "shape", "int16")


# ---------------------------------------------------------------------------------------------------------------- entries
# name -> (operands(): dict name -> tensor, build(o, **kw) -> zero-argument callable, {operand: fault names})

def _visible_ops():
    return dict(bboxes=_f(B, G, 4), depths=_f(B, G), sample_sizes=_i(B) + G, image_hw=_i(B, 2, dtype=torch.int32) + 64)


def _visible(o, **kw):
    kw.setdefault("image_hw", o["image_hw"])
    return lambda: visible_bbox_mask(Rag(o["bboxes"], o["sample_sizes"]), o["depths"], **kw)


def _camera_ops():
    return dict(bboxes=_f(B, G, 4), transforms=_f(B, 2, 3), centers=_f(B, G, 2), depths=_f(B, G), categories=_i(B, G),
                valid=torch.ones((B, G), dtype=torch.bool), sample_sizes=_i(B) + G, image_hw=_i(B, 2, dtype=torch.int32) + 64,
                matrix=_f(B, 3, 4))


def _camera(o, **kw):
    kw.setdefault("image_hw", o["image_hw"])
    kw.setdefault("projection_matrices", (o["matrix"],))
    return lambda: camera_augment_boxes(Rag(o["bboxes"], o["sample_sizes"]), o["transforms"], centers=o["centers"],
                                        depths=o["depths"], categories=o["categories"], valid=o["valid"], **kw)


def _heatmap_ops():
    return dict(bboxes=_f(B, G, 4), centers=_f(B, G, 2), categories=_i(B, G), is_valid=torch.ones((B, G), dtype=torch.bool),
                sample_sizes=_i(B) + G, image_hw=_i(B, 2, dtype=torch.int32) + 64, out=_f(B, 2, 4, 4))


def _heatmap(o, **kw):
    kw.setdefault("image_hw", o["image_hw"])
    kw.setdefault("heatmap_hw", (4, 4))
    kw.setdefault("num_categories", 2)
    return lambda: boxes_to_heatmap(Rag(o["bboxes"], o["sample_sizes"]), centers=o["centers"], categories=o["categories"],
                                    is_valid=o["is_valid"], out=o["out"], **kw)


def _bev_ops():
    return dict(boxes=_f(B, G, 7), params=_f(B, 7), labels=_i(B, G), valid=torch.ones((B, G), dtype=torch.bool),
                sample_sizes=_i(B) + G, point=_f(B, 1, 4, 4), frame=_f(B, 1, 4, 4))


def _bev(o, **kw):
    return lambda: bev_augment_boxes(Rag(o["boxes"], o["sample_sizes"]), o["params"], labels=o["labels"], valid=o["valid"],
                                     point_transforms=(o["point"],), frame_transforms=(o["frame"],), **kw)


def _targets_ops():
    return dict(boxes=_f(B, G, 7), labels=_i(B, G), sample_sizes=_i(B) + G)


def _targets(o, **kw):
    for k, v in dict(pc_range=(-8.0, -8.0), voxel_size=(0.5, 0.5), out_size_factor=2, grid_size=(16, 16)).items():
        kw.setdefault(k, v)
    kw.setdefault("tasks", [[0], [1]])
    return lambda: center_point_targets(Rag(o["boxes"], o["sample_sizes"]), o["labels"], kw.pop("tasks"), **kw)


def _decode_ops():
    return dict(scores=_f(B, 4), indices=_i(B, 4), classes=_i(B, 4), feats=_f(B, 8, 4, 4))


def _decode(o, **kw):
    for k, v in dict(pc_range=(-8.0, -8.0), voxel_size=(0.5, 0.5), out_size_factor=2).items():
        kw.setdefault(k, v)
    peaks = HeatmapPeaks(o["scores"], o["indices"], o["classes"], None, None)
    return lambda: center_point_decode(peaks, o["feats"], [[0, 1]], **kw)


def _iou_ops():
    return dict(boxes_a=_f(B, G, 5), sizes_a=_i(B) + G, boxes_b=_f(B, 2, 5), sizes_b=_i(B) + 2)


def _iou(o):
    return lambda: rotated_iou_bev(Rag(o["boxes_a"], o["sizes_a"]), Rag(o["boxes_b"], o["sizes_b"]))


def _nms_ops():
    return dict(boxes=_f(B, G, 7), scores=_f(B, G), labels=_i(B, G), source=_i(B, G, dtype=torch.int32), sample_sizes=_i(B) + G)


def _nms(o, **kw):
    kw.setdefault("iou_threshold", 0.5)
    det = tuple(Rag(o[k], o["sample_sizes"]) for k in ("boxes", "scores", "labels", "source"))
    return lambda: rotated_nms_bev(det, kw.pop("iou_threshold"), **kw)


def _prepare_ops():
    return dict(images=_i(B, 4, 6, 3, dtype=torch.uint8), transforms=_f(B, 2, 3), photometric=_f(B, 6),
                source_hw=_i(B, 2, dtype=torch.int32) + 4, out=_f(B, 3, 4, 6))


def _prepare(o, **kw):
    return lambda: prepare_images(o["images"], transforms=o["transforms"], photometric=o["photometric"],
                                  source_hw=o["source_hw"], out=o["out"], **kw)


def _nv12_ops():
    return dict(y=_i(B, 4, 6, dtype=torch.uint8), uv=_i(B, 2, 3, 2, dtype=torch.uint8), out=_i(B, 4, 6, 3, dtype=torch.uint8))


def _nv12(o, **kw):
    return lambda: nv12_to_rgb(o["y"], o["uv"], out=o["out"], **kw)


def _prepare_nv12_ops():
    return dict(y=_i(B, 4, 6, dtype=torch.uint8), uv=_i(B, 2, 3, 2, dtype=torch.uint8), transforms=_f(B, 2, 3),
                photometric=_f(B, 6), source_hw=_i(B, 2, dtype=torch.int32) + 4, out=_f(B, 3, 4, 6))


def _prepare_nv12(o, **kw):
    return lambda: prepare_images_nv12(o["y"], o["uv"], transforms=o["transforms"], photometric=o["photometric"],
                                       source_hw=o["source_hw"], out=o["out"], **kw)


def _cost_ops():
    return dict(pred_scores=_f(B, 4, 3), gt_labels=_i(B, G), pred_boxes=_f(B, 4, 4), gt_boxes=_f(B, G, 4), sample_sizes=_i(B) + G)


def _cost(o, **kw):
    kw.setdefault("l1_weight", 1.0)
    labels = RaggedBatch(o["gt_labels"], sample_sizes=o["sample_sizes"])
    boxes = RaggedBatch(o["gt_boxes"], sample_sizes=o["sample_sizes"])
    return lambda: batched_matching_cost(o["pred_scores"], labels, o["pred_boxes"], boxes, **kw)


def _lsa_ops():
    return dict(cost=_f(B, G, 4), sample_sizes=_i(B) + 4)


def _lsa(o, **kw):
    cost = RaggedBatch(o["cost"], sample_sizes=o["sample_sizes"], non_uniform_dim=2)
    return lambda: batched_linear_sum_assignment(cost, **kw)


def _lines_ops():
    return dict(pred_lines=_f(B, 4, 5, 2), gt_lines=_f(B, G, 5, 2), pred_scores=_f(B, 4, 3), gt_labels=_i(B, G),
                gt_closed=torch.zeros((B, G), dtype=torch.bool), sample_sizes=_i(B) + G)


def _lines(o, **kw):
    kw.setdefault("class_weight", 1.0)
    rb = {k: RaggedBatch(o[k], sample_sizes=o["sample_sizes"]) for k in ("gt_lines", "gt_labels", "gt_closed")}
    return lambda: batched_polyline_matching_cost(o["pred_lines"], rb["gt_lines"], o["pred_scores"], rb["gt_labels"],
                                                  gt_closed=rb["gt_closed"], **kw)


_BOOL = ("not_tensor", "meta", "noncontig", "float32", "shape", "int16")
_U8 = ("not_tensor", "meta", "noncontig", "float32", "shape")
ENTRIES = {
    "visible_bbox_mask": (_visible_ops, _visible, dict(bboxes=_FLOAT, depths=_FLOAT, sample_sizes=_INT, image_hw=_INT)),
    "camera_augment_boxes": (_camera_ops, _camera, dict(bboxes=_FLOAT, transforms=_FLOAT, centers=_FLOAT, depths=_FLOAT,
                                                        categories=_INT, valid=_BOOL, sample_sizes=_INT, image_hw=_INT,
                                                        matrix=_FLOAT)),
    "boxes_to_heatmap": (_heatmap_ops, _heatmap, dict(bboxes=_FLOAT, centers=_FLOAT, categories=_INT, is_valid=_BOOL,
                                                      sample_sizes=_INT, image_hw=_INT, out=_FLOAT)),
    "bev_augment_boxes": (_bev_ops, _bev, dict(boxes=_FLOAT, params=_FLOAT, labels=_INT, valid=_BOOL, sample_sizes=_INT,
                                               point=_FLOAT, frame=_FLOAT)),
    "center_point_targets": (_targets_ops, _targets, dict(boxes=_FLOAT, labels=_INT, sample_sizes=_INT)),
    "center_point_decode": (_decode_ops, _decode, dict(scores=_FLOAT, indices=_INT, classes=_INT, feats=_FLOAT)),
    "rotated_iou_bev": (_iou_ops, _iou, dict(boxes_a=_FLOAT, sizes_a=_INT, boxes_b=_FLOAT, sizes_b=_INT)),
    "rotated_nms_bev": (_nms_ops, _nms, dict(boxes=_FLOAT, scores=_FLOAT, labels=_INT, source=_INT, sample_sizes=_INT)),
    "prepare_images": (_prepare_ops, _prepare, dict(images=_U8, transforms=_FLOAT, photometric=_FLOAT, source_hw=_INT,
                                                    out=_FLOAT)),
    "nv12_to_rgb": (_nv12_ops, _nv12, dict(y=_U8, uv=_U8, out=_U8)),
    "prepare_images_nv12": (_prepare_nv12_ops, _prepare_nv12, dict(y=_U8, uv=_U8, transforms=_FLOAT, photometric=_FLOAT,
                                                                   source_hw=_INT, out=_FLOAT)),
    "batched_matching_cost": (_cost_ops, _cost, dict(pred_scores=_FLOAT, gt_labels=_INT, pred_boxes=_FLOAT, gt_boxes=_FLOAT,
                                                     sample_sizes=_INT)),
    "batched_linear_sum_assignment": (_lsa_ops, _lsa, dict(cost=_FLOAT, sample_sizes=_INT)),
    "batched_polyline_matching_cost": (_lines_ops, _lines, dict(pred_lines=_FLOAT, gt_lines=_FLOAT, pred_scores=_FLOAT,
                                                                gt_labels=_INT, gt_closed=_BOOL, sample_sizes=_INT)),
}

# which fault wins: two operands spoilt in one call (operand.fault + operand.fault)
PAIRS = {
    "visible_bbox_mask": ("depths.float64+depths.noncontig", "bboxes.float64+sample_sizes.meta", "bboxes.shape+depths.float64",
                          "depths.shape+sample_sizes.int16", "sample_sizes.shape+image_hw.float32",
                          "image_hw.noncontig+bboxes.rank"),
    "camera_augment_boxes": ("transforms.float64+bboxes.shape", "bboxes.float64+transforms.noncontig",
                             "centers.shape+depths.float64", "matrix.shape+matrix.noncontig", "matrix.meta+image_hw.float32",
                             "categories.float32+valid.noncontig", "valid.int16+sample_sizes.shape"),
    "boxes_to_heatmap": ("centers.float64+bboxes.shape", "bboxes.float64+out.noncontig", "out.float64+image_hw.shape",
                         "categories.int16+centers.shape", "is_valid.float32+sample_sizes.int16", "out.shape+sample_sizes.rank"),
    "bev_augment_boxes": ("params.float64+boxes.shape", "boxes.float64+labels.noncontig", "labels.int16+valid.float32",
                          "point.shape+point.noncontig", "frame.meta+point.float64", "sample_sizes.int16+frame.shape"),
    "center_point_targets": ("boxes.float64+labels.noncontig", "labels.int16+boxes.shape", "sample_sizes.shape+labels.shape",
                             "sample_sizes.meta+boxes.float64"),
    "center_point_decode": ("scores.float64+scores.noncontig", "indices.float32+scores.float64", "feats.float64+feats.noncontig",
                            "feats.meta+classes.float32"),
    "rotated_iou_bev": ("boxes_a.float64+boxes_a.noncontig", "boxes_a.shape+boxes_b.float64", "sizes_a.int16+boxes_b.noncontig",
                        "sizes_b.noncontig+sizes_a.meta"),
    "rotated_nms_bev": ("boxes.float64+boxes.noncontig", "scores.rank+boxes.shape", "labels.float32+scores.noncontig",
                        "sample_sizes.int16+source.shape"),
    "prepare_images": ("images.float32+images.noncontig", "transforms.float64+photometric.shape", "out.float64+transforms.meta",
                       "source_hw.float32+photometric.float64", "out.noncontig+images.noncontig"),
    "nv12_to_rgb": ("y.float32+uv.float32", "uv.shape+y.noncontig", "out.float32+uv.noncontig", "out.meta+out.shape"),
    "prepare_images_nv12": ("y.noncontig+transforms.float64", "uv.meta+out.float64", "transforms.noncontig+out.noncontig",
                            "source_hw.int16+photometric.meta"),
    "batched_matching_cost": ("pred_scores.float64+gt_labels.float32", "pred_boxes.rank+gt_boxes.rank",
                              "pred_boxes.meta+pred_scores.shape", "gt_boxes.shape+pred_boxes.float64"),
    "batched_linear_sum_assignment": ("cost.int16+cost.rank",),
    "batched_polyline_matching_cost": ("pred_lines.float64+gt_lines.rank", "pred_scores.meta+gt_labels.float32",
                                       "gt_closed.float32+gt_lines.shape", "pred_lines.noncontig+pred_scores.rank"),
}


def _extras():
    """(id, build): faults of the arguments that are no tensors, and the refusals that need every operand spoilt alike"""
    out = []

    def add(entry, tag, change=None, **kw):
        ops, build, _ = ENTRIES[entry]

        def make():
            o = ops()
            if change is not None:
                change(o)
            return build(o, **kw)
        out.append((f"{entry}/{tag}", make))

    def all_meta(o):
        for k in o:
            o[k] = o[k].to("meta")

    def many_boxes(n):
        def change(o):
            for k, t in o.items():
                if t.dim() >= 2 and t.shape[1] == G and k not in ("transforms", "matrix", "out", "image_hw"):
                    o[k] = torch.zeros((B, n) + tuple(t.shape[2:]), dtype=t.dtype)
        return change

    hw_faults = dict(hw_floats=[64.0, 64.0], hw_bool=(True, 64), hw_three=(64, 64, 64), hw_none=None,
                     hw_shape=_i(B, 3, dtype=torch.int32), hw_float_tensor=_f(B, 2))
    for entry in ("visible_bbox_mask", "camera_augment_boxes", "boxes_to_heatmap"):
        for tag, v in hw_faults.items():
            add(entry, tag, image_hw=v)
        add(entry, "all_meta", all_meta)
        add(entry, "too_many_boxes", many_boxes(257))
        add(entry, "too_many_boxes+hw_bool", many_boxes(257), image_hw=(True, 64))
    for entry in ("visible_bbox_mask", "camera_augment_boxes"):
        add(entry, "minimum_size_str", minimum_size="2")
        add(entry, "minimum_size_bool", minimum_size=True)
        add(entry, "minimum_size_str+too_many_boxes", many_boxes(257), minimum_size="2")
        add(entry, "no_depths", lambda o: o.update(depths=None))
    add("visible_bbox_mask", "no_check", check_occlusion=False)
    add("visible_bbox_mask", "depths.float64+no_size_check", lambda o: o.update(depths=o["depths"].double()), minimum_size="2")
    add("camera_augment_boxes", "matrices_no_sequence", projection_matrices=_f(B, 3, 4))
    add("camera_augment_boxes", "matrices_too_many", projection_matrices=(_f(B, 3, 4),) * 5)
    add("camera_augment_boxes", "matrices_too_many+too_many_boxes", many_boxes(257), projection_matrices=(_f(B, 3, 4),) * 5)
    for tag, kw in dict(no_categories=dict(num_categories=None, use_per_category_heatmap=True),
                        heatmap_hw_floats=dict(heatmap_hw=(4.0, 4.0)), heatmap_hw_zero=dict(heatmap_hw=(0, 4)),
                        max_radius_str=dict(max_radius="3"), max_radius_zero=dict(max_radius=0), sigma_zero=dict(radius_to_sigma_factor=0.0),
                        min_object_size_one=dict(min_object_size=(1,)), both_sizes=dict(min_object_size=(1, 1),
                                                                                       per_category_min_object_sizes=[(1, 1)] * 2),
                        k_for_classes_short=dict(k_for_classes=[1.0]), too_many_categories=dict(num_categories=129)).items():
        add("boxes_to_heatmap", tag, **kw)
    add("boxes_to_heatmap", "max_radius_str+bboxes.float64", lambda o: o.update(bboxes=o["bboxes"].double()), max_radius="3")
    for entry in ("bev_augment_boxes", "center_point_targets"):
        add(entry, "all_meta", all_meta)
    for tag, kw in dict(range_check_on=dict(range_check_on="both"), point_range_pair=dict(point_range=(0, 1, 2)),
                        point_range_nan=dict(point_range=((0, 0, float("nan")), (1, 1, 1)))).items():
        add("bev_augment_boxes", tag, **kw)
    add("bev_augment_boxes", "range_check_on+frame.shape", lambda o: o.update(frame=_f(B, 1, 3, 4)), range_check_on="both")
    for tag, kw in dict(tasks_empty=dict(tasks=[]), tasks_twice=dict(tasks=[[0], [0]]), tasks_bool=dict(tasks=[[True]]),
                        voxel_size_zero=dict(voxel_size=(0.0, 0.5)), grid_size_float=dict(grid_size=(16.0, 16)),
                        pc_range_short=dict(pc_range=(0.0,)), max_objs_negative=dict(max_objs=-1),
                        out_size_factor_str=dict(out_size_factor="2")).items():
        add("center_point_targets", tag, **kw)
    add("center_point_targets", "tasks_empty+labels.int16", lambda o: o.update(labels=o["labels"].to(torch.int16)), tasks=[])
    for tag, kw in dict(voxel_size_zero=dict(voxel_size=(0.0, 0.5)), score_threshold_nan=dict(score_threshold=float("nan")),
                        post_center_range_five=dict(post_center_range=(0, 0, 0, 1, 1)), nms_threshold_str=dict(nms_threshold="1"),
                        post_max_size_zero=dict(post_max_size=0), out_size_factor_bool=dict(out_size_factor=True)).items():
        add("center_point_decode", tag, **kw)
    add("center_point_decode", "all_meta", all_meta)
    add("center_point_decode", "feats_nine_channels", lambda o: o.update(feats=_f(B, 9, 4, 4)))
    add("rotated_iou_bev", "all_meta", all_meta)
    add("rotated_iou_bev", "frames_differ", lambda o: o.update(boxes_b=_f(3, 2, 5), sizes_b=_i(3)))
    add("rotated_nms_bev", "all_meta", all_meta)
    for tag, kw in dict(iou_threshold_str=dict(iou_threshold="0.5"), iou_threshold_nan=dict(iou_threshold=float("nan")),
                        iou_threshold_bool=dict(iou_threshold=True), pre_max_size_zero=dict(pre_max_size=0),
                        post_max_size_float=dict(post_max_size=1.5)).items():
        add("rotated_nms_bev", tag, **kw)
    add("rotated_nms_bev", "boxes_wide", lambda o: o.update(boxes=_f(B, G, 17)))
    for entry in ("prepare_images", "prepare_images_nv12"):
        for tag, kw in dict(std_zero=dict(std=0.0), mean_four=dict(mean=(1, 2, 3, 4)), layout=dict(layout="NCHW"),
                            dtype=dict(dtype=torch.float64), tile_hw_zero=dict(tile_hw=0), output_hw_floats=dict(output_hw=(4.0, 6)),
                            output_hw_large=dict(output_hw=(4, 16385)), std_zero_layout=dict(std=0.0, layout="NCHW")).items():
            add(entry, tag, **kw)
        add(entry, "all_meta", all_meta)
    add("prepare_images", "output_hw_without_transforms", lambda o: o.update(transforms=None, out=None), output_hw=(8, 8))
    add("nv12_to_rgb", "all_meta", all_meta)
    add("nv12_to_rgb", "chroma_order", chroma_order="yuv")
    add("nv12_to_rgb", "chroma_order+out.float32", lambda o: o.update(out=o["out"].float()), chroma_order="yuv")
    for tag, kw in dict(class_cost=dict(class_cost="softmax"), box_format=dict(box_format="xywh"), giou_five=dict(giou_weight=1.0)).items():
        add("batched_matching_cost", tag, (lambda o: o.update(pred_boxes=_f(B, 4, 5), gt_boxes=_f(B, G, 5))) if tag == "giou_five"
            else None, **kw)
    add("batched_matching_cost", "all_meta", all_meta)
    add("batched_linear_sum_assignment", "all_meta", all_meta)
    add("batched_linear_sum_assignment", "threads", _threads=128)
    add("batched_linear_sum_assignment", "too_large", lambda o: o.update(cost=torch.zeros((B, 1, 4097)).expand(B, 1025, 4097)))
    add("batched_polyline_matching_cost", "all_meta", all_meta)
    add("batched_polyline_matching_cost", "class_cost", class_cost="softmax")
    add("batched_polyline_matching_cost", "one_point", lambda o: o.update(pred_lines=_f(B, 4, 1, 2), gt_lines=_f(B, G, 1, 2)))
    add("batched_polyline_matching_cost", "four_dims", lambda o: o.update(pred_lines=_f(B, 4, 5, 4), gt_lines=_f(B, G, 5, 4)))

    # calls whose spoilt argument is not one of the operands above
    direct = {
        "visible_bbox_mask/bboxes_no_ragged": lambda: visible_bbox_mask(_f(B, G, 4), _f(B, G), image_hw=(64, 64)),
        "visible_bbox_mask/depths_ragged.float64": lambda: visible_bbox_mask(Rag(_f(B, G, 4), _i(B)), Rag(_f(B, G).double(), _i(B)),
                                                                             image_hw=(64, 64)),
        "camera_augment_boxes/bboxes_no_ragged": lambda: camera_augment_boxes(_f(B, G, 4), _f(B, 2, 3), image_hw=(64, 64)),
        "camera_augment_boxes/bboxes_tensor_none": lambda: camera_augment_boxes(Rag(None, _i(B)), _f(B, 2, 3), image_hw=(64, 64),
                                                                                check_occlusion=False),
        "camera_augment_boxes/transforms_none": lambda: camera_augment_boxes(Rag(_f(B, G, 4), _i(B)), None, image_hw=(64, 64),
                                                                             check_occlusion=False),
        "boxes_to_heatmap/bboxes_no_ragged": lambda: boxes_to_heatmap(_f(B, G, 4), image_hw=(64, 64), heatmap_hw=(4, 4),
                                                                      use_per_category_heatmap=False),
        "boxes_to_heatmap/categories_unused": lambda: boxes_to_heatmap(Rag(_f(B, G, 4), _i(B)), image_hw=(64, 64), heatmap_hw=(4, 4),
                                                                       use_per_category_heatmap=False, categories=_i(B, G)),
        "bev_augment_boxes/boxes_no_ragged": lambda: bev_augment_boxes(_f(B, G, 7), _f(B, 7)),
        "bev_augment_boxes/params_none": lambda: bev_augment_boxes(Rag(_f(B, G, 7), _i(B)), None),
        "bev_augment_boxes/point_transforms_too_many": lambda: bev_augment_boxes(Rag(_f(B, G, 7), _i(B)), _f(B, 7),
                                                                                 point_transforms=(_f(B, 1, 4, 4),) * 5),
        "bev_augment_boxes/frame_transforms_no_sequence": lambda: bev_augment_boxes(Rag(_f(B, G, 7), _i(B)), _f(B, 7),
                                                                                    frame_transforms=_f(B, 1, 4, 4)),
        "center_point_targets/boxes_no_ragged": lambda: center_point_targets(_f(B, G, 7), _i(B, G), [[0]], pc_range=(0, 0),
                                                                             voxel_size=(1, 1), out_size_factor=1, grid_size=(4, 4)),
        "center_point_targets/labels_none": lambda: center_point_targets(Rag(_f(B, G, 7), _i(B)), None, [[0]], pc_range=(0, 0),
                                                                         voxel_size=(1, 1), out_size_factor=1, grid_size=(4, 4)),
        "center_point_decode/peaks_count": lambda: center_point_decode([], [], [[0]], pc_range=(0, 0), voxel_size=(1, 1),
                                                                       out_size_factor=1),
        "center_point_decode/peaks_no_peaks": lambda: center_point_decode([_f(B, 4)], [_f(B, 8, 4, 4)], [[0]], pc_range=(0, 0),
                                                                          voxel_size=(1, 1), out_size_factor=1),
        "gather_at_centers/feats_no_tensor": lambda: gather_at_centers("maps", _i(B, G)),
        "gather_at_centers/feats_empty": lambda: gather_at_centers([], _i(B, G)),
        "gather_at_centers/feats_too_many": lambda: gather_at_centers([_f(B, 1, 4, 4)] * 9, _i(B, G)),
        "gather_at_centers/feats_entry_no_tensor": lambda: gather_at_centers([[1.0]], _i(B, G)),
        "gather_at_centers/feats_cpu": lambda: gather_at_centers(_f(B, 2, 4, 4), _i(B, G)),
        "gather_at_centers/feats_meta": lambda: gather_at_centers(_f(B, 2, 4, 4).to("meta"), _i(B, G)),
        "gather_at_centers/feats_cpu+where_no_tensor": lambda: gather_at_centers(_f(B, 2, 4, 4), "where"),
        "gather_at_centers/feats_too_many+where_no_tensor": lambda: gather_at_centers([_f(B, 1, 4, 4)] * 9, "where"),
        "gather_at_centers/feats_entry_no_tensor+feats_too_many": lambda: gather_at_centers([[1.0]] * 9, _i(B, G)),
        "gather_at_centers/feats_meta+feats_three_dims": lambda: gather_at_centers(_f(B, 4, 4).to("meta"), _i(B, G)),
        "center_regression_loss/feats_no_tensor": lambda: center_regression_loss(None, Rag(_i(B, G, 2), _i(B)), _f(B, G, 2)),
        "center_regression_loss/feats_cpu": lambda: center_regression_loss(_f(B, 2, 4, 4), Rag(_i(B, G, 2), _i(B)), _f(B, G, 2)),
        "center_regression_loss/feats_cpu+kind": lambda: center_regression_loss([_f(B, 2, 4, 4)], Rag(_i(B, G, 2), _i(B)),
                                                                                _f(B, G, 2), kind="l2"),
        "center_regression_loss/feats_too_many+centers_no_ragged": lambda: center_regression_loss([_f(B, 1, 4, 4)] * 9, _i(B, G, 2),
                                                                                                  _f(B, G, 2)),
        "center_regression_loss/feats_cpu+targets_no_tensor": lambda: center_regression_loss(_f(B, 2, 4, 4), Rag(_i(B, G, 2), _i(B)),
                                                                                             "targets"),
        "center_regression_loss/feats_no_tensor+kind": lambda: center_regression_loss(None, Rag(_i(B, G, 2), _i(B)), _f(B, G, 2),
                                                                                      kind="l2"),
        "rotated_iou_bev/boxes_no_ragged": lambda: rotated_iou_bev(_f(B, G, 5), _f(B, G, 5)),
        "rotated_nms_bev/detections_no_sequence": lambda: rotated_nms_bev(_f(B, G, 7), 0.5),
        "rotated_nms_bev/member_no_ragged": lambda: rotated_nms_bev([(_f(B, G, 7), _f(B, G), _i(B, G), _i(B, G))], 0.5),
        "rotated_nms_bev/sizes_not_shared": lambda: rotated_nms_bev((Rag(_f(B, G, 7), _i(B)), Rag(_f(B, G), _i(B)), Rag(_i(B, G), _i(B)),
                                                                     Rag(_i(B, G, dtype=torch.int32), _i(B))), 0.5),
        "batched_matching_cost/labels_no_ragged": lambda: batched_matching_cost(_f(B, 4, 3), _i(B, G)),
        "batched_matching_cost/no_predictions": lambda: batched_matching_cost(None, RaggedBatch(_i(B, G), sample_sizes=_i(B)),
                                                                              class_weight=0.0),
        "batched_linear_sum_assignment/cost_no_tensor": lambda: batched_linear_sum_assignment([[1.0]]),
        "batched_linear_sum_assignment/cost_one_dim": lambda: batched_linear_sum_assignment(_f(4)),
        "batched_linear_sum_assignment/cost_int": lambda: batched_linear_sum_assignment(_i(B, G, G)),
        "batched_linear_sum_assignment/cost_no_tensor+threads": lambda: batched_linear_sum_assignment([[1.0]], _threads=128),
        "batched_linear_sum_assignment/cost_one_dim+threads": lambda: batched_linear_sum_assignment(_f(4), _threads=128),
        "batched_linear_sum_assignment/cost_int+too_large": lambda: batched_linear_sum_assignment(
            torch.zeros((B, 1, 4097), dtype=torch.int64).expand(B, 1025, 4097)),
        "batched_linear_sum_assignment/threads+too_large": lambda: batched_linear_sum_assignment(
            torch.zeros((B, 1, 4097)).expand(B, 1025, 4097), _threads=128),
        "batched_polyline_matching_cost/lines_none": lambda: batched_polyline_matching_cost(None, None),
        "batched_polyline_matching_cost/gt_no_ragged": lambda: batched_polyline_matching_cost(_f(B, 4, 5, 2), _f(B, G, 5, 2)),
    }
    return out + [(k, (lambda fn=fn: fn)) for k, fn in direct.items()]


# legal there, so no case: a strided plane or prediction, sizes and a cost of any dtype (they are converted), an extra
# channel or box column inside the limits; and a meta sample_sizes that torch itself refuses to convert
ACCEPTED = {
    "center_point_decode/feats.shape", "rotated_nms_bev/boxes.shape",
    "nv12_to_rgb/y.noncontig", "nv12_to_rgb/uv.noncontig", "prepare_images_nv12/y.noncontig", "prepare_images_nv12/uv.noncontig",
    "batched_matching_cost/pred_scores.noncontig", "batched_matching_cost/pred_scores.shape",
    "batched_matching_cost/gt_labels.noncontig", "batched_matching_cost/pred_boxes.noncontig",
    "batched_matching_cost/gt_boxes.noncontig", "batched_matching_cost/sample_sizes.noncontig",
    "batched_matching_cost/sample_sizes.float32", "batched_matching_cost/sample_sizes.int16",
    "batched_matching_cost/sample_sizes.meta",
    "batched_linear_sum_assignment/cost.noncontig", "batched_linear_sum_assignment/cost.float64",
    "batched_linear_sum_assignment/cost.shape", "batched_linear_sum_assignment/sample_sizes.noncontig",
    "batched_linear_sum_assignment/sample_sizes.float32", "batched_linear_sum_assignment/sample_sizes.int16",
    "batched_linear_sum_assignment/sample_sizes.meta",
    "batched_polyline_matching_cost/pred_lines.noncontig", "batched_polyline_matching_cost/gt_lines.noncontig",
    "batched_polyline_matching_cost/pred_scores.noncontig", "batched_polyline_matching_cost/pred_scores.shape",
    "batched_polyline_matching_cost/gt_labels.noncontig", "batched_polyline_matching_cost/gt_closed.noncontig",
    "batched_polyline_matching_cost/sample_sizes.noncontig", "batched_polyline_matching_cost/sample_sizes.float32",
    "batched_polyline_matching_cost/sample_sizes.int16",
}


def _spoil(o, spec):
    for part in spec.split("+"):
        operand, fault = part.split(".")
        o[operand] = FAULTS[fault](o[operand])


def cases():
    """id -> zero-argument callable that makes the refused call.  A case whose inputs cannot be built (a real RaggedBatch
    that its own constructor refuses with the spoilt tensor) is left out, the same at every commit."""
    out = {}
    specs = []
    for entry, (ops, build, faults) in ENTRIES.items():
        specs += [(entry, f"{operand}.{fault}") for operand, names in faults.items() for fault in names]
        specs += [(entry, spec) for spec in PAIRS[entry]]
    for entry, spec in specs:
        if f"{entry}/{spec}" in ACCEPTED:
            continue
        ops, build, _ = ENTRIES[entry]
        o = ops()
        try:
            _spoil(o, spec)
            out[f"{entry}/{spec}"] = build(o)
        except (AssertionError, AttributeError):   # the RaggedBatch constructor: no tensor, or sizes of another batch shape
            continue
    for key, make in _extras():
        out[key] = make()
    return out


def outcome(call):
    """[exception type name, message] of a case; a call that is not refused gives ["", ""]"""
    try:
        call()
    except Exception as e:   # noqa: BLE001 - the type is what is recorded
        return [type(e).__name__, str(e)]
    return ["", ""]
