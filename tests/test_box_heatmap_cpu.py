"""boxes_to_heatmap without a GPU: every case of box_heatmap_cases.py and the reference's own test through the library's host
entry against the numpy oracle (per-object outputs bit for bit, the map to 1e-5 x max(1, max k), zeros outside every patch),
the argument rules of the Python layer, and the export."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_heatmap_cases as bc  # noqa: E402

import accvlab.draw_heatmap as dh  # noqa: E402
from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import BoxHeatmapTargets, boxes_to_heatmap  # noqa: E402
from accvlab.draw_heatmap.box_heatmap import MAX_BOXES, MAX_CATEGORIES  # noqa: E402

op = boxes_to_heatmap
REFERENCE, GOLDEN = bc.reference_cases()


def test_exported():
    assert "boxes_to_heatmap" in dh.__all__ and "BoxHeatmapTargets" in dh.__all__
    assert (MAX_BOXES, MAX_CATEGORIES) == (256, 128) and (bc.TW, bc.TH) == (64, 16)
    assert BoxHeatmapTargets._fields == ("heatmap", "is_active", "center", "center_offset", "height_width", "bboxes_heatmap",
                                         "radii")


@pytest.mark.parametrize("name", bc.case_names())
def test_case_against_the_oracle(name):
    """`out=` arrives full of NaN: every element of the map must be written"""
    case = bc.cases()[name]
    want = bc.oracle(case)
    out = torch.full(want["heatmap"].shape, float("nan"))
    got = bc.run(op, case, "cpu", out=out)
    assert got.heatmap is out
    bc.check(got, case)


@pytest.mark.parametrize("case", REFERENCE, ids=repr)
def test_reference_test_vector(case):
    """the flags the reference's test expects pin the oracle, the oracle pins the library"""
    expected = GOLDEN["expected_is_active"]
    for s in GOLDEN["single_heatmap"]:
        if case.name == "reference_single_" + s["id"]:
            expected = s["expected_is_active"]
    assert bc.oracle(case)["is_active"][0].tolist() == expected
    got = bc.run(op, case, "cpu")
    assert got.is_active.tensor[0].tolist() == expected
    bc.check(got, case)
    # object 4: a given centre lies outside its box, the radius is the minimum and the object is drawn
    assert float(got.radii.tensor[0, 4]) == (0.5 if "centers" in case.frames[0] else 5.0)
    cx, cy = got.center.tensor[0, 4].tolist()
    hm = got.heatmap[0, 0] if got.heatmap.dim() == 4 else got.heatmap[0]
    assert float(hm[cy, cx]) == 1.0


def test_cases_show_what_they_are_named_after():
    o = {n: bc.oracle(c) for n, c in bc.cases().items() if not n.startswith(("sweep", "shape"))}
    assert set(np.unique(o["tile_edges"]["radii"]).tolist()) == {0.5, 2.5, 10.0} and o["tile_edges"]["is_active"].all()
    assert o["map_corners"]["center"][0].tolist() == [[0, 0], [bc.TW, 0], [0, bc.TH], [bc.TW, bc.TH]]
    assert [o[f"fraction_threshold_{t}"]["is_active"][0, 0] for t in ("at", "above", "below")] == [True, False, True]
    assert [o[f"size_minimum_{t}"]["is_active"][0].tolist() for t in ("at", "h_one_ulp_below", "w_one_ulp_below")] == \
        [[True, True], [False, False], [False, False]]
    assert o["category_range_int64"]["is_active"][0].tolist() == [False, False, False, False, True, True]
    assert o["category_range_int32"]["is_active"][0].tolist() == [False, False, True, False]
    assert not o["is_valid_all_false"]["is_active"].any() and not o["is_valid_all_false"]["heatmap"].any()
    assert o["centre_outside_its_box"]["is_active"].all() and (o["centre_outside_its_box"]["radii"] == 1.5).all()
    assert o["zero_area_boxes"]["is_active"][0].tolist() == [False, False, False, True]
    bad = o["non_finite_box_and_centre"]
    assert bad["is_active"][0].tolist() == [False] * 8 + [True]
    assert not bad["bboxes_heatmap"][0, :7].any() and not bad["radii"][0, :7].any() and not bad["center"][0, :7].any()
    # 3e38 stays finite at scale 0.5: the object keeps its outputs, and its area fraction of 0 switches it off
    assert bad["bboxes_heatmap"][0, 7].tolist() == [47.0, 2.0, 10.0, 6.0] and bad["radii"][0, 7] == 0.5
    hw = o["image_hw_per_frame_int32"]["is_active"]
    assert hw[0].any() and hw[1].any() and not hw[2].any() and not hw[3].any() and hw[4].any()
    assert not o["image_hw_negative_and_huge"]["is_active"][0].any()
    # the far object of the overlap wins pixels of the near one, and the near one wins others
    pair = bc.cases()["overlap_and_same_pixel"]
    hm = o["overlap_and_same_pixel"]["heatmap"][0, 0]
    alone = lambda i: bc._oracle(bc.Case("alone", [dict(boxes=pair.frames[0]["boxes"][i:i + 1], cats=[0])], pair.image_hw[0],   # noqa: E731
                                         pair.heatmap_hw, **pair.kw))["heatmap"][0, 0]
    near, far = alone(0), alone(1)
    both = (near > 0) & (far > 0)
    assert (near > far)[both].any() and (far > near)[both].any() and np.array_equal(hm[both], np.maximum(near, far)[both])


def test_results_share_the_sample_sizes_and_padding_is_zero():
    case = bc.cases()["sizes_0_1_G_in_one_batch"]
    bboxes, kw = bc.batch(case, "cpu")
    got = op(bboxes, **kw)
    assert got.heatmap.shape == (3, 2, bc.TH + 1, bc.TW + 1) and got.heatmap.dtype == torch.float32
    for r, dt, tail in zip(got[1:], (torch.bool, torch.int32) + (torch.float32,) * 4, ((), (2,), (2,), (2,), (4,), ())):
        assert isinstance(r, RaggedBatch) and r.sample_sizes is bboxes.sample_sizes
        assert r.tensor.dtype == dt and r.tensor.shape == (3, 9) + tail
        assert not r.tensor[0].any() and not r.tensor[1, 1:].any()


def _args(G=3, device="cpu", **kw):
    sizes = torch.tensor([G], dtype=torch.int64, device=device)
    boxes = RaggedBatch(torch.zeros((1, G, 4), device=device), sample_sizes=sizes)
    base = dict(image_hw=(32, 32), heatmap_hw=(16, 16), categories=torch.zeros((1, G), dtype=torch.int32, device=device),
                num_categories=2)
    base.update(kw)
    return boxes, {k: v for k, v in base.items() if v is not ...}


@pytest.mark.parametrize("kw, exc, match", [
    (dict(categories=...), RuntimeError, "categories must be given"),
    (dict(num_categories=...), RuntimeError, "num_categories must be a positive"),
    (dict(num_categories=0), RuntimeError, "num_categories must be a positive"),
    (dict(num_categories=MAX_CATEGORIES + 1), RuntimeError, "MAX_CATEGORIES"),
    (dict(num_categories=..., use_per_category_heatmap=False), RuntimeError, "nothing uses them"),
    (dict(categories=..., num_categories=..., use_per_category_heatmap=False, per_category_min_object_sizes=[(1, 1)]),
     RuntimeError, "categories must be given"),
    (dict(min_object_size=(1, 1), per_category_min_object_sizes=[(1, 1), (2, 2)]), RuntimeError, "exclude each other"),
    (dict(per_category_min_object_sizes=[(1, 1)]), RuntimeError, "must hold num_categories = 2 pairs"),
    (dict(per_category_min_object_sizes=[(1, 1), (2,)]), RuntimeError, "pair"),
    (dict(min_object_size=3.0), RuntimeError, "pair"),
    (dict(heatmap_hw=(0, 16)), RuntimeError, "heatmap_hw"),
    (dict(heatmap_hw=(16.0, 16)), RuntimeError, "heatmap_hw"),
    (dict(image_hw=(32.0, 32)), RuntimeError, "image_hw"),
    (dict(image_hw=torch.zeros((2, 2), dtype=torch.int32)), RuntimeError, "image_hw tensor"),
    (dict(image_hw=torch.zeros((1, 2))), RuntimeError, "image_hw tensor"),
    (dict(max_radius=0.0), RuntimeError, "max_radius"),
    (dict(max_radius=float("inf")), RuntimeError, "max_radius"),
    (dict(min_radius=float("nan")), RuntimeError, "min_radius"),
    (dict(radius_to_sigma_factor=0.0), RuntimeError, "radius_to_sigma_factor"),
    (dict(k_for_classes=[1.0]), RuntimeError, "k_for_classes must hold 2"),
    (dict(k_for_classes=[1.0, float("nan")]), RuntimeError, "k_for_classes"),
    (dict(categories=torch.zeros((1, 3))), RuntimeError, "categories must be int32 or int64"),
    (dict(categories=torch.zeros((1, 4), dtype=torch.int32)), RuntimeError, "categories must be int32 or int64"),
    (dict(centers=torch.zeros((1, 3, 2), dtype=torch.float64)), TypeError, "centers must be float32"),
    (dict(centers=torch.zeros((1, 3, 3))), RuntimeError, "centers must be float32"),
    (dict(centers=torch.zeros((1, 3, 4))[..., :2]), RuntimeError, "centers must be contiguous"),
    (dict(is_valid=torch.zeros((1, 3), dtype=torch.uint8)), RuntimeError, "is_valid must be bool"),
    (dict(out=torch.zeros((1, 2, 16, 16), dtype=torch.float16)), TypeError, "out must be float32"),
    (dict(out=torch.zeros((1, 16, 16))), RuntimeError, "out must be float32"),
    (dict(out=torch.zeros((1, 2, 16, 32))[..., ::2]), RuntimeError, "out must be contiguous"),
])
def test_argument_rules(kw, exc, match):
    boxes, kw = _args(**kw)
    with pytest.raises(exc, match="boxes_to_heatmap.*" + match):
        op(boxes, **kw)


def test_bboxes_rules_and_the_box_limit():
    boxes, kw = _args()
    with pytest.raises(RuntimeError, match="boxes_to_heatmap: bboxes must be a RaggedBatch"):
        op(boxes.tensor, **kw)
    with pytest.raises(TypeError, match="boxes_to_heatmap: bboxes must be float32"):
        op(RaggedBatch(boxes.tensor.double(), sample_sizes=boxes.sample_sizes), **kw)
    with pytest.raises(RuntimeError, match="boxes_to_heatmap: bboxes must be float32 \\[B, G_max, 4\\]"):
        op(RaggedBatch(torch.zeros((1, 3, 5)), sample_sizes=boxes.sample_sizes), **kw)
    with pytest.raises(RuntimeError, match="boxes_to_heatmap: sample_sizes must be int32 or int64"):
        op(RaggedBatch(boxes.tensor, sample_sizes=torch.zeros(1, dtype=torch.int16)), **kw)
    big, kw = _args(G=MAX_BOXES + 1)
    with pytest.raises(RuntimeError, match="boxes_to_heatmap.*MAX_BOXES"):
        op(big, **kw)
    full, kw = _args(G=MAX_BOXES)
    assert op(full, **kw).is_active.tensor.shape == (1, MAX_BOXES)


def test_no_categories_at_all_and_an_empty_batch():
    boxes, kw = _args(categories=..., num_categories=..., use_per_category_heatmap=False, min_object_size=(1, 1))
    assert op(boxes, **kw).heatmap.shape == (1, 16, 16)
    empty = RaggedBatch(torch.zeros((0, 3, 4)), sample_sizes=torch.zeros(0, dtype=torch.int64))
    got = op(empty, image_hw=(32, 32), heatmap_hw=(16, 16), categories=torch.zeros((0, 3), dtype=torch.int64), num_categories=2)
    assert got.heatmap.shape == (0, 2, 16, 16) and got.center.tensor.shape == (0, 3, 2)
