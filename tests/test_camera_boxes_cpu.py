"""camera_augment_boxes on the CPU: the host entry against the two numpy oracles of camera_boxes_cases.py, the named cases
stage by stage, the argument checks of the Python layer and of the C entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import camera_boxes_cases as cases
import visible_boxes_cases as vb
from camera_boxes_cases import H0, W0, built, check_case, run

DEV = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_entry_equals_the_float32_oracle_and_lies_within_the_bar_of_the_float64_one(name):
    check_case(name, DEV)


def test_the_bars_are_the_rounding_counts_the_header_derives():
    text = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "camera_boxes_arith.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (k\w+Roundings) = (\d+);", text)}
    assert consts == {"kPointRoundings": cases.N_POINT, "kMatrixRoundings": cases.N_MATRIX}


def check_identity_cross_check(device):
    """identity matrix, crop off, no categories: `visible` is visible_bbox_mask of the raw boxes, and the compacted fields
    are select_visible_bboxes"""
    from accvlab.draw_heatmap import camera_augment_boxes, select_visible_bboxes, visible_bbox_mask

    case, _ = built("identity")
    for extra in (dict(), dict(minimum_size=2), dict(shrink_to_int=True), dict(check_occlusion=False, minimum_size=1.5)):
        boxes, transforms, kw = cases.to_torch(case, device, ragged_fields=True)
        kw.update(extra)
        out = camera_augment_boxes(boxes, transforms, **kw)
        vkw = {k: kw[k] for k in ("image_hw", "check_occlusion", "minimum_size", "shrink_to_int")}
        mask = visible_bbox_mask(boxes, kw["depths"], **vkw)
        assert torch.equal(out.visible.tensor, mask.tensor) and torch.equal(out.keep.tensor, mask.tensor)
        m2, b2, d2 = select_visible_bboxes(boxes, kw["depths"], **vkw)
        assert torch.equal(out.bboxes.sample_sizes, b2.sample_sizes.to(torch.int64))
        n = b2.tensor.shape[1]
        assert torch.equal(out.bboxes.tensor[:, :n], b2.tensor) and torch.equal(out.depths.tensor[:, :n], d2.tensor)
        assert not bool(out.bboxes.tensor[:, n:].any()) and bool((out.source.tensor[:, n:] == -1).all())
    assert int(mask.tensor.sum()) > 20


def test_identity_cross_check_with_the_existing_operators():
    check_identity_cross_check(DEV)


def test_horizontal_flip_keeps_the_hidden_box_hidden_and_leaves_x1_above_x2():
    case, a = built("flip")
    got = run(case, DEV)
    assert got["visible"][0].tolist() == [False, True, True, True] and got["sizes"].tolist() == [3]
    kept = got["bboxes"][0, :3]
    assert kept[0].tolist() == [W0 - 8.0, 8.0, W0 - 32.0, 32.0] and bool((kept[:2, 0] > kept[:2, 2]).all())
    assert kept[2].tolist() == [W0 - 30.5, 20.25, W0 - 20.125, 38.0]          # flipped on input: ordered by the flip
    assert got["centers"][0, 0].tolist() == [W0 - 20.0, 20.0]
    ordered = run(built("flip-ordered")[0], DEV)
    assert torch.equal(ordered["visible"], got["visible"]) and torch.equal(ordered["source"], got["source"])
    ob = ordered["bboxes"][0, :3]
    assert bool((ob[:, 0] <= ob[:, 2]).all()) and bool((ob[:, 1] <= ob[:, 3]).all())
    assert ob[0].tolist() == [W0 - 32.0, 8.0, W0 - 8.0, 32.0]
    assert torch.equal(ordered["centers"], got["centers"])


def test_warp_moves_boxes_across_the_image_border():
    case, a = built("border")
    got = run(case, DEV)
    assert got["visible"][0].tolist() == [False, True, True, False, True]
    assert got["source"][0].tolist() == [1, 2, 4, -1, -1]
    assert got["bboxes"][0, 0].tolist() == [0.0, 4.0, 10.0, 20.0]             # (-10, 4, 10, 20) cropped to the border
    assert got["bboxes"][0, 1].tolist() == [20.0, 10.0, 40.0, 30.0]
    assert got["bboxes"][0, 2].tolist() == [49.0, 30.5, float(W0), float(H0)]
    assert got["centers"][0, 0].tolist() == [0.0, 12.0]


def test_a_box_that_is_not_kept_still_occludes():
    case, a = built("condition")
    got = run(case, DEV)
    assert got["visible"].tolist() == [[True, False, True], [True, False, True], [True, False, True]]
    assert got["keep"].tolist() == [[False, False, True], [False, False, False], [True, False, True]]
    assert got["sizes"].tolist() == [1, 0, 2] and got["categories"][2, :2].tolist() == [4, 2]


def test_crop_at_the_borders_nan_and_inf():
    got, off = run(built("crop")[0], DEV), run(built("crop-off")[0], DEV)
    b = got["bboxes"]
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))       # noqa: E731
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))    # noqa: E731
    assert b[0, 0].tolist() == [0.0, up(0), down(W0), float(H0)]
    assert b[0, 1].tolist() == [up(0), 0.0, float(W0), float(H0)]
    # a NaN x makes the y of its corner NaN too: 0 * NaN is computed as written
    assert b[0, 2, 0] == 5 and b[0, 2, 1] == down(H0) and bool(b[0, 2, 2:].isnan().all())
    assert bool(b[0, 3].isnan().all()) and got["sizes"].tolist() == [6, 3]
    assert b[0, 5].tolist() == [0.0, 0.0, float(W0), float(H0)]
    assert b[1, 0].tolist() == [0.0, 5.0, float(W0), 7.0] and b[1, 1].tolist() == [float(W0), float(H0), 0.0, 0.0]
    ob = off["bboxes"]
    assert ob[0, 0].tolist() == [down(0), up(0), down(W0), up(W0)] and ob[0, 5].tolist() == [-3.0, -4.0, 100.0, 90.0]
    assert ob[1, 0].tolist() == [-np.inf, 5.0, np.inf, 7.0]
    assert torch.equal(got["keep"], off["keep"])


@pytest.mark.parametrize("name", ["matrices-shapes", "matrices-big"])
def test_rows_2_and_3_of_the_matrices_are_bit_identical_to_the_input(name):
    case, a = built(name)
    got = run(case, DEV)
    for g, m in zip(got["mats"], case.mats):
        assert torch.equal(g[..., 2:, :].contiguous().view(torch.int32), torch.from_numpy(m[..., 2:, :].copy()).view(torch.int32))
    assert max(m[0].size for m in case.mats) > 256 or name != "matrices-big"


@pytest.mark.parametrize("sizes_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("categories_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("valid_dtype,hw_dtype", [(torch.bool, torch.int32), (torch.uint8, torch.int64)])
def test_count_category_valid_and_image_hw_dtypes(valid_dtype, hw_dtype, categories_dtype, sizes_dtype):
    case, a = built("dtypes")
    typed = cases.Case(case.boxes, case.sizes, case.transforms, hw=case.hw, centers=case.centers, depths=case.depths,
                       categories=case.categories, valid=case.valid, mats=case.mats, sizes_dtype=sizes_dtype, **case.kw)
    got = run(typed, DEV, categories_dtype=categories_dtype, valid_dtype=valid_dtype, hw_dtype=hw_dtype)
    assert got["categories"].dtype == categories_dtype
    cases.assert_same(got, a)


def test_optional_fields_as_ragged_batches_and_views_with_a_storage_offset():
    for name in ("dtypes", "partition-G65", "matrices-shapes"):
        case, a = built(name)
        cases.assert_same(run(case, DEV, ragged_fields=True, offset=True), a, name)


def test_neither_check_requested_keeps_every_real_slot():
    case, _ = built("clamped")
    free = cases.Case(case.boxes, case.sizes, case.transforms, categories=None, crop=False)
    got = run(free, DEV)
    assert got["sizes"].tolist() == [70, 0, 41] and got["visible"].sum(1).tolist() == [70, 0, 41]


def check_refusals(device):
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import camera_augment_boxes as op

    case, _ = built("dtypes")
    boxes, t, kw = cases.to_torch(case, device)
    Fr, G = case.boxes.shape[:2]
    rb = lambda x: RaggedBatch(x, sample_sizes=boxes.sample_sizes)   # noqa: E731
    with pytest.raises(TypeError, match="float32"):
        op(rb(boxes.tensor.double()), t, **kw)
    with pytest.raises(TypeError, match="float32"):
        op(boxes, t, **{**kw, "depths": kw["depths"].double()})
    wrong = [
        lambda: op(boxes.tensor, t, **kw),                                                      # not a RaggedBatch
        lambda: op(rb(boxes.tensor[..., :3].contiguous()), t, **kw),                            # wrong shapes
        lambda: op(boxes, t[:, :, :2].contiguous(), **kw),
        lambda: op(boxes, t, **{**kw, "centers": kw["centers"][:, :, :1].contiguous()}),
        lambda: op(boxes, t, **{**kw, "categories": kw["categories"][:, :-1].contiguous()}),
        lambda: op(boxes, t, **{**kw, "valid": kw["valid"].to(torch.int32)}),
        lambda: op(boxes, t, **{**kw, "categories": kw["categories"].to(torch.int16)}),
        lambda: op(boxes, t, **{**kw, "image_hw": (40.0, 56)}),
        lambda: op(boxes, t, **{**kw, "image_hw": kw["image_hw"][:, :1].contiguous()}),
        lambda: op(boxes, t, **{**kw, "depths": None}),                                         # occlusion without depths
        lambda: op(boxes, t, **{**kw, "minimum_size": "2"}),
        lambda: op(boxes, t, **{**kw, "projection_matrices": [torch.zeros((Fr, 4, 4), device=device)] * 5}),
        lambda: op(boxes, t, **{**kw, "projection_matrices": [torch.zeros((Fr, 2, 4), device=device)]}),
        lambda: op(boxes, t, **{**kw, "projection_matrices": [torch.zeros((Fr, 4, 4, 2), device=device).transpose(2, 3)]}),
        lambda: op(rb(boxes.tensor.transpose(0, 1).contiguous().transpose(0, 1)), t, **kw),     # non-contiguous
        lambda: op(boxes, t.transpose(1, 2).contiguous().transpose(1, 2), **kw),
    ]
    for i, call in enumerate(wrong):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} was accepted")
    big = RaggedBatch(torch.zeros((1, 257, 4), device=device), sample_sizes=torch.tensor([3], device=device))
    with pytest.raises(RuntimeError, match="257"):
        op(big, torch.zeros((1, 2, 3), device=device), image_hw=(10, 10), check_occlusion=False)


def test_wrong_dtypes_shapes_and_layouts_are_refused():
    check_refusals(DEV)


def check_c_entry_refusals(device):
    """the C entries' own checks: each returns ACCV_EINVAL and leaves a message"""
    from accvlab import _amd_native as nat

    case, _ = built("dtypes")
    base, p, out, keepalive = cases.c_entry_args(case, device)
    assert cases.call_c_entry(list(base), device) == 0

    def refused(change, params=None):
        args = list(base)
        for k, v in change.items():
            args[k] = v
        if params is not None:
            args[10] = ctypes.addressof(params)
        status = cases.call_c_entry(args, device)
        assert status != 0 and nat.ctypes_lib().accv_last_error()

    def variant(**fields):
        q = nat.CameraBoxesParams()
        ctypes.memmove(ctypes.addressof(q), ctypes.addressof(p), ctypes.sizeof(p))
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    refused({10: None})                                  # null params
    refused({0: None})                                   # null boxes
    refused({1: None})                                   # null transforms
    refused({6: None})                                   # null counts
    refused({11: None})                                  # null output
    refused({18: None})                                  # null sizes
    refused({3: None})                                   # occlusion without depths (and depths without their input)
    refused({12: None})                                  # centres without their output
    refused({0: base[0] + 2})                            # misaligned boxes
    refused({18: base[18] + 4})                          # misaligned sizes
    refused({7: base[7] | 64})                           # unknown flag
    refused({8: -1})                                     # negative size
    refused({9: 257})                                    # G above the maximum
    refused({8: 1 << 40})                                # more workgroups than a grid holds
    refused({}, variant(num_matrices=5))
    q = variant()
    q.mat_rows[0] = 2
    refused({}, q)
    q = variant()
    q.mat_in[0] = None
    refused({}, q)
    q = variant()
    q.mat_out[0] = p.mat_out[0] + 1
    refused({}, q)


def test_the_c_entries_check_their_arguments_before_anything_is_read():
    check_c_entry_refusals(DEV)


@pytest.mark.parametrize("name", ["partition-G65", "matrices-big", "dtypes"])
def test_every_output_lies_between_guard_bands_through_the_host_entry(name):
    cases.check_guard_bands(name, DEV)


def test_boxes_to_heatmap_takes_the_result_as_is():
    from accvlab.draw_heatmap import boxes_to_heatmap, camera_augment_boxes

    case, a = built("sweep-1")
    boxes, t, kw = cases.to_torch(case, DEV)
    out = camera_augment_boxes(boxes, t, **kw)
    maps = boxes_to_heatmap(out.bboxes, centers=out.centers, categories=out.categories, image_hw=kw["image_hw"],
                            heatmap_hw=(16, 44), num_categories=10)
    assert int(maps.is_active.tensor.sum()) > 5
