"""query_box_decode_3d and query_box_decode_2d on CPU tensors: the library's host entries against the per-rank float32
definitions of query_decode_cases.py on every input class, the margin condition of the cases, every argument check, B == 0."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import query_decode_cases as qc  # noqa: E402
from query_decode_cases import HW, KINDS, RANGE, THR, check, definition_2d, definition_3d, logits, matrices, max_nums, rows_2d, rows_3d, run  # noqa: E402

import accvlab.draw_heatmap as dh  # noqa: E402
from accvlab.draw_heatmap import (BoxDetections, CenterPointDetections, nms_boxes, query_box_decode_2d, query_box_decode_3d,  # noqa: E402
                                  rotated_nms_bev)

op3, op2 = query_box_decode_3d, query_box_decode_2d
FULL3 = dict(score_threshold=THR, post_center_range=RANGE)


def test_exports():
    for name in ("query_box_decode_3d", "query_box_decode_2d"):
        assert name in dh.__all__ and hasattr(dh, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q,C", [(1, 1), (21, 3), (13, 10), (103, 80), (1025, 1)])
def test_host_entry_equals_the_3d_definition(Q, C, kind):
    cls, rows = logits(3, Q, C, kind, seed=Q), rows_3d(3, Q, 10 if C % 2 else 8, seed=C, special=kind == "special")
    for M in max_nums(Q * C):
        for kw in (FULL3, dict(), dict(scores_are_logits=False, score_threshold=-0.6, bottom_center=True)):
            got, want = run(op3, definition_3d, cls, rows, M, **kw)
            check(got, want, f"{kind} Q={Q} C={C} M={M} {sorted(kw)}")
            assert isinstance(got, CenterPointDetections) and got.boxes.tensor.shape == (3, M, rows.shape[2] - 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("box_format,normalized", [("cxcywh", True), ("xyxy", True), ("cxcywh", False), ("xyxy", False)])
def test_host_entry_equals_the_2d_definition(box_format, normalized, kind):
    B, Q, C = 4, 47, 10
    cls = logits(B, Q, C, kind, seed=3)
    rows = rows_2d(B, Q, box_format, normalized, seed=5, special=kind == "special")
    hw_t = torch.tensor([[96, 160], [64, 64], [33, 1000], [0, 7]], dtype=torch.int64 if normalized else torch.int32)
    mats = matrices(B, seed=1, singular=(2,))
    for M in (1, 65, Q * C):
        for kw in (dict(image_hw=HW), dict(image_hw=hw_t, image_matrices=mats, score_threshold=THR, order_corners=False),
                   dict(image_hw=hw_t, image_matrices=mats, clip=False), dict(image_hw=HW, scores_are_logits=False, score_threshold=-0.6)):
            got, want = run(op2, definition_2d, cls, rows, M, box_format=box_format, normalized=normalized, **kw)
            check(got, want, f"{kind} {box_format} normalized={normalized} M={M} {sorted(kw)}")
            assert isinstance(got, BoxDetections)
    got, want = run(op2, definition_2d, cls, rows, 65, box_format=box_format, normalized=normalized, image_hw=hw_t, image_matrices=mats)
    assert want["sizes"][2] > 0 and not got.boxes.tensor[2].any(), "a singular matrix: zero boxes, the count kept"


@pytest.mark.parametrize("dtype,row_dtype", [(torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)])
def test_half_precision_scores_and_rows(dtype, row_dtype):
    for kind in ("distinct", "special"):
        cls = logits(2, 60, 10, kind, dtype=dtype, seed=8)
        got, want = run(op3, definition_3d, cls, rows_3d(2, 60, 10, dtype=row_dtype, seed=2), 100, bottom_center=True, **FULL3)
        check(got, want, f"3d {dtype} {row_dtype} {kind}")
        got, want = run(op2, definition_2d, cls, rows_2d(2, 60, dtype=row_dtype, seed=2), 100, image_hw=HW, score_threshold=THR)
        check(got, want, f"2d {dtype} {row_dtype} {kind}")
        if kind == "distinct" and dtype != torch.float32:
            assert len(np.unique(qc._np32(cls))) < cls.numel(), "the cast leaves no tie: the case shows nothing about them"


def test_raw_half_precision_scores_keep_the_sign_and_payload_of_a_nan():
    qc.check_raw_half_nan(op3, op2, "cpu")


def test_the_cut_falls_inside_a_tie_group_and_equal_logits_come_in_index_order():
    cls = logits(2, 50, 10, "two", seed=4)
    high = int((cls[0] > 0).sum())
    assert 0 < high - 20 and high + 20 < 500
    for M in (high - 20, high + 20):
        got, want = run(op3, definition_3d, cls, rows_3d(2, 50), M)
        check(got, want, f"two-valued M={M}")
    flat = (got.source.tensor.long() * 10 + got.labels.tensor)[0]
    assert torch.equal(flat[:high], torch.nonzero(cls[0].view(-1) > 0).view(-1)) and bool((flat[high:].diff() > 0).all())
    got, _ = run(op3, definition_3d, logits(1, 70, 3, "equal"), rows_3d(1, 70), 65)
    assert torch.equal(got.source.tensor[0].long() * 3 + got.labels.tensor[0], torch.arange(65))


def test_saturated_logits_rank_by_logit_then_index():
    cls = logits(1, 40, 10, "saturated", seed=6)
    got, want = run(op3, definition_3d, cls, rows_3d(1, 40), 30)
    check(got, want, "saturated")
    assert int((got.scores.tensor[0] == 1.0).sum()) >= 20, "float32 sigmoid saturates: equal scores"
    picked = cls.view(-1)[got.source.tensor[0].long() * 10 + got.labels.tensor[0]]
    assert bool((picked.diff() < 0).all()), "the logits, not the saturated scores, give the order"


def test_centres_on_every_face_of_the_range_are_kept_and_one_ulp_outside_dropped():
    Q = 12
    cls = torch.linspace(3.0, -3.0, Q).view(1, Q, 1).contiguous()
    rows = rows_3d(1, Q, 8, seed=1)
    rows[0, :, 0], rows[0, :, 1], rows[0, :, 4] = 1.0, -2.0, 0.5
    outside = lambda v, up: float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))   # noqa: E731
    for n, (col, lo, hi) in enumerate(((0, RANGE[0], RANGE[3]), (1, RANGE[1], RANGE[4]), (4, RANGE[2], RANGE[5]))):
        rows[0, 4 * n, col], rows[0, 4 * n + 1, col] = lo, hi
        rows[0, 4 * n + 2, col], rows[0, 4 * n + 3, col] = outside(lo, False), outside(hi, True)
    got, want = run(op3, definition_3d, cls, rows, Q, post_center_range=RANGE)
    check(got, want, "faces")
    assert got.source.tensor[0, :6].tolist() == [0, 1, 4, 5, 8, 9] and int(got.boxes.sample_sizes[0]) == 6


def test_frames_with_no_valid_row_and_with_every_row_valid():
    cls = logits(3, 30, 10, seed=2)
    cls[0] -= 20.0
    cls[2] += 20.0
    rows = rows_3d(3, 30, seed=2)
    got, want = run(op3, definition_3d, cls, rows, 300, score_threshold=THR)
    check(got, want, "none / some / all")
    sizes = got.boxes.sample_sizes.tolist()
    assert sizes[0] == 0 and 0 < sizes[1] < 300 and sizes[2] == 300 and bool((got.source.tensor[0] == -1).all())


def test_the_nms_operators_take_the_results_unchanged():
    cls = logits(2, 80, 10, seed=9)
    d3 = op3(cls, rows_3d(2, 80), 100, **FULL3)
    out = rotated_nms_bev(d3, None)[0]
    d2 = op2(cls, rows_2d(2, 80), 100, image_hw=HW, score_threshold=THR)
    for a, b in ((d3, out), (d2, nms_boxes(d2, None))):
        for x, y in zip(a, b):
            assert torch.equal(x.tensor.view(torch.uint8), y.tensor.view(torch.uint8)) and torch.equal(x.sample_sizes, y.sample_sizes)
    assert int(rotated_nms_bev(d3, 0.1)[0].boxes.sample_sizes.sum()) <= int(d3.boxes.sample_sizes.sum())
    assert int(nms_boxes(d2, 0.3).boxes.sample_sizes.sum()) < int(d2.boxes.sample_sizes.sum())


def test_the_margin_condition_holds_for_every_generated_case():
    for kind in KINDS:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            x = logits(2, 500, 10, kind, dtype=dtype, seed=11).double()
            gap = (torch.sigmoid(x[~x.isnan()]) - THR).abs().min()
            assert gap > qc.MARGIN, f"{kind} {dtype}: {gap:.2e}"
    with pytest.raises(AssertionError, match="from the threshold"):
        qc.assert_margin(dict(logits=True, all_scores=[THR + 0.5 * qc.MARGIN]), THR)


@pytest.mark.parametrize("B", [0])
def test_an_empty_batch_gives_empty_outputs(B):
    d3 = op3(torch.zeros((B, 9, 4)), torch.zeros((B, 9, 10)), 7, **FULL3)
    assert d3.boxes.tensor.shape == (0, 7, 9) and d3.scores.tensor.shape == (0, 7) and d3.boxes.sample_sizes.shape == (0,)
    d2 = op2(torch.zeros((B, 9, 4)), torch.zeros((B, 9, 4)), 7, image_hw=HW)
    assert d2.boxes.tensor.shape == (0, 7, 4) and d2.extras.tensor.shape == (0, 7, 0) and d2.source.tensor.dtype == torch.int32


def test_argument_errors():
    cls, r3, r2 = torch.zeros((2, 9, 4)), torch.zeros((2, 9, 10)), torch.zeros((2, 9, 4))
    bad3 = [
        (dict(cls_scores=cls[:, :, ::2]), "cls_scores must be contiguous"),
        (dict(cls_scores=cls.double()), "cls_scores must be float32, float16 or bfloat16"),
        (dict(cls_scores=cls[0]), r"cls_scores must be \[B, Q, C\]"),
        (dict(bbox_preds=torch.zeros((2, 8, 10))), r"bbox_preds must be \[2, 9, D\] like cls_scores"),
        (dict(bbox_preds=torch.zeros((2, 9, 9))), "bbox_preds must hold 8 or 10 values per query, got 9"),
        (dict(bbox_preds=r3.tolist()), "bbox_preds must be a tensor"),
        (dict(max_num=0), r"max_num must be an integer in 1\.\.1024, got 0"),
        (dict(max_num=1025), r"max_num must be an integer in 1\.\.1024, got 1025"),
        (dict(max_num=True), "max_num must be an integer"),
        (dict(max_num=37), "max_num = 37 exceeds Q \\* C = 36"),
        (dict(score_threshold=float("nan")), "score_threshold must not be NaN"),
        (dict(score_threshold="0.3"), "score_threshold must be a Python number"),
        (dict(post_center_range=RANGE[:5]), "post_center_range must be a sequence of 6 numbers"),
        (dict(post_center_range=RANGE[:5] + [float("nan")]), "post_center_range must not hold NaN"),
    ]
    for change, text in bad3:
        kw = dict(cls_scores=cls, bbox_preds=r3, max_num=5)
        kw.update(change)
        with pytest.raises(RuntimeError, match="query_box_decode_3d: " + text):
            op3(kw.pop("cls_scores"), kw.pop("bbox_preds"), kw.pop("max_num"), **kw)
    bad2 = [
        (dict(bbox_preds=r3), "bbox_preds must hold 4 values per query, got 10"),
        (dict(image_hw=(96,)), "image_hw must be"),
        (dict(image_hw=torch.zeros((3, 2), dtype=torch.int32)), r"an image_hw tensor must be int32 or int64 \[2, 2\]"),
        (dict(image_matrices=torch.zeros((2, 3, 3))), r"image_matrices must be float32 \[2, 2, 3\]"),
        (dict(box_format="xywh"), "box_format must be 'cxcywh' or 'xyxy'"),
        (dict(score_threshold=float("nan")), "score_threshold must not be NaN"),
        (dict(max_num=37), "max_num = 37 exceeds"),
    ]
    for change, text in bad2:
        kw = dict(cls_scores=cls, bbox_preds=r2, max_num=5, image_hw=HW)
        kw.update(change)
        with pytest.raises(RuntimeError, match="query_box_decode_2d: " + text):
            op2(kw.pop("cls_scores"), kw.pop("bbox_preds"), kw.pop("max_num"), **kw)


def test_the_c_entries_refuse_what_the_wrapper_cannot_pass():
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    p3, p2 = nat.QueryDecode3dParams(), nat.QueryDecode2dParams()
    d = ctypes.c_void_p(64)
    for entry, args in ((lib.accv_query_decode_3d_cpu, (ctypes.addressof(p3), 2, 9, 4, 10)), (lib.accv_query_decode_2d_cpu, (ctypes.addressof(p2), 2, 9, 4))):
        assert entry(*args, 37, d, d, d, d, d) == -1 and b"exceeds Q * C" in lib.accv_last_error()
        assert entry(*args, 5, d, d, d, d, d) == -1 and b"null input pointer" in lib.accv_last_error()
        assert entry(*args, 5, None, d, d, d, d) == -1 and b"null output pointer" in lib.accv_last_error()
        assert entry(args[0], 0, *args[2:], 5, None, None, None, None, None) == 0
    assert lib.accv_query_decode_3d_cpu(ctypes.addressof(p3), 2, 9, 4, 9, 5, d, d, d, d, d) == -1 and b"D must be 8 or 10" in lib.accv_last_error()
    assert lib.accv_query_decode_3d_cpu(None, 2, 9, 4, 10, 5, d, d, d, d, d) == -1 and b"null params" in lib.accv_last_error()
    assert lib.accv_query_decode_3d_cpu(ctypes.addressof(p3), 2, 1 << 31, 4, 10, 5, d, d, d, d, d) == -1 and b"2^32 - 1" in lib.accv_last_error()
