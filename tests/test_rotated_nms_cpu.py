"""rotated_iou_bev and rotated_nms_bev through the library's host entries (no GPU): IoU literals with closed forms, random
frames against the float64 world-coordinate definition of rotated_nms_cases.py, keep decisions ON the threshold where the
arithmetic is exact, the cuts, argument checks and empty batches; and, at the end, boxes off the dataset-like range
(rotated_iou_hard_cases.py): yaws many turns from zero, strips, quarter-turn and axis yaws, closed forms that hold the
definition too, and keep decisions that a single float32 subtraction of the yaws got wrong."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rotated_nms_cases import (BAR, BEV, BIG, CHAIN, CHAIN_THR, SMALL, Case, assert_margin, check, definition, iou64, kept_slots,  # noqa: E402
                               make_case, pick_threshold, placed_case, ragged5, share)

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import CenterPointDetections, rotated_iou_bev, rotated_nms_bev  # noqa: E402

BELOW = float(np.nextafter(np.float32(0.25), np.float32(0)))


def iou(a, b):
    """the operator on one frame of host boxes: float32 [Na, Nb]"""
    a, b = np.asarray(a, np.float32).reshape(-1, 5), np.asarray(b, np.float32).reshape(-1, 5)
    out = rotated_iou_bev(ragged5(a, [len(a)]), ragged5(b, [len(b)]))
    assert out.tensor.dtype == torch.float32 and tuple(out.tensor.shape) == (1, len(a), len(b))
    return out.tensor[0].numpy()


def one(a, b):
    return float(iou([a], [b])[0, 0])


# ------------------------------------------------------------------------------------------------------- IoU literals
def test_a_2x2_box_inside_a_4x4_box_is_a_quarter_exactly_both_ways():
    assert one(SMALL, BIG) == 0.25 and one(BIG, SMALL) == 0.25
    assert one((3.0, 5.0, 2.0, 2.0, 0.0), (3.5, 4.5, 4.0, 4.0, 0.0)) == 0.25


@pytest.mark.parametrize("l,s", [(4.0, 2.0), (4.5, 1.9), (10.0, 0.5)])
def test_a_box_crossed_with_itself_turned_by_a_right_angle(l, s):
    want = s * s / (2 * l * s - s * s)
    for yaw in (0.0, 0.3, -2.0):
        got = one((7.0, -3.0, l, s, yaw), (7.0, -3.0, l, s, yaw + math.pi / 2))
        assert abs(got - want) <= BAR, (got, want)


def test_a_square_against_itself_turned_by_45_degrees():
    # the octagon: 8 (sqrt 2 - 1) of an area of 4; iou = inter / (8 - inter)
    inter = 8 * (math.sqrt(2) - 1)
    want = inter / (8 - inter)
    assert abs(want - 1 / math.sqrt(2)) < 1e-12
    for yaw in (0.0, 1.1):
        got = one((1.0, 2.0, 2.0, 2.0, yaw), (1.0, 2.0, 2.0, 2.0, yaw + math.pi / 4))
        assert abs(got - want) <= BAR, (got, want)


@pytest.mark.parametrize("box", [(0.0, 0.0, 4.5, 1.9, 0.0), (-37.25, 48.5, 4.5, 1.9, 2.7), (51.2, -51.2, 0.7, 0.6, -3.1), (3.0, 4.0, 10.0, 2.8, 1e-4)])
def test_identical_boxes_give_one_exactly(box):
    assert one(box, box) == 1.0


def test_boxes_sharing_only_an_edge_or_a_corner_and_disjoint_boxes_give_zero():
    a = (2.0, 1.0, 4.0, 2.0, 0.0)
    for b in ((6.0, 1.0, 4.0, 2.0, 0.0), (2.0, 3.0, 4.0, 2.0, 0.0), (-2.0, 1.0, 4.0, 2.0, 0.0), (2.0, -1.0, 4.0, 2.0, 0.0),      # an edge
              (6.0, 3.0, 4.0, 2.0, 0.0),                                                                                       # a corner
              (6.5, 1.0, 4.0, 2.0, 0.0), (40.0, -30.0, 4.0, 2.0, 1.0), (2.0, 3.5, 4.0, 2.0, 0.0)):                              # disjoint
        assert one(a, b) == 0.0 and one(b, a) == 0.0, b
        assert iou64([a], [b])[0, 0] == 0.0


def test_a_small_twist_agrees_with_the_definition():
    a, b = (10.0, 20.0, 4.5, 1.9, 0.7), (10.0, 20.0, 4.5, 1.9, 0.7 + 1e-4)
    want = iou64(np.float32([a]), np.float32([b]))[0, 0]
    assert 0.999 < want < 1 and abs(one(a, b) - want) <= BAR


def test_symmetry_and_invariance_under_a_common_motion():
    """the motions are exact in float32 (centres on a 2^-10 lattice, shifts on it too, quarter turns), so that the moved boxes
    ARE the same boxes and the IoU bar applies; only yaw + k pi / 2 is rounded, by 2.4e-7 rad at most"""
    rng = np.random.default_rng(5)
    from rotated_nms_cases import random_boxes

    boxes = random_boxes(rng, 60, 0, bad=0.0)
    boxes[:, :2] = np.round(boxes[:, :2] * 1024) / 1024
    m = iou(boxes, boxes)
    assert (m > 0.05).sum() > 100
    assert np.abs(m - m.T).max() <= BAR
    for shift, quarter in (((13.25, -8.5), 0), ((0.0, 0.0), 1), ((-20.0, 30.125), 2), ((1.0, 0.0), 3)):
        moved = boxes.copy()
        x, y = boxes[:, 0], boxes[:, 1]
        mx, my = ((x, y), (-y, x), (-x, -y), (y, -x))[quarter]
        moved[:, 0], moved[:, 1] = mx + np.float32(shift[0]), my + np.float32(shift[1])
        assert np.array_equal(moved[:, 0].astype(np.float64), mx.astype(np.float64) + shift[0]), "the motion is not exact"
        moved[:, 4] = (boxes[:, 4].astype(np.float64) + quarter * math.pi / 2).astype(np.float32)
        assert np.abs(iou(moved, moved) - m).max() <= BAR


@pytest.mark.parametrize("col,value", [(0, np.nan), (1, np.inf), (2, 0.0), (2, -1.0), (3, 0.0), (3, -np.inf), (2, np.inf), (4, np.nan), (4, np.inf)])
def test_degenerate_boxes_give_plus_zero(col, value):
    good = np.float32([[1.0, 1.0, 4.0, 2.0, 0.3]])
    bad = good.copy()
    bad[0, col] = value
    for m in (iou(bad, good), iou(good, bad), iou(bad, bad)):
        assert m.view(np.uint32)[0, 0] == 0


def test_huge_finite_values_do_not_make_nan():
    big = np.float32([[3e38, -3e38, 3e30, 3e30, 1.0], [1.0, 1.0, 3e20, 3e20, 0.0], [0.0, 0.0, 1e-30, 1e-30, 0.0]])
    m = iou(big, big)
    assert np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()


# ------------------------------------------------------------------------------------------------------ random frames
@pytest.mark.parametrize("Na,Nb,sizes_a,sizes_b", [(1, 1, [1, 0], [1, 1]), (37, 70, [37, 20, 0], [70, 0, 33]), (130, 65, [130, 64], [65, 1])])
def test_iou_matrix_against_the_definition_with_ragged_sizes(Na, Nb, sizes_a, sizes_b):
    from rotated_nms_cases import random_boxes

    rng = np.random.default_rng(Na)
    B = len(sizes_a)
    both = [np.stack([random_boxes(rng, Na + Nb, b) for b in range(B)])]
    a, b = both[0][:, :Na].copy(), both[0][:, Na:].copy()
    got = rotated_iou_bev(ragged5(a, sizes_a), ragged5(b, sizes_b))
    assert got.sample_sizes.tolist() == sizes_a
    got = got.tensor.numpy()
    overlapping = 0
    for f in range(B):
        want = np.zeros((Na, Nb))
        want[:sizes_a[f], :sizes_b[f]] = iou64(a[f, :sizes_a[f]], b[f, :sizes_b[f]])
        assert np.abs(got[f] - want).max() <= BAR
        outside = np.ones((Na, Nb), bool)
        outside[:sizes_a[f], :sizes_b[f]] = False
        assert not got[f].view(np.uint32)[outside].any(), "a pair beyond a size is not +0"
        overlapping += int((want > 0.01).sum())
    assert Na == 1 or overlapping > 20


def thresholds_of(case, pattern):
    """per task: a number picked by the margin walk from the pattern's start, or None"""
    return [None if start is None else pick_threshold(case, t, start) for t, start in enumerate(pattern)]


@pytest.mark.parametrize("N,B,D", [(1, 1, 7), (70, 3, 9), (300, 2, 7), (1024, 1, 16)])
def test_host_nms_equals_the_definition(N, B, D):
    case = make_case(B, N, 3, D, seed=1)
    thr = thresholds_of(case, (0.2, None, 0.5))
    assert_margin(case, thr)
    got = rotated_nms_bev(case.detections(), thr)
    want = definition(case, thr)
    check(got, want, case, f"N={N}")
    if N >= 70:
        kept, dead, total = share(want, case, thr)
        assert kept >= total / 10 and dead >= total / 10, (kept, dead, total)


def test_a_single_detections_object_a_plain_tuple_and_a_scalar_threshold():
    case = make_case(2, 70, 1, 9, seed=2)
    thr = pick_threshold(case, 0)
    want = definition(case, [thr])
    det = case.detections()[0]
    check(rotated_nms_bev(det, thr), want, case, "single")
    check(rotated_nms_bev([tuple(det)], [thr]), want, case, "tuple")
    check(rotated_nms_bev(tuple(det), thr), want, case, "bare tuple")


# ------------------------------------------------------------------------------------------------ decisions on the edge
def test_iou_equal_to_the_threshold_keeps_and_one_ulp_below_suppresses():
    case = placed_case(6, {2: BIG, 4: SMALL})
    assert kept_slots(rotated_nms_bev(case.detections(), 0.25)) == [0, 1, 2, 3, 4, 5]
    assert kept_slots(rotated_nms_bev(case.detections(), BELOW)) == [0, 1, 2, 3, 5]
    case = placed_case(6, {2: SMALL, 4: BIG})
    assert kept_slots(rotated_nms_bev(case.detections(), BELOW)) == [0, 1, 2, 3, 5]


def test_a_suppressed_box_suppresses_nothing():
    case = placed_case(8, {1: CHAIN[0], 3: CHAIN[1], 6: CHAIN[2]})
    got = rotated_nms_bev(case.detections(), CHAIN_THR)
    check(got, definition(case, [CHAIN_THR]), case)
    assert kept_slots(got) == [0, 1, 2, 4, 5, 6, 7]


def test_a_degenerate_box_is_kept_and_suppresses_nothing_even_under_a_negative_threshold():
    nan = (float("nan"), -100.0, 4.0, 4.0, 0.0)
    flat = (-100.0, -100.0, 0.0, 4.0, 0.0)
    case = placed_case(6, {0: BIG, 1: nan, 2: flat, 3: SMALL})
    assert kept_slots(rotated_nms_bev(case.detections(), 0.2)) == [0, 1, 2, 4, 5]
    # iou = +0 > -1 for every pair of valid boxes: only the first valid box and the degenerate ones stay
    got = rotated_nms_bev(case.detections(), -1.0)
    check(got, definition(case, [-1.0]), case)
    assert kept_slots(got) == [0, 1, 2]


def test_pre_max_size_hides_a_suppressor_and_post_max_size_counts_kept_boxes():
    case = placed_case(10, {1: CHAIN[0], 3: CHAIN[1], 6: CHAIN[2], 8: CHAIN[1]})
    det = case.detections()
    assert kept_slots(rotated_nms_bev(det, CHAIN_THR)) == [0, 1, 2, 4, 5, 6, 7, 9]
    got = rotated_nms_bev(det, CHAIN_THR, pre_max_size=8)                      # without slot 8 nothing changes before it
    assert kept_slots(got) == [0, 1, 2, 4, 5, 6, 7] and got[0].boxes.tensor.shape == (1, 8, 7)
    case2 = placed_case(10, {3: CHAIN[0], 1: CHAIN[1]})
    assert kept_slots(rotated_nms_bev(case2.detections(), CHAIN_THR)) == [0, 1, 2, 4, 5, 6, 7, 8, 9]
    assert kept_slots(rotated_nms_bev(case2.detections(), CHAIN_THR, pre_max_size=1)) == [0]
    # the suppressor of slot 3 hidden: it lies beyond the sample size
    short = Case([(*case2.tasks[0][:4], torch.tensor([1], dtype=torch.int64))])
    assert kept_slots(rotated_nms_bev(short.detections(), CHAIN_THR)) == [0]
    # post_max_size counts kept boxes: slot 3 is suppressed, so the fourth kept box is slot 5
    got = rotated_nms_bev(det, CHAIN_THR, post_max_size=4)
    assert kept_slots(got) == [0, 1, 2, 4] and got[0].boxes.tensor.shape == (1, 4, 7)
    for pre, post in ((None, 1), (5, 3), (3, 5), (2000, 2000), (7, None)):
        got = rotated_nms_bev(det, CHAIN_THR, pre_max_size=pre, post_max_size=post)
        check(got, definition(case, [CHAIN_THR], pre, post), case, f"pre={pre} post={post}")


def test_mixed_thresholds_copy_a_task_without_one_through_with_the_cuts():
    case = placed_case(12, {1: BIG, 2: SMALL, 5: CHAIN[0], 6: CHAIN[1]}, T=3)
    thr = [0.2, None, 0.6]
    got = rotated_nms_bev(case.detections(), thr, pre_max_size=11, post_max_size=9)
    check(got, definition(case, thr, 11, 9), case)
    assert kept_slots(got, 0) == [0, 1, 3, 4, 5, 7, 8, 9, 10]
    assert kept_slots(got, 1) == list(range(9))
    assert kept_slots(got, 2) == list(range(9))


def test_outputs_are_views_of_single_allocations_and_empty_batches_launch_nothing():
    case = make_case(2, 20, 3, 9, seed=3)
    got = rotated_nms_bev(case.detections(), 0.3, post_max_size=8)
    for i, name in enumerate(("boxes", "scores", "labels", "source")):
        base = {r[i].tensor.untyped_storage().data_ptr() for r in got}
        assert len(base) == 1, f"{name}: one allocation for all tasks"
    empty = make_case(0, 20, 2, 9, seed=3)
    got = rotated_nms_bev(empty.detections(), [0.3, None], post_max_size=8)
    assert len(got) == 2
    for r in got:
        assert tuple(r.boxes.tensor.shape) == (0, 8, 9) and tuple(r.source.tensor.shape) == (0, 8) and tuple(r.boxes.sample_sizes.shape) == (0,)
        assert r.labels.tensor.dtype == torch.int64 and r.source.tensor.dtype == torch.int32
    out = rotated_iou_bev(ragged5(np.zeros((0, 3, 5)), []), ragged5(np.zeros((0, 4, 5)), []))
    assert tuple(out.tensor.shape) == (0, 3, 4)
    out = rotated_iou_bev(ragged5(np.zeros((2, 3, 5)), [3, 3]), RaggedBatch(torch.zeros((2, 0, 5)), sample_sizes=torch.zeros(2, dtype=torch.int64)))
    assert tuple(out.tensor.shape) == (2, 3, 0)


# ---------------------------------------------------------------------------------------------------- argument checks
def _det(**over):
    """the five parts of one valid task [2, 6, 9], some replaced"""
    case = make_case(2, 6, 1, 9, seed=4)
    parts = dict(zip(("boxes", "scores", "labels", "source", "sizes"), (x.clone() for x in case.tasks[0])))
    parts.update(over)
    return parts


def _build(parts, sizes_for=None):
    sizes_for = sizes_for or {}
    return CenterPointDetections(*(RaggedBatch(parts[n], sample_sizes=sizes_for.get(n, parts["sizes"])) for n in ("boxes", "scores", "labels", "source")))


NMS_ERRORS = [
    (r"detections\[0\].boxes must be \[B, N, D\], got \(2, 54\)", lambda p: p.update(boxes=p["boxes"].reshape(2, 54)) or {}),
    (r"detections\[0\].scores must be \[B, N\], got \(2, 6, 1\)", lambda p: p.update(scores=p["scores"][..., None]) or {}),
    (r"detections\[0\].boxes must be float32, got torch.float64", lambda p: p.update(boxes=p["boxes"].double()) or {}),
    (r"detections\[0\].scores must be float32, got torch.float16", lambda p: p.update(scores=p["scores"].half()) or {}),
    (r"detections\[0\].labels must be int64, got torch.int32", lambda p: p.update(labels=p["labels"].int()) or {}),
    (r"detections\[0\].source must be int32, got torch.int64", lambda p: p.update(source=p["source"].long()) or {}),
    (r"detections\[0\].boxes must be contiguous", lambda p: p.update(boxes=p["boxes"].transpose(0, 1).contiguous().transpose(0, 1)) or {}),
    (r"detections\[0\].labels must be contiguous", lambda p: p.update(labels=p["labels"].t().contiguous().t()) or {}),
    (r"N must be in 1..1024, got 1025", lambda p: p.update(boxes=torch.zeros(2, 1025, 9), scores=torch.zeros(2, 1025), labels=torch.zeros(2, 1025, dtype=torch.int64),
                                                           source=torch.zeros(2, 1025, dtype=torch.int32)) or {}),
    (r"D must be in 7..16 \(x, y, z, dx, dy, dz, yaw, ...\), got 6", lambda p: p.update(boxes=p["boxes"][..., :6].contiguous()) or {}),
    (r"D must be in 7..16 \(x, y, z, dx, dy, dz, yaw, ...\), got 17", lambda p: p.update(boxes=torch.zeros(2, 6, 17)) or {}),
    (r"detections\[0\].scores must be \(2, 6\) on cpu, got \(2, 5\)", lambda p: p.update(scores=p["scores"][:, :5].contiguous()) or {}),
    (r"the sample_sizes of detections\[0\].boxes must be an int64 tensor \(2,\) on cpu", lambda p: p.update(sizes=p["sizes"].int()) or {}),
    (r"detections\[0\].labels does not share the sample_sizes of detections\[0\].boxes", lambda p: {"labels": p["sizes"].clone()}),
]


@pytest.mark.parametrize("match,mutate", NMS_ERRORS)
def test_argument_checks_of_the_detections(match, mutate):
    parts = _det()
    sizes_for = mutate(parts)
    with pytest.raises(RuntimeError, match="rotated_nms_bev: " + match):
        rotated_nms_bev(_build(parts, sizes_for), 0.2)


def test_argument_checks_of_the_options_and_the_task_list():
    det = _build(_det())
    other = _build(_det(boxes=torch.zeros(2, 6, 7)))
    for match, call in (
            (r"iou_threshold must be a number, a sequence of 1 numbers or Nones \(one per task\) or None, got \[0.2, 0.3\]", lambda: rotated_nms_bev(det, [0.2, 0.3])),
            (r"iou_threshold must be a number, a sequence of 2 numbers or Nones", lambda: rotated_nms_bev([det, det], "0.2")),
            (r"iou_threshold\[1\] must be a Python number or None, got '0.2'", lambda: rotated_nms_bev([det, det], [0.2, "0.2"])),
            (r"iou_threshold\[0\] must not be NaN", lambda: rotated_nms_bev(det, float("nan"))),
            (r"pre_max_size must be a Python integer or None, got 2.0", lambda: rotated_nms_bev(det, 0.2, pre_max_size=2.0)),
            (r"pre_max_size must be at least 1, got 0", lambda: rotated_nms_bev(det, 0.2, pre_max_size=0)),
            (r"post_max_size must be at least 1, got -3", lambda: rotated_nms_bev(det, 0.2, post_max_size=-3)),
            (r"post_max_size must be a Python integer or None, got True", lambda: rotated_nms_bev(det, 0.2, post_max_size=True)),
            (r"detections must be a CenterPointDetections or a sequence of 1..8 of them", lambda: rotated_nms_bev([], 0.2)),
            (r"detections must be a CenterPointDetections or a sequence of 1..8 of them", lambda: rotated_nms_bev([det] * 9, 0.2)),
            (r"detections\[1\] must be a CenterPointDetections \(boxes, scores, labels, source\)", lambda: rotated_nms_bev([det, det[:3]], 0.2)),
            (r"detections\[0\].boxes must be a RaggedBatch", lambda: rotated_nms_bev([(det[0].tensor, det[1], det[2], det[3])], 0.2)),
            (r"detections\[1\].boxes is \(2, 6, 7\) on cpu, detections\[0\].boxes \(2, 6, 9\) on cpu: all tasks share B, N, D and device",
             lambda: rotated_nms_bev([det, other], 0.2))):
        with pytest.raises(RuntimeError, match="rotated_nms_bev: " + match):
            call()


def test_argument_checks_of_the_iou_operator():
    a, b = ragged5(np.zeros((2, 3, 5)), [3, 3]), ragged5(np.zeros((2, 4, 5)), [4, 4])
    six = RaggedBatch(torch.zeros(2, 3, 6), sample_sizes=a.sample_sizes)
    for match, call in (
            (r"boxes_a must hold a tensor", lambda: rotated_iou_bev(a.tensor, b)),
            (r"boxes_b must be \[B, N, 5\], got \(2, 20\)", lambda: rotated_iou_bev(a, RaggedBatch(torch.zeros(2, 20), sample_sizes=b.sample_sizes))),
            (r"boxes_a must be float32, got torch.float64", lambda: rotated_iou_bev(RaggedBatch(a.tensor.double(), sample_sizes=a.sample_sizes), b)),
            (r"boxes_b must be contiguous", lambda: rotated_iou_bev(a, RaggedBatch(torch.zeros(4, 2, 5).transpose(0, 1), sample_sizes=b.sample_sizes))),
            (r"the boxes must be \[B, N, 5\] as \(x, y, dx, dy, yaw\), got \(2, 3, 6\) and \(2, 4, 5\)", lambda: rotated_iou_bev(six, b)),
            (r"boxes_a holds 2 frames, boxes_b 1", lambda: rotated_iou_bev(a, ragged5(np.zeros((1, 4, 5)), [4]))),
            (r"the sample_sizes of boxes_b must be an int64 tensor \(2,\) on cpu",
             lambda: rotated_iou_bev(a, RaggedBatch(b.tensor, sample_sizes=b.sample_sizes.int())))):
        with pytest.raises(RuntimeError, match="rotated_iou_bev: " + match):
            call()


def test_the_c_entries_refuse_what_the_python_layer_cannot_produce():
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    case = make_case(1, 6, 1, 9, seed=4)
    bx, sc, lb, src, sizes = case.tasks[0]
    out = [torch.zeros(1, 1, 6, 9), torch.zeros(1, 1, 6), torch.zeros(1, 1, 6, dtype=torch.int64), torch.zeros(1, 1, 6, dtype=torch.int32),
           torch.zeros(1, 1, dtype=torch.int64)]

    def call(B=1, N=6, D=9, pre=6, M=6, T=1, thr=0.2, null_input=False, null_output=False, params=True):
        p = nat.RotatedNmsParams()
        p.boxes[0], p.scores[0], p.labels[0], p.source[0], p.sizes[0] = (x.data_ptr() for x in (bx, sc, lb, src, sizes))
        if null_input:
            p.scores[0] = None
        p.has_threshold[0], p.iou_threshold[0], p.num_tasks = 1, thr, T
        ptrs = [x.data_ptr() for x in out]
        if null_output:
            ptrs[3] = None
        status = lib.accv_rotated_nms_bev_host(ctypes.addressof(p) if params else None, B, N, D, pre, M, *ptrs)
        return status, lib.accv_last_error().decode()

    assert call()[0] == 0
    for kw, text in ((dict(params=False), "rotated_nms_bev (host): null params"), (dict(B=-1), "rotated_nms_bev (host): negative size"),
                     (dict(T=0), "rotated_nms_bev (host): 1..8 tasks supported, got 0"), (dict(T=9), "rotated_nms_bev (host): 1..8 tasks supported, got 9"),
                     (dict(N=0), "rotated_nms_bev (host): N must be in 1..1024, got 0"), (dict(N=1025), "rotated_nms_bev (host): N must be in 1..1024, got 1025"),
                     (dict(D=6), "rotated_nms_bev (host): D must be in 7..16, got 6"), (dict(D=17), "rotated_nms_bev (host): D must be in 7..16, got 17"),
                     (dict(pre=0), "rotated_nms_bev (host): pre_max_size must be at least 1, got 0"),
                     (dict(M=0), "rotated_nms_bev (host): M must be in 1..min(N, pre_max_size) = 6, got 0"),
                     (dict(M=7), "rotated_nms_bev (host): M must be in 1..min(N, pre_max_size) = 6, got 7"),
                     (dict(pre=3, M=4), "rotated_nms_bev (host): M must be in 1..min(N, pre_max_size) = 3, got 4"),
                     (dict(thr=float("nan")), "rotated_nms_bev (host): iou_threshold[0] is NaN"),
                     (dict(null_output=True), "rotated_nms_bev (host): null output pointer"),
                     (dict(null_input=True), "rotated_nms_bev (host): null input pointer of task 0")):
        assert call(**kw) == (-1, text), kw
    assert call(B=0, null_output=True)[0] == 0
    a = torch.zeros(1, 3, 5)
    n = torch.tensor([3], dtype=torch.int64)
    o = torch.zeros(1, 3, 3)
    f = lib.accv_rotated_iou_bev_host
    assert f(a.data_ptr(), n.data_ptr(), a.data_ptr(), n.data_ptr(), 1, 3, 3, o.data_ptr()) == 0
    assert f(a.data_ptr(), n.data_ptr(), a.data_ptr(), n.data_ptr(), 1, -3, 3, o.data_ptr()) == -1
    assert lib.accv_last_error() == b"rotated_iou_bev (host): negative size"
    assert f(a.data_ptr(), None, a.data_ptr(), n.data_ptr(), 1, 3, 3, o.data_ptr()) == -1
    assert lib.accv_last_error() == b"rotated_iou_bev (host): null pointer"
    assert f(a.data_ptr() + 2, n.data_ptr(), a.data_ptr(), n.data_ptr(), 1, 3, 3, o.data_ptr()) == -1
    assert lib.accv_last_error() == b"rotated_iou_bev (host): a float32 tensor is not aligned to its element size"
    assert f(None, None, None, None, 0, 3, 3, None) == 0
    assert f(a.data_ptr(), n.data_ptr(), a.data_ptr(), n.data_ptr(), 1 << 40, 1 << 20, 1 << 20, o.data_ptr()) == -1
    assert lib.accv_last_error() == b"rotated_iou_bev (host): sizes overflow"


# ----------------------------------------------------------------------------- boxes off the dataset-like range
import rotated_iou_hard_cases as hard  # noqa: E402


@pytest.mark.parametrize("name", hard.NAMES)
def test_hard_geometry_family_against_the_definition_and_symmetric(name):
    a, b, want = hard.family(name)
    got = hard.op_pairs(a, b)
    err = float(np.abs(got - want).max())
    assert err <= BAR, f"{name}: IoU off by {err:.3e} (bar {BAR})"
    sym = float(np.abs(got - hard.op_pairs(b, a)).max())
    assert sym <= BAR, f"{name}: iou(a, b) and iou(b, a) differ by {sym:.3e}"


@pytest.mark.parametrize("form", [hard.crossing_strips, hard.box_inside_box])
def test_closed_forms_hold_the_definition_and_the_operator(form):
    """the oracle is trusted on strips and at any relative angle only because it, too, meets forms that do not use it"""
    a, b, want = form()
    assert want.min() > 0.005 and want.max() > 0.19
    assert np.abs(hard.iou64_pairs(a, b) - want).max() <= BAR
    assert np.abs(np.diag(iou64(a[:64], b[:64])) - want[:64]).max() <= BAR
    assert np.abs(hard.op_pairs(a, b) - want).max() <= BAR
    assert np.abs(hard.op_pairs(b, a) - want).max() <= BAR


def test_a_rectangle_written_with_its_sides_exchanged_is_the_same_rectangle():
    r, q, third = hard.rewritten_rectangles()
    assert (hard.iou64_pairs(r, third) > hard.OVERLAP).mean() > 0.9
    for pairs in (hard.iou64_pairs, hard.op_pairs):
        assert pairs(r, q).min() >= 1 - BAR and pairs(q, r).min() >= 1 - BAR, pairs.__name__
        assert np.abs(pairs(r, third) - pairs(q, third)).max() <= BAR, pairs.__name__
        assert np.abs(pairs(third, r) - pairs(third, q)).max() <= BAR, pairs.__name__


def test_strips_moved_along_their_length_stay_within_the_bar_plus_the_rotation_of_the_centre_offset():
    """what the bar does not cover, pinned to the bound its cause gives (rotated_iou_hard_cases.py)"""
    a, b, want, bound = hard.shifted_strips()
    for got in (hard.op_pairs(a, b), hard.op_pairs(b, a)):
        err = np.abs(got - want)
        print(f"strips moved along their length: largest error {err.max():.3e}, largest error / bound {(err / bound).max():.3f}, bound up to {bound.max():.2e}")
        assert (err <= bound).all(), f"{(err / bound).max():.3f} of the bound"


@pytest.mark.parametrize("yaw", [2 * math.pi * 100 + 0.7, -4084.5, hard.YAW_DOMAIN])
def test_identical_boxes_many_turns_out_still_give_one_exactly(yaw):
    """equal yaws leave no rounding to correct: the relative angle is +0 and its cosine 1, as before the correction"""
    for box in ((10.0, 20.0, 4.5, 1.9, yaw), (-37.25, 48.5, 50.0, 0.02, yaw)):
        assert one(box, box) == 1.0


def test_beyond_the_yaw_domain_the_value_is_still_a_finite_number_in_0_1():
    a = np.float32([[1.0, 2.0, 4.5, 1.9, 2 * math.pi * 1e5 + 0.3], [1.0, 2.0, 4.5, 1.9, 3e38], [1.0, 2.0, 50.0, 0.02, -1e9], [1.0, 2.0, 4.5, 1.9, 0.3]])
    b = a.copy()
    b[:, 4] = np.float32([0.3, -3e38, 1e9, -2 * math.pi * 1e5])
    m = iou(a, b)
    assert np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()


def test_the_frozen_pairs_are_what_their_records_say():
    for a, b, want, was in hard.FROZEN:
        assert abs(hard.iou64_pairs(np.float32([a]), np.float32([b]))[0] - want) < 1e-12
        assert abs(was - want) > 3e-5 and a[0] < -10 and a[1] < -10 and b[0] < -10 and b[1] < -10
    assert {was > want for _, _, want, was in hard.FROZEN} == {True, False}, "both wrong directions"


@pytest.mark.parametrize("k", range(len(hard.FROZEN)))
def test_keep_decisions_that_one_float32_subtraction_of_the_yaws_got_wrong(k):
    """the threshold lies 2e-5 from the float64 IoU, twice the margin, on the side where the old arithmetic's value was"""
    a, b, want, was = hard.FROZEN[k]
    thr = hard.frozen_threshold(want, was)
    case = placed_case(70, {63: b, 64: a})
    assert_margin(case, [thr])
    got = rotated_nms_bev(case.detections(), thr)
    check(got, definition(case, [thr]), case, f"frozen pair {k}")
    assert kept_slots(got) == [s for s in range(70) if s != 64 or want <= thr]
