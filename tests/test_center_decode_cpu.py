"""center_point_decode without a GPU: the library's host entry (the same arithmetic header as the kernel) against the
per-peak float32 definition of center_decode_cases.py, special values, and every argument check."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_decode_cases import NUSC, NUSC_RANGE, NUSC_TASKS, UNIT, check, kept_ranks, make_case, placed_case, run  # noqa: E402

from accvlab.draw_heatmap import CenterPointDetections, HeatmapPeaks, center_point_decode  # noqa: E402

op = center_point_decode
NUSC_RADII = [4.0, 12.0, 10.0, 1.0, 0.85, 0.175]        # mmdet3d's nuScenes min_radius per task
FULL = dict(score_threshold=0.1, post_center_range=NUSC_RANGE, nms_threshold=NUSC_RADII, post_max_size=83)


def _tasks(T):
    return {1: ((3, 0, 7),), 2: ((5, 2), (7,)), 6: NUSC_TASKS}[T]


# ------------------------------------------------------------------------------------------------ against the definition
@pytest.mark.parametrize("T", [1, 2, 6])
@pytest.mark.parametrize("C", [8, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_host_entry_equals_the_definition(dtype, C, T):
    tasks = _tasks(T)
    case = make_case(2, 150, tasks, C=C, dtype=dtype, seed=10 * T + C)
    if T == 6:
        assert {len(f) for f in case.feats} == {1, 2, 4, 5}
    kw = dict(FULL, nms_threshold=NUSC_RADII[:T])
    got, want = run(op, case, NUSC, **kw)
    check(got, want, f"T={T} C={C} {dtype}")
    assert all(isinstance(r, CenterPointDetections) and r.boxes.tensor.shape == (2, 83, C - 1) for r in got)
    assert sum(int(w["sizes"].sum()) for w in want) > 20 * T, "the case keeps too few peaks to show anything"


@pytest.mark.parametrize("kw", [
    dict(), dict(score_threshold=0.3), dict(post_center_range=NUSC_RANGE), dict(nms_threshold=4.0), dict(post_max_size=7),
    dict(norm_bbox=False), dict(bottom_center=True), dict(bottom_center=True, norm_bbox=False),
    dict(nms_threshold=[None, 2.0, None, 0.5, 100.0, 0.0], post_max_size=40), dict(FULL, bottom_center=True)],
    ids=lambda kw: "-".join(kw) or "defaults")
def test_every_option_alone_and_together(kw):
    case = make_case(3, 70, seed=5)
    got, want = run(op, case, NUSC, **kw)
    check(got, want, str(kw))


def test_logit_scores_with_the_margin_asserted_and_mixed_score_dtype():
    for score_dtype, seed in ((torch.float32, 2), (torch.bfloat16, 3)):
        case = make_case(2, 200, dtype=torch.float16, score_dtype=score_dtype, seed=seed, logits=True)
        got, want = run(op, case, NUSC, scores_are_logits=True, **FULL)
        check(got, want, f"logits {score_dtype}")
        assert sum(int(w["sizes"].sum()) for w in want) > 100


def test_a_single_peaks_object_for_one_task_and_a_single_map():
    case = make_case(2, 40, ((4, 9),), C=8, seed=3)
    s, i, c = case.peaks[0]
    got = op(HeatmapPeaks(s, i, c, i, i), case.feats[0][0], case.tasks, **NUSC, nms_threshold=3.0)
    again, want = run(op, case, NUSC, nms_threshold=3.0)
    check(got, want, "single")
    assert torch.equal(got[0].boxes.tensor, again[0].boxes.tensor)
    assert set(got[0].labels.tensor.unique().tolist()) <= {0, 4, 9}


def test_outputs_are_views_of_single_allocations_and_empty_batches_launch_nothing():
    case = make_case(2, 20, seed=4)
    got = op(*case.op_args(), **NUSC, post_max_size=5)
    for name in ("boxes", "scores", "labels", "source"):
        base = getattr(got[0], name).tensor
        step = base.numel() * base.element_size()
        assert [getattr(r, name).tensor.data_ptr() - base.data_ptr() for r in got] == [t * step for t in range(6)]
    sizes = [r.boxes.sample_sizes for r in got]
    assert [s.data_ptr() - sizes[0].data_ptr() for s in sizes] == [t * 2 * 8 for t in range(6)]
    empty = make_case(0, 20, seed=4)
    for r in op(*empty.op_args(), **NUSC, post_max_size=5):
        assert r.boxes.tensor.shape == (0, 5, 9) and r.source.tensor.shape == (0, 5) and r.boxes.sample_sizes.shape == (0,)


# -------------------------------------------------------------------------------------------------------- special values
INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("value", [NAN, INF, -INF])
@pytest.mark.parametrize("channel", range(10))
def test_nan_and_infinities_in_each_channel(channel, value):
    """peak 3 of 8 reads the special value.  With a range it is dropped where the value reaches x, y or z; without one it
    is kept, a NaN distance suppresses nothing and is suppressed by nothing, and the value reaches its own row only."""
    placed = {k: (4.0 + 2 * k, 5.5) for k in range(8)}
    case = placed_case(8, placed, C=10)
    cell = int(case.peaks[0][1][0, 3])
    case.feats[0][0][0, channel].view(-1)[cell] = value
    for kw in (dict(nms_threshold=1.0), dict(nms_threshold=1.0, post_center_range=[0.0, 0.0, -1.0, 32.0, 24.0, 1.0]),
               dict(nms_threshold=1.0, norm_bbox=False, bottom_center=True)):
        got, want = run(op, case, UNIT, **kw)
        check(got, want, f"channel {channel} {value} {kw}")
        dropped = "post_center_range" in kw and channel < 3
        assert kept_ranks(got) == [k for k in range(8) if not (dropped and k == 3)]
        bad = ~torch.isfinite(got[0].boxes.tensor[0])
        assert set(bad.any(1).nonzero().flatten().tolist()) <= (set() if dropped else {3}), kw


def test_special_scores_and_illegal_indices_and_class_positions():
    placed = {k: (3.0 + 2 * k, 7.5) for k in range(10)}
    case = placed_case(10, placed, tasks=((6, 2),), scores=[NAN, INF, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, -INF, 0.05])
    s, idx, cls = case.peaks[0]
    idx[0, 3], idx[0, 4], idx[0, 5] = -1, 32 * 24, 2 ** 40          # illegal cells: nothing is read
    cls[0, 6], cls[0, 7] = -1, 2                                    # illegal positions in a task of two
    cls[0, 2] = 1
    got, want = run(op, case, UNIT, score_threshold=0.1)
    check(got, want, "illegal")
    assert kept_ranks(got) == [1, 2]                                # NaN fails score > thr, +inf passes
    assert got[0].labels.tensor[0, :2].tolist() == [6, 2]
    got, want = run(op, case, UNIT)                                 # without a threshold the NaN score is kept and reported
    check(got, want, "illegal, no threshold")
    assert kept_ranks(got) == [0, 1, 2, 8, 9] and bool(torch.isnan(got[0].scores.tensor[0, 0]))


def test_pinned_vector():
    """One frame, UNIT geometry (x = xs + off_x), tasks ((5, 2), (7,)), worked out by hand.  Cell (10, 7) holds offsets
    (0.25, 0.5), z -1, d (0, 0, 0), sin 1, cos 0; cell (11, 7) holds offsets (0, 0.5).
      rank 0  cell (10, 7), position 1: x 10.25, y 7.5, dims exp(0) = 1, yaw atan2(1, 0) = pi / 2, label 2, score 0.9
      rank 1  cell (11, 7): x 11, y 7.5: squared distance to rank 0 is 0.5625 <= 0.5625: suppressed
      rank 2  cell (0, 0), score 0.1: not above the threshold 0.1: dropped"""
    maps = torch.zeros((1, 8, 24, 32))
    maps[0, :, 7, 10] = torch.tensor([0.25, 0.5, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    maps[0, :, 7, 11] = torch.tensor([0.0, 0.5, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    peaks = HeatmapPeaks(torch.tensor([[0.9, 0.5, 0.1]]), torch.tensor([[7 * 32 + 10, 7 * 32 + 11, 0]]), torch.tensor([[1, 0, 0]]), None, None)
    none = HeatmapPeaks(torch.tensor([[0.9, 0.5, 0.1]]), torch.tensor([[-1, -1, -1]]), torch.tensor([[0, 0, 0]]), None, None)
    r0, r1 = op([peaks, none], [maps, maps], ((5, 2), (7,)), **UNIT, score_threshold=0.1, nms_threshold=0.5625, bottom_center=True)
    assert r0.boxes.sample_sizes.tolist() == [1] and r1.boxes.sample_sizes.tolist() == [0]
    row = r0.boxes.tensor[0, 0].tolist()
    assert row[:2] == [10.25, 7.5] and row[2] == -1.5 and row[3:6] == [1.0, 1.0, 1.0] and abs(row[6] - np.pi / 2) < 1e-6
    assert r0.scores.tensor.tolist() == [[np.float32(0.9), 0.0, 0.0]] and r0.labels.tensor.tolist() == [[2, 0, 0]]
    assert r0.source.tensor.tolist() == [[0, -1, -1]] and not r0.boxes.tensor[0, 1:].any()
    assert r1.source.tensor.tolist() == [[-1, -1, -1]] and not r1.boxes.tensor.any() and not r1.scores.tensor.any()


def test_circle_rule_on_the_host():
    """equal to the threshold suppresses, one ulp above does not, a suppressed peak suppresses nothing"""
    thr = 0.5625                                                    # 0.75 * 0.75
    below = float(np.nextafter(np.float32(thr), np.float32(0)))
    chain = {2: (5.5, 3.5), 4: (6.25, 3.5), 6: (7.0, 3.5)}
    case = placed_case(9, chain)
    for t, want_kept in ((thr, [0, 1, 2, 3, 5, 6, 7, 8]), (below, list(range(9)))):
        got, want = run(op, case, UNIT, nms_threshold=t)
        check(got, want, f"thr {t}")
        assert kept_ranks(got) == want_kept


# ------------------------------------------------------------------------------------------------------- argument checks
def _good():
    case = make_case(2, 12, ((0, 1), (2,)), C=8, seed=0, splits=[(2, 1, 3, 2), (8,)])
    peaks, feats, tasks = case.op_args()
    return peaks, feats, tasks, dict(NUSC)


def _refused(match, mutate):
    peaks, feats, tasks, kw = _good()
    args = dict(peaks=peaks, feats=feats, tasks=tasks, **kw)
    mutate(args)
    with pytest.raises(RuntimeError, match="center_point_decode: " + match):
        op(args.pop("peaks"), args.pop("feats"), args.pop("tasks"), **args)


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _peak(t, **fields):
    def mutate(a):
        a["peaks"][t] = a["peaks"][t]._replace(**{k: f(getattr(a["peaks"][t], k)) for k, f in fields.items()})
    return mutate


def _map(t, i, f):
    def mutate(a):
        a["feats"][t][i] = f(a["feats"][t][i])
    return mutate


@pytest.mark.parametrize("match,mutate", [
    ("tasks must be a sequence of 1..8", _set("tasks", ())),
    ("tasks must be a sequence of 1..8", _set("tasks", tuple((i,) for i in range(9)))),
    (r"tasks\[1\] must be a sequence", _set("tasks", ((0, 1), 2))),
    ("class ids must be integers in", _set("tasks", ((0, 64), (2,)))),
    ("class ids must be integers in", _set("tasks", ((0, True), (2,)))),
    ("class 1 is in more than one task", _set("tasks", ((0, 1), (1,)))),
    ("peaks must hold one HeatmapPeaks per task", lambda a: a["peaks"].pop()),
    ("feats must hold one entry per task", lambda a: a["feats"].pop()),
    (r"peaks\[1\] must be a HeatmapPeaks", lambda a: a["peaks"].__setitem__(1, torch.zeros(2, 12))),
    (r"peaks\[0\].indices must be \[B, K\]", _peak(0, indices=lambda x: x[None])),
    (r"peaks\[1\].scores must be contiguous", _peak(1, scores=lambda x: x.t().contiguous().t())),
    (r"peaks\[0\].scores must be float32, float16 or bfloat16", _peak(0, scores=lambda x: x.double())),
    (r"peaks\[1\].scores is torch.float16", _peak(1, scores=lambda x: x.half())),
    (r"peaks\[1\].scores is torch.float32 \(2, 11\)", lambda a: a["peaks"].__setitem__(1, HeatmapPeaks(*(x[:, :11].contiguous() for x in a["peaks"][1])))),
    (r"peaks\[1\].classes must be int64", _peak(1, classes=lambda x: x.int())),
    (r"peaks\[0\].indices must be int64 \(2, 12\)", _peak(0, indices=lambda x: x[:1])),
    ("K must be in 1..1024", lambda a: a["peaks"].__setitem__(0, HeatmapPeaks(torch.zeros(2, 1025), *(torch.zeros(2, 1025, dtype=torch.int64),) * 4))),
    ("K must be in 1..1024", lambda a: a["peaks"].__setitem__(0, HeatmapPeaks(torch.zeros(2, 0), *(torch.zeros(2, 0, dtype=torch.int64),) * 4))),
    (r"feats\[1\] must be a tensor or a non-empty sequence", lambda a: a["feats"].__setitem__(1, [])),
    (r"at most 8 maps per task", lambda a: a["feats"].__setitem__(0, [torch.zeros(2, 1, 64, 64)] * 9)),
    (r"feats\[0\]\[1\] must be a tensor", _map(0, 1, lambda m: None)),
    (r"feats\[0\]\[0\] must be \[B, C, H, W\]", _map(0, 0, lambda m: m[0])),
    (r"feats\[0\]\[2\] must be contiguous", _map(0, 2, lambda m: m.transpose(2, 3))),
    ("feats must be float32, float16 or bfloat16", _map(0, 0, lambda m: m.double())),
    (r"feats\[1\]\[0\] has dtype torch.float16", _map(1, 0, lambda m: m.half())),
    (r"feats\[0\]\[1\] has shape .*must agree", _map(0, 1, lambda m: m[:, :, :32].contiguous())),
    (r"feats\[1\]\[0\] has shape .*must agree", _map(1, 0, lambda m: m[:1])),
    (r"the maps of a task must hold 8 or 10 channels in total.*feats\[0\] holds 7", _map(0, 1, lambda m: m[:, :0])),
    (r"the maps of a task must hold 8 or 10 channels in total.*feats\[1\] holds 10", _map(1, 0, lambda m: torch.zeros(2, 10, 64, 64))),
    ("pc_range must be a sequence of at least 2 numbers", _set("pc_range", [0.0])),
    (r"voxel_size\[1\] must be a Python number", _set("voxel_size", [0.2, "a"])),
    ("voxel_size and out_size_factor must be positive and finite", _set("voxel_size", [0.2, 0.0])),
    ("voxel_size and out_size_factor must be positive and finite", _set("out_size_factor", float("inf"))),
    ("out_size_factor must be a Python number", _set("out_size_factor", None)),
    ("pc_range must be finite", _set("pc_range", [0.0, float("nan")])),
    ("score_threshold must be a Python number", _set("score_threshold", torch.tensor(0.1))),
    ("score_threshold must not be NaN", _set("score_threshold", float("nan"))),
    ("post_center_range must be a sequence of 6 numbers", _set("post_center_range", [0.0] * 5)),
    ("post_center_range must not hold NaN", _set("post_center_range", [0.0] * 5 + [float("nan")])),
    ("nms_threshold must be a number, a sequence of 2 numbers", _set("nms_threshold", [1.0])),
    (r"nms_threshold\[1\] must be a Python number", _set("nms_threshold", [1.0, "x"])),
    (r"nms_threshold\[0\] must not be NaN", _set("nms_threshold", float("nan"))),
    ("post_max_size must be a Python integer", _set("post_max_size", 3.0)),
    ("post_max_size must be at least 1", _set("post_max_size", 0)),
])
def test_argument_checks(match, mutate):
    _refused(match, mutate)


def test_the_c_entry_refuses_what_the_python_layer_cannot_produce():
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    p = nat.CenterPointDecodeParams()
    call = lambda *a: lib.accv_center_point_decode_host(ctypes.addressof(p), *a, None, None, None, None, None)   # noqa: E731
    assert lib.accv_center_point_decode_host(None, 1, 1, 1, 1, 1, None, None, None, None, None) == -1
    assert b"null params" in lib.accv_last_error()
    assert call(1, 4, 8, 8, 4) == -1 and b"1..8 tasks" in lib.accv_last_error()
    p.num_tasks = 1
    assert call(1, 0, 8, 8, 1) == -1 and b"K must be in 1..1024" in lib.accv_last_error()
    assert call(1, 4, 8, 8, 5) == -1 and b"M must be in 1..K" in lib.accv_last_error()
    assert call(1, 4, 0, 8, 4) == -1 and b"grid" in lib.accv_last_error()
    p.score_dtype = 3
    assert call(1, 4, 8, 8, 4) == -1 and b"unknown dtype" in lib.accv_last_error()
    p.score_dtype = 0
    p.task_first[1] = 65
    assert call(1, 4, 8, 8, 4) == -1 and b"task_first" in lib.accv_last_error()
    p.task_first[1] = 1
    assert call(1, 4, 8, 8, 4) == -1 and b"maps per task" in lib.accv_last_error()
    p.num_maps[0], p.channels[0][0] = 1, 9
    assert call(1, 4, 8, 8, 4) == -1 and b"8 or 10" in lib.accv_last_error()
    p.channels[0][0] = 8
    assert call(1, 4, 8, 8, 4) == -1 and b"positive" in lib.accv_last_error()
    p.voxel_size[0] = p.voxel_size[1] = p.out_size_factor = 1.0
    assert call(0, 4, 8, 8, 4) == 0                                           # an empty batch touches no pointer
    assert call(1, 4, 8, 8, 4) == -1 and b"null output" in lib.accv_last_error()
