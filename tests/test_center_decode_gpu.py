"""center_point_decode on the GPU: the kernel against the per-peak float32 definition of center_decode_cases.py and against
the host entry, at the edges of its work partition (wave block, chunk of kThreads peaks, the post_max_size cut), the
validity and circle rules ON their boundaries, a round trip through center_point_targets and heatmap_peaks, guard bands,
reproducibility, graph capture, no host synchronisation and a non-default stream."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import center_targets_cases as ct  # noqa: E402
from center_decode_cases import (BAR, NUSC, NUSC_GRID, NUSC_RANGE, NUSC_TASKS, UNIT, UNIT_GRID, check,  # noqa: E402
                                 check_device_against_host, definition, kept_ranks, make_case, placed_case, run)

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import CenterPointDetections, center_point_decode, center_point_targets, heatmap_peaks  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = center_point_decode


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "center_decode.hip")).read()
WAVE = int(_constant(_SRC, "kWave"))
THREADS = int(_constant(_SRC, "kThreads"))          # peaks per chunk
assert (WAVE, THREADS) == (64, 256)
NUSC_RADII = [4.0, 12.0, 10.0, 1.0, 0.85, 0.175]    # mmdet3d's nuScenes min_radius per task
THR = 0.5625                                        # 0.75 * 0.75: two centres 0.75 apart are ON the circle
BELOW = float(np.nextafter(np.float32(THR), np.float32(0)))
BIG = (64, 64)                                      # a UNIT-geometry grid with room for 1024 fillers


def both(case, cfg, what="", **kw):
    """`case` lives on the host: the device against the definition, and against the host path on the same inputs"""
    dev_case = case.to(DEV)
    got, want = run(op, dev_case, cfg, **kw)
    assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for r in got for x in r)
    check(got, want, what + " device")
    host = op(*case.op_args(), **cfg, **kw)
    check_device_against_host(got, host, want[0]["approx_channels"], want[0]["logits"], what + " device against host")
    return got, want


# --------------------------------------------------------------------------------------------- the kernel's work partition
@pytest.mark.parametrize("B", [0, 1, 3])
@pytest.mark.parametrize("K", [1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, 1024])
def test_peak_counts_across_wave_blocks_and_chunks(K, B):
    tasks = ((5, 2), (7,), (0, 1, 3))
    for grid, cfg, rng, nms in ((NUSC_GRID, NUSC, NUSC_RANGE, [4.0, None, 0.85]), (UNIT_GRID, UNIT, [2.0, 2.0, -4.0, 30.0, 20.0, 2.0], 0.75)):
        case = make_case(B, K, tasks, grid=grid, seed=K + B)
        got, want = both(case, cfg, f"B={B} K={K} {grid}", score_threshold=0.05, post_center_range=rng, nms_threshold=nms)
        assert all(r.boxes.tensor.shape == (B, K, 9) for r in got)
    if B == 3 and K >= WAVE:
        assert sum(int(w["sizes"].sum()) for w in want) > K // 4, "the case keeps too few peaks to show anything"
    both(case, cfg, f"B={B} K={K} no options")


@pytest.mark.parametrize("C", [8, 10])
@pytest.mark.parametrize("dtype,score_dtype", [(torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)])
def test_map_and_score_dtypes_channel_counts_map_splits_and_six_tasks(dtype, score_dtype, C):
    case = make_case(3, THREADS + 9, C=C, dtype=dtype, score_dtype=score_dtype, seed=C)
    for kw in (dict(bottom_center=True), dict(norm_bbox=False, bottom_center=True)):
        got, want = both(case, NUSC, f"{dtype} {score_dtype} C={C}", score_threshold=0.1, post_center_range=NUSC_RANGE,
                         nms_threshold=NUSC_RADII, post_max_size=83, **kw)
    assert sum(int(w["sizes"].sum()) for w in want) > 200


def test_logit_scores():
    case = make_case(3, 300, dtype=torch.float16, score_dtype=torch.float32, seed=2, logits=True)
    got, want = both(case, NUSC, "logits", scores_are_logits=True, score_threshold=0.1, nms_threshold=NUSC_RADII, post_max_size=83)
    assert sum(int(w["sizes"].sum()) for w in want) > 300


# ------------------------------------------------------------------------------------------------------------- validity
def test_score_equal_to_the_threshold_is_dropped_and_one_ulp_above_is_kept():
    up = float(np.nextafter(np.float32(0.5), np.float32(1)))
    scores = [0.9, up, 0.5, 0.5, up, float(np.nextafter(np.float32(0.5), np.float32(0)))] + [0.5] * WAVE + [up]
    case = placed_case(len(scores), {}, scores=scores)
    got, _ = both(case, UNIT, "score edge", score_threshold=0.5)
    assert kept_ranks(got) == [0, 1, 4, len(scores) - 1]


def test_centres_on_every_face_of_the_range_are_kept_and_one_ulp_outside_dropped():
    rng = [2.0, 3.0, -1.0, 10.0, 12.0, 1.0]
    f = np.float32
    out_lo, out_hi = (lambda v: float(np.nextafter(f(v), f(-np.inf)))), (lambda v: float(np.nextafter(f(v), f(np.inf))))
    on = [(2.0, 4.5, 0.0), (10.0, 4.5, 0.0), (4.5, 3.0, 0.0), (5.5, 12.0, 0.0), (6.5, 6.5, -1.0), (7.5, 6.5, 1.0), (2.0, 3.0, -1.0), (10.0, 12.0, 1.0)]
    off = [(out_lo(2.0), 5.5, 0.0), (out_hi(10.0), 5.5, 0.0), (6.5, out_lo(3.0), 0.0), (7.5, out_hi(12.0), 0.0), (6.5, 8.5, out_lo(-1.0)),
           (7.5, 8.5, out_hi(1.0))]
    placed = {}
    for n, (a, b) in enumerate(zip(on, off)):
        placed[2 * n], placed[2 * n + 1] = a, b
    placed[12], placed[13] = on[6], on[7]
    case = placed_case(14, placed)
    got, want = both(case, UNIT, "range faces", post_center_range=rng)
    assert kept_ranks(got) == [0, 2, 4, 6, 8, 10, 12, 13]
    x = got[0].boxes.tensor[0, :8, :3].cpu()
    assert x[0, 0] == 2.0 and x[1, 0] == 10.0 and x[2, 1] == 3.0 and x[3, 1] == 12.0 and x[4, 2] == -1.0 and x[5, 2] == 1.0


@pytest.mark.parametrize("K", [WAVE + 1, THREADS + WAVE + 1])
def test_all_peaks_invalid_and_all_peaks_valid(K):
    case = placed_case(K, {}, grid=BIG)
    for kw in (dict(), dict(nms_threshold=THR)):
        got, _ = both(case, UNIT, "all valid", **kw)
        assert kept_ranks(got) == list(range(K))
        got, _ = both(case, UNIT, "all invalid", score_threshold=0.95, **kw)
        assert kept_ranks(got) == [] and bool((got[0].source.tensor == -1).all())


# ------------------------------------------------------------------------------------------------------------ circle NMS
A, B_, C_ = (5.5, 3.5), (6.25, 3.5), (7.0, 3.5)      # A-B and B-C are exactly 0.75 apart, A-C 1.5


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_distance_equal_to_the_threshold_suppresses_and_one_ulp_above_does_not_across_a_boundary(edge):
    K = edge + WAVE
    case = placed_case(K, {edge - 1: A, edge: B_}, grid=BIG)
    got, _ = both(case, UNIT, "equal", nms_threshold=THR)
    assert kept_ranks(got) == [k for k in range(K) if k != edge]
    got, _ = both(case, UNIT, "one ulp above", nms_threshold=BELOW)
    assert kept_ranks(got) == list(range(K))


@pytest.mark.parametrize("edge", [WAVE, THREADS])
@pytest.mark.parametrize("first", [-2, -1])
def test_a_suppressed_peak_suppresses_nothing_across_a_boundary(first, edge):
    """A kills B, only B would kill C: C survives — with A and B before the boundary and C behind it, and with only A before it"""
    K = edge + WAVE
    a = edge + first
    case = placed_case(K, {a: A, a + 1: B_, a + 2: C_}, grid=BIG)
    got, _ = both(case, UNIT, "chain", nms_threshold=THR)
    assert kept_ranks(got) == [k for k in range(K) if k != a + 1]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_an_invalid_peak_between_two_close_valid_ones_suppresses_nothing(edge):
    K = edge + WAVE
    scores = torch.linspace(0.9, 0.2, K).tolist()
    scores[edge] = 0.01                                   # B sits behind the boundary and fails the score test
    case = placed_case(K, {edge - 1: A, edge: B_, edge + 1: C_}, grid=BIG, scores=scores)
    got, _ = both(case, UNIT, "invalid between", nms_threshold=THR, score_threshold=0.1)
    assert kept_ranks(got) == [k for k in range(K) if k != edge]


@pytest.mark.parametrize("K", [WAVE + 1, THREADS + 1, 1024])
def test_all_peaks_on_one_centre_leave_one_survivor(K):
    case = placed_case(K, {k: A for k in range(K)}, grid=BIG)
    got, _ = both(case, UNIT, "one centre", nms_threshold=THR)
    assert kept_ranks(got) == [0]
    got, _ = both(case, UNIT, "one centre, threshold 0", nms_threshold=0.0)
    assert kept_ranks(got) == [0]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_threshold_zero_with_two_identical_centres(edge):
    K = edge + 2
    case = placed_case(K, {edge - 1: A, edge: A, 3: B_}, grid=BIG)
    got, _ = both(case, UNIT, "zero", nms_threshold=0.0)
    assert kept_ranks(got) == [k for k in range(K) if k != edge]
    got, _ = both(case, UNIT, "negative", nms_threshold=-1.0)       # nothing is within a negative distance
    assert kept_ranks(got) == list(range(K))


def test_per_task_thresholds_differ_and_tasks_do_not_see_each_others_peaks():
    """the same peaks in three tasks: B is suppressed where the threshold reaches it, and nowhere by another task's A"""
    K = THREADS + 2
    case = placed_case(K, {THREADS - 1: A, THREADS: B_}, grid=BIG, tasks=((4,), (9,), (1,)))
    case.peaks[2][1][0, THREADS - 1] = -1                            # task 2 has no A: its B must survive
    got, _ = both(case, UNIT, "per task", nms_threshold=[THR, BELOW, THR])
    assert kept_ranks(got, 0) == [k for k in range(K) if k != THREADS]
    assert kept_ranks(got, 1) == list(range(K))
    assert kept_ranks(got, 2) == [k for k in range(K) if k != THREADS - 1]
    got, _ = both(case, UNIT, "some without", nms_threshold=[None, THR, None])
    assert kept_ranks(got, 0) == list(range(K)) and kept_ranks(got, 1) == [k for k in range(K) if k != THREADS]


@pytest.mark.parametrize("post_max_size", [1, WAVE - 1, WAVE, WAVE + 1, 2000])
def test_the_cut_counts_kept_peaks_not_ranks(post_max_size):
    K = 2 * THREADS + 9
    case = make_case(3, K, ((5, 2), (7,)), seed=17)
    got, want = both(case, NUSC, f"post_max_size={post_max_size}", score_threshold=0.05, nms_threshold=[1.0, 4.0],
                     post_max_size=post_max_size)
    M = min(K, post_max_size)
    assert all(r.boxes.tensor.shape == (3, M, 9) for r in got)
    if 1 < post_max_size <= WAVE + 1:
        src = want[1]["source"]
        assert (want[1]["sizes"] == M).all() and (src[:, M - 1] > M - 1).all(), "the cut falls on a rank: it shows nothing"


# ------------------------------------------------------------------------------------------------------------ round trip
def test_round_trip_returns_every_kept_ground_truth_box():
    """boxes -> center_point_targets -> maps that hold the targets at the centres and a heat map of distinct scores there ->
    heatmap_peaks(kernel=1) -> center_point_decode: every kept ground-truth box comes back.  x, y within 1e-4 m: |x| <=
    51.2, where a float32 ulp is 3.8e-6, and at most six rounded operations lie each way; z, raw dims and velocity exact;
    yaw = the input wrapped to (-pi, pi], within BAR."""
    B, N, K = 3, 40, 32
    W, H = ct.NUSC["grid_size"]
    boxes, labels = ct.make_case(B, N, [40, 23, 31], seed=7, device=DEV)
    targets = center_point_targets(boxes, labels, NUSC_TASKS, **ct.NUSC, norm_bbox=False)
    peaks, feats, expect = [], [], []
    g = torch.Generator().manual_seed(3)
    for r, ids in zip(targets, NUSC_TASKS):
        n = r.indices.sample_sizes.cpu()
        assert 1 <= int(n.sum()) and int(n.max()) <= K, "a task without an object, or with more than K in a frame: pick another seed"
        heat = torch.zeros((B, len(ids), H, W), device=DEV)
        maps = torch.zeros((B, 10, H, W), device=DEV)
        per_frame = []
        for b in range(B):
            m = int(n[b])
            ind, lab = r.indices.tensor[b, :m], r.labels.tensor[b, :m].long()
            assert len(set(ind.tolist())) == m, "two objects of a task share a cell: pick another seed"
            score = (0.2 + 0.7 * torch.rand(m, generator=g)).to(DEV)
            heat[b, lab, ind // W, ind % W] = score
            maps[b, :, ind // W, ind % W] = r.targets.tensor[b, :m].t()
            per_frame.append((score.cpu(), r.source.tensor[b, :m].cpu().long(), [ids[i] for i in lab.tolist()]))
        expect.append(per_frame)
        peaks.append(heatmap_peaks(heat, K, kernel=1))
        feats.append([maps[:, :2].contiguous(), maps[:, 2:3].contiguous(), maps[:, 3:6].contiguous(), maps[:, 6:].contiguous()])
    out = op(peaks, feats, NUSC_TASKS, **NUSC, score_threshold=0.1, norm_bbox=False)
    gt = boxes.tensor.cpu()
    total = 0
    for d, per_frame in zip(out, expect):
        for b, (score, slots, ids) in enumerate(per_frame):
            m = len(slots)
            assert int(d.boxes.sample_sizes[b]) == m
            if m == 0:
                continue
            order = torch.argsort(score, descending=True)
            assert torch.equal(d.scores.tensor[b, :m].cpu(), score[order])
            assert d.labels.tensor[b, :m].tolist() == [ids[i] for i in order.tolist()]
            got, want = d.boxes.tensor[b, :m].cpu(), gt[b, slots[order]]
            assert float((got[:, :2] - want[:, :2]).abs().max()) <= 1e-4
            assert torch.equal(got[:, 2:6], want[:, 2:6]) and torch.equal(got[:, 7:], want[:, 7:])
            yaw = want[:, 6].double()
            assert float((got[:, 6].double() - torch.atan2(yaw.sin(), yaw.cos())).abs().max()) <= BAR
            total += m
    assert total >= 40


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,K,M,C", [(3, 70, 70, 10), (2, THREADS + 3, 83, 8), (1, 5, 1, 10)])
def test_guard_bands_and_complete_write_of_all_four_outputs_and_the_sizes(B, K, M, C):
    from accvlab import _amd_native as nat

    tasks, pad = NUSC_TASKS, 512
    T = len(tasks)
    case = make_case(B, K, tasks, C=C, seed=K, device=DEV)

    def banded(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
        return buf, buf[pad: pad + nbytes].view(dtype).view(shape)

    shapes = dict(boxes=((T, B, M, C - 1), torch.float32), scores=((T, B, M), torch.float32), labels=((T, B, M), torch.int64),
                  source=((T, B, M), torch.int32), sizes=((T, B), torch.int64))
    bands = {k: banded(*v) for k, v in shapes.items()}
    p = nat.CenterPointDecodeParams()
    first = 0
    for t, ((s, i, c), maps) in enumerate(zip(case.peaks, case.feats)):
        p.scores[t], p.indices[t], p.classes[t], p.num_maps[t] = s.data_ptr(), i.data_ptr(), c.data_ptr(), len(maps)
        for n, m in enumerate(maps):
            p.maps[t][n], p.channels[t][n] = m.data_ptr(), m.shape[1]
        p.has_nms[t], p.nms_threshold[t] = 1, NUSC_RADII[t]
        for cid in tasks[t]:
            p.class_ids[first] = cid
            first += 1
        p.task_first[t + 1] = first
    p.pc_range[0], p.pc_range[1], p.voxel_size[0], p.voxel_size[1], p.out_size_factor = -51.2, -51.2, 0.2, 0.2, 8.0
    p.has_score_threshold, p.score_threshold, p.num_tasks, p.norm_bbox = 1, 0.1, T, 1
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    status = nat.ctypes_lib().accv_center_point_decode(
        ctypes.addressof(p), B, K, 64, 64, M, *(bands[k][1].data_ptr() for k in ("boxes", "scores", "labels", "source", "sizes")), stream)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    torch.cuda.synchronize()
    for name, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{name}: wrote outside its buffer"
    # every slot inside was written: the pre-filled sentinel is gone wherever the definition has a value, padding included
    got = [CenterPointDetections(*(RaggedBatch(bands[k][1][t].clone(), sample_sizes=sizes) for k in ("boxes", "scores", "labels", "source")))
           for t, sizes in enumerate(bands["sizes"][1].clone().unbind(0))]
    check(got, definition(case.peaks, case.feats, tasks, **NUSC, score_threshold=0.1, nms_threshold=NUSC_RADII, post_max_size=M), "banded")


# -------------------------------------------------------------- reproducibility, no synchronisation, graphs, other streams
FULL = dict(score_threshold=0.1, post_center_range=NUSC_RANGE, nms_threshold=NUSC_RADII, post_max_size=83)


def _flat(result):
    return [x.tensor for r in result for x in r] + [r.boxes.sample_sizes for r in result]


def test_two_runs_are_bitwise_identical():
    case = make_case(3, 2 * THREADS + 1, seed=8, device=DEV)
    first = _flat(op(*case.op_args(), **NUSC, **FULL))
    for _ in range(2):
        for a, b in zip(first, _flat(op(*case.op_args(), **NUSC, **FULL))):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_no_host_synchronisation():
    case = make_case(3, 70, seed=9, device=DEV)
    args = case.op_args()
    op(*args, **NUSC, **FULL)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = op(*args, **NUSC, **FULL)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    check(got, definition(case.peaks, case.feats, case.tasks, **NUSC, **FULL))


def test_a_non_default_stream():
    case = make_case(3, THREADS + 9, seed=10, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = op(*case.op_args(), **NUSC, **FULL)
    stream.synchronize()
    check(got, definition(case.peaks, case.feats, case.tasks, **NUSC, **FULL), "side stream")


def test_graph_capture_and_replay_equal_eager():
    K = THREADS + 9
    a, b = make_case(3, K, seed=12, device=DEV), make_case(3, K, seed=13, device=DEV)
    live = a.clone()
    args = live.op_args()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            op(*args, **NUSC, **FULL)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(*args, **NUSC, **FULL)
    for case in (b, a):
        live.copy_(case)
        graph.replay()
        torch.cuda.synchronize()
        eager = op(*case.op_args(), **NUSC, **FULL)
        for x, y in zip(_flat(out), _flat(eager)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        check(out, definition(case.peaks, case.feats, case.tasks, **NUSC, **FULL), "replay")


def test_wrong_devices_are_refused():
    case = make_case(2, 6, ((0,), (1,)), seed=6, device=DEV)
    peaks, feats, tasks = case.op_args()
    feats[1][0] = feats[1][0].cpu()
    with pytest.raises(RuntimeError, match=r"center_point_decode: feats\[1\]\[0\] is on cpu, the peaks on cuda"):
        op(peaks, feats, tasks, **NUSC)
    peaks, feats, tasks = case.op_args()
    peaks[1] = peaks[1]._replace(indices=peaks[1].indices.cpu())
    with pytest.raises(RuntimeError, match=r"center_point_decode: peaks\[1\].indices must be int64 \(2, 6\) on cuda"):
        op(peaks, feats, tasks, **NUSC)
