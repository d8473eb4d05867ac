"""query_box_decode_3d and query_box_decode_2d on the GPU: the kernel against the per-rank float32 definitions of
query_decode_cases.py and against the host entries, at the edges of its work partition (a wave, the workgroup's T lanes, one
step of T * U scores of the select loop), on every input class (equal and two-valued logits, NaN / inf / signed zeros,
saturated logits, half precision), against heatmap_peaks and torch.topk, through the two NMS operators, with guard bands,
twice for reproducibility, captured in a graph and without host synchronisation."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from query_decode_cases import (HW, KINDS, RANGE, THR, check, check_device_against_host, definition_2d, definition_3d, logits,  # noqa: E402
                                matrices, max_nums, rows_2d, rows_3d, run)

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import (BoxDetections, CenterPointDetections, heatmap_peaks, nms_boxes, query_box_decode_2d,  # noqa: E402
                                  query_box_decode_3d, rotated_nms_bev)

pytestmark = pytest.mark.gpu

DEV = "cuda"
op3, op2 = query_box_decode_3d, query_box_decode_2d


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "query_decode.hip")).read()
T = int(_constant(_SRC, "kThreads"))          # lanes of a frame's workgroup
U = int(_constant(_SRC, "kUnroll"))           # loads per lane and step of the select loop
assert (T, U) == (1024, 8)
FULL3 = dict(score_threshold=THR, post_center_range=RANGE)
# (Q, C): N = Q * C takes 1, 63 / 64 / 65, T - 1 / T / T + 1 and T * U -+ 1; C takes 1, 3, 10 and 80, the last two next to T and T * U
SHAPES = [(1, 1), (21, 3), (64, 1), (65, 1), (341, 3), (T, 1), (T + 1, 1), (T * U - 1, 1), (2731, 3), (102, 10), (13, 80), (819, 10), (103, 80)]
assert {q * c for q, c in SHAPES} >= {1, 63, 64, 65, T - 1, T, T + 1, T * U - 1, T * U + 1}
assert any(q * c < T * U < (q + 1) * c for q, c in SHAPES if c == 10) and any((q - 1) * c < T * U < q * c for q, c in SHAPES if c == 80)


def _on(kw, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def both(op, definition, cls, rows, M, what="", **kw):
    """the inputs live on the host: the device against the definition, and against the host path on the same inputs"""
    got, want = run(op, definition, cls.to(DEV), rows.to(DEV), M, **_on(kw, DEV))
    assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for x in got)
    check(got, want, what + " device")
    host = op(cls, rows, M, **kw)
    check_device_against_host(got, host, want["approx_channels"], want["logits"], what + " device against host")
    return got, want


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert x.tensor.shape == y.tensor.shape and torch.equal(x.tensor.contiguous().view(torch.uint8), y.tensor.contiguous().view(torch.uint8)), what
        assert torch.equal(x.sample_sizes, y.sample_sizes), what


# ------------------------------------------------------------------------------------------- the kernel's work partition
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q,C", SHAPES)
def test_group_sizes_across_a_wave_the_workgroup_and_a_select_step(Q, C, B):
    N = Q * C
    kind = KINDS[(Q + C) % len(KINDS)]
    D = 10 if Q % 2 else 8
    cls, rows = logits(B, Q, C, kind, seed=N), rows_3d(B, Q, D, seed=N, special=kind == "special")
    for M in max_nums(N):
        got, _ = both(op3, definition_3d, cls, rows, M, f"3d {kind} Q={Q} C={C} B={B} M={M}", bottom_center=M % 2 == 1, **FULL3)
        assert isinstance(got, CenterPointDetections) and got.boxes.tensor.shape == (B, M, D - 1)
        both(op3, definition_3d, cls, rows, M, f"3d {kind} Q={Q} C={C} B={B} M={M} raw", scores_are_logits=False)
    r2 = rows_2d(B, Q, seed=N, special=kind == "special")
    for M in (max_nums(N)[0], max_nums(N)[-1]):
        got, _ = both(op2, definition_2d, cls, r2, M, f"2d {kind} Q={Q} C={C} B={B} M={M}", image_hw=HW, score_threshold=THR)
        assert isinstance(got, BoxDetections) and got.extras.tensor.shape == (B, M, 0)


def test_max_num_above_the_group_size_raises():
    cls, rows = logits(2, 9, 4).to(DEV), rows_3d(2, 9).to(DEV)
    with pytest.raises(RuntimeError, match=r"max_num = 37 exceeds Q \* C = 36"):
        op3(cls, rows, 37)
    with pytest.raises(RuntimeError, match=r"max_num must be an integer in 1\.\.1024, got 1025"):
        op2(logits(1, 400, 3).to(DEV), rows_2d(1, 400).to(DEV), 1025, image_hw=HW)
    with pytest.raises(RuntimeError, match="bbox_preds must be on the scores' device"):
        op3(cls, rows.cpu(), 5)


# ------------------------------------------------------------------------------------------------------- input classes
@pytest.mark.parametrize("kind", KINDS)
def test_every_input_class_across_a_select_step(kind):
    B, Q, C = 3, 2731, 3                      # N = T * U + 1
    cls = logits(B, Q, C, kind, seed=1)
    rows = rows_3d(B, Q, 10, seed=1, special=kind == "special")
    for M in (1, 65, 1024):
        both(op3, definition_3d, cls, rows, M, f"{kind} M={M}", **FULL3)
        both(op3, definition_3d, cls, rows, M, f"{kind} M={M} raw", scores_are_logits=False, score_threshold=-0.6, bottom_center=True)
    if kind == "two":
        assert bool(((cls.view(B, -1) > 0).sum(1) > 1024).all()), "every cut must fall inside the tie group of the high value"
    if kind == "equal":
        got = op3(cls.to(DEV), rows.to(DEV), 1024)
        assert torch.equal((got.source.tensor.long() * C + got.labels.tensor).cpu(), torch.arange(1024).expand(B, 1024))


def test_the_cut_inside_a_tie_group_takes_the_lowest_indices():
    B, Q, C = 2, 900, 10
    cls = logits(B, Q, C, "two", seed=4)
    high = (cls.view(B, -1) > 0).sum(1)
    assert bool((high > 1024).all())           # about 0.4 * 9000: the top 300 are all the high value
    got, _ = both(op3, definition_3d, cls, rows_3d(B, Q), 300, "two-valued")
    for b in range(B):
        want = torch.nonzero(cls[b].view(-1) > 0).view(-1)[:300]
        assert torch.equal((got.source.tensor[b].long() * C + got.labels.tensor[b]).cpu(), want)


def test_saturated_logits_rank_by_logit_then_index():
    cls = logits(2, 400, 10, "saturated", seed=6)
    got, _ = both(op3, definition_3d, cls, rows_3d(2, 400), 30, "saturated")
    assert int((got.scores.tensor[0] == 1.0).sum()) >= 20, "float32 sigmoid saturates: equal scores"
    picked = cls[0].view(-1)[(got.source.tensor[0].long() * 10 + got.labels.tensor[0]).cpu()]
    assert bool((picked.diff() < 0).all()), "the logits, not the saturated scores, give the order"


@pytest.mark.parametrize("dtype,row_dtype", [(torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)])
def test_half_precision_scores_and_rows(dtype, row_dtype):
    B, Q, C = 3, T + 1, 10
    for kind in ("distinct", "special"):
        cls = logits(B, Q, C, kind, dtype=dtype, seed=8)
        both(op3, definition_3d, cls, rows_3d(B, Q, 10, dtype=row_dtype, seed=2, special=kind == "special"), 300, f"3d {dtype} {row_dtype} {kind}",
             bottom_center=True, **FULL3)
        both(op2, definition_2d, cls, rows_2d(B, Q, dtype=row_dtype, seed=2), 300, f"2d {dtype} {row_dtype} {kind}", image_hw=HW, score_threshold=THR)


def test_raw_half_precision_scores_keep_the_sign_and_payload_of_a_nan():
    import query_decode_cases as qc

    qc.check_raw_half_nan(op3, op2, DEV)
    cls = logits(2, 40, 3, "special", dtype=torch.float16, seed=5)
    both(op3, definition_3d, cls, rows_3d(2, 40, 10, seed=5), 120, "raw float16 special", scores_are_logits=False)


def test_frames_with_no_valid_row_and_with_every_row_valid():
    cls = logits(3, 130, 10, seed=2)
    cls[0] -= 20.0
    cls[2] += 20.0
    got, _ = both(op3, definition_3d, cls, rows_3d(3, 130, seed=2), 1024, "none / some / all", score_threshold=THR)
    sizes = got.boxes.sample_sizes.tolist()
    assert sizes[0] == 0 and 0 < sizes[1] < 1024 and sizes[2] == 1024 and bool((got.source.tensor[0] == -1).all())


@pytest.mark.parametrize("D", [8, 10])
def test_centres_on_every_face_of_the_range_are_kept_and_one_ulp_outside_dropped(D):
    Q = 12
    cls = torch.linspace(3.0, -3.0, Q).view(1, Q, 1).contiguous()
    rows = rows_3d(1, Q, D, seed=1)
    rows[0, :, 0], rows[0, :, 1], rows[0, :, 4] = 1.0, -2.0, 0.5
    outside = lambda v, up: float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))   # noqa: E731
    for n, (col, lo, hi) in enumerate(((0, RANGE[0], RANGE[3]), (1, RANGE[1], RANGE[4]), (4, RANGE[2], RANGE[5]))):
        rows[0, 4 * n, col], rows[0, 4 * n + 1, col] = lo, hi
        rows[0, 4 * n + 2, col], rows[0, 4 * n + 3, col] = outside(lo, False), outside(hi, True)
    for bottom in (False, True):
        got, _ = both(op3, definition_3d, cls, rows, Q, f"faces D={D}", post_center_range=RANGE, bottom_center=bottom)
        assert got.source.tensor[0, :6].tolist() == [0, 1, 4, 5, 8, 9] and int(got.boxes.sample_sizes[0]) == 6


@pytest.mark.parametrize("box_format,normalized", [("cxcywh", True), ("xyxy", True), ("cxcywh", False), ("xyxy", False)])
def test_2d_formats_pixel_rows_per_frame_extents_and_matrices(box_format, normalized):
    B, Q, C = 4, 260, 10
    cls = logits(B, Q, C, "special", seed=3)
    rows = rows_2d(B, Q, box_format, normalized, seed=5, special=True)
    hw_t = torch.tensor([[96, 160], [64, 64], [33, 1000], [0, 7]], dtype=torch.int64 if normalized else torch.int32)
    mats = matrices(B, seed=1, singular=(2,))
    fmt = dict(box_format=box_format, normalized=normalized)
    for M in (65, 1024):
        both(op2, definition_2d, cls, rows, M, f"{fmt} M={M} plain", image_hw=HW, **fmt)
        both(op2, definition_2d, cls, rows, M, f"{fmt} M={M} unordered", image_hw=hw_t, image_matrices=mats, score_threshold=THR, order_corners=False, **fmt)
        got, want = both(op2, definition_2d, cls, rows, M, f"{fmt} M={M} unclipped", image_hw=hw_t, image_matrices=mats, clip=False, **fmt)
    assert want["sizes"][2] > 0 and not bool(got.boxes.tensor[2].any()), "a singular matrix: zero boxes, the count kept"
    assert got.scores.tensor[2, 0].isnan() or got.scores.tensor[2, 0] > 0


# -------------------------------------------------------------------------------------- against heatmap_peaks and topk
@pytest.mark.parametrize("Q,C,K", [(900, 10, 300), (103, 80, 1024), (21, 3, 63)])
def test_selection_equals_heatmap_peaks_on_the_same_view(Q, C, K):
    B = 3
    for kind in ("distinct", "two", "special"):
        cls = logits(B, Q, C, kind, seed=K).to(DEV)
        got = op3(cls, rows_3d(B, Q).to(DEV), K, scores_are_logits=False)
        peaks = heatmap_peaks(cls.view(B, 1, Q, C), K, kernel=1)
        assert got.boxes.sample_sizes.tolist() == [K] * B
        assert torch.equal(got.source.tensor.long(), peaks.ys) and torch.equal(got.labels.tensor, peaks.xs), kind
        if kind != "special":                     # peaks folds -0.0 onto +0.0 and NaN payloads; the decode copies the value
            assert torch.equal(got.scores.tensor.view(torch.int32), peaks.scores.view(torch.int32)), kind


def test_on_distinct_logits_the_pairs_are_those_of_sigmoid_topk():
    B, Q, C, K = 3, 900, 10, 300
    cls = logits(B, Q, C, "distinct", seed=12).to(DEV)
    assert all(len(torch.unique(cls[b])) == Q * C for b in range(B))
    got = op2(cls, rows_2d(B, Q).to(DEV), K, image_hw=HW, clip=True)
    assert got.boxes.sample_sizes.tolist() == [K] * B
    idx = cls.sigmoid().view(B, -1).topk(K).indices
    mine = got.source.tensor.long() * C + got.labels.tensor
    assert torch.equal(mine.sort(1).values, idx.sort(1).values)


# ------------------------------------------------------------------------------------------------------------- pipeline
def test_the_nms_operators_take_the_results_unchanged():
    cls = logits(3, 300, 10, seed=9).to(DEV)
    d3 = op3(cls, rows_3d(3, 300).to(DEV), 300, **FULL3)
    d2 = op2(cls, rows_2d(3, 300).to(DEV), 300, image_hw=HW, score_threshold=THR)
    _same(d3, rotated_nms_bev(d3, None)[0], "rotated_nms_bev without a threshold")
    _same(d2, nms_boxes(d2, None), "nms_boxes without a threshold")
    assert 0 < int(rotated_nms_bev(d3, 0.1)[0].boxes.sample_sizes.sum()) <= int(d3.boxes.sample_sizes.sum())
    assert 0 < int(nms_boxes(d2, 0.3).boxes.sample_sizes.sum()) < int(d2.boxes.sample_sizes.sum())


# ------------------------------------------------------------------------------------------------------------ guard bands
def _banded(shape, dtype, pad=512):
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
    return buf, buf[pad: pad + nbytes].view(dtype).view(shape)


def _bands(B, M, W):
    shapes = dict(boxes=((B, M, W), torch.float32), scores=((B, M), torch.float32), labels=((B, M), torch.int64),
                  source=((B, M), torch.int32), sizes=((B,), torch.int64))
    return {k: _banded(*v) for k, v in shapes.items()}


def _check_bands(bands, kind, pad=512):
    torch.cuda.synchronize()
    for name, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{name}: wrote outside its buffer"
    sizes = bands["sizes"][1].clone()
    members = [RaggedBatch(bands[k][1].clone(), sample_sizes=sizes) for k in ("boxes", "scores", "labels", "source")]
    if kind is BoxDetections:
        members.append(RaggedBatch(torch.empty(tuple(members[0].tensor.shape[:2]) + (0,), device=DEV), sample_sizes=sizes))
    return kind(*members)


@pytest.mark.parametrize("B,Q,C,M", [(3, 70, 1, 70), (2, T + 3, 3, 83), (1, 5, 1, 1), (2, 103, 80, 1024)])
def test_guard_bands_and_complete_write_of_every_output(B, Q, C, M):
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    cls = logits(B, Q, C, seed=M).to(DEV)
    r3, r2 = rows_3d(B, Q, 10, seed=M).to(DEV), rows_2d(B, Q, seed=M).to(DEV)
    names = ("boxes", "scores", "labels", "source", "sizes")

    bands = _bands(B, M, 9)
    p = nat.QueryDecode3dParams()
    p.cls_scores, p.bbox_preds, p.scores_are_logits = cls.data_ptr(), r3.data_ptr(), 1
    p.has_score_threshold, p.score_threshold, p.has_post_center_range = 1, THR, 1
    for n, v in enumerate(RANGE):
        p.post_center_range[n] = v
    assert lib.accv_query_decode_3d(ctypes.addressof(p), B, Q, C, 10, M, *(bands[k][1].data_ptr() for k in names), stream) == 0, lib.accv_last_error()
    # every slot inside was written: the pre-filled sentinel is gone wherever the definition has a value, padding included
    check(_check_bands(bands, CenterPointDetections), definition_3d(cls, r3, M, **FULL3), "banded 3d")

    bands = _bands(B, M, 4)
    q = nat.QueryDecode2dParams()
    q.cls_scores, q.bbox_preds, q.scores_are_logits, q.cxcywh, q.normalized, q.clip = cls.data_ptr(), r2.data_ptr(), 1, 1, 1, 1
    q.image_h, q.image_w, q.has_score_threshold, q.score_threshold = HW[0], HW[1], 1, THR
    assert lib.accv_query_decode_2d(ctypes.addressof(q), B, Q, C, M, *(bands[k][1].data_ptr() for k in names), stream) == 0, lib.accv_last_error()
    check(_check_bands(bands, BoxDetections), definition_2d(cls, r2, M, image_hw=HW, score_threshold=THR), "banded 2d")


# ----------------------------------------------------------------------------- reproducibility, no host synchronisation
def _call(cls, r3, r2, mats):
    return (op3(cls, r3, 300, bottom_center=True, **FULL3),
            op2(cls, r2, 300, image_hw=HW, image_matrices=mats, score_threshold=THR))


def _inputs(seed):
    B, Q, C = 3, 900, 10
    return (logits(B, Q, C, "special", seed=seed).to(DEV), rows_3d(B, Q, seed=seed).to(DEV), rows_2d(B, Q, seed=seed).to(DEV),
            matrices(B, seed=seed).to(DEV))


def test_two_runs_are_bitwise_identical():
    args = _inputs(8)
    first = _call(*args)
    for _ in range(2):
        for a, b in zip(first, _call(*args)):
            _same(a, b)


def test_graph_capture_and_replay_equal_eager():
    a, b = _inputs(12), _inputs(13)
    live = tuple(x.clone() for x in a)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            _call(*live)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _call(*live)
    for case in (b, a):
        for x, y in zip(live, case):
            x.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, _call(*case)):
            _same(x, y, "replay against eager")


def test_no_host_synchronisation():
    args = _inputs(9)
    _call(*args)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d3, d2 = _call(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    cls, r3, r2, mats = args
    check(d3, definition_3d(cls, r3, 300, bottom_center=True, **FULL3), "no sync 3d")
    check(d2, definition_2d(cls, r2, 300, image_hw=HW, image_matrices=mats.cpu(), score_threshold=THR), "no sync 2d")
