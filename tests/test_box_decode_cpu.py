"""box_heatmap_decode and nms_boxes on CPU tensors: the library's host entries against the float32 restatement of
box_decode_cases.py, bit for bit; the NMS decisions against a float64 greedy loop; every argument check; F == 0."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from box_decode_cases import (Case, check, definition, greedy_nms_f64, kept_ranks, make_case, nms_definition,  # noqa: E402
                              placed_case, run)

import accvlab.draw_heatmap as dh  # noqa: E402
from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import BoxDetections, HeatmapPeaks, box_heatmap_decode, nms_boxes  # noqa: E402

op = box_heatmap_decode
HW = (96, 160)       # image (H, W) over a 64 x 64 map: ux = 2.5, uy = 1.5


def matrices(Fn, seed=0, singular=()):
    """flip + scale + crop per frame: [[+-s, 0, tx], [0, t, ty]], and the frames of `singular` with a zero row"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros((Fn, 2, 3))
    for f in range(Fn):
        s, t = (0.4 + 0.9 * torch.rand(2, generator=g)).tolist()
        flip = f % 2 == 1
        m[f] = torch.tensor([[-s if flip else s, 0.0, (150.0 if flip else -13.5)], [0.0, t, -7.25 * f]])
        if f in singular:
            m[f, 1, :2] = 0.0
    return m


FULL = dict(image_hw=HW, score_threshold=0.05, min_size=(2.0, 3.0), iou_threshold=0.5, post_max_size=200)


def test_exports():
    for name in ("box_heatmap_decode", "nms_boxes", "BoxDetections"):
        assert name in dh.__all__ and hasattr(dh, name)
    assert BoxDetections._fields == ("boxes", "scores", "labels", "source", "extras")
    assert all(hasattr(dh, n) for n in dh.__all__)


@pytest.mark.parametrize("K", [1, 63, 65, 257, 1024])
@pytest.mark.parametrize("grid", [(12, 8), (64, 64)])
def test_host_entry_equals_the_definition(K, grid):
    case = make_case(3, K, grid, E=1, seed=K, split=K)
    for kw in (FULL, dict(image_hw=HW), dict(image_hw=HW, iou_threshold=0.3, class_agnostic=True, clip=False)):
        got, want = run(op, case, **kw)
        check(got, want, f"K={K} {grid} {sorted(kw)}")
    if K >= 63:
        assert 0 < want["sizes"].sum() < want["valid"].sum()


@pytest.mark.parametrize("dtype,score_dtype", [(torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)])
@pytest.mark.parametrize("E", [0, 1, 4])
def test_dtypes_extras_map_splits_logits_matrices_and_per_frame_extents(dtype, score_dtype, E):
    case = make_case(4, 300, E=E, dtype=dtype, score_dtype=score_dtype, seed=E, logits=True, split=E + 1)
    case.tensors["image_hw"] = torch.tensor([[96, 160], [64, 64], [33, 1000], [0, 7]], dtype=torch.int32 if E else torch.int64)
    case.tensors["image_matrices"] = matrices(4, seed=E, singular=(2,))
    for order in (True, False):
        got, want = run(op, case, scores_are_logits=True, score_threshold=0.1, iou_threshold=0.45, post_max_size=83, order_corners=order)
        check(got, want, f"{dtype} {score_dtype} E={E} order={order}")
    assert got.extras.tensor.shape == (4, 83, E)
    assert want["sizes"][2] > 0 and not got.boxes.tensor[2].any(), "a singular matrix: zero boxes, the count kept"
    assert got.scores.tensor[2, 0] > 0
    flipped = want["boxes"][1, : want["sizes"][1]]
    assert (flipped[:, 0] > flipped[:, 2]).any(), "order_corners=False leaves a flipped frame with x1 > x2"


def test_nan_and_inf_in_every_input_channel_and_invalid_indices():
    case = make_case(2, 200, E=2, seed=5, illegal=0.2)
    s, idx, cls = case.peaks
    full = torch.cat(case.feats, 1)
    H, W = full.shape[2:]
    specials = [float("nan"), float("inf"), float("-inf")]
    n = 0
    for c in range(6):
        for v in specials:
            f, k = n % 2, 10 + n
            cell = int(idx[f, k]) if 0 <= int(idx[f, k]) < H * W else 5
            idx[f, k], cls[f, k] = cell, 1
            full[f, c, cell // W, cell % W] = v
            n += 1
    for j, v in enumerate(specials):
        s[1, 60 + j] = v
    case = Case([s, idx, cls], [full[:, :3].contiguous(), full[:, 3:].contiguous()])
    for kw in (dict(image_hw=HW, iou_threshold=0.5), dict(image_hw=HW, iou_threshold=0.5, clip=False, score_threshold=0.0),
               dict(image_hw=HW, min_size=1.0)):
        got, want = run(op, case, **kw)
        check(got, want, f"specials {sorted(kw)}")
    assert np.isnan(want["extras"]).any() and np.isinf(want["extras"]).any()


@pytest.mark.parametrize("seed,K,thr,agnostic,size", [(1, 300, 0.5, False, (0.2, 0.6)), (2, 500, 0.4, True, (0.1, 0.3)),
                                                      (2, 1024, 0.6, False, (0.2, 0.6)), (1, 100, 0.45, True, (0.2, 0.6))])
def test_nms_decisions_equal_the_float64_greedy_loop(seed, K, thr, agnostic, size):
    """The decoded float32 boxes, then a float64 greedy NMS over them: the kept ranks are the operator's.  No compared pair
    may lie within 1e-5 of the threshold (the seeds above were chosen so), and the cases must suppress a meaningful share."""
    Fn = 3
    case = make_case(Fn, K, seed=seed, illegal=0.0, size=size, classes=2)
    plain = op(*case.op_args(), image_hw=HW, score_threshold=0.02)
    got = op(*case.op_args(), image_hw=HW, score_threshold=0.02, iou_threshold=thr, class_agnostic=agnostic)
    again = nms_boxes(plain, thr, class_agnostic=agnostic)
    valid = kept = 0
    for f in range(Fn):
        n = int(plain.boxes.sample_sizes[f])
        boxes, labels = plain.boxes.tensor[f, :n].double().numpy(), plain.labels.tensor[f, :n].tolist()
        keep, gap = greedy_nms_f64(boxes, labels, thr, agnostic)
        assert gap > 1e-5, f"a pair's IoU lies {gap:.2e} from the threshold: pick another seed"
        assert kept_ranks(got, f) == plain.source.tensor[f, keep].tolist() == kept_ranks(again, f)
        valid, kept = valid + n, kept + len(keep)
    assert valid - kept > valid / 4 and kept > valid / 4, f"{kept} of {valid} kept: the case shows too little"


def _tensors(det):
    return tuple(x.tensor for x in det) + (det.boxes.sample_sizes,)


@pytest.mark.parametrize("pre,post", [(None, None), (100, None), (None, 17), (130, 64), (1, 1)])
def test_nms_boxes_equals_its_definition_and_the_fused_call(pre, post):
    case = make_case(3, 300, E=2, seed=11)
    plain = op(*case.op_args(), image_hw=HW, score_threshold=0.05)
    for thr, agnostic in ((0.5, False), (0.2, True), (None, False)):
        got = nms_boxes(plain, thr, class_agnostic=agnostic, pre_max_size=pre, post_max_size=post)
        check(got, nms_definition(_tensors(plain), thr, class_agnostic=agnostic, pre_max_size=pre, post_max_size=post), f"{thr} {pre} {post}")
        if pre is None and thr is not None:
            fused = op(*case.op_args(), image_hw=HW, score_threshold=0.05, iou_threshold=thr, class_agnostic=agnostic, post_max_size=post)
            for a, b in zip(_tensors(got), _tensors(fused)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_nms_boxes_on_user_built_boxes_with_unordered_sizes_and_non_finite_rows():
    g = torch.Generator().manual_seed(3)
    Fn, N = 3, 70
    xy = torch.rand(Fn, N, 2, generator=g) * 50
    boxes = torch.cat([xy, xy + 5 + torch.rand(Fn, N, 2, generator=g) * 30], 2)
    boxes[0, 3, 1], boxes[1, 0, 2], boxes[2, 5, 0] = float("nan"), float("inf"), float("-inf")
    sizes = torch.tensor([70, 0, 33])
    det = BoxDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in (
        boxes, torch.rand(Fn, N, generator=g), torch.randint(0, 2, (Fn, N), generator=g), torch.arange(N, dtype=torch.int32).repeat(Fn, 1),
        torch.rand(Fn, N, 0))))
    got = nms_boxes(det, 0.3)
    want = nms_definition(_tensors(det), 0.3)
    check(got, want, "user boxes")
    assert 3 in kept_ranks(got, 0) and 5 in kept_ranks(got, 2) and want["sizes"].tolist()[1] == 0 and 0 < want["sizes"][0] < 70


def test_placed_rules_on_the_host():
    """the placed cases of the GPU file, on the host entry (they are cheap here)"""
    A, B_ = (8, 8, 11, 12), (9, 8, 12, 12)                     # inter 8, union 16: IoU exactly 0.5
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    case = placed_case(6, {1: A, 4: B_})
    got, want = run(op, case, image_hw=(64, 64), iou_threshold=0.5)
    check(got, want, "equal")
    assert kept_ranks(got) == [0, 1, 2, 3, 4, 5] and got.boxes.tensor[0, 1].tolist() == list(A)
    got, _ = run(op, case, image_hw=(64, 64), iou_threshold=below)
    assert kept_ranks(got) == [0, 1, 2, 3, 5]
    case = placed_case(4, {0: A, 2: A + (1,)})                 # identical boxes of two classes
    assert kept_ranks(run(op, case, image_hw=(64, 64), iou_threshold=0.5)[0]) == [0, 1, 2, 3]
    assert kept_ranks(run(op, case, image_hw=(64, 64), iou_threshold=0.5, class_agnostic=True)[0]) == [0, 1, 3]
    case = placed_case(5, {0: (10, 9, 10, 11), 1: A, 2: (10, 9, 10, 11), 3: (9, 11, 9, 11)})   # boxes without area
    assert kept_ranks(run(op, case, image_hw=(64, 64), iou_threshold=0.0)[0]) == [0, 1, 2, 3, 4]


def test_empty_batch():
    case = make_case(0, 7, E=2)
    got = op(*case.op_args(), image_hw=HW, iou_threshold=0.5, post_max_size=5)
    assert [tuple(x.tensor.shape) for x in got] == [(0, 5, 4), (0, 5), (0, 5), (0, 5), (0, 5, 2)]
    assert got.boxes.sample_sizes.shape == (0,) and got.boxes.sample_sizes.dtype == torch.int64
    again = nms_boxes(got, 0.5, post_max_size=3)
    assert [tuple(x.tensor.shape) for x in again] == [(0, 3, 4), (0, 3), (0, 3), (0, 3), (0, 3, 2)]
    check(got, definition(case.peaks, case.feats, image_hw=HW, iou_threshold=0.5, post_max_size=5), "F == 0")


# ------------------------------------------------------------------------------------------------------ argument checks
def _launches(monkeypatch):
    """every native call of the two operators is counted; a refused call must leave the list empty"""
    from accvlab._amd_native import operands

    calls = []
    real = operands.run
    monkeypatch.setattr(operands, "run", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    return calls


def test_decode_argument_checks(monkeypatch):
    calls = _launches(monkeypatch)
    case = make_case(2, 6, E=1)
    peaks, feats = case.op_args()
    ok = dict(image_hw=HW)

    def refused(match, p=peaks, f=feats, exc=RuntimeError, **kw):
        with pytest.raises(exc, match=match):
            op(p, f, **dict(ok, **kw))

    refused("peaks must be a HeatmapPeaks", p=(1, 2, 3))
    refused(r"peaks.scores must be \[F, K\]", p=peaks._replace(scores=peaks.scores[0]))
    refused("peaks.indices must be contiguous", p=peaks._replace(indices=peaks.indices.t().contiguous().t()))
    refused("peaks.scores must be float32, float16 or bfloat16", p=peaks._replace(scores=peaks.scores.double()))
    refused(r"peaks.classes must be int64 \(2, 6\)", p=peaks._replace(classes=peaks.classes.int()))
    refused(r"peaks.indices must be int64 \(2, 6\)", p=peaks._replace(indices=peaks.indices[:, :5].contiguous()))
    big = torch.zeros((1, 1025))
    refused("K must be in 1..1024", p=HeatmapPeaks(big, big.long(), big.long(), big.long(), big.long()), f=[feats[0][:1]])
    refused("feats must be a tensor or a non-empty sequence", f=[])
    refused("at most 8 maps", f=[feats[0]] * 9)
    refused(r"feats\[1\] must be a tensor", f=[feats[0], 3])
    refused(r"feats\[0\] must be \[F, C, H, W\]", f=[feats[0][0]])
    refused(r"feats\[0\] must be contiguous", f=[feats[0].transpose(2, 3)])
    refused("feats must be float32, float16 or bfloat16", f=[f.double() for f in feats])
    refused(r"feats\[1\] has dtype", f=[feats[0], feats[1].half()] if len(feats) > 1 else [feats[0], feats[0].half()])
    refused(r"feats\[0\] has shape", f=[feats[0][:1]])
    refused(r"4..8 channels in total", f=[feats[0][:, :3].contiguous()])
    refused(r"4..8 channels in total", f=[feats[0], feats[0]])
    refused("image_hw must be", image_hw=(96.0, 160))
    refused("image_hw tensor must be int32 or int64", image_hw=torch.zeros((2, 2)))
    refused("image_hw tensor must be int32 or int64", image_hw=torch.zeros((3, 2), dtype=torch.int32))
    refused("image_matrices must be a tensor", image_matrices=[1.0])
    refused(r"image_matrices must be float32 \[2, 2, 3\]", image_matrices=torch.zeros((2, 3, 3)))
    refused(r"image_matrices must be float32 \[2, 2, 3\]", image_matrices=torch.zeros((2, 2, 3), dtype=torch.float64))
    refused("image_matrices must be contiguous", image_matrices=torch.zeros((2, 3, 2)).transpose(1, 2))
    refused("score_threshold must be a Python number", score_threshold="0.1")
    refused("score_threshold must not be NaN", score_threshold=float("nan"))
    refused("iou_threshold must be a Python number", iou_threshold=torch.tensor(0.5))
    refused("iou_threshold must not be NaN", iou_threshold=float("nan"))
    refused("min_size must be a Python number, an", min_size=(1, 2, 3))
    refused("min_size must not hold NaN", min_size=(1.0, float("nan")))
    refused("post_max_size must be a Python integer", post_max_size=2.0)
    refused("post_max_size must be at least 1", post_max_size=0)
    with pytest.raises(TypeError):
        op(peaks, feats)                                          # image_hw is required
    assert calls == []
    op(peaks, feats, **ok)
    assert calls == ["accv_box_decode"]


def test_nms_boxes_argument_checks(monkeypatch):
    case = make_case(2, 6, E=1)
    det = op(*case.op_args(), image_hw=HW)
    calls = _launches(monkeypatch)

    def refused(match, d=det, thr=0.5, **kw):
        with pytest.raises(RuntimeError, match=match):
            nms_boxes(d, thr, **kw)

    refused("detections must be a BoxDetections", d=tuple(det)[:4])
    refused("detections.scores must be a RaggedBatch", d=det._replace(scores=det.scores.tensor))
    sizes = det.boxes.sample_sizes
    rb = lambda t, s=sizes: RaggedBatch(t, sample_sizes=s)   # noqa: E731
    refused(r"detections.boxes must be \[F, N, 4\]", d=det._replace(boxes=rb(det.boxes.tensor[..., 0])))
    refused(r"detections.boxes must be \[F, N, 4\] as", d=det._replace(boxes=rb(det.boxes.tensor[..., :3].contiguous())))
    refused("detections.boxes must be float32", d=det._replace(boxes=rb(det.boxes.tensor.double())))
    refused("detections.labels must be int64", d=det._replace(labels=rb(det.labels.tensor.int())))
    refused("detections.source must be int32", d=det._replace(source=rb(det.source.tensor.long())))
    refused("detections.extras must be contiguous", d=det._replace(extras=rb(torch.zeros((6, 2, 1)).transpose(0, 1))))
    refused(r"detections.scores must be \(2, 6\)", d=det._replace(scores=rb(det.scores.tensor[:, :5].contiguous())))
    refused("E must be in 0..4", d=det._replace(extras=rb(torch.zeros((2, 6, 5)))))
    refused("sample_sizes of detections.boxes must be an int64 tensor", d=det._replace(boxes=rb(det.boxes.tensor, sizes.int())))
    refused("does not share the sample_sizes", d=det._replace(labels=rb(det.labels.tensor, sizes.clone())))
    wide = torch.zeros((1, 1025))
    one = torch.zeros((1,), dtype=torch.int64)
    refused("N must be in 1..1024", d=BoxDetections(rb(torch.zeros((1, 1025, 4)), one), rb(wide, one), rb(wide.long(), one),
                                                     rb(wide.int(), one), rb(torch.zeros((1, 1025, 0)), one)))
    refused("iou_threshold must be a Python number", thr="x")
    refused("iou_threshold must not be NaN", thr=float("nan"))
    refused("pre_max_size must be a Python integer", pre_max_size=1.5)
    refused("pre_max_size must be at least 1", pre_max_size=0)
    refused("post_max_size must be at least 1", post_max_size=-3)
    assert calls == []
    nms_boxes(det, 0.5)
    assert calls == ["accv_box_nms"]


def test_c_abi_checks_refuse_before_reading():
    """the native checks behind the Python ones, through plain ctypes: status and message, nothing read or written"""
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    p = nat.BoxDecodeParams()
    d = ctypes.c_void_p(64)
    call = lambda fn, *a: (fn(ctypes.addressof(p), *a), lib.accv_last_error().decode())   # noqa: E731
    assert lib.accv_box_decode_cpu(None, 1, 1, 1, 1, 1, d, d, d, d, d, d) == -1 and b"null params" in lib.accv_last_error()
    assert call(lib.accv_box_decode_cpu, 1, 0, 4, 4, 1, d, d, d, d, d, d) == (-1, "box_heatmap_decode (host): K must be in 1..1024, got 0")
    assert call(lib.accv_box_decode_cpu, 1, 4, 4, 4, 5, d, d, d, d, d, d)[1].endswith("M must be in 1..K = 4, got 5")
    assert "1..8 maps" in call(lib.accv_box_decode_cpu, 1, 4, 4, 4, 4, d, d, d, d, d, d)[1]
    p.num_maps, p.channels[0] = 1, 3
    assert "hold 3 channels" in call(lib.accv_box_decode_cpu, 1, 4, 4, 4, 4, d, d, d, d, d, d)[1]
    p.channels[0] = 4
    assert call(lib.accv_box_decode_cpu, 0, 4, 4, 4, 4, None, None, None, None, None, None)[0] == 0
    assert "null output pointer" in call(lib.accv_box_decode_cpu, 1, 4, 4, 4, 4, None, d, d, d, d, d)[1]
    assert "null peaks pointer" in call(lib.accv_box_decode_cpu, 1, 4, 4, 4, 4, d, d, d, d, None, d)[1]
    q = nat.BoxNmsParams()
    call = lambda fn, *a: (fn(ctypes.addressof(q), *a), lib.accv_last_error().decode())   # noqa: E731
    assert call(lib.accv_box_nms_cpu, 1, 1025, 0, 1, 1, d, d, d, d, d, d) == (-1, "nms_boxes (host): N must be in 1..1024, got 1025")
    assert "M must be in 1..min(N, pre_max_size) = 3" in call(lib.accv_box_nms_cpu, 1, 8, 0, 3, 4, d, d, d, d, d, d)[1]
    assert "null input pointer" in call(lib.accv_box_nms_cpu, 1, 8, 0, 3, 3, d, d, d, d, d, d)[1]
    assert call(lib.accv_box_nms_cpu, 0, 8, 0, 3, 3, None, None, None, None, None, None)[0] == 0


def test_the_host_entries_stay_on_ctypes():
    from accvlab import _amd_native as nat

    lib = nat.lib()
    for name in ("accv_box_decode_cpu", "accv_box_nms_cpu"):
        assert name in nat.SIGNATURES and not name.endswith("_host") and name not in nat._BLOCKING
        assert getattr(lib, name) is getattr(nat.ctypes_lib(), name)
