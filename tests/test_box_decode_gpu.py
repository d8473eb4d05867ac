"""box_heatmap_decode and nms_boxes on the GPU: the kernels against the per-peak float32 definition of box_decode_cases.py and
against the host entries, bit for bit, at the edges of their work partition (wave block, chunk of kThreads slots, the
post_max_size cut), the IoU rule ON its boundary, a round trip through boxes_to_heatmap and heatmap_peaks (and through
camera_augment_boxes' matrix and back), guard bands, reproducibility, graph capture, no host synchronisation and a
non-default stream."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from box_decode_cases import (Case, check, check_device_against_host, definition, kept_ranks, make_case, nms_definition,  # noqa: E402
                              placed_case, run)

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import (BoxDetections, box_heatmap_decode, boxes_to_heatmap, camera_augment_boxes, heatmap_peaks,  # noqa: E402
                                  nms_boxes)

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = box_heatmap_decode


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "box_decode.hip")).read()
WAVE = int(_constant(_SRC, "kWave"))
THREADS = int(_constant(_SRC, "kThreads"))          # slots per chunk
assert (WAVE, THREADS) == (64, 256)
HW = (96, 160)                                      # image (H, W) over a 64 x 64 map: ux = 2.5, uy = 1.5
UNIT = (64, 64)                                     # image == map: ux = uy = 1, placed boxes come back exactly
BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))
A, B_ = (8, 8, 11, 12), (9, 8, 12, 12)              # integer corners: inter 8, union 16, IoU exactly 0.5


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


def both(case, what="", **kw):
    """`case` lives on the host: the device against the definition, and against the host path on the same inputs"""
    got, want = run(op, case.to(DEV), **kw)
    assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for x in got)
    check(got, want, what + " device")
    host = op(*case.op_args(), **dict(case.tensors, **kw))
    check_device_against_host(got, host, want["logits"], what + " device against host")
    return got, want


def _tensors(det):
    return tuple(x.tensor for x in det) + (det.boxes.sample_sizes,)


def _same(a, b, what=""):
    for x, y in zip(_tensors(a), _tensors(b)):
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), what


# --------------------------------------------------------------------------------------------- the kernels' work partition
@pytest.mark.parametrize("Fn", [0, 1, 3])
@pytest.mark.parametrize("K", [1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, 1024])
def test_peak_counts_across_wave_blocks_and_chunks(K, Fn):
    for grid in ((12, 8), (64, 64)):
        case = make_case(Fn, K, grid, E=1, seed=K + Fn, split=K)
        got, want = both(case, f"F={Fn} K={K} {grid}", image_hw=HW, score_threshold=0.05, min_size=(2.0, 3.0), iou_threshold=0.5)
        assert got.boxes.tensor.shape == (Fn, K, 4) and got.extras.tensor.shape == (Fn, K, 1)
        both(case, f"F={Fn} K={K} {grid} agnostic", image_hw=HW, iou_threshold=0.3, class_agnostic=True, clip=False)
        plain, _ = both(case, f"F={Fn} K={K} {grid} no options", image_hw=HW)
        again = nms_boxes(plain, 0.5)
        check(again, nms_definition(_tensors(plain), 0.5), f"F={Fn} K={K} {grid} nms_boxes")
    if Fn == 3 and K >= WAVE:
        assert 0 < want["sizes"].sum() < want["valid"].sum(), "the case suppresses nothing, or everything"


@pytest.mark.parametrize("dtype,score_dtype", [(torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)])
@pytest.mark.parametrize("E", [0, 1, 4])
def test_dtypes_extras_map_splits_logits_matrices_and_per_frame_extents(dtype, score_dtype, E):
    case = make_case(4, THREADS + 44, E=E, dtype=dtype, score_dtype=score_dtype, seed=E, logits=True, split=E + 1)
    case.tensors["image_hw"] = torch.tensor([[96, 160], [64, 64], [33, 1000], [0, 7]], dtype=torch.int32 if E else torch.int64)
    case.tensors["image_matrices"] = matrices(4, seed=E, singular=(2,))
    for order in (True, False):
        got, want = both(case, f"{dtype} {score_dtype} E={E} order={order}", scores_are_logits=True, score_threshold=0.1,
                         iou_threshold=0.45, post_max_size=83, order_corners=order)
    assert got.extras.tensor.shape == (4, 83, E)
    assert want["sizes"][2] > 0 and not bool(got.boxes.tensor[2].any()), "a singular matrix: zero boxes, the count kept"
    flipped = want["boxes"][1, : want["sizes"][1]]
    assert (flipped[:, 0] > flipped[:, 2]).any(), "order_corners=False leaves a flipped frame with x1 > x2"


def test_nan_and_inf_in_every_input_channel_and_invalid_indices():
    case = make_case(2, THREADS + 10, E=2, seed=5, illegal=0.2)
    s, idx, cls = case.peaks
    full = torch.cat(case.feats, 1)
    H, W = full.shape[2:]
    specials = [float("nan"), float("inf"), float("-inf")]
    n = 0
    for c in range(6):
        for v in specials:
            f, k = n % 2, 10 + 13 * n
            cell = int(idx[f, k]) if 0 <= int(idx[f, k]) < H * W else 5
            idx[f, k], cls[f, k] = cell, 1
            full[f, c, cell // W, cell % W] = v
            n += 1
    for j, v in enumerate(specials):
        s[1, 60 + j] = v
    case = Case([s, idx, cls], [full[:, :3].contiguous(), full[:, 3:].contiguous()])
    for kw in (dict(image_hw=HW, iou_threshold=0.5), dict(image_hw=HW, iou_threshold=0.5, clip=False, score_threshold=0.0),
               dict(image_hw=HW, min_size=1.0)):
        got, want = both(case, f"specials {sorted(kw)}", **kw)
    assert np.isnan(want["extras"]).any() and np.isinf(want["extras"]).any()


# ------------------------------------------------------------------------------------------------------------- IoU NMS
@pytest.mark.parametrize("later", [300, THREADS + WAVE, 1023])
def test_a_kept_box_of_block_0_suppresses_a_box_of_a_later_chunk(later):
    K = 1024
    case = placed_case(K, {5: A, later: A})
    got, _ = both(case, "later chunk", image_hw=UNIT, iou_threshold=0.5)
    assert kept_ranks(got) == [k for k in range(K) if k != later]
    got, _ = both(case, "later chunk, no NMS", image_hw=UNIT)
    assert kept_ranks(got) == list(range(K))
    assert kept_ranks(nms_boxes(got, 0.5)) == [k for k in range(K) if k != later]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_iou_equal_to_the_threshold_keeps_both_and_one_ulp_above_drops_one_across_a_boundary(edge):
    K = edge + WAVE
    case = placed_case(K, {edge - 1: A, edge: B_})
    got, _ = both(case, "equal", image_hw=UNIT, iou_threshold=0.5)
    assert kept_ranks(got) == list(range(K))
    assert got.boxes.tensor[0, edge - 1].tolist() == list(A) and got.boxes.tensor[0, edge].tolist() == list(B_)
    got, _ = both(case, "one ulp above", image_hw=UNIT, iou_threshold=BELOW)
    assert kept_ranks(got) == [k for k in range(K) if k != edge]
    plain = op(*case.to(DEV).op_args(), image_hw=UNIT)
    assert kept_ranks(nms_boxes(plain, 0.5)) == list(range(K))
    assert kept_ranks(nms_boxes(plain, BELOW)) == [k for k in range(K) if k != edge]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
@pytest.mark.parametrize("first", [-2, -1])
def test_a_suppressed_box_suppresses_nothing_across_a_boundary(first, edge):
    """P kills Q, only Q would kill R: R survives — with P and Q before the boundary and R behind it, and with only P before it"""
    K = edge + WAVE
    a = edge + first
    P, Q, R = (8, 8, 14, 12), (10, 8, 16, 12), (12, 8, 18, 12)       # neighbours overlap 4 / 8 = 0.5, P and R 2 / 10
    case = placed_case(K, {a: P, a + 1: Q, a + 2: R})
    got, _ = both(case, "chain", image_hw=UNIT, iou_threshold=0.4)
    assert kept_ranks(got) == [k for k in range(K) if k != a + 1]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_identical_boxes_of_two_classes_are_both_kept_and_one_with_class_agnostic(edge):
    K = edge + 3
    case = placed_case(K, {edge - 1: A, edge: A + (1,), edge + 1: A + (1,)})
    got, _ = both(case, "classes", image_hw=UNIT, iou_threshold=0.5)
    assert kept_ranks(got) == [k for k in range(K) if k != edge + 1]
    got, _ = both(case, "agnostic", image_hw=UNIT, iou_threshold=0.5, class_agnostic=True)
    assert kept_ranks(got) == [k for k in range(K) if k not in (edge, edge + 1)]


def test_a_box_without_area_is_kept_and_suppresses_nothing():
    K = WAVE + 3
    case = placed_case(K, {0: (10, 9, 10, 11), 1: A, WAVE: (10, 9, 10, 11), WAVE + 1: (9, 11, 9, 11)})
    for thr in (0.0, 0.5):
        got, _ = both(case, f"no area {thr}", image_hw=UNIT, iou_threshold=thr)
        assert kept_ranks(got) == list(range(K))
    got, _ = both(case, "no area, size test", image_hw=UNIT, iou_threshold=0.5, min_size=0.25)
    assert kept_ranks(got) == [k for k in range(K) if k not in (0, WAVE, WAVE + 1)]


@pytest.mark.parametrize("K", [WAVE + 1, THREADS + 1, 1024])
def test_all_peaks_on_one_box_leave_one_survivor(K):
    case = placed_case(K, {k: A for k in range(K)})
    got, _ = both(case, "one box", image_hw=UNIT, iou_threshold=0.5)
    assert kept_ranks(got) == [0]
    got, _ = both(case, "all invalid", image_hw=UNIT, iou_threshold=0.5, score_threshold=0.95)
    assert kept_ranks(got) == [] and bool((got.source.tensor == -1).all())


@pytest.mark.parametrize("post_max_size", [1, 30, WAVE, THREADS, 2000])
def test_the_cut_counts_kept_boxes_not_ranks(post_max_size):
    """inside a block, on a block edge, on a chunk edge"""
    K = 1024
    case = make_case(3, K, seed=17)
    got, want = both(case, f"post_max_size={post_max_size}", image_hw=HW, score_threshold=0.02, iou_threshold=0.3, post_max_size=post_max_size)
    M = min(K, post_max_size)
    assert got.boxes.tensor.shape == (3, M, 4)
    if 1 < post_max_size <= THREADS:
        assert (want["sizes"] == M).all() and (want["source"][:, M - 1] > M - 1).all(), "the cut falls on a rank: it shows nothing"
    plain = op(*case.to(DEV).op_args(), image_hw=HW, score_threshold=0.02)
    _same(nms_boxes(plain, 0.3, post_max_size=post_max_size), got, "nms_boxes against the fused call")


@pytest.mark.parametrize("pre,post", [(None, None), (100, None), (THREADS, 17), (THREADS + 1, WAVE), (1, 1)])
def test_nms_boxes_equals_its_definition_the_host_entry_and_the_fused_call(pre, post):
    case = make_case(3, THREADS + 70, E=2, seed=11)
    plain = op(*case.to(DEV).op_args(), image_hw=HW, score_threshold=0.05)
    host_sizes = plain.boxes.sample_sizes.cpu()
    host_in = BoxDetections(*(RaggedBatch(x.tensor.cpu(), sample_sizes=host_sizes) for x in plain))
    for thr, agnostic in ((0.5, False), (0.2, True), (None, False)):
        got = nms_boxes(plain, thr, class_agnostic=agnostic, pre_max_size=pre, post_max_size=post)
        check(got, nms_definition(_tensors(plain), thr, class_agnostic=agnostic, pre_max_size=pre, post_max_size=post), f"{thr} {pre} {post}")
        check_device_against_host(got, nms_boxes(host_in, thr, class_agnostic=agnostic, pre_max_size=pre, post_max_size=post), False)
        if pre is None and thr is not None:
            fused = op(*case.to(DEV).op_args(), image_hw=HW, score_threshold=0.05, iou_threshold=thr, class_agnostic=agnostic,
                       post_max_size=post)
            _same(got, fused, "nms_boxes against the fused call")


def test_nms_boxes_on_user_built_boxes_with_ragged_sizes_and_non_finite_rows():
    g = torch.Generator().manual_seed(3)
    Fn, N = 3, THREADS + 70
    xy = torch.rand(Fn, N, 2, generator=g) * 50
    boxes = torch.cat([xy, xy + 5 + torch.rand(Fn, N, 2, generator=g) * 30], 2)
    boxes[0, 3, 1], boxes[1, 0, 2], boxes[2, 5, 0], boxes[0, 300, 3] = float("nan"), float("inf"), float("-inf"), float("nan")
    sizes = torch.tensor([N, 0, 33]).to(DEV)
    det = BoxDetections(*(RaggedBatch(x.to(DEV), sample_sizes=sizes) for x in (
        boxes, torch.rand(Fn, N, generator=g), torch.randint(0, 2, (Fn, N), generator=g), torch.arange(N, dtype=torch.int32).repeat(Fn, 1),
        torch.rand(Fn, N, 0))))
    got = nms_boxes(det, 0.3)
    want = nms_definition(_tensors(det), 0.3)
    check(got, want, "user boxes")
    assert {3, 300} <= set(kept_ranks(got, 0)) and 5 in kept_ranks(got, 2) and want["sizes"][1] == 0 and 0 < want["sizes"][0] < N


# ------------------------------------------------------------------------------------------------------------ round trip
IMG, MAP, SRC = (100, 150), (24, 40), (120, 200)        # (H, W): the prepared image, the map, the source image
N_DECODE = 9


def _inner_boxes(Fn, G, seed):
    """float64 boxes [F, G, 4] (x1 < x2, y1 < y2) inside the part of IMG that boxes_to_heatmap does not clip, at least three
    map cells wide and high, with centres in distinct map cells"""
    rng = np.random.default_rng(seed)
    (Hi, Wi), (Hm, Wm) = IMG, MAP
    out = np.zeros((Fn, G, 4))
    for f in range(Fn):
        cells = set()
        g = 0
        while g < G:
            cx, cy = rng.uniform(12, Wi * (Wm - 1) / Wm - 12), rng.uniform(12, Hi * (Hm - 1) / Hm - 12)
            cell = (int(cx * Wm / Wi), int(cy * Hm / Hi))
            if any(abs(cell[0] - c[0]) <= 1 and abs(cell[1] - c[1]) <= 1 for c in cells):
                continue
            cells.add(cell)
            hw_, hh = rng.uniform(6, 11), rng.uniform(6, 11)
            out[f, g] = (cx - hw_, cy - hh, cx + hw_, cy + hh)
            g += 1
    return out


def _decode_targets(boxes, cats, sizes, K, **kw):
    """boxes_to_heatmap -> maps that hold center_offset and height_width at center and distinct scores there ->
    heatmap_peaks(kernel=1) -> box_heatmap_decode; returns the detections and the scores per frame and slot"""
    Fn, G = boxes.shape[:2]
    (Hm, Wm) = MAP
    t = boxes_to_heatmap(RaggedBatch(boxes, sample_sizes=sizes), image_hw=IMG, heatmap_hw=MAP, categories=cats, num_categories=3)
    assert bool(t.is_active.tensor.all()), "a box of the round trip is not active: the case is wrong"
    heat = torch.zeros((Fn, 3, Hm, Wm), device=DEV)
    feats = torch.zeros((Fn, 4, Hm, Wm), device=DEV)
    score = (0.2 + 0.7 * torch.rand(Fn, G, generator=torch.Generator().manual_seed(3))).to(DEV)
    f_ix = torch.arange(Fn, device=DEV)[:, None].expand(Fn, G)
    cx, cy = t.center.tensor[..., 0].long(), t.center.tensor[..., 1].long()
    heat[f_ix, cats.long(), cy, cx] = score
    feats[f_ix, :, cy, cx] = torch.cat([t.center_offset.tensor, t.height_width.tensor], 2)
    peaks = heatmap_peaks(heat, K, kernel=1)
    return op(peaks, feats, image_hw=IMG, score_threshold=0.1, **kw), score


def test_round_trip_returns_every_active_box():
    """boxes -> boxes_to_heatmap -> heatmap_peaks(kernel=1) -> box_heatmap_decode: every box comes back, in score order,
    within n * 2^-24 * L of its corner, L = 150 the largest image extent (every intermediate of the chain, taken back to
    image pixels, is at most L).  n counts the roundings that reach a corner, in units of 2^-24 * L: the scaled centre
    sx * ((b0 + b2) * 0.5) carries 3 (sx, the mean, the product; floor and the offset are exact, as is xs + off); each scaled
    corner sx * b carries 2, and w = X2 - X1 one more: 5, halved to 2.5; cx -+ 0.5 * w rounds once: 6.5; ux and the product
    by it: 8.5, so n = 9."""
    Fn, G, K = 3, 12, 16
    boxes = torch.tensor(_inner_boxes(Fn, G, 1), dtype=torch.float32, device=DEV)
    cats = torch.randint(0, 3, (Fn, G), generator=torch.Generator().manual_seed(2)).to(DEV)
    sizes = torch.full((Fn,), G, dtype=torch.int64, device=DEV)
    det, score = _decode_targets(boxes, cats, sizes, K)
    tol = N_DECODE * 2.0 ** -24 * max(IMG)
    assert det.boxes.sample_sizes.tolist() == [G] * Fn
    order = torch.argsort(score, 1, descending=True)
    assert torch.equal(det.scores.tensor[:, :G], score.gather(1, order))
    assert torch.equal(det.labels.tensor[:, :G], cats.gather(1, order))
    want = boxes.gather(1, order[..., None].expand(Fn, G, 4))
    err = float((det.boxes.tensor[:, :G].double() - want.double()).abs().max())
    assert 0 < err <= tol, f"round trip off by {err:.3e}, bar {tol:.3e}"


def test_round_trip_through_the_image_matrix_and_back():
    """source boxes -> camera_augment_boxes (the forward matrix, flip + scale + crop) -> the chain above -> box_heatmap_decode
    with image_matrices: every source box comes back.  The bar, derived the same way: the warp rounds 4 times
    (camera_boxes_arith.h's kPointRoundings) at magnitude P, the largest float64 intermediate of a*x + tx; the chain above
    adds 9 at L; both reach the source image through the inverse, whose gain is g = max(1 / |a|, 1 / |d|); the inverse
    itself rounds 8 times (box_decode_arith.h's kInverseRoundings) at Q, the largest float64 intermediate of
    d * (x - tx) / det: bar = ((4 * P + 9 * L) * g + 8 * Q) * 2^-24."""
    Fn, G, K = 3, 12, 16
    m = torch.tensor([[[0.7, 0.0, 4.5], [0.0, 0.8, 2.25]], [[-0.75, 0.0, 149.0], [0.0, 0.8, -3.5]], [[1.3, 0.0, -60.0], [0.0, 1.1, -20.0]]])
    prepared = _inner_boxes(Fn, G, 4)
    m64 = m.double().numpy()
    a, tx, d, ty = m64[:, 0, 0, None], m64[:, 0, 2, None], m64[:, 1, 1, None], m64[:, 1, 2, None]
    src = np.stack([(prepared[..., 0] - tx) / a, (prepared[..., 1] - ty) / d, (prepared[..., 2] - tx) / a, (prepared[..., 3] - ty) / d], -1)
    src = np.stack([np.minimum(src[..., 0], src[..., 2]), src[..., 1], np.maximum(src[..., 0], src[..., 2]), src[..., 3]], -1)
    boxes = torch.tensor(src, dtype=torch.float32, device=DEV)
    cats = torch.randint(0, 3, (Fn, G), generator=torch.Generator().manual_seed(2)).to(DEV)
    sizes = torch.full((Fn,), G, dtype=torch.int64, device=DEV)
    warped = camera_augment_boxes(RaggedBatch(boxes, sample_sizes=sizes), m.to(DEV), image_hw=IMG, check_occlusion=False, order_corners=True)
    assert warped.bboxes.sample_sizes.tolist() == [G] * Fn and torch.equal(warped.source.tensor, torch.arange(G, device=DEV).int().expand(Fn, G))
    det, score = _decode_targets(warped.bboxes.tensor, cats, sizes, K, image_matrices=m.to(DEV))
    order = torch.argsort(score, 1, descending=True)
    assert det.boxes.sample_sizes.tolist() == [G] * Fn and torch.equal(det.labels.tensor[:, :G], cats.gather(1, order))
    want = boxes.gather(1, order[..., None].expand(Fn, G, 4)).double().cpu()
    got = det.boxes.tensor[:, :G].double().cpu()
    for f in range(Fn):
        af, df, txf, tyf = (abs(float(v[f, 0])) for v in (a, d, tx, ty))
        P = max(af * max(SRC) + txf, df * max(SRC) + tyf, max(IMG))
        g = max(1 / af, 1 / df)
        Q = max((max(IMG) + txf) / af, (max(IMG) + tyf) / df)
        bar = ((4 * P + N_DECODE * max(IMG)) * g + 8 * Q) * 2.0 ** -24
        err = float((got[f] - want[f]).abs().max())
        assert 0 < err <= bar, f"frame {f}: round trip off by {err:.3e}, bar {bar:.3e}"


# ------------------------------------------------------------------------------------------------------------ guard bands
def _banded(shape, dtype, pad=512):
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
    return buf, buf[pad: pad + nbytes].view(dtype).view(shape)


def _bands(Fn, M, E):
    shapes = dict(boxes=((Fn, M, 4), torch.float32), scores=((Fn, M), torch.float32), labels=((Fn, M), torch.int64),
                  source=((Fn, M), torch.int32), extras=((Fn, M, E), torch.float32), sizes=((Fn,), torch.int64))
    return {k: _banded(*v) for k, v in shapes.items()}


def _check_bands(bands, pad=512):
    torch.cuda.synchronize()
    for name, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{name}: wrote outside its buffer"
    sizes = bands["sizes"][1].clone()
    return BoxDetections(*(RaggedBatch(bands[k][1].clone(), sample_sizes=sizes) for k in ("boxes", "scores", "labels", "source", "extras")))


@pytest.mark.parametrize("Fn,K,M,E", [(3, 70, 70, 1), (2, THREADS + 3, 83, 4), (1, 5, 1, 0)])
def test_guard_bands_and_complete_write_of_every_output(Fn, K, M, E):
    from accvlab import _amd_native as nat

    case = make_case(Fn, K, E=E, seed=K).to(DEV)
    s, i, c = case.peaks
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    bands = _bands(Fn, M, E)
    p = nat.BoxDecodeParams()
    p.scores, p.indices, p.classes, p.num_maps = s.data_ptr(), i.data_ptr(), c.data_ptr(), len(case.feats)
    for n, m in enumerate(case.feats):
        p.maps[n], p.channels[n] = m.data_ptr(), m.shape[1]
    p.image_h, p.image_w, p.clip = HW[0], HW[1], 1
    p.has_score_threshold, p.score_threshold, p.has_iou_threshold, p.iou_threshold = 1, 0.05, 1, 0.5
    outs = [bands[k][1].data_ptr() for k in ("boxes", "scores", "labels", "source", "extras", "sizes")]
    assert nat.ctypes_lib().accv_box_decode(ctypes.addressof(p), Fn, K, 64, 64, M, *outs, stream) == 0, nat.ctypes_lib().accv_last_error()
    # every slot inside was written: the pre-filled sentinel is gone wherever the definition has a value, padding included
    check(_check_bands(bands), definition(case.peaks, case.feats, image_hw=HW, score_threshold=0.05, iou_threshold=0.5, post_max_size=M), "banded")

    plain = op(*case.op_args(), image_hw=HW)
    pre = max(1, K - 2)
    M = min(M, pre)
    bands = _bands(Fn, M, E)
    q = nat.BoxNmsParams()
    q.boxes, q.scores, q.labels, q.source, q.sizes = (x.data_ptr() for x in _tensors(plain)[:4] + _tensors(plain)[5:])
    q.extras, q.has_threshold, q.iou_threshold = (plain.extras.tensor.data_ptr() if E else None), 1, 0.5
    outs = [bands[k][1].data_ptr() for k in ("boxes", "scores", "labels", "source", "extras", "sizes")]
    assert nat.ctypes_lib().accv_box_nms(ctypes.addressof(q), Fn, K, E, pre, M, *outs, stream) == 0, nat.ctypes_lib().accv_last_error()
    check(_check_bands(bands), nms_definition(_tensors(plain), 0.5, pre_max_size=pre, post_max_size=M), "banded nms")


# -------------------------------------------------------------- reproducibility, no synchronisation, graphs, other streams
FULL = dict(score_threshold=0.05, min_size=(2.0, 3.0), iou_threshold=0.5, post_max_size=183)


def _full_case(seed):
    case = make_case(3, 2 * THREADS + 1, E=2, seed=seed, split=1)
    case.tensors["image_hw"] = torch.tensor([[96, 160], [64, 64], [33, 1000]], dtype=torch.int32)
    case.tensors["image_matrices"] = matrices(3, seed=seed)
    return case.to(DEV)


def _call(case):
    det = op(*case.op_args(), **case.tensors, **FULL)
    return det, nms_boxes(op(*case.op_args(), **case.tensors), 0.4, pre_max_size=400, post_max_size=90)


def _want(case):
    plain = op(*case.op_args(), **case.tensors)
    return (definition(case.peaks, case.feats, **case.tensors, **FULL),
            nms_definition(_tensors(plain), 0.4, pre_max_size=400, post_max_size=90))


def test_two_runs_are_bitwise_identical():
    case = _full_case(8)
    first = _call(case)
    for _ in range(2):
        for a, b in zip(first, _call(case)):
            _same(a, b)


def test_no_host_synchronisation():
    case = _full_case(9)
    _call(case)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _call(case)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for g, w in zip(got, _want(case)):
        check(g, w, "no sync")


def test_a_non_default_stream():
    case = _full_case(10)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = _call(case)
    stream.synchronize()
    for g, w in zip(got, _want(case)):
        check(g, w, "side stream")


def test_graph_capture_and_replay_equal_eager():
    a, b = _full_case(12), _full_case(13)
    live = a.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            _call(live)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _call(live)
    for case in (b, a):
        live.copy_(case)
        graph.replay()
        torch.cuda.synchronize()
        for x, y, w in zip(out, _call(case), _want(case)):
            _same(x, y, "replay against eager")
            check(x, w, "replay")


def test_wrong_devices_are_refused():
    case = make_case(2, 6, E=1, seed=6).to(DEV)
    peaks, feats = case.op_args()
    with pytest.raises(RuntimeError, match=r"box_heatmap_decode: feats\[0\] is on cpu, the peaks on cuda"):
        op(peaks, [feats[0].cpu()] + feats[1:], image_hw=HW)
    with pytest.raises(RuntimeError, match=r"box_heatmap_decode: peaks.indices must be int64 \(2, 6\) on cuda"):
        op(peaks._replace(indices=peaks.indices.cpu()), feats, image_hw=HW)
    with pytest.raises(RuntimeError, match=r"image_matrices must be on the peaks' device"):
        op(peaks, feats, image_hw=HW, image_matrices=torch.zeros((2, 2, 3)))
    det = op(peaks, feats, image_hw=HW)
    with pytest.raises(RuntimeError, match=r"nms_boxes: detections.scores must be \(2, 6\) on cuda"):
        nms_boxes(det._replace(scores=RaggedBatch(det.scores.tensor.cpu(), sample_sizes=det.boxes.sample_sizes)), 0.5)
