"""batched_matching_cost on the GPU (the HIP kernel of csrc/matching_cost.hip) against the float64 oracle and the host
entry: every term but the focal one is the same operation sequence on both sides and must agree bit for bit."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matching_cost_cases import (BOX_TERMS, DTYPES, KINDS, assert_close_nan_aware, make_case, oracle,  # noqa: E402
                                 ragged, term_kwargs, tolerance)

DEV = torch.device("cuda", 0)
SIZES = [0, 6, 3, 1, 6]


def mc(*args, **kw):
    from accvlab.batching_helpers import batched_matching_cost

    return batched_matching_cost(*args, **kw)


def to_cpu(inp):
    scores, labels, pboxes, gboxes = inp
    return (scores.cpu(), ragged(labels.tensor.cpu(), labels.sample_sizes.cpu()), pboxes.cpu(),
            ragged(gboxes.tensor.cpu(), gboxes.sample_sizes.cpu()))


def bits(t):
    """bit patterns, every NaN as the same quiet NaN (its sign and payload are not specified)"""
    t = t.contiguous().cpu()
    t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def check_against_host(inp, kw, dtype, what):
    out = mc(*inp, **kw)
    assert out.tensor.device == inp[0].device and out.tensor.is_contiguous() and out.non_uniform_dim == 2
    want, _, mag = oracle(*inp, **kw)
    assert_close_nan_aware(out.tensor, want, tolerance(dtype), what + " vs oracle", scale=mag)
    host = mc(*to_cpu(inp), **kw)
    if kw.get("class_cost") == "focal" and kw.get("class_weight", 1.0) != 0.0:
        # the focal term (device expf / logf / powf against the host's) within 2e-6 (1 + |ref|) on its own; in a sum
        # with other terms that may cancel it, relative to its own size
        only = dict(kw, l1_weight=0.0, iou_weight=0.0, giou_weight=0.0)
        focal_host = mc(*to_cpu(inp), **only).tensor
        assert_close_nan_aware(mc(*inp, **only).tensor, focal_host.double(), 2e-6, what + " focal term vs host")
        assert_close_nan_aware(out.tensor, host.tensor.double(), 2e-6, what + " vs host", scale=focal_host)
    else:
        assert torch.equal(bits(out.tensor), bits(host.tensor)), what + ": GPU and host differ"
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("box_terms", sorted(BOX_TERMS))
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_matches_oracle_and_host(kind, box_terms, dtype):
    kw, D = term_kwargs(kind, box_terms)
    inp = make_case(5, 37, 11, SIZES, kind, D, kw["box_format"], dtype, seed=4, device=DEV)
    check_against_host(inp, kw, dtype, f"{kind}/{box_terms}/{dtype}")


@pytest.mark.parametrize("shape", [(1, 1, 3, [1]), (3, 1, 4, [2, 0, 5]), (2, 300, 5, [257, 300]), (3, 70, 7, [65, 0, 129]),
                                   (2, 4, 2, [0, 0]), (0, 5, 3, [])])
@pytest.mark.parametrize("label_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_gpu_shapes(shape, label_dtype):
    B, Q, C, sizes = shape
    kw, D = term_kwargs("one_minus_prob", "l1_iou_giou_cxcywh")
    inp = make_case(B, Q, C, sizes, "one_minus_prob", D, kw["box_format"], torch.float32, seed=Q, device=DEV,
                    label_dtype=label_dtype)
    check_against_host(inp, kw, torch.float32, str(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_gpu_strided_view_and_filler(dtype):
    inp = make_case(3, 40, 10, [4, 7, 2], "focal", 8, "xyxy", dtype, seed=5, device=DEV, width=10)
    kw = dict(class_cost="focal", class_weight=2.0, l1_weight=0.25, filler=-1e9)
    a = mc(*inp, **kw)
    b = mc(inp[0], inp[1], inp[2].contiguous(), inp[3], **kw)
    assert torch.equal(bits(a.tensor), bits(b.tensor))
    pad = oracle(*inp, **kw)[1]
    want = torch.full((int(pad.sum()),), -1e9, dtype=a.tensor.dtype)
    assert torch.equal(bits(a.tensor.cpu()[pad]), bits(want))
    check_against_host(inp, kw, dtype, f"strided/{dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_special_values(kind, dtype):
    kw, D = term_kwargs(kind, "l1_iou_giou_cxcywh")
    kw["box_format"] = "xyxy"
    scores, labels, pboxes, gboxes = make_case(3, 8, 5, [6, 6, 4], kind, D, "xyxy", dtype, seed=2)
    scores[0, 1, :] = float("nan")
    scores[1, 2, labels.tensor[1, 0]] = float("inf")
    scores[1, 3, labels.tensor[1, 1]] = -float("inf")
    pboxes[0, 4, 2] = float("nan")
    pboxes[2, 5, 2] = float("inf")
    pboxes[2, 6, 0] = -float("inf")
    gboxes.tensor[1, 3, 1] = float("nan")
    gboxes.tensor[2, 2, 3] = float("inf")
    labels.tensor[0, 2] = -1
    labels.tensor[2, 0] = 5
    labels.tensor[2, 1] = 1 << 40
    inp = (scores.to(DEV), ragged(labels.tensor.to(DEV), [6, 6, 4]), pboxes.to(DEV), ragged(gboxes.tensor.to(DEV), [6, 6, 4]))
    check_against_host(inp, kw, dtype, f"special/{kind}/{dtype}")


def test_fused_cost_matcher_equals_composed_matcher():
    import matched_loss as ml

    import accvlab.batching_helpers as bh

    for seed in range(5):
        gb_l, gl_l, _, pred_boxes, pred_scores, _ = ml.make_inputs(8, 900, 10, 100, DEV, seed=seed)
        gt_boxes = bh.combine_data(gb_l)
        gt_labels = bh.combine_data(gl_l, other_with_same_sample_sizes=gt_boxes)
        want_gt, want_pred = ml.match_batched_on_device(gt_boxes, gt_labels, pred_boxes, pred_scores)
        got_gt, got_pred = ml.match_batched_fused_cost(gt_boxes, gt_labels, pred_boxes, pred_scores)
        assert torch.equal(want_gt.sample_sizes, got_gt.sample_sizes)
        assert torch.equal(want_gt.tensor, got_gt.tensor) and torch.equal(want_pred.tensor, got_pred.tensor), seed
        composed = (1.0 - ml._iou(pred_boxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
                   (1.0 - torch.einsum("bqc,bgc->bqg", pred_scores, ml._one_hot(gt_labels.tensor, 10)))
        total = []
        for gt_i, pred_i in ((want_gt, want_pred), (got_gt, got_pred)):
            b = torch.arange(8, device=DEV).unsqueeze(1).expand_as(gt_i.tensor)
            v = composed[b, pred_i.tensor, gt_i.tensor]
            total.append(v.masked_fill(~gt_i.mask, 0.0).double().sum(1))
        assert float((total[0] - total[1]).abs().max()) <= 1e-4, seed


def test_hungarian_match_graph_capture_equals_eager():
    from accvlab.batching_helpers import batched_hungarian_match

    kw, D = term_kwargs("focal", "l1_giou_cxcywh")
    sizes = [30, 0, 50, 12]
    static = make_case(4, 100, 10, sizes, "focal", D, kw["box_format"], torch.float32, seed=0, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            batched_hungarian_match(*static, **kw, check=False)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = batched_hungarian_match(*static, **kw, check=False)
    for seed in (1, 2):
        new = make_case(4, 100, 10, sizes, "focal", D, kw["box_format"], torch.float32, seed=seed, device=DEV)
        static[0].copy_(new[0]), static[1].tensor.copy_(new[1].tensor), static[2].copy_(new[2])
        static[3].tensor.copy_(new[3].tensor)
        graph.replay()
        want = batched_hungarian_match(*new, **kw, check=False)
        torch.cuda.synchronize()
        for a, b in zip(out[:2], want[:2]):
            assert torch.equal(a.tensor, b.tensor) and torch.equal(a.sample_sizes, b.sample_sizes)
        assert torch.equal(out[2], want[2])


def test_label_out_of_range_raises_through_check():
    from accvlab.batching_helpers import batched_hungarian_match

    inp = make_case(2, 20, 4, [5, 3], "neg_prob", 4, "xyxy", torch.float32, seed=0, device=DEV)
    inp[1].tensor[1, 2] = 4
    with pytest.raises(ValueError, match="invalid numeric entries"):
        batched_hungarian_match(*inp, class_cost="neg_prob", giou_weight=1.0)
    status = batched_hungarian_match(*inp, class_cost="neg_prob", giou_weight=1.0, check=False)[2]
    assert status.tolist() == [0, 2]


# the benchmark cases at full size: F3, DETR, StreamPETR-like
FULL = {
    "f3": (8, 900, 10, 100, "one_minus_prob", dict(iou_weight=1.0), 4, "xyxy", None),
    "detr": (16, 100, 92, 50, "neg_prob", dict(l1_weight=5.0, giou_weight=2.0), 4, "cxcywh", None),
    "streampetr": (8, 900, 10, 150, "focal", dict(class_weight=2.0, l1_weight=0.25), 8, "xyxy", 10),
}


@pytest.mark.parametrize("case", sorted(FULL))
def test_full_size_cases(case):
    B, Q, C, G, kind, extra, D, fmt, width = FULL[case]
    g = torch.Generator().manual_seed(7)
    sizes = torch.randint(0, G + 1, (B,), generator=g).tolist()
    sizes[0] = G
    inp = make_case(B, Q, C, sizes, kind, D, fmt, torch.float32, seed=7, device=DEV, width=width)
    kw = dict(class_cost=kind, box_format=fmt, **extra)
    check_against_host(inp, kw, torch.float32, case)
