"""batched_matching_cost / batched_hungarian_match on the host path (accv_matching_cost_host) against a float64 oracle
of the per-pair formulas, the f32 composition of examples/matched_loss.py and scipy.  Needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matching_cost_cases import (BOX_TERMS, DTYPES, KINDS, assert_close_nan_aware, make_case, oracle,  # noqa: E402
                                 ragged, term_kwargs, tolerance)

SIZES = [0, 6, 3, 1, 6]   # ragged, an empty frame, G_b = G_max


def mc(*args, **kw):
    from accvlab.batching_helpers import batched_matching_cost

    return batched_matching_cost(*args, **kw)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("box_terms", sorted(BOX_TERMS))
@pytest.mark.parametrize("kind", KINDS)
def test_host_matches_float64_oracle(kind, box_terms, dtype):
    kw, D = term_kwargs(kind, box_terms)
    inp = make_case(5, 7, 11, SIZES, kind, D, kw["box_format"], dtype, seed=3)
    out = mc(*inp, **kw)
    want, pad, mag = oracle(*inp, **kw)
    assert out.tensor.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert out.tensor.shape == (5, 7, 6) and out.tensor.is_contiguous() and out.non_uniform_dim == 2
    assert torch.equal(out.sample_sizes, inp[1].sample_sizes)
    assert_close_nan_aware(out.tensor, want, tolerance(dtype), f"{kind}/{box_terms}/{dtype}", scale=mag)
    assert bool((out.tensor[pad] == 0.0).all())


@pytest.mark.parametrize("shape", [(1, 1, 3, [1]), (3, 1, 4, [2, 0, 5]), (2, 9, 5, [5, 5]), (2, 4, 2, [0, 0])])
@pytest.mark.parametrize("kind", KINDS)
def test_host_shapes(kind, shape):
    B, Q, C, sizes = shape
    kw, D = term_kwargs(kind, "l1_iou_giou_cxcywh")
    inp = make_case(B, Q, C, sizes, kind, D, kw["box_format"], torch.float32, seed=B + Q, label_dtype=torch.int32)
    out = mc(*inp, **kw)
    want, _, mag = oracle(*inp, **kw)
    assert_close_nan_aware(out.tensor, want, 1e-5, scale=mag)


def test_empty_batches_and_queries():
    for B, Q, sizes in ((0, 5, []), (3, 0, [1, 2, 0])):
        scores = torch.rand(B, Q, 4)
        labels = ragged(torch.zeros(B, max(sizes, default=0), dtype=torch.int64), sizes)
        out = mc(scores, labels)
        assert out.tensor.shape == (B, Q, max(sizes, default=0)) and out.non_uniform_dim == 2


def test_agrees_with_the_example_composition():
    import matched_loss as ml

    import accvlab.batching_helpers as bh

    for seed in range(3):
        gb_l, gl_l, _, pred_boxes, pred_scores, _ = ml.make_inputs(4, 60, 10, 25, "cpu", seed=seed)
        gt_boxes = bh.combine_data(gb_l)
        gt_labels = bh.combine_data(gl_l, other_with_same_sample_sizes=gt_boxes)
        want = (1.0 - ml._iou(pred_boxes.unsqueeze(2), gt_boxes.tensor.unsqueeze(1))) + \
               (1.0 - torch.einsum("bqc,bgc->bqg", pred_scores, ml._one_hot(gt_labels.tensor, 10)))
        got = mc(pred_scores, gt_labels, pred_boxes, gt_boxes, iou_weight=1.0, iou_eps=ml.EPS)
        valid = gt_labels.mask.unsqueeze(1).expand_as(want)
        assert float((got.tensor - want)[valid].abs().max()) <= 2e-6


@pytest.mark.parametrize("filler", [0.0, -0.0, -7.5, 1e30, -1e9, float("inf"), float("nan")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_padded_columns_hold_filler_bitwise(filler, dtype):
    kw, D = term_kwargs("neg_prob", "giou")
    inp = make_case(4, 5, 6, [3, 0, 6, 2], "neg_prob", D, "xyxy", dtype, seed=1)
    out = mc(*inp, **kw, filler=filler)
    pad = oracle(*inp, **kw)[1]
    want = torch.full((int(pad.sum()),), filler, dtype=out.tensor.dtype)
    assert torch.equal(bits(out.tensor[pad]), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_strided_box_view_equals_contiguous_bitwise(dtype):
    inp = make_case(3, 9, 10, [4, 7, 2], "focal", 8, "xyxy", dtype, seed=5, width=10)
    assert inp[2].stride(1) == 10 and not inp[2].is_contiguous()
    kw = dict(class_cost="focal", class_weight=2.0, l1_weight=0.25)
    strided_scores = torch.stack([inp[0], inp[0]], 1)[:, 0]   # a batch stride of two frames
    a = mc(strided_scores, inp[1], inp[2], inp[3], **kw)
    assert strided_scores.stride(0) == 2 * 9 * 10
    b = mc(inp[0].contiguous(), inp[1], inp[2].contiguous(), inp[3], **kw)
    assert torch.equal(bits(a.tensor), bits(b.tensor))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_special_values(kind, dtype):
    kw, D = term_kwargs(kind, "l1_iou_giou_cxcywh")
    kw["box_format"] = "xyxy"
    scores, labels, pboxes, gboxes = make_case(3, 8, 5, [6, 6, 4], kind, D, "xyxy", dtype, seed=2)
    scores[0, 1, :] = float("nan")
    scores[1, 2, labels.tensor[1, 0]] = float("inf")
    scores[1, 3, labels.tensor[1, 1]] = -float("inf")
    pboxes[0, 4, 2] = float("nan")
    pboxes[2, 5, 2] = float("inf")        # an infinitely wide box
    pboxes[2, 6, 0] = -float("inf")
    gboxes.tensor[1, 3, 1] = float("nan")
    gboxes.tensor[2, 2, 3] = float("inf")
    labels.tensor[0, 2] = -1               # out of range: NaN class term
    labels.tensor[2, 0] = 5
    labels.tensor[2, 1] = 1 << 40
    inp = (scores, labels, pboxes, gboxes)
    out = mc(*inp, **kw)
    want, _, mag = oracle(*inp, **kw)
    assert_close_nan_aware(out.tensor, want, tolerance(dtype), f"{kind}/{dtype}", scale=mag)
    assert bool(torch.isnan(out.tensor[0, :, 2]).all()) and bool(torch.isnan(out.tensor[0, 1, :6]).all())
    # a term whose weight is 0 is not evaluated: NaN in its inputs does not reach the pair
    only_cls = mc(*inp, class_cost=kind)
    assert not bool(torch.isnan(only_cls.tensor[0, 4, [0, 1, 3, 4, 5]]).any())
    assert not bool(torch.isnan(only_cls.tensor[1, :, 3]).any())
    only_box = mc(None, None, pboxes, gboxes, class_weight=0.0, iou_weight=1.0)
    assert not bool(torch.isnan(only_box.tensor[0, 1, :]).any())
    assert torch.equal(only_box.sample_sizes, gboxes.sample_sizes)


def test_bad_arguments_raise():
    kw, D = term_kwargs("one_minus_prob", "giou")
    scores, labels, pboxes, gboxes = make_case(2, 4, 3, [2, 1], "one_minus_prob", 4, "xyxy", torch.float32)
    cases = [
        (ValueError, dict(class_cost="softmax")),
        (ValueError, dict(box_format="xywh", iou_weight=1.0)),
        (TypeError, dict(iou_weight=1.0, boxes=(None, gboxes))),
        (TypeError, dict(iou_weight=1.0, boxes=(pboxes, gboxes.tensor))),
        (TypeError, dict(scores=scores.double(), iou_weight=1.0)),
        (TypeError, dict(scores=scores.long())),
        (TypeError, dict(labels=ragged(labels.tensor.float(), [2, 1]))),
        (ValueError, dict(scores=scores.transpose(1, 2).contiguous().transpose(1, 2))),
        (ValueError, dict(scores=scores[:1])),
        (ValueError, dict(scores=scores[:, :3], iou_weight=1.0)),
        (ValueError, dict(iou_weight=1.0, boxes=(torch.rand(2, 4, 5), ragged(torch.rand(2, 2, 5), [2, 1])))),
        (ValueError, dict(l1_weight=1.0, boxes=(torch.rand(2, 4, 17), ragged(torch.rand(2, 2, 17), [2, 1])))),
        (ValueError, dict(l1_weight=1.0, boxes=(pboxes, ragged(torch.rand(2, 2, 5), [2, 1])))),
        (ValueError, dict(l1_weight=1.0, boxes=(pboxes, ragged(torch.rand(2, 3, 4), [2, 1])))),
        (ValueError, dict(scores=scores.unsqueeze(0))),
    ]
    for err, c in cases:
        pb, gb = c.pop("boxes", (pboxes, gboxes))
        with pytest.raises(err):
            mc(c.pop("scores", scores), c.pop("labels", labels), pb, gb, **c)


@pytest.mark.parametrize("kind", KINDS)
def test_hungarian_match_on_cpu_equals_scipy(kind):
    from accvlab.batching_helpers import batched_hungarian_match

    kw, D = term_kwargs(kind, "l1_giou_cxcywh")
    inp = make_case(4, 30, 7, [12, 0, 30, 5], kind, D, kw["box_format"], torch.float32, seed=11)
    cost = mc(*inp, **kw)
    pred_ind, gt_ind = batched_hungarian_match(*inp, **kw)
    for b in range(4):
        g = int(cost.sample_sizes[b])
        rows, cols = linear_sum_assignment(cost.tensor[b, :, :g].numpy())
        n = int(pred_ind.sample_sizes[b])
        assert n == len(rows)
        assert np.array_equal(pred_ind.tensor[b, :n].numpy(), rows)
        assert np.array_equal(gt_ind.tensor[b, :n].numpy(), cols)
    # maximize and the device-status form pass through
    p2, g2, status = batched_hungarian_match(*inp, **kw, maximize=True, check=False)
    assert int(status.abs().sum()) == 0
    rows, cols = linear_sum_assignment(cost.tensor[0, :, :12].numpy(), maximize=True)
    assert np.array_equal(p2.tensor[0, :12].numpy(), rows) and np.array_equal(g2.tensor[0, :12].numpy(), cols)


def test_out_of_range_label_is_an_invalid_entry():
    from accvlab.batching_helpers import batched_hungarian_match

    scores, labels, pboxes, gboxes = make_case(2, 5, 4, [3, 2], "neg_prob", 4, "xyxy", torch.float32)
    labels.tensor[1, 1] = 4
    with pytest.raises(ValueError, match="invalid numeric entries"):
        batched_hungarian_match(scores, labels, class_cost="neg_prob")
    status = batched_hungarian_match(scores, labels, class_cost="neg_prob", check=False)[2]
    assert status.tolist() == [0, 2]
