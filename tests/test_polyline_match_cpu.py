"""batched_polyline_matching_cost, batched_polyline_hungarian_match and matched_polyline_loss on CPU tensors (the host
entries of csrc/polyline_match.hip) against the float64 definition of tests/polyline_match_cases.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from polyline_match_cases import (DTYPES, MARGIN, PAIRS, SIZES, bits, check_cost, compare, cost_definition, definition,  # noqa: E402
                                  make_case, name, orders, ragged, run)

from accvlab.batching_helpers import RaggedBatch, batched_linear_sum_assignment  # noqa: E402
from accvlab.lane_helpers.polyline import (batched_polyline_hungarian_match, batched_polyline_matching_cost,  # noqa: E402
                                           matched_polyline_loss)

mpl = matched_polyline_loss
cost_op = batched_polyline_matching_cost


# ----------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("P", [2, 5, 20])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("closed", ["open", "closed", "mixed"])
@pytest.mark.parametrize("reversible", [True, False])
def test_loss_matches_definition(reversible, closed, D, P, dtype):
    inp = make_case(5, 7, P, D, SIZES, PAIRS, dtype, seed=P + D, closed=closed, reversible=reversible)
    g = torch.Generator().manual_seed(1)
    out, grad = compare(mpl, inp, f"{name(dtype)}/P{P}/D{D}/{closed}/rev{reversible}", reversible=reversible,
                        grad_out=torch.rand(2, 5, generator=g) + 0.5)
    assert bool((out[:, 1:3] == 0).all()) and bool((bits(grad[1:3]) == 0).all())   # no ground truth / no pairs: exactly 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms_and_dir_loss_off(dtype):
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, dtype, seed=7)
    for factor in (None, 1.0, 3.7, torch.tensor(2.5)):
        compare(mpl, inp, f"avg_factor {factor}", avg_factor=factor)
    out, _ = compare(mpl, inp, "dir off", dir_loss=False)
    assert bool((out[1] == 0).all())
    compare(mpl, inp, "dir_eps", dir_eps=1e-3)


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("closed_dtype", [torch.bool, torch.uint8, torch.int32, torch.int64], ids=name)
def test_index_and_closed_dtypes(closed_dtype, index_dtype):
    inp = make_case(5, 9, 5, 2, SIZES, PAIRS, torch.float32, seed=5, index_dtype=index_dtype, closed_dtype=closed_dtype)
    compare(mpl, inp, f"{name(index_dtype)}/{name(closed_dtype)}")
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4]), inp, "cost")


def test_either_output_alone_and_pair_rule():
    inp = make_case(5, 7, 5, 3, SIZES, PAIRS, torch.float64, seed=11)
    for row in (0, 1):
        go = torch.zeros(2, 5, dtype=torch.float64)
        go[row] = 1.0
        x = inp[0].detach().requires_grad_(True)
        outs = mpl(x, *inp[1:4], gt_closed=inp[4])
        got, = torch.autograd.grad(outs[row].sum(), x)
        _, want, _, _ = definition(*inp[:4], gt_closed=inp[4], grad_out=go)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # out-of-range indices are skipped, a query named twice takes the lowest slot, slots past n_b are never read
    lines, gt, pind, gind, closed = inp
    pi, gi = pind.tensor.clone(), gind.tensor.clone()
    pi[0, 2], gi[0, 2] = pi[0, 0], (gi[0, 0] + 1) % 3    # the duplicate in a later slot loses
    pi[4, 1] = 7                                          # query out of range
    gi[4, 2] = 5                                          # object out of range (G_max = 5)
    pi[3, 1:], gi[3, 1:] = 99, -4                         # past n_3 = 1
    changed = (lines, gt, ragged(pi, PAIRS), ragged(gi, PAIRS), closed)
    out, _ = compare(mpl, changed, "pair rule")
    assert float(out[0, 4]) > 0


def test_exact_ties_take_the_lowest_order():
    """small-integer coordinates, whose sums are exact in every dtype: a palindromic open line (its reverse is the same
    point sequence, so the gradient is the same either way), a regular polygon against a prediction on its axis (the
    forward order 0 and the reversed order P tie) and an asymmetric open tie — the lowest order decides the gradient"""
    from polyline_match_cases import check_grad, check_losses

    palindrome = torch.tensor([[0., 0.], [2., 1.], [4., 0.], [2., 1.], [0., 0.]])
    x_pal = torch.tensor([[1., 0.], [2., 2.], [3., 1.], [1., 1.], [0., 1.]])
    square = torch.tensor([[2., 0.], [0., 2.], [-2., 0.], [0., -2.]])
    x_axis = torch.tensor([[3., 0.], [1., 0.], [-3., 0.], [-1., 0.]])
    ind = ragged(torch.zeros(1, 1, dtype=torch.int64), [1])
    for dtype in DTYPES:
        for t, x, closed, tied in ((palindrome, x_pal, False, (0, 1)), (square, x_axis, True, (0, 4))):
            sums = (x[None] - t[orders(t.shape[0], closed, True)]).abs().sum((1, 2))
            assert float(sums[tied[0]]) == float(sums[tied[1]]) == float(sums.min())
            lines, gt = x.to(dtype)[None, None], ragged(t.to(dtype)[None, None], [1])
            cl = ragged(torch.tensor([[closed]]), [1])
            want, gwant, _, _ = definition(lines, gt, ind, ind, gt_closed=cl)
            out, grad = run(mpl, lines, gt, ind, ind, gt_closed=cl)
            assert float(out[0, 0]) == float(sums.min())
            check_losses(out, want, dtype, "tie")
            check_grad(grad, gwant, dtype, "tie")
            cost = cost_op(lines, gt, gt_closed=cl).tensor
            assert float(cost[0, 0, 0]) == float(sums.min())
        # forward: |1 - 0| + |1 - 4|, reversed: |1 - 4| + |1 - 0|; the signs differ
        t, x = torch.tensor([[0., 0.], [4., 0.]]), torch.tensor([[1., 0.], [1., 0.]])
        lines, gt = x.to(dtype)[None, None], ragged(t.to(dtype)[None, None], [1])
        _, grad = run(mpl, lines, gt, ind, ind, dir_loss=False, avg_factor=1.0)
        assert grad[0, 0, :, 0].tolist() == [1.0, -1.0]    # the forward order: sgn(1 - 0), sgn(1 - 4)
        _, gwant, _, _ = definition(lines, gt, ind, ind, dir_loss=False, avg_factor=1.0)
        assert torch.equal(grad.double(), gwant)


def test_empty_extents():
    for B, Q, n in ((0, 6, 0), (3, 0, 0), (3, 6, 0)):
        inp = make_case(B, Q, 5, 2, [2] * B, [n] * B, torch.float32, seed=1)
        out, grad = run(mpl, *inp[:4])
        assert out.shape == (2, B) and bool((out == 0).all()) and grad.shape == (B, Q, 5, 2) and bool((bits(grad) == 0).all())
        cost = cost_op(inp[0], inp[1])
        assert tuple(cost.tensor.shape) == (B, Q, 2 if B else 0)


# ----------------------------------------------------------------------------------------------------------------- cost
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("P", [2, 5, 20])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("closed", ["open", "closed", "mixed"])
@pytest.mark.parametrize("reversible", [True, False])
def test_cost_matches_definition(reversible, closed, D, P, dtype):
    inp = make_case(5, 7, P, D, SIZES, PAIRS, dtype, seed=P * D, closed=closed, reversible=reversible)
    cost = cost_op(inp[0], inp[1], gt_closed=inp[4], reversible=reversible, pts_weight=1.5, filler=-7.25)
    check_cost(cost, inp, f"{name(dtype)}/P{P}/D{D}/{closed}", reversible=reversible, pts_weight=1.5, filler=-7.25)
    assert torch.equal(cost.sample_sizes, inp[1].sample_sizes)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("kind", ["one_minus_prob", "neg_prob", "focal"])
def test_cost_with_class_term(kind, dtype):
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, dtype, seed=3)
    g = torch.Generator().manual_seed(2)
    raw = torch.randn(5, 7, 4, generator=g, dtype=torch.float64) * 3
    scores = (raw if kind == "focal" else raw.softmax(-1)).to(dtype)
    labels = ragged(torch.randint(0, 4, (5, 5), generator=g), SIZES)
    labels.tensor[2, 1] = 9    # outside [0, C): a NaN class term
    kw = dict(class_cost=kind, class_weight=2.0, pts_weight=5.0)
    check_cost(cost_op(inp[0], inp[1], scores, labels, gt_closed=inp[4], **kw), inp, kind, scores=scores, labels=labels, **kw)
    # a term of weight 0 is not evaluated: its inputs may be None
    only_cls = cost_op(None, None, scores, labels, pts_weight=0.0, class_cost=kind, class_weight=2.0)
    want, _, mag = cost_definition(None, None, scores, labels, pts_weight=0.0, class_cost=kind, class_weight=2.0)
    from polyline_match_cases import assert_close_nan_aware, tolerance
    assert_close_nan_aware(only_cls.tensor, want, tolerance(dtype), "class only", scale=mag)
    only_pts = cost_op(inp[0], inp[1], None, None, gt_closed=inp[4])
    check_cost(only_pts, inp, "points only")


def test_cost_nan_reaches_its_pairs_only():
    inp = make_case(3, 6, 5, 2, [4, 2, 3], [0, 0, 0], torch.float32, seed=4, closed="mixed")
    inp[0][1, 2, 3, 1] = float("nan")
    inp[1].tensor[2, 1, 0, 0] = float("nan")
    cost = cost_op(inp[0], inp[1], gt_closed=inp[4]).tensor
    want = torch.zeros(3, 6, 4, dtype=torch.bool)
    want[1, 2, :2] = True
    want[2, :, 1] = True
    assert torch.equal(torch.isnan(cost), want)


def test_hungarian_match_total_cost():
    inp = make_case(4, 9, 5, 2, [4, 0, 6, 9], [0, 0, 0, 0], torch.float32, seed=6)
    pind, gind = batched_polyline_hungarian_match(inp[0], inp[1], gt_closed=inp[4])
    want, _, _ = cost_definition(inp[0], inp[1], gt_closed=inp[4])
    rp, rg = batched_linear_sum_assignment(RaggedBatch(want, sample_sizes=inp[1].sample_sizes, non_uniform_dim=2))
    assert torch.equal(pind.sample_sizes, rp.sample_sizes)
    for b in range(4):
        n = int(pind.sample_sizes[b])
        got = want[b, pind.tensor[b, :n], gind.tensor[b, :n]].sum()
        ref = want[b, rp.tensor[b, :n], rg.tensor[b, :n]].sum()
        assert abs(float(got - ref)) <= 1e-5 * (1 + abs(float(ref)))


# ----------------------------------------------------------------------------------------------------------- validation
def test_validation_errors():
    lines, gt, pind, gind, closed = make_case(2, 4, 5, 2, [2, 3], [2, 2], torch.float32, seed=1)
    with pytest.raises(TypeError):
        mpl(lines.tolist(), gt, pind, gind)
    with pytest.raises(ValueError):
        mpl(lines[..., 0], gt, pind, gind)
    with pytest.raises(TypeError):
        mpl(lines.to(torch.int32), gt, pind, gind)
    with pytest.raises(ValueError, match="P"):
        mpl(lines[:, :, :1], gt, pind, gind)
    with pytest.raises(ValueError, match="P"):
        cost_op(torch.zeros(2, 4, 129, 2), ragged(torch.zeros(2, 3, 129, 2), [2, 3]))
    with pytest.raises(ValueError, match="D"):
        mpl(torch.zeros(2, 4, 5, 4), ragged(torch.zeros(2, 3, 5, 4), [2, 3]), pind, gind)
    with pytest.raises(ValueError, match="contiguous"):
        mpl(lines.transpose(2, 3).contiguous().transpose(2, 3), gt, pind, gind)
    with pytest.raises(TypeError):
        mpl(lines, gt.tensor, pind, gind)
    with pytest.raises(TypeError):
        mpl(lines, ragged(gt.tensor.double(), [2, 3]), pind, gind)
    with pytest.raises(ValueError):
        mpl(lines, ragged(gt.tensor[:, :, :4], [2, 3]), pind, gind)
    with pytest.raises(TypeError):
        mpl(lines, gt, ragged(pind.tensor.float(), [2, 2]), gind)
    with pytest.raises(TypeError):
        mpl(lines, gt, ragged(pind.tensor.int(), [2, 2]), gind)
    with pytest.raises(ValueError):
        mpl(lines, gt, ragged(pind.tensor[:, :1], [1, 1]), gind)
    with pytest.raises(TypeError):
        mpl(lines, gt, pind, gind, gt_closed=ragged(closed.tensor.float(), [2, 3]))
    with pytest.raises(ValueError):
        mpl(lines, gt, pind, gind, gt_closed=ragged(closed.tensor[:, :2], [2, 2]))
    with pytest.raises(ValueError):
        mpl(lines, gt, pind, gind, dir_eps=-1.0)
    with pytest.raises(ValueError):
        mpl(lines, gt, pind, gind, avg_factor=torch.tensor([1.0]))
    with pytest.raises(ValueError):
        cost_op(lines, gt, class_cost="softmax")
    with pytest.raises(TypeError):
        cost_op(lines, gt, None, None, class_weight=1.0)
    with pytest.raises(ValueError):
        cost_op(lines, gt, torch.zeros(2, 5, 3), ragged(torch.zeros(2, 3, dtype=torch.int64), [2, 3]), class_weight=1.0)
    assert MARGIN == 1e-3
