"""The seeded sweeps of tests/operator_sweep_cases.py through the host paths of the matching, loss and detection operators,
against their float64 definitions — the same draws as test_operator_sweeps_gpu.py, without a GPU: this is what shows that
the references hold over the swept ranges.  The three operators without a host path (heatmap_peaks, gaussian_focal_loss,
centre regression) get a plain float32 torch evaluation of their definition instead, which must stay inside the
operator's bounds over the same draws.  ACCV_FUZZ_SCALE=k runs k times as many seeds."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import operator_sweep_cases as sw  # noqa: E402
from test_fuzz_gpu import _seeds  # noqa: E402


def seeds(op):
    return _seeds(sw.SWEEPS[op][1])


def report_redraws(op, cases, redrawn):
    """at most a tenth of a test's cases may have been drawn again or skipped: a sweep never passes by looking away"""
    print(f"{op}: {redrawn} of {cases} cases redrawn or skipped")
    assert redrawn <= 0.1 * cases, f"{op}: {redrawn} of {cases} cases redrawn or skipped"


# ------------------------------------------------------------------------------------------------------ the loss side
@pytest.mark.parametrize("seed", seeds("matched_focal_loss"))
def test_matched_focal_loss_host_sweep(seed):
    from test_matched_focal_loss_cpu import compare

    for tag, inp, kw in sw.sweep("matched_focal_loss", seed):
        compare(inp, tag, **kw)


@pytest.mark.parametrize("seed", seeds("matched_box_loss"))
def test_matched_box_loss_host_sweep(seed):
    from matched_box_loss_cases import compare

    from accvlab.batching_helpers import matched_box_loss

    for tag, inp, kw in sw.sweep("matched_box_loss", seed):
        compare(matched_box_loss, inp, tag, **kw)


@pytest.mark.parametrize("seed", seeds("batched_matching_cost"))
def test_batched_matching_cost_host_sweep(seed):
    from matching_cost_cases import assert_close_nan_aware, oracle, tolerance

    from accvlab.batching_helpers import batched_matching_cost

    for tag, inp, kw in sw.sweep("batched_matching_cost", seed):
        out = batched_matching_cost(*inp, **kw)
        want, pad, mag = oracle(*inp, **kw)
        dtype = inp[0].dtype
        assert out.tensor.dtype == (torch.float64 if dtype == torch.float64 else torch.float32) and out.tensor.is_contiguous(), tag
        assert out.non_uniform_dim == 2 and torch.equal(out.sample_sizes, inp[1].sample_sizes), tag
        assert_close_nan_aware(out.tensor, want, tolerance(dtype), tag, scale=mag)
        assert bool((out.tensor[pad] == kw.get("filler", 0.0)).all()), f"{tag}: padded columns are not the filler"


def polyline_case(mpl, cost_op, tag, inp, kw):
    """loss and cost of one drawn case against polyline_match_cases; -> False when the order margin refuses the case"""
    from polyline_match_cases import MARGIN, check_cost, compare, definition

    lines, gt, pind, gind, closed = inp
    margin = definition(lines, gt, pind, gind, gt_closed=closed, **kw["loss"])[3]
    check_cost(cost_op(lines, gt, gt_closed=closed, **kw["cost"]), inp, tag + " cost", **kw["cost"])
    if not margin > MARGIN:
        return False
    compare(mpl, inp, tag, **kw["loss"])
    return True


@pytest.mark.parametrize("seed", seeds("polyline"))
def test_polyline_cost_and_loss_host_sweep(seed):
    from accvlab.lane_helpers.polyline import batched_polyline_matching_cost, matched_polyline_loss

    cases = skipped = 0
    for tag, inp, kw in sw.sweep("polyline", seed):
        cases += 1
        skipped += not polyline_case(matched_polyline_loss, batched_polyline_matching_cost, tag, inp, kw)
    report_redraws("polyline", cases, skipped)


# ------------------------------------------------------------------------------------------------- the detection side
@pytest.mark.parametrize("seed", seeds("center_point_decode"))
def test_center_point_decode_host_sweep(seed):
    from center_decode_cases import check, run

    from accvlab.draw_heatmap import center_point_decode

    before, cases = sw.REDRAWS["center_point_decode"], 0
    for tag, case, kw in sw.sweep("center_point_decode", seed):
        cases += 1
        got, want = run(center_point_decode, case, kw["cfg"], **kw["options"])
        check(got, want, tag)
    report_redraws("center_point_decode", cases, sw.REDRAWS["center_point_decode"] - before)


def iou_matrix_error(case, device="cpu"):
    """largest |rotated_iou_bev - float64 IoU| over the existing slots of task 0 of a drawn NMS case"""
    from rotated_nms_cases import BEV, ragged5

    from accvlab.draw_heatmap import rotated_iou_bev

    boxes, sizes = case.tasks[0][0], case.tasks[0][4].tolist()
    r = ragged5(boxes[..., BEV].numpy(), sizes, device)
    got = rotated_iou_bev(r, r).tensor.cpu().numpy()
    return max([float(np.abs(got[b, :n, :n] - case.ious[0][b][:n, :n]).max()) for b, n in enumerate(sizes) if n] + [0.0])


@pytest.mark.parametrize("seed", seeds("rotated_nms_bev"))
def test_rotated_nms_and_iou_host_sweep(seed):
    from rotated_nms_cases import BAR, assert_margin, check, definition

    from accvlab.draw_heatmap import rotated_nms_bev

    for tag, case, kw in sw.sweep("rotated_nms_bev", seed):
        thr, opt = kw["thresholds"], kw["options"]
        assert_margin(case, thr)
        got = rotated_nms_bev(case.detections(), thr, **opt)
        check(got, definition(case, thr, opt.get("pre_max_size"), opt.get("post_max_size")), case, tag)
        err = iou_matrix_error(case)
        assert err <= BAR, f"{tag}: IoU matrix off by {err:.3e} (bar {BAR})"


@pytest.mark.parametrize("seed", seeds("center_point_targets"))
def test_center_point_targets_host_sweep(seed):
    from center_targets_cases import check, run

    from accvlab.draw_heatmap import center_point_targets

    for tag, (boxes, labels), kw in sw.sweep("center_point_targets", seed):
        got, want = run(center_point_targets, boxes, labels, kw["tasks"], kw["cfg"], **kw["options"])
        check(got, want, tag)


@pytest.mark.parametrize("seed", seeds("batched_linear_sum_assignment"))
def test_batched_linear_sum_assignment_host_sweep(seed):
    from accvlab.batching_helpers import batched_linear_sum_assignment

    for tag, cost, kw in sw.sweep("batched_linear_sum_assignment", seed):
        sw.check_assignment_against_scipy(batched_linear_sum_assignment(cost, check=False, **kw), cost, kw["maximize"], tag)


# ------------------------------------------------- the operators without a host path: float32 evaluations of the definition
@pytest.mark.parametrize("seed", seeds("heatmap_peaks"))
def test_heatmap_peaks_float32_evaluation_of_the_definition_is_exact_over_the_sweep(seed):
    """the operator copies values and indices: its definition must give the same five tensors in float32 as in float64,
    and sweep_cases.peaks_definition in float64 must be test_heatmap_peaks_gpu.reference"""
    from test_heatmap_peaks_gpu import reference

    for tag, heat, kw in sw.sweep("heatmap_peaks", seed):
        want = reference(heat, **kw)
        for dtype in (torch.float64, torch.float32):
            for g, w in zip(sw.peaks_definition(heat, dtype=dtype, **kw), want):
                assert g.dtype == w.dtype and torch.equal(g, w), f"{tag}: evaluation in {dtype}"


@pytest.mark.parametrize("seed", seeds("gaussian_focal_loss"))
def test_gaussian_focal_loss_float32_evaluation_of_the_definition_meets_the_bounds(seed):
    """a float32 torch evaluation of the composition stays within the operator's bounds over the swept ranges (loss 1e-5
    relative; gradients test_heatmap_loss_gpu.assert_grad_close, a 16-bit gradient being the float32 one rounded).  The
    float32 evaluation takes 1 - sigmoid(x) as sigmoid(-x), like the kernel: with the literal subtraction 1 - p holds
    6e-8 / 1.2e-4 = 5e-4 of relative error at x = 9, and on a map of a few elements, where nothing averages out, the loss
    misses its bound (1.075e-5 on a (1, 1, 7) map, alpha 1, in a six-fold soak of this sweep; the figure is printed).
    In float64 both spellings are one function to 1e-10."""
    from test_heatmap_loss_gpu import assert_grad_close, composition

    for tag, (logits, target), kw in sw.sweep("gaussian_focal_loss", seed):
        ref, g64 = composition(logits, target, **kw)
        same, gsame = sw.gaussian_focal_definition(logits, target, **kw)
        assert torch.equal(ref, same) and torch.equal(g64, gsame), f"{tag}: the two spellings of the definition differ"
        alt, galt = sw.gaussian_focal_definition(logits, target, literal=False, **kw)
        assert abs(float(alt) - float(ref)) <= 1e-10 * abs(float(ref)), f"{tag}: sigmoid(-x) for 1 - sigmoid(x) changes the loss"
        assert bool(((galt - g64).abs() <= 1e-10 * g64.abs() + 1e-12 * g64.abs().max()).all()), f"{tag}: ... changes the gradient"
        literal, _ = sw.gaussian_focal_definition(logits, target, dtype=torch.float32, **kw)
        loss, g = sw.gaussian_focal_definition(logits, target, dtype=torch.float32, literal=False, **kw)
        rel = abs(float(loss) - float(ref)) / abs(float(ref))
        print(f"{tag}: float32 evaluation, loss relative error {rel:.3e} (with the literal 1 - p: "
              f"{abs(float(literal) - float(ref)) / abs(float(ref)):.3e})")
        assert rel <= 1e-5, f"{tag}: float32 evaluation of the loss off by {rel:.3e}"
        try:
            assert_grad_close(g.to(logits.dtype), g64, logits.dtype)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None


@pytest.mark.parametrize("seed", seeds("center_regression"))
def test_center_regression_float32_evaluation_of_the_definition_meets_the_bounds(seed):
    """center_regression_cases.composition_loss on float32 copies of the maps (the float32 form of the oracle) stays within
    the operator's bounds over the swept ranges; the gather is a copy and must be exact"""
    import center_regression_cases as cr

    for tag, (maps, xy, sizes, targets, weights), kw in sw.sweep("center_regression", seed):
        dtype = maps[0].dtype
        assert torch.equal(cr.oracle_gather(maps, xy, sizes).to(dtype), cr.oracle_gather([m.float() for m in maps], xy, sizes).to(dtype)), tag
        ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights, kw["kind"], kw["beta"], kw.get("avg_factor"))
        leaves = [m.float().requires_grad_(True) for m in maps]
        loss = cr.composition_loss(leaves, xy, sizes, targets, weights, kw["kind"], kw["beta"])
        if "avg_factor" in kw:      # composition_loss divides by the number of valid centres
            valid, _ = cr.valid_and_index(xy, sizes, maps[0].shape[2], maps[0].shape[3])
            loss = loss * (valid.sum().clamp(min=1) / float(kw["avg_factor"]))
        cr.assert_loss_close(loss.detach(), ref, tag)
        if loss.requires_grad:
            loss.backward()
        for i, (m, want) in enumerate(zip(leaves, ref_grads)):
            g = m.grad if m.grad is not None else torch.zeros_like(m)
            cr.assert_grad_close(g.to(dtype), want, dtype, f"{tag} map {i}")
