"""The seeded sweeps of tests/operator_sweep_cases.py on the GPU: the HIP kernels of the matching, loss and detection
operators against their float64 definitions and against their host paths, through the comparison functions of the
operators' own test modules, over random combinations of shape, dtype, stride, index type, ragged sizes and flags that the
hand-picked cases cross one at a time.  The same draws run through the host paths alone in
test_operator_sweeps_cpu.py.  ACCV_FUZZ_SCALE=k runs k times as many seeds.  After a complete run the worst error seen per
operator and dtype goes to profiles/operator_sweeps_accuracy.log."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import operator_sweep_cases as sw  # noqa: E402
from test_operator_sweeps_cpu import iou_matrix_error, polyline_case, report_redraws, seeds  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = "exact"      # the dtype column of an operator whose outputs are compared bit for bit


@pytest.fixture(scope="module")
def worst():
    """every sweep records its largest errors here; written out once every seed of every sweep of the module is through"""
    seen = sw.Worst()
    seen.done = set()
    yield seen
    if seen.done != {(op, s) for op in sw.SWEEPS for s in seeds(op)}:      # a partial run (-k, -x) leaves no log
        return
    lines = [f"operator sweeps on {torch.cuda.get_device_name(0)} (tests/test_operator_sweeps_gpu.py, ACCV_FUZZ_SCALE "
             f"{os.environ.get('ACCV_FUZZ_SCALE', '1')}): the largest error seen per operator and input dtype.",
             "loss: |out - ref| / |ref| against the float64 definition (bound 1e-5; float64 1e-12).  gradient: float32 / float64 as a",
             "share of the bound 1e-4 |g| + 1e-6 max|g| (float64 1e-12 / 1e-14), float16 / bfloat16 in representable steps from the",
             "rounded float64 gradient (bound 1; matched_box_loss and the polyline loss also accept the float32 bound there).",
             "cost: |out - ref| / (1 + |ref| + sum |terms|) (bound 1e-5; float64 1e-12).  abs: absolute error of the inexact channels",
             "(bar 1e-5).  'vs host' figures compare the device with the host path where that comparison is a tolerance;",
             "cost_vs_host is |device - host| / (1 + |host|) of the focal class cost (asserted at 2e-6 (1 + |host| + |focal term|))."]
    lines += seen.lines()
    try:
        with open(os.path.join(ROOT, "profiles", "operator_sweeps_accuracy.log"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:      # a read-only checkout: the figures were asserted all the same
        pass


def float_of(kw):
    return {k: (float(v) if isinstance(v, torch.Tensor) and k == "avg_factor" else v) for k, v in kw.items()}


# ------------------------------------------------------------------------------------------------------ the loss side
@pytest.mark.parametrize("seed", seeds("matched_focal_loss"))
def test_matched_focal_loss_sweep(seed, worst):
    from matched_focal_loss_cases import definition
    from test_matched_focal_loss_gpu import compare

    for tag, inp, kw in sw.sweep("matched_focal_loss", seed, DEV):
        out, grad = compare(inp, tag, **kw)
        want, gwant, _ = definition(*inp[:4], query_weights=inp[4], **kw)
        worst.add("matched_focal_loss", inp[0].dtype, loss=sw.loss_error(out, want), gradient=sw.grad_error(grad, gwant, inp[0].dtype))
    worst.done.add(("matched_focal_loss", seed))


@pytest.mark.parametrize("seed", seeds("matched_box_loss"))
def test_matched_box_loss_sweep(seed, worst):
    from matched_box_loss_cases import definition
    from test_matched_box_loss_gpu import compare

    for tag, inp, kw in sw.sweep("matched_box_loss", seed, DEV):
        out, grad = compare(inp, tag, **kw)
        want, gwant, _ = definition(*inp[:4], query_weights=inp[4], **kw)
        worst.add("matched_box_loss", inp[0].dtype, loss=sw.loss_error(out, want), gradient=sw.grad_error(grad, gwant, inp[0].dtype))
    worst.done.add(("matched_box_loss", seed))


@pytest.mark.parametrize("seed", seeds("batched_matching_cost"))
def test_batched_matching_cost_sweep(seed, worst):
    from matching_cost_cases import oracle
    from test_matching_cost_gpu import check_against_host, mc, to_cpu

    for tag, inp, kw in sw.sweep("batched_matching_cost", seed, DEV):
        dtype = inp[0].dtype
        out = check_against_host(inp, kw, dtype, tag).tensor.cpu().double()
        want, pad, mag = oracle(*inp, **kw)
        fin = torch.isfinite(want) & ~pad
        figs = dict(cost=float(((out - want).abs() / (1 + want.abs() + mag))[fin].max()) if bool(fin.any()) else 0.0)
        if kw["class_cost"] == "focal":
            host = mc(*to_cpu(inp), **kw).tensor.double()
            figs["cost_vs_host"] = float(((out - host).abs() / (1 + host.abs()))[fin].max()) if bool(fin.any()) else 0.0
        worst.add("batched_matching_cost", dtype, **figs)
    worst.done.add(("batched_matching_cost", seed))


@pytest.mark.parametrize("seed", seeds("polyline"))
def test_polyline_cost_and_loss_sweep(seed, worst):
    from polyline_match_cases import cost_definition, definition, run, to_host

    from accvlab.lane_helpers.polyline import batched_polyline_matching_cost as cost_op, matched_polyline_loss as mpl

    cases = skipped = 0
    for tag, inp, kw in sw.sweep("polyline", seed, DEV):
        cases += 1
        dtype = inp[0].dtype
        compared = polyline_case(mpl, cost_op, tag + " device", inp, kw)
        polyline_case(mpl, cost_op, tag + " host", to_host(inp), kw)
        skipped += not compared
        want, pad, mag = cost_definition(inp[0], inp[1], gt_closed=inp[4], **kw["cost"])
        out = cost_op(inp[0], inp[1], gt_closed=inp[4], **kw["cost"]).tensor.cpu().double()
        fin = torch.isfinite(want) & ~pad
        figs = dict(cost=float(((out - want).abs() / (1 + want.abs() + mag))[fin].max()) if bool(fin.any()) else 0.0)
        if compared:
            lout, grad = run(mpl, *inp[:4], gt_closed=inp[4], **kw["loss"])
            lwant, gwant, _, _ = definition(*inp[:4], gt_closed=inp[4], **float_of(kw["loss"]))
            figs.update(loss=sw.loss_error(lout, lwant), gradient=sw.grad_error(grad, gwant, dtype))
        worst.add("polyline cost + loss", dtype, **figs)
    report_redraws("polyline", cases, skipped)
    worst.done.add(("polyline", seed))


# ------------------------------------------------------------------------------------------------- the detection side
def approx_error(got, want, channels):
    g, a = np.asarray(got, np.float64)[..., channels], np.asarray(want, np.float64)[..., channels]
    with np.errstate(invalid="ignore"):
        err = np.where((np.isnan(g) & np.isnan(a)) | (g == a), 0.0, np.abs(g - a))
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("seed", seeds("center_point_decode"))
def test_center_point_decode_sweep(seed, worst):
    from test_center_decode_gpu import both, op

    before, cases = sw.REDRAWS["center_point_decode"], 0
    for tag, case, kw in sw.sweep("center_point_decode", seed):
        cases += 1
        got, want = both(case, kw["cfg"], tag, **kw["options"])
        host = op(*case.op_args(), **kw["cfg"], **kw["options"])
        ch = want[0]["approx_channels"]
        figs = dict(abs=max(approx_error(r.boxes.tensor.cpu(), w["approx"], ch) for r, w in zip(got, want)),
                    abs_vs_host=max(approx_error(r.boxes.tensor.cpu(), h.boxes.tensor, ch) for r, h in zip(got, host)))
        if want[0]["logits"]:
            figs["score"] = max(approx_error(r.scores.tensor.cpu(), w["score_approx"], slice(None)) for r, w in zip(got, want))
            figs["score_vs_host"] = max(approx_error(r.scores.tensor.cpu(), h.scores.tensor, slice(None)) for r, h in zip(got, host))
        worst.add("center_point_decode", case.feats[0][0].dtype, **figs)
    report_redraws("center_point_decode", cases, sw.REDRAWS["center_point_decode"] - before)
    worst.done.add(("center_point_decode", seed))


@pytest.mark.parametrize("seed", seeds("rotated_nms_bev"))
def test_rotated_nms_and_iou_sweep(seed, worst):
    from rotated_nms_cases import BAR, BEV, ragged5
    from test_rotated_nms_gpu import both

    from accvlab.draw_heatmap import rotated_iou_bev

    for tag, case, kw in sw.sweep("rotated_nms_bev", seed):
        both(case, kw["thresholds"], tag, **kw["options"])       # kept rows bit-equal to the definition's and to the host's
        err = iou_matrix_error(case, DEV)
        assert err <= BAR, f"{tag}: IoU matrix off by {err:.3e} (bar {BAR})"
        boxes, sizes = case.tasks[0][0][..., BEV].numpy(), case.tasks[0][4].tolist()
        dev, host = (rotated_iou_bev(r, r).tensor.cpu().numpy() for r in (ragged5(boxes, sizes, DEV), ragged5(boxes, sizes)))
        vs_host = max([float(np.abs(dev[b, :n, :n] - host[b, :n, :n]).max()) for b, n in enumerate(sizes) if n] + [0.0])
        assert vs_host <= BAR, f"{tag}: IoU matrix, device against host {vs_host:.3e} (bar {BAR})"
        worst.add("rotated_nms_bev / rotated_iou_bev", torch.float32, iou_abs=err, iou_abs_vs_host=vs_host)
    worst.done.add(("rotated_nms_bev", seed))


@pytest.mark.parametrize("seed", seeds("center_point_targets"))
def test_center_point_targets_sweep(seed, worst):
    from test_center_targets_gpu import both, op, to_host

    for tag, (boxes, labels), kw in sw.sweep("center_point_targets", seed, DEV):
        got, want = both(boxes, labels, kw["tasks"], kw["cfg"], tag, **kw["options"])
        host = op(to_host(boxes), to_host(labels), kw["tasks"], **kw["cfg"], **kw["options"])
        ch = want[0]["approx_channels"]
        worst.add("center_point_targets", torch.float32,
                  abs=max(approx_error(r.targets.tensor.cpu(), w["approx"], ch) for r, w in zip(got, want)),
                  abs_vs_host=max(approx_error(r.targets.tensor.cpu(), h.targets.tensor, ch) for r, h in zip(got, host)))
    worst.done.add(("center_point_targets", seed))


@pytest.mark.parametrize("seed", seeds("batched_linear_sum_assignment"))
def test_batched_linear_sum_assignment_sweep(seed, worst):
    from test_linear_assignment_gpu import assert_same_as_host

    for tag, cost, kw in sw.sweep("batched_linear_sum_assignment", seed, DEV):
        try:
            got = assert_same_as_host(cost, **kw)
        except AssertionError as e:
            raise AssertionError(f"{tag}: device and host differ: {e}") from None
        sw.check_assignment_against_scipy(got, cost, kw["maximize"], tag)
        worst.add("batched_linear_sum_assignment", EXACT)
    worst.done.add(("batched_linear_sum_assignment", seed))


# ------------------------------------------------------------------------------------- the operators without a host path
@pytest.mark.parametrize("seed", seeds("heatmap_peaks"))
def test_heatmap_peaks_sweep(seed, worst):
    from test_heatmap_peaks_gpu import assert_matches

    for tag, heat, kw in sw.sweep("heatmap_peaks", seed, DEV):
        print(tag)
        assert_matches(heat, kw["k"], kernel=kw["kernel"], per_class=kw["per_class"])
        worst.add("heatmap_peaks", EXACT)
    worst.done.add(("heatmap_peaks", seed))


@pytest.mark.parametrize("seed", seeds("gaussian_focal_loss"))
def test_gaussian_focal_loss_sweep(seed, worst):
    from test_heatmap_loss_gpu import assert_grad_close, composition

    from accvlab.draw_heatmap import gaussian_focal_loss

    for tag, (logits, target), kw in sw.sweep("gaussian_focal_loss", seed, DEV):
        x = logits.detach().requires_grad_(True)        # no copy: the drawn offset from the alignment stays
        loss = gaussian_focal_loss(x, target, **kw)
        loss.backward()
        ref, g64 = composition(logits, target, **kw)
        assert loss.dtype == torch.float32 and loss.dim() == 0, tag
        loss = loss.detach()
        rel = abs(float(loss) - float(ref)) / abs(float(ref))
        assert rel <= 1e-5, f"{tag}: loss {float(loss)!r} against {float(ref)!r}: {rel:.3e}"
        try:
            assert_grad_close(x.grad, g64, logits.dtype)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
        worst.add("gaussian_focal_loss", logits.dtype, loss=rel, gradient=sw.grad_error(x.grad, g64, logits.dtype))
    worst.done.add(("gaussian_focal_loss", seed))


@pytest.mark.parametrize("seed", seeds("center_regression"))
def test_center_regression_sweep(seed, worst):
    import center_regression_cases as cr

    from accvlab.draw_heatmap import center_regression_loss, gather_at_centers

    for tag, (maps, xy, sizes, targets, weights), kw in sw.sweep("center_regression", seed, DEV):
        dtype = maps[0].dtype
        centers = cr.ragged(xy, sizes.cpu(), sizes.dtype)
        feats = maps if len(maps) > 1 else maps[0]
        got = gather_at_centers(feats, centers)
        assert got.tensor.dtype == dtype and got.sample_sizes is centers.sample_sizes, tag
        assert torch.equal(got.tensor, cr.oracle_gather(maps, xy, sizes).to(dtype)), f"{tag}: gather_at_centers"
        leaves = [m.detach().clone().requires_grad_(True) for m in maps]
        loss = center_regression_loss(leaves if len(leaves) > 1 else leaves[0], centers, targets, weights, **kw)
        loss.backward()
        ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights, kw["kind"], kw["beta"], kw.get("avg_factor"))
        cr.assert_loss_close(loss.detach(), ref, tag)
        for i, (m, want) in enumerate(zip(leaves, ref_grads)):
            cr.assert_grad_close(m.grad, want, dtype, f"{tag} map {i}")
        worst.add("gather_at_centers / center_regression_loss", dtype, loss=sw.loss_error(loss, ref),
                  gradient=max(sw.grad_error(m.grad, w, dtype) for m, w in zip(leaves, ref_grads)))
    worst.done.add(("center_regression", seed))
