"""matched_box_loss on the device (accv_matched_box_loss / _bwd) against the float64 definition of
tests/matched_box_loss_cases.py and against the host path: values, gradients, kernel edges, reproducibility, complete
writes, guard bands, no synchronisation, graph capture, the end-to-end criterion, special values."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matched_box_loss_cases import (DTYPES, PAIRS, SIZES, bits, check_grad, check_loss, check_losses, definition,  # noqa: E402
                                    make_case, name, ragged, run, shape_case)

from accvlab.batching_helpers import matched_box_loss as mbl  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 256   # queries per workgroup (kThreads of csrc/matched_box.hip)
SHAPES = {"a": (8, 900, 4, 100), "b": (16, 300, 4, 40), "c": (48, 900, 10, 60)}
CODE_WEIGHTS_10 = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.2, 0.2, 2.0, 0.0]


def to_host(inp):
    boxes, gt, pind, gind, w = inp
    cpu = lambda rb: ragged(rb.tensor.cpu(), rb.sample_sizes.cpu().tolist())
    return boxes.cpu(), cpu(gt), cpu(pind), cpu(gind), None if w is None else w.cpu()


def compare(inp, what="", grad_out=None, host=True, **kw):
    """device against the float64 definition and (host=True) the host path against it on the same inputs"""
    boxes, gt, pind, gind, w = inp
    ref = dict(kw)
    if isinstance(ref.get("avg_factor"), torch.Tensor):
        ref["avg_factor"] = float(ref["avg_factor"])
    if isinstance(ref.get("code_weights"), torch.Tensor):
        ref["code_weights"] = ref["code_weights"].cpu()
    want, gwant, _ = definition(boxes, gt, pind, gind, grad_out=grad_out, query_weights=w, **ref)
    out, grad = run(mbl, boxes, gt, pind, gind, grad_out=grad_out, query_weights=w, **kw)
    assert out.is_cuda and grad.is_cuda and grad.is_contiguous()
    assert out.dtype == (torch.float64 if boxes.dtype == torch.float64 else torch.float32)
    check_losses(out, want, boxes.dtype, what + " device")
    check_grad(grad, gwant, boxes.dtype, what + " device")
    if host:
        h = to_host(inp)
        hkw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        hout, hgrad = run(mbl, *h[:4], grad_out=grad_out, query_weights=h[4], **hkw)
        check_losses(hout, want, boxes.dtype, what + " host")
        check_grad(hgrad, gwant, boxes.dtype, what + " host")
    return out, grad


# ---------------------------------------------------------------------------------------------------- definition match
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("box_format", ["xyxy", "cxcywh"])
@pytest.mark.parametrize("iou_kind", ["giou", "iou", None])
@pytest.mark.parametrize("weights", [False, True])
def test_device_and_host_match_definition(weights, iou_kind, box_format, dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=3, box_format=box_format, weights=weights, device=DEV)
    g = torch.Generator().manual_seed(1)
    cw = [1.0, 0.5, 2.0, 0.25] if weights else None
    compare(inp, f"{name(dtype)}/{box_format}/{iou_kind}/w{weights}", grad_out=torch.rand(2, 5, generator=g) + 0.5,
            box_format=box_format, iou_kind=iou_kind, code_weights=cw)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("form", ["none", "sequence", "tensor"])
def test_ten_value_codes_l1_only(form, dtype):
    inp = make_case(5, 7, 10, SIZES, PAIRS, dtype, seed=4, weights=True, device=DEV)
    cw = {"none": None, "sequence": CODE_WEIGHTS_10,
          "tensor": torch.tensor(CODE_WEIGHTS_10, dtype=torch.float64).to(dtype).to(DEV)}[form]
    out, _ = compare(inp, f"D10/{form}/{name(dtype)}", iou_kind=None, code_weights=cw)
    assert bool((out[1] == 0).all())


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
def test_index_dtypes(dtype, index_dtype):
    compare(make_case(5, 9, 4, SIZES, PAIRS, dtype, seed=5, index_dtype=index_dtype, box_format="cxcywh", device=DEV),
            box_format="cxcywh")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms(dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=7, device=DEV)
    for factor in (None, 1.0, 3.7, torch.tensor(2.5, device=DEV)):
        compare(inp, f"avg_factor {factor}", avg_factor=factor)


# --------------------------------------------------------------------------------------------------------- kernel edges
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=name)
@pytest.mark.parametrize("Q", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_queries_across_workgroup_chunks(Q, dtype):
    """pairs on both sides of every chunk boundary: the first and the last query of the frame are matched"""
    n = [40, 0, 17]
    inp = make_case(3, Q, 4, [40, 5, 20], n, dtype, seed=Q, box_format="cxcywh", weights=True, device=DEV)
    for b, k in enumerate(n):
        if k:
            edge = torch.tensor([0, Q - 1, min(CHUNK - 1, Q - 2), min(CHUNK, Q - 3)], device=DEV)
            rest = torch.tensor([q for q in range(1, Q - 4) if q not in (CHUNK - 1, CHUNK)][: k - 4], device=DEV)
            inp[2].tensor[b, :k] = torch.cat([edge, rest])
    compare(inp, f"Q {Q}", box_format="cxcywh")


@pytest.mark.parametrize("K", [63, 64, 65, 130])
def test_slot_counts_across_waves(K):
    inp = make_case(2, 300, 4, [K, K], [K, K - 1], torch.float32, seed=K, device=DEV)
    compare(inp, f"K {K}")
    # a query named in the first and in the last slot: the first one is its pair, whichever wave reads it
    inp[2].tensor[0, K - 1] = inp[2].tensor[0, 0]
    compare(inp, f"K {K} duplicate")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("D", [1, 3, 4, 10, 16])
def test_coordinate_counts_and_one_frame(D, dtype):
    inp = make_case(1, CHUNK + 5, D, [9], [9], dtype, seed=D, weights=True, device=DEV)
    cw = [0.5 + 0.25 * d for d in range(D)]
    compare(inp, f"B 1 D {D}", iou_kind=None, code_weights=cw)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("width", [5, 7, 12])
def test_strided_and_misaligned_boxes(width, dtype):
    """code[..., :4] of a wider tensor, and contiguous boxes whose base is not 16-byte aligned, against the contiguous copy
    bit for bit"""
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=9, width=width, weights=True, box_format="cxcywh", device=DEV)
    assert not inp[0].is_contiguous()
    out, grad = compare(inp, host=False, box_format="cxcywh")
    out_c, grad_c = run(mbl, inp[0].contiguous(), *inp[1:4], query_weights=inp[4], box_format="cxcywh")
    assert torch.equal(bits(out), bits(out_c)) and torch.equal(bits(grad), bits(grad_c))
    shifted = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=9, width=width, weights=True, box_format="cxcywh", device=DEV,
                        offset=1)
    assert shifted[0].data_ptr() % 16 != 0
    out_s, grad_s = run(mbl, shifted[0], *inp[1:4], query_weights=inp[4], box_format="cxcywh")
    assert torch.equal(bits(out_s), bits(out_c)) and torch.equal(bits(grad_s), bits(grad_c))


# ------------------------------------------------------------------------------------------------------ realistic shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_realistic_shapes(shape, dtype):
    B, Q, D, objects = SHAPES[shape]
    kw = dict(iou_kind=None, code_weights=CODE_WEIGHTS_10) if D == 10 else dict(box_format="cxcywh")
    inp = shape_case(B, Q, D, objects, dtype, seed=B, device=DEV, weights=shape == "b", box_format=kw.get("box_format", "xyxy"))
    compare(inp, f"({shape}) {name(dtype)}", **kw)


# ----------------------------------------------------------------------------------- complete write, guard bands, bits
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_bitwise_reproducible_and_completely_written(dtype):
    inp = shape_case(16, 300, 4, 40, dtype, seed=2, device=DEV, weights=True)
    first = run(mbl, *inp[:4], query_weights=inp[4])
    for _ in range(5):
        # the allocator hands the freed block of a same-size tensor to the next gradient: NaN in every element
        poison = torch.full(inp[0].shape, float("nan"), dtype=dtype, device=DEV)
        del poison
        again = run(mbl, *inp[:4], query_weights=inp[4])
        assert torch.equal(bits(again[0]), bits(first[0])) and torch.equal(bits(again[1]), bits(first[1]))
    assert bool(torch.isfinite(first[1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", [(3, 7, 4, "giou"), (2, CHUNK + 3, 4, "iou"), (2, 130, 10, None), (1, 5, 3, None)])
def test_guard_bands_around_outputs_gradient_and_workspace(shape, dtype):
    from accvlab import _amd_native as nat

    B, Q, D, kind = shape
    sizes = [min(Q, 5)] * B
    boxes, gt, pind, gind, w = make_case(B, Q, D, sizes, sizes, dtype, seed=4, device=DEV, weights=True)
    lib = nat.ctypes_lib()
    out_dtype = torch.float64 if dtype == torch.float64 else torch.float32
    pad = 512

    def banded(nbytes, as_dtype):
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        inner = buf[pad: pad + nbytes]
        inner.view(as_dtype).fill_(float("nan"))
        return buf, inner

    ws_bytes = lib.accv_matched_box_loss_workspace_bytes(B, Q, D)
    out_buf, out_in = banded(2 * B * (8 if dtype == torch.float64 else 4), out_dtype)
    den_buf, den_in = banded(8, torch.float64)
    ws_buf, ws_in = banded(ws_bytes, torch.float64)
    grad_buf, grad_in = banded(B * Q * D * boxes.element_size(), dtype)
    p = nat.MatchedBoxParams()
    p.iou_eps, p.avg_mode, p.iou_kind = 1e-6, nat.FL_AVG_NUM_POS, {None: nat.MB_IOU_NONE, "iou": nat.MB_IOU, "giou": nat.MB_GIOU}[kind]
    for d in range(D):
        p.code_weights[d] = 1.0
    p.query_weights = w.data_ptr()
    counts = pind.sample_sizes.to(torch.int64)
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}[dtype]
    common = (boxes.data_ptr(), gt.tensor.data_ptr(), pind.tensor.data_ptr(), gind.tensor.data_ptr(), counts.data_ptr())
    shape_args = (dt, nat.MB_IDX_I64, B, Q, D, gt.tensor.shape[1], pind.tensor.shape[1], Q * D, D, ctypes.addressof(p))
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    assert lib.accv_matched_box_loss(*common, *shape_args, out_in.data_ptr(), den_in.data_ptr(), ws_in.data_ptr(), ws_bytes,
                                     stream) == 0, lib.accv_last_error()
    go = torch.ones(2, B, dtype=out_dtype, device=DEV)
    assert lib.accv_matched_box_loss_bwd(*common, go[0].data_ptr(), go[1].data_ptr(), den_in.data_ptr(), *shape_args, grad_in.data_ptr(),
                                         stream) == 0, lib.accv_last_error()
    torch.cuda.synchronize()
    for buf, inner in ((out_buf, out_in), (den_buf, den_in), (ws_buf, ws_in), (grad_buf, grad_in)):
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + inner.numel():] == 0xA5).all())
    grad = grad_in.view(dtype).view(B, Q, D)
    assert bool(torch.isfinite(grad).all()), "the NaN-filled gradient buffer was not written completely"
    out = out_in.view(out_dtype).view(2, B)
    assert bool(torch.isfinite(out).all()), "the NaN-filled outputs were not written completely"
    want, gwant, factor = definition(boxes, gt, pind, gind, query_weights=w, iou_kind=kind)
    check_losses(out, want, dtype)
    check_grad(grad.clone(), gwant, dtype)
    assert float(den_in.view(torch.float64)) == factor


# ------------------------------------------------------------------------------------------- no synchronisation, graphs
def test_no_synchronisation_forward_and_backward():
    inp = shape_case(8, 900, 4, 100, torch.float32, seed=3, device=DEV, weights=True)
    wide = shape_case(8, 300, 10, 40, torch.float32, seed=3, device=DEV)
    avg = torch.tensor(17.0, device=DEV)
    cw_dev = torch.tensor(CODE_WEIGHTS_10, device=DEV)
    x = inp[0].detach().requires_grad_(True)
    y = wide[0].detach().requires_grad_(True)
    go = torch.ones(8, device=DEV)
    torch.autograd.grad(mbl(x, *inp[1:4]), x, (go, go))    # warm-up: library load, allocator
    torch.autograd.grad(mbl(y, *wide[1:4], iou_kind=None), y, (go, go))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in ({}, {"avg_factor": avg, "iou_kind": "iou"},
                   {"avg_factor": 3.0, "query_weights": inp[4], "box_format": "cxcywh", "code_weights": [1.0, 2.0, 1.0, 0.5]}):
            grad, = torch.autograd.grad(mbl(x, *inp[1:4], **kw), x, (go, go))
        for cw in (CODE_WEIGHTS_10, cw_dev):
            grad10, = torch.autograd.grad(mbl(y, *wide[1:4], iou_kind=None, code_weights=cw), y, (go, go))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(grad10).all())


def test_graph_capture_and_replay_with_changed_boxes_and_matches():
    a = shape_case(8, 300, 4, 30, torch.float32, seed=5, device=DEV, box_format="cxcywh")
    b = shape_case(8, 300, 4, 30, torch.float32, seed=6, device=DEV, box_format="cxcywh")
    assert a[2].tensor.shape == b[2].tensor.shape and a[1].tensor.shape == b[1].tensor.shape
    x = a[0].clone().requires_grad_(True)
    gt, pind, gind = (ragged(rb.tensor.clone(), [0] * 8) for rb in a[1:4])
    for rb, src in zip((gt, pind, gind), a[1:4]):
        rb.sample_sizes.copy_(src.sample_sizes)
    go = torch.ones(8, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            l1, iou = mbl(x, gt, pind, gind, box_format="cxcywh")
            grad, = torch.autograd.grad((l1, iou), x, (go, go))
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l1, iou = mbl(x, gt, pind, gind, box_format="cxcywh")
        grad, = torch.autograd.grad((l1, iou), x, (go, go))
    for case in (b, a):
        with torch.no_grad():
            x.copy_(case[0])
        for rb, src in zip((gt, pind, gind), case[1:4]):
            rb.tensor.copy_(src.tensor)
            rb.sample_sizes.copy_(src.sample_sizes)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(mbl, *case[:4], box_format="cxcywh")
        out = torch.stack([l1, iou])
        assert torch.equal(bits(out), bits(eager[0])) and torch.equal(bits(grad), bits(eager[1]))
        want, gwant, _ = definition(*case[:4], box_format="cxcywh")
        check_losses(out, want, torch.float32, "replay")
        check_grad(grad.clone(), gwant, torch.float32, "replay")


# ----------------------------------------------------------------------------------------------------------- end to end
def test_set_criterion_fused_equals_the_composed_criterion():
    """matching cost -> assignment -> focal + box losses of examples/matched_loss.py, fused against composed, values and
    both gradients, with the tolerances of matched_focal_loss_cases.end_to_end"""
    import matched_loss as ml
    import accvlab.batching_helpers as bh

    gt_boxes_l, gt_labels_l, _, pred_boxes, pred_scores, _ = ml.make_inputs(6, 40, 7, 9, DEV, seed=4)
    logits = (pred_scores.clamp_min(1e-6).log() * 3 + 4).detach()
    gt_boxes = bh.combine_data(gt_boxes_l)
    gt_labels = bh.combine_data(gt_labels_l, other_with_same_sample_sizes=gt_boxes)
    matching = ml.set_criterion_match(logits, pred_boxes, gt_labels, gt_boxes, box_format="xyxy")
    assert int(matching[0].sample_sizes.sum()) == int(gt_boxes.sample_sizes.sum()) > 0
    xa, ba = logits.clone().requires_grad_(True), pred_boxes.clone().requires_grad_(True)
    xb, bb = logits.clone().requires_grad_(True), pred_boxes.clone().requires_grad_(True)
    fused = ml.set_criterion_fused(xa, ba, gt_labels, gt_boxes, box_format="xyxy", matching=matching)
    composed = ml.set_criterion_composed(xb, bb, gt_labels, gt_boxes, box_format="xyxy", matching=matching)
    torch.testing.assert_close(fused, composed, rtol=1e-5, atol=0)
    fused.sum().backward()
    composed.sum().backward()
    torch.testing.assert_close(ba.grad, bb.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-3, atol=1e-6 * float(xb.grad.abs().max()))
    # without a given matching the criterion matches by itself, to the same pairs
    again = ml.set_criterion_fused(logits, pred_boxes, gt_labels, gt_boxes, box_format="xyxy")
    assert torch.equal(bits(again), bits(fused.detach()))
    # the two box compositions on their own, cxcywh included
    for fmt in ("xyxy", "cxcywh"):
        boxes = pred_boxes if fmt == "xyxy" else torch.cat([(pred_boxes[..., :2] + pred_boxes[..., 2:]) / 2,
                                                            pred_boxes[..., 2:] - pred_boxes[..., :2]], -1)
        gtb = gt_boxes if fmt == "xyxy" else gt_boxes.create_with_sample_sizes_like_self(
            torch.cat([(gt_boxes.tensor[..., :2] + gt_boxes.tensor[..., 2:]) / 2, gt_boxes.tensor[..., 2:] - gt_boxes.tensor[..., :2]], -1),
            non_uniform_dim=1)
        f = ml.box_loss_fused(boxes, gtb, *matching, box_format=fmt)
        c = ml.box_loss_composed(boxes, gtb, *matching, box_format=fmt)
        torch.testing.assert_close(f[0], c[0], rtol=1e-5, atol=0)
        torch.testing.assert_close(f[1], c[1], rtol=1e-5, atol=0)


def test_iou_term_equals_matched_pair_loss_sum():
    import accvlab.batching_helpers as bh

    boxes, gt, pind, gind, _ = shape_case(8, 300, 4, 30, torch.float32, seed=7, device=DEV)
    got = mbl(boxes, gt, pind, gind, iou_kind="iou", box_format="xyxy", avg_factor=1.0)[1]
    want = bh.matched_pair_loss_sum(gt, boxes, gind, pind, kind="iou_xyxy", eps=1e-6)
    check_loss(got, want.cpu().double(), torch.float32, "against matched_pair_loss_sum")


# -------------------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("kind", ["giou", "iou", None])
def test_special_values_device_and_host_agree(kind):
    inp = make_case(5, 7, 4, SIZES, PAIRS, torch.float32, seed=17, weights=True, device=DEV)
    boxes, gt, pind, gind, w = inp
    clean = run(mbl, boxes, gt, pind, gind, query_weights=w, iou_kind=kind)
    matched = torch.zeros(5, 7, dtype=torch.bool, device=DEV)
    for b, n in enumerate(PAIRS):
        matched[b, pind.tensor[b, :n]] = True
    # NaN / inf in unmatched rows and their weights, and slots past n_b that point at them: nothing changes
    junk, junk_w = boxes.clone(), w.clone()
    junk[~matched] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device=DEV)
    junk_w[~matched] = float("nan")
    junk_p = pind.tensor.clone()
    for b, n in enumerate(PAIRS):
        junk_p[b, n:] = (~matched[b]).nonzero().flatten()[0]
    out, grad = run(mbl, junk, gt, ragged(junk_p, PAIRS), gind, query_weights=junk_w, iou_kind=kind)
    assert torch.equal(bits(out), bits(clean[0])) and torch.equal(bits(grad), bits(clean[1]))
    assert bool((bits(grad)[~matched] == 0).all())   # exactly +0
    # NaN in a matched prediction: its frame's sums and that query's gradient only
    q = int(pind.tensor[1, 1])
    junk[1, q, 2] = float("nan")
    out, grad = run(mbl, junk, gt, ragged(junk_p, PAIRS), gind, query_weights=junk_w, iou_kind=kind)
    rows = [0] if kind is None else [0, 1]
    assert bool(torch.isnan(out[rows, 1]).all()) and bool(torch.isfinite(out[:, [0, 2, 3, 4]]).all())
    nan = torch.isnan(grad)
    want = torch.zeros_like(nan)
    if kind is None:
        want[1, q, 2] = True
    else:
        want[1, q] = True
    assert torch.equal(nan, want)
    h = to_host((junk, gt, ragged(junk_p, PAIRS), gind, junk_w))
    hout, hgrad = run(mbl, *h[:4], query_weights=h[4], iou_kind=kind)
    assert torch.equal(torch.isnan(out).cpu(), torch.isnan(hout)) and torch.equal(nan.cpu(), torch.isnan(hgrad))


def test_empty_extents_and_frames_without_pairs():
    for B, Q, n in ((0, 6, 0), (3, 0, 0), (3, 6, 0)):
        boxes, gt, pind, gind, _ = make_case(B, Q, 4, [2] * B, [n] * B, torch.float32, seed=1, device=DEV)
        out, grad = run(mbl, boxes, gt, pind, gind)
        assert out.shape == (2, B) and bool((out == 0).all()) and grad.shape == (B, Q, 4) and bool((bits(grad) == 0).all())
    inp = make_case(3, 6, 4, [4, 0, 4], [2, 0, 0], torch.float32, seed=15, device=DEV)
    out, grad = compare(inp, "frames without pairs")
    assert bool((out[:, 1:] == 0).all()) and bool((bits(grad[1:]) == 0).all())
