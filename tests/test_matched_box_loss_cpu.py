"""matched_box_loss on the host path (accv_matched_box_loss_host / _bwd_host) against the float64 definition of
tests/matched_box_loss_cases.py, the pair rule's corners, ties and floors against autograd, strides, special values and
the argument checks.  Needs no GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matched_box_loss_cases import (DTYPES, PAIRS, SIZES, bits, check_grad, check_loss, check_losses, compare,  # noqa: E402
                                    definition, make_case, name, ragged, run, shape_case)

from accvlab.batching_helpers import matched_box_loss as mbl  # noqa: E402

CODE_WEIGHTS_10 = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.2, 0.2, 2.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("box_format", ["xyxy", "cxcywh"])
@pytest.mark.parametrize("iou_kind", ["giou", "iou", None])
@pytest.mark.parametrize("weights", [False, True])
def test_host_matches_definition(weights, iou_kind, box_format, dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=3, box_format=box_format, weights=weights)
    g = torch.Generator().manual_seed(1)
    cw = [1.0, 0.5, 2.0, 0.25] if weights else None
    compare(mbl, inp, f"{name(dtype)}/{box_format}/{iou_kind}/w{weights}", grad_out=torch.rand(2, 5, generator=g) + 0.5,
            box_format=box_format, iou_kind=iou_kind, code_weights=cw)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("form", ["none", "sequence", "tensor"])
def test_ten_value_codes_l1_only(form, dtype):
    inp = make_case(5, 7, 10, SIZES, PAIRS, dtype, seed=4, weights=True)
    cw = {"none": None, "sequence": CODE_WEIGHTS_10, "tensor": torch.tensor(CODE_WEIGHTS_10, dtype=torch.float64).to(dtype)}[form]
    out, _ = compare(mbl, inp, f"D10/{form}/{name(dtype)}", iou_kind=None, code_weights=cw)
    assert bool((out[1] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_float32_torch_evaluation_of_the_definition_meets_the_bounds(dtype):
    """the reference alone: a plain float32 torch evaluation of the definition against its float64 evaluation, on the
    inputs the tests use, under the bounds the operator is held to (float64 inputs: the float32 bounds)"""
    for seed, fmt, kind, shape in ((3, "xyxy", "giou", None), (3, "cxcywh", "giou", None), (3, "cxcywh", "iou", None),
                                   (8, "cxcywh", "giou", (8, 900, 100)), (16, "xyxy", "giou", (16, 300, 40))):
        inp = shape_case(shape[0], shape[1], 4, shape[2], dtype, seed=seed, box_format=fmt, weights=True) if shape else \
            make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=seed, box_format=fmt, weights=True)
        boxes, gt, pind, gind, w = inp
        want, gwant, _ = definition(boxes, gt, pind, gind, box_format=fmt, iou_kind=kind, query_weights=w)
        got, ggot, _ = definition(boxes, gt, pind, gind, box_format=fmt, iou_kind=kind, query_weights=w, dtype=torch.float32)
        check_losses(got, want, torch.float32, f"f32 torch {fmt}/{kind}/{shape}")
        check_grad(ggot, gwant, torch.float32, f"f32 torch {fmt}/{kind}/{shape}")


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
def test_index_dtypes(dtype, index_dtype):
    inp = make_case(5, 9, 4, SIZES, PAIRS, dtype, seed=5, index_dtype=index_dtype, box_format="cxcywh")
    compare(mbl, inp, box_format="cxcywh")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms(dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=7)
    out_none, _ = compare(mbl, inp)
    out_raw, _ = compare(mbl, inp, avg_factor=1.0)
    out_num, _ = compare(mbl, inp, avg_factor=3.7)
    out_dev, _ = compare(mbl, inp, avg_factor=torch.tensor(2.5))
    for k in range(2):
        check_loss(out_none[k] * float(sum(PAIRS)), out_raw[k].double(), torch.float32)
        check_loss(out_num[k] * 3.7, out_raw[k].double(), torch.float32)
        check_loss(out_dev[k] * 2.5, out_raw[k].double(), torch.float32)


def test_either_output_alone_can_be_differentiated():
    boxes, gt, pind, gind, _ = make_case(5, 7, 4, SIZES, PAIRS, torch.float32, seed=8)
    for k in range(2):
        go = torch.zeros(2, 5)
        go[k] = 1.0
        x = boxes.clone().requires_grad_(True)
        mbl(x, gt, pind, gind)[k].sum().backward()
        _, gwant, _ = definition(boxes, gt, pind, gind, grad_out=go)
        check_grad(x.grad, gwant, torch.float32, f"output {k}")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("width", [5, 7, 12])
def test_strided_boxes(width, dtype):
    """code[..., :4] of a wider tensor is read in place and equals its contiguous copy bit for bit"""
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=9, width=width, weights=True, box_format="cxcywh")
    assert not inp[0].is_contiguous()
    out, grad = compare(mbl, inp, box_format="cxcywh")
    out_c, grad_c = run(mbl, inp[0].contiguous(), *inp[1:4], query_weights=inp[4], box_format="cxcywh")
    assert torch.equal(bits(out), bits(out_c)) and torch.equal(bits(grad), bits(grad_c))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_base_off_16_byte_alignment_and_query_slices(dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=9, offset=1)
    assert inp[0].data_ptr() % 16 != 0
    compare(mbl, inp)
    sliced = make_case(5, 9, 4, SIZES, PAIRS, dtype, seed=9)[0][:, 1:8]   # a query slice: free query / batch strides
    compare(mbl, (sliced, *inp[1:4], None))


@pytest.mark.parametrize("shape", [(8, 900, 4, 100, "giou"), (16, 300, 4, 40, "iou"), (6, 300, 10, 60, None)])
def test_realistic_shapes_float32(shape):
    B, Q, D, objects, kind = shape
    compare(mbl, shape_case(B, Q, D, objects, torch.float32, seed=B, weights=True), f"{B}x{Q}x{D}", iou_kind=kind)


# ------------------------------------------------------------------------------------------------------------- corners
def _small(dtype=torch.float32, **kw):
    return make_case(3, 6, 4, [4, 4, 4], [3, 3, 3], dtype, seed=11, **kw)


@pytest.mark.parametrize("which", ["pred", "gt"])
@pytest.mark.parametrize("value", [-1, 10 ** 6, -2 ** 40])
def test_indices_outside_their_range_are_skipped_not_wrapped(which, value):
    boxes, gt, pind, gind, _ = _small()
    (pind if which == "pred" else gind).tensor[2, 1] = value
    out, grad = compare(mbl, (boxes, gt, pind, gind, None), avg_factor=1.0)
    # the same as the matching without slot 1 of frame 2
    pind2, gind2 = ragged(pind.tensor.clone(), [3, 3, 2]), ragged(gind.tensor.clone(), [3, 3, 2])
    pind2.tensor[2, 1], gind2.tensor[2, 1] = pind.tensor[2, 2], gind.tensor[2, 2]
    out2, grad2 = run(mbl, boxes, gt, pind2, gind2, avg_factor=1.0)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))


def test_query_named_twice_takes_the_lowest_slot():
    boxes, gt, pind, gind, _ = _small()
    pind.tensor[0] = torch.tensor([4, 2, 4])
    gind.tensor[0] = torch.tensor([1, 0, 3])       # query 4: object 1 (slot 0), not object 3 (slot 2)
    out, grad = compare(mbl, (boxes, gt, pind, gind, None), avg_factor=1.0)
    gind.tensor[0, 2] = 2                          # what the later pair says changes nothing
    out2, grad2 = run(mbl, boxes, gt, pind, gind, avg_factor=1.0)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))
    # a lower slot whose object index is out of range does not name the query: the later slot is its pair
    gind.tensor[0, 0] = 99
    compare(mbl, (boxes, gt, pind, gind, None), avg_factor=1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=name)
def test_sample_sizes_are_clamped_and_slots_past_them_never_read(dtype):
    inp = make_case(5, 7, 4, SIZES, PAIRS, dtype, seed=13, weights=True)
    boxes, gt, pind, gind, w = inp
    out, grad = run(mbl, boxes, gt, pind, gind, query_weights=w)
    junk_p, junk_g = pind.tensor.clone(), gind.tensor.clone()
    for b, n in enumerate(PAIRS):
        junk_p[b, n:] = torch.tensor([3, -5, 2 ** 40, 0, 1, 2 ** 62])[: 6 - n]
        junk_g[b, n:] = torch.tensor([2 ** 50, 0, -1, 1, 2 ** 31, 0])[: 6 - n]
    out2, grad2 = run(mbl, boxes, gt, ragged(junk_p, PAIRS), ragged(junk_g, PAIRS), query_weights=w)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))
    # n_b > K counts as K, n_b < 0 as 0 — in the pairs and in the denominator
    over = [-3, 9, 2, 1, 2 ** 40]
    out3, grad3 = compare(mbl, (boxes, gt, ragged(pind.tensor, over), ragged(gind.tensor, over), w))
    assert torch.equal(bits(out3), bits(out)) and torch.equal(bits(grad3), bits(grad))


def test_frames_without_pairs_give_zero():
    inp = make_case(3, 6, 4, [4, 0, 4], [2, 0, 0], torch.float32, seed=15)
    out, grad = compare(mbl, inp)
    assert bool((out[:, 1:] == 0).all()) and bool((bits(grad[1:]) == 0).all())


@pytest.mark.parametrize("shape", [(0, 6, 0), (3, 0, 0), (3, 6, 0), (3, 6, 2)])
def test_empty_extents_give_zeros(shape):
    B, Q, n = shape
    boxes, gt, pind, gind, _ = make_case(B, Q, 4, [2] * B, [min(n, Q)] * B, torch.float32, seed=1)
    if shape == (3, 6, 2):   # pairs, but no object: G == 0
        gt = ragged(gt.tensor[:, :0], [0] * B)
    out, grad = run(mbl, boxes, gt, pind, gind)
    assert out.shape == (2, B) and out.dtype == torch.float32 and bool((out == 0).all())
    assert grad.shape == (B, Q, 4) and bool((bits(grad) == 0).all())


def test_calling_twice_gives_the_same_bits():
    inp = shape_case(4, 300, 4, 40, torch.float32, seed=2, weights=True)
    a = run(mbl, *inp[:4], query_weights=inp[4])
    b = run(mbl, *inp[:4], query_weights=inp[4])
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


# ------------------------------------------------------------------------------------------------------ ties and floors
# (prediction, ground truth) in the format named; the expected gradient is float64 autograd's over the definition
TIES = {
    "identical": ("xyxy", [0.25, 0.25, 0.75, 0.5], [0.25, 0.25, 0.75, 0.5]),
    "identical_cxcywh": ("cxcywh", [0.5, 0.375, 0.5, 0.25], [0.5, 0.375, 0.5, 0.25]),
    "disjoint": ("xyxy", [0.0, 0.0, 0.25, 0.25], [0.5, 0.5, 0.75, 1.0]),
    "touching_edges": ("xyxy", [0.0, 0.0, 0.5, 0.5], [0.5, 0.25, 1.0, 0.75]),
    "touching_corner": ("xyxy", [0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 1.0, 1.0]),
    "one_shared_edge": ("xyxy", [0.25, 0.25, 0.75, 0.5], [0.25, 0.125, 0.5, 0.75]),
    "contained": ("xyxy", [0.375, 0.375, 0.5, 0.5], [0.25, 0.25, 0.75, 0.75]),
    "zero_area_prediction": ("xyxy", [0.5, 0.25, 0.5, 0.75], [0.25, 0.25, 0.75, 0.75]),
    "zero_area_both_union_floored": ("xyxy", [0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]),
    "point_prediction_far_union_and_enclosure_floored": ("xyxy", [0.25, 0.5, 0.25, 0.5], [0.25, 0.5, 0.25, 0.5000001]),
    "negative_width_cxcywh": ("cxcywh", [0.5, 0.5, -0.25, 0.25], [0.5, 0.5, 0.5, 0.5]),
    "negative_width_cxcywh_disjoint": ("cxcywh", [0.125, 0.5, -0.125, 0.25], [0.75, 0.5, 0.25, 0.5]),
    "l1_equal_coordinates": ("cxcywh", [0.5, 0.25, 0.5, 0.5], [0.5, 0.5, 0.5, 0.25]),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
@pytest.mark.parametrize("kind", ["giou", "iou"])
@pytest.mark.parametrize("case", sorted(TIES))
def test_ties_and_floors_follow_float64_autograd(case, kind, dtype):
    fmt, p, t = TIES[case]
    boxes = torch.tensor([[p]], dtype=torch.float64).to(dtype)
    gt = ragged(torch.tensor([[t]], dtype=torch.float64).to(dtype), [1])
    ind = ragged(torch.zeros(1, 1, dtype=torch.int64), [1])
    go = torch.tensor([[0.5], [2.0]])
    out, grad = run(mbl, boxes, gt, ind, ind, grad_out=go, box_format=fmt, iou_kind=kind)
    want, gwant, _ = definition(boxes, gt, ind, ind, grad_out=go, box_format=fmt, iou_kind=kind)
    print(case, kind, "loss", out.flatten().tolist(), "grad", grad.flatten().tolist(), "autograd", gwant.flatten().tolist())
    check_losses(out, want, dtype, case)
    check_grad(grad, gwant, dtype, case)


# -------------------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("kind", ["giou", "iou", None])
def test_nan_in_a_matched_prediction_stays_in_its_frame_and_query(kind):
    boxes, gt, pind, gind, _ = _small()
    q = int(pind.tensor[1, 1])
    boxes[1, q, 2] = float("nan")
    out, grad = run(mbl, boxes, gt, pind, gind, iou_kind=kind)
    rows = [0] if kind is None else [0, 1]
    assert bool(torch.isnan(out[rows, 1]).all()) and bool(torch.isfinite(out[:, [0, 2]]).all())
    nan = torch.isnan(grad)
    want = torch.zeros_like(nan)
    if kind is None:
        want[1, q, 2] = True
    else:
        want[1, q] = True
    assert torch.equal(nan, want) and bool(torch.isfinite(grad[~nan]).all())
    if kind is not None:   # autograd agrees on the query (for L1 alone torch's sgn(NaN) is 0: it would hide the NaN)
        _, gwant, _ = definition(boxes, gt, pind, gind, iou_kind=kind)
        assert torch.equal(torch.isnan(gwant).any(-1), want.any(-1))


def test_nan_and_inf_in_rows_nothing_points_at_reach_nothing():
    boxes, gt, pind, gind, w = make_case(5, 7, 4, SIZES, PAIRS, torch.float32, seed=17, weights=True)
    out, grad = run(mbl, boxes, gt, pind, gind, query_weights=w)
    junk, junk_w, junk_gt = boxes.clone(), w.clone(), gt.tensor.clone()
    matched = torch.zeros(5, 7, dtype=torch.bool)
    used = torch.zeros(5, 6, dtype=torch.bool)
    for b, n in enumerate(PAIRS):
        matched[b, pind.tensor[b, :n]] = True
        used[b, gind.tensor[b, :n]] = True
    junk[~matched] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")])
    junk_w[~matched] = float("nan")
    junk_gt[~used] = float("nan")
    # slots past n_b point at (now junk) rows
    junk_p, junk_g = pind.tensor.clone(), gind.tensor.clone()
    for b, n in enumerate(PAIRS):
        free = (~matched[b]).nonzero().flatten()
        junk_p[b, n:] = free[0]
        junk_g[b, n:] = 0
    out2, grad2 = run(mbl, junk, ragged(junk_gt, SIZES), ragged(junk_p, PAIRS), ragged(junk_g, PAIRS), query_weights=junk_w)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))
    assert bool((bits(grad2)[~matched] == 0).all())   # exactly +0


# ------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_name_the_operator():
    boxes, gt, pind, gind, w = _small(weights=True)
    wide = make_case(3, 6, 10, [4, 4, 4], [3, 3, 3], torch.float32, seed=11)
    bad = [
        (lambda: mbl(boxes.to(torch.int32), gt, pind, gind), TypeError),
        (lambda: mbl(boxes.tolist(), gt, pind, gind), TypeError),
        (lambda: mbl(boxes[0], gt, pind, gind), ValueError),
        (lambda: mbl(boxes.transpose(1, 2), gt, pind, gind), ValueError),
        (lambda: mbl(boxes[:, :, None, 0].expand(3, 6, 4), gt, pind, gind), ValueError),
        (lambda: mbl(torch.zeros(3, 6, 17), gt, pind, gind, iou_kind=None), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, box_format="xywh"), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, iou_kind="diou"), ValueError),
        (lambda: mbl(*wide[:4]), ValueError),                                               # an IoU kind with D = 10
        (lambda: mbl(boxes, gt, pind, gind, iou_eps=-1.0), ValueError),
        (lambda: mbl(boxes, gt.tensor, pind, gind), TypeError),
        (lambda: mbl(boxes, ragged(gt.tensor.double(), [4, 4, 4]), pind, gind), TypeError),
        (lambda: mbl(boxes, ragged(gt.tensor[..., :3], [4, 4, 4]), pind, gind), ValueError),
        (lambda: mbl(boxes, ragged(gt.tensor[..., 0], [4, 4, 4]), pind, gind), ValueError),
        (lambda: mbl(boxes, gt, ragged(pind.tensor.float(), [3, 3, 3]), gind), TypeError),
        (lambda: mbl(boxes, gt, ragged(pind.tensor.to(torch.int32), [3, 3, 3]), gind), TypeError),
        (lambda: mbl(boxes, gt, ragged(pind.tensor[:, :2], [2, 2, 2]), gind), ValueError),
        (lambda: mbl(boxes, ragged(gt.tensor[:2], [4, 4]), pind, gind), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, query_weights=w[:, :3]), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, query_weights=w.double()), TypeError),
        (lambda: mbl(boxes, gt, pind, gind, code_weights=[1.0, 2.0]), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, code_weights=torch.ones(3)), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, code_weights=torch.ones(4, dtype=torch.float64)), TypeError),
        (lambda: mbl(boxes, gt, pind, gind, code_weights=3.0), TypeError),
        (lambda: mbl(boxes, gt, pind, gind, avg_factor=torch.tensor([2.0])), ValueError),
        (lambda: mbl(boxes, gt, pind, gind, avg_factor=torch.tensor(2.0, dtype=torch.float64)), ValueError),
        (lambda: mbl(boxes.to("meta"), gt, pind, gind), (RuntimeError, ValueError)),
    ]
    for call, exc in bad:
        with pytest.raises(exc, match="matched_box_loss"):
            call()
    l1, iou = mbl(boxes, gt, pind, gind, query_weights=w)
    assert l1.shape == (3,) and iou.shape == (3,)


def test_operator_is_exported():
    import accvlab.batching_helpers as bh

    assert "matched_box_loss" in bh.__all__ and bh.matched_box_loss is mbl


def test_c_abi_argument_validation():
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    p = nat.MatchedBoxParams()
    p.iou_eps, p.avg_mode, p.iou_kind = 1e-6, nat.FL_AVG_NUM_POS, nat.MB_GIOU
    d = ctypes.c_void_p(64)
    fwd = lambda *, params=ctypes.addressof(p), dtype=0, flags=0, B=2, Q=3, D=4, sq=4, boxes=d, ws=d, nbytes=1 << 20: \
        lib.accv_matched_box_loss(boxes, d, d, d, d, dtype, flags, B, Q, D, 5, 2, 12, sq, params, d, d, ws, nbytes, None)
    assert fwd(params=None) == -1 and b"null params" in lib.accv_last_error()
    assert fwd(dtype=4) == -1 and fwd(flags=8) == -1 and fwd(B=-1) == -1
    assert fwd(sq=3) == -1 and b"stride" in lib.accv_last_error()
    assert fwd(D=17) == -1 and fwd(D=0) == -1 and b"D <= 16" in lib.accv_last_error()
    assert fwd(D=5, sq=5) == -1 and b"D == 4" in lib.accv_last_error()
    assert fwd(boxes=None) == -1
    assert fwd(boxes=ctypes.c_void_p(66)) == -1 and b"aligned" in lib.accv_last_error()
    assert fwd(nbytes=8) == -3 and fwd(ws=None) == -3
    assert fwd(B=0) == 0 and fwd(Q=0) == 0
    p.iou_kind = 3
    assert fwd() == -1 and b"IoU kind" in lib.accv_last_error()
    p.iou_kind, p.avg_mode = nat.MB_IOU, 7
    assert fwd() == -1 and b"avg_factor mode" in lib.accv_last_error()
    p.avg_mode = nat.FL_AVG_DEVICE
    assert fwd() == -1 and b"avg_factor pointer" in lib.accv_last_error()
    assert lib.accv_matched_box_loss_workspace_bytes(8, 900, 4) >= 2 * 8 * 8
    assert lib.accv_matched_box_loss_workspace_bytes(0, 900, 4) == 0
