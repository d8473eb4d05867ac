"""The GPU twin of test_detection_intake_cpu.py for gather_at_centers and center_regression_loss, which have no CPU path:
the same table of malformed inputs on maps [1, 1, 2, 2] and one centre, full message text and exception type, every row
raised before any launch.  Then one well-formed call of every detection operator at that size — against the library's host
entry where it has one, against the definition where it has none — so that each kernel is launched once."""
from types import SimpleNamespace as NS

import pytest
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import (BoxDetections, CenterPointDetections, HeatmapPeaks, box_heatmap_decode, center_point_decode,
                                  center_regression_loss, gather_at_centers, nms_boxes, query_box_decode_2d, query_box_decode_3d,
                                  rotated_iou_bev, rotated_nms_bev)

pytestmark = pytest.mark.gpu

GAC, CRL = "gather_at_centers", "center_regression_loss"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
DEV = torch.device("cuda", 0)
# exp, atan2 and the sigmoid of kernel and host entry agree to a few ulp: the 5 ulp of float32 that center_decode_cases.py
# derives for these operators; everything else is compared bit for bit
ULPS = dict(rtol=5 * 2.0 ** -23, atol=0.0)


def zeros(shape, dtype=F32, dev=DEV):
    return torch.zeros(shape, dtype=dtype, device=dev)


def strided(shape, dtype=F32):
    t = zeros(shape[:-1] + (2 * shape[-1],), dtype)[..., ::2]
    assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
    return t


def centers(t=None, sizes=None):
    return NS(tensor=zeros((1, 1, 2), I32) if t is None else t, sample_sizes=zeros((1,), I64) + 1 if sizes is None else sizes)


def gac(feats=None, where=None):
    return gather_at_centers(zeros((1, 1, 2, 2)) if feats is None else feats, zeros((1, 1), I64) if where is None else where)


def crl(feats=None, c=None, targets=None, weights=None, **kw):
    return center_regression_loss(zeros((1, 1, 2, 2)) if feats is None else feats, centers() if c is None else c,
                                  zeros((1, 1, 1)) if targets is None else targets, weights, **kw)


def both(name, feats, message):
    """a row about the maps, which both operators check with the same words"""
    return [(f"gac-{name}", lambda: gac(feats()), f"{GAC}: {message}"), (f"crl-{name}", lambda: crl(feats()), f"{CRL}: {message}")]


ROWS = [
    *both("feats-none", lambda: (), "feats must be a tensor or a non-empty sequence of tensors"),
    *both("feats-number", lambda: 3.0, "feats must be a tensor or a non-empty sequence of tensors"),
    *both("map-not-tensor", lambda: [zeros((1, 1, 2, 2)), 3.0], "feats[1] must be a tensor"),
    *both("nine-maps", lambda: [zeros((1, 1, 2, 2))] * 9, "at most 8 maps are supported, got 9"),
    *both("cpu-map", lambda: zeros((1, 1, 2, 2), dev="cpu"), "feats[0] must be a CUDA tensor (there is no CPU path)"),
    *both("map-rank", lambda: zeros((1, 2, 2)), "feats[0] must be [B, C, H, W], got 3 dimensions"),
    *both("map-strided", lambda: [zeros((1, 1, 2, 2)), strided((1, 1, 2, 2))], "feats[1] must be contiguous (a map is not copied silently)"),
    *both("map-f64", lambda: zeros((1, 1, 2, 2), F64), "feats must be float32, float16 or bfloat16, got torch.float64"),
    *both("map-dtypes", lambda: [zeros((1, 1, 2, 2)), zeros((1, 1, 2, 2), torch.float16)], "feats[1] has dtype torch.float16, feats[0] torch.float32"),
    *both("map-H", lambda: [zeros((1, 1, 2, 2)), zeros((1, 1, 3, 2))],
          "feats[1] has shape (1, 1, 3, 2), feats[0] (1, 1, 2, 2): B, H and W must agree"),
    *both("channels", lambda: [zeros((1, 33, 2, 2))] * 2, "at most 64 channels in total are supported, got 66"),
    # order: the count before the members, a member's type before its device, its device before its rank, rank before
    # contiguity, all of that before any dtype, the dtype before the shape
    *both("order-nine-not-tensor", lambda: [3.0] * 9, "at most 8 maps are supported, got 9"),
    *both("order-cpu-not-tensor", lambda: [zeros((1, 1, 2, 2), dev="cpu"), 3.0], "feats[0] must be a CUDA tensor (there is no CPU path)"),
    *both("order-cpu-rank", lambda: zeros((1, 2, 2), dev="cpu"), "feats[0] must be a CUDA tensor (there is no CPU path)"),
    *both("order-rank-strided", lambda: strided((1, 2, 2)), "feats[0] must be [B, C, H, W], got 3 dimensions"),
    *both("order-f64-then-rank", lambda: [zeros((1, 1, 2, 2), F64), zeros((1, 2, 2))], "feats[1] must be [B, C, H, W], got 3 dimensions"),
    *both("order-dtype-H", lambda: [zeros((1, 1, 2, 2)), zeros((1, 1, 3, 2), F64)], "feats[1] has dtype torch.float64, feats[0] torch.float32"),
    # the centres: indices
    ("gac-where-text", lambda: gac(where="centres"), f"{GAC}: where must be a RaggedBatch of int32 centres or an int64 tensor [B, K] of indices"),
    ("gac-where-cpu", lambda: gac(where=zeros((1, 1), I64, "cpu")), f"{GAC}: where must be on the maps' device cuda:0, got cpu"),
    ("gac-indices-i32", lambda: gac(where=zeros((1, 1), I32)), f"{GAC}: indices must be int64 [B, K] with B = 1, got torch.int32 (1, 1)"),
    ("gac-indices-rank", lambda: gac(where=zeros((1,), I64)), f"{GAC}: indices must be int64 [B, K] with B = 1, got torch.int64 (1,)"),
    ("gac-indices-B", lambda: gac(where=zeros((2, 1), I64)), f"{GAC}: indices must be int64 [B, K] with B = 1, got torch.int64 (2, 1)"),
    ("gac-indices-strided", lambda: gac(where=strided((1, 2), I64)), f"{GAC}: indices must be contiguous"),
    ("gac-order-indices-i32-strided", lambda: gac(where=strided((1, 2), I32)),
     f"{GAC}: indices must be int64 [B, K] with B = 1, got torch.int32 (1, 2)"),
    # the centres: ragged
    ("crl-centers-tensor", lambda: crl(c=zeros((1, 1, 2), I32)), f"{CRL}: centers must be a RaggedBatch of int32 [B, Nmax, 2] (x, y)"),
    ("gac-centers-cpu", lambda: gac(where=centers(zeros((1, 1, 2), I32, "cpu"))), f"{GAC}: centers must be on the maps' device cuda:0, got cpu"),
    ("crl-sizes-cpu", lambda: crl(c=centers(sizes=torch.ones((1,), dtype=I64))), f"{CRL}: sample_sizes must be on the maps' device cuda:0, got cpu"),
    ("gac-centers-strided", lambda: gac(where=centers(strided((1, 1, 2), I32))), f"{GAC}: centers must be contiguous"),
    ("gac-centers-i64", lambda: gac(where=centers(zeros((1, 1, 2), I64))), f"{GAC}: centers must be int32 [B, Nmax, 2] with B = 1, got torch.int64 (1, 1, 2)"),
    ("crl-centers-rank", lambda: crl(c=centers(zeros((1, 2), I32))), f"{CRL}: centers must be int32 [B, Nmax, 2] with B = 1, got torch.int32 (1, 2)"),
    ("crl-sizes-float", lambda: crl(c=centers(sizes=zeros((1,)))), f"{CRL}: sample_sizes must be int32 or int64 [B], got torch.float32 (1,)"),
    ("gac-sizes-shape", lambda: gac(where=centers(sizes=zeros((2,), I32))), f"{GAC}: sample_sizes must be int32 or int64 [B], got torch.int32 (2,)"),
    # what only the loss takes
    ("crl-kind", lambda: crl(kind="l2"), f"{CRL}: kind must be 'l1' or 'smooth_l1', got 'l2'"),
    ("crl-beta", lambda: crl(kind="smooth_l1", beta=0.0), f"{CRL}: smooth_l1 needs beta > 0, got 0.0"),
    ("crl-beta-nan", lambda: crl(kind="smooth_l1", beta=float("nan")), f"{CRL}: smooth_l1 needs beta > 0, got nan"),
    ("crl-targets-list", lambda: crl(targets=[[[0.0]]]), f"{CRL}: targets must be a tensor or a RaggedBatch"),
    ("crl-targets-cpu", lambda: crl(targets=zeros((1, 1, 1), dev="cpu")), f"{CRL}: targets must be on the maps' device cuda:0, got cpu"),
    ("crl-targets-f64", lambda: crl(targets=zeros((1, 1, 1), F64)), f"{CRL}: targets must be float32, got torch.float64"),
    ("crl-targets-shape", lambda: crl(targets=zeros((1, 2, 1))), f"{CRL}: targets must have shape [1, 1, 1], got [1, 2, 1]"),
    ("crl-weights-shape", lambda: crl(weights=zeros((1,))), f"{CRL}: weights must have shape [1, 1] or [1, 1, 1], got [1]"),
    ("crl-weights-grad", lambda: crl(weights=zeros((1, 1)).requires_grad_()), f"{CRL}: no gradient flows to weights; detach it"),
    ("crl-targets-grad", lambda: crl(targets=zeros((1, 1, 1)).requires_grad_()), f"{CRL}: no gradient flows to targets; detach it"),
    ("crl-order-feats-centers", lambda: crl(feats=zeros((1, 2, 2)), c=zeros((1, 1, 2), I32)), f"{CRL}: feats[0] must be [B, C, H, W], got 3 dimensions"),
    ("crl-order-centers-kind", lambda: crl(c=zeros((1, 1, 2), I32), kind="l2"), f"{CRL}: centers must be a RaggedBatch of int32 [B, Nmax, 2] (x, y)"),
    ("crl-order-kind-targets", lambda: crl(kind="l2", targets=zeros((1, 2, 1))), f"{CRL}: kind must be 'l1' or 'smooth_l1', got 'l2'"),
    ("crl-order-targets-f64-shape", lambda: crl(targets=zeros((1, 2, 1), F64)), f"{CRL}: targets must be float32, got torch.float64"),
]


@pytest.mark.parametrize("call,message", [pytest.param(c, m, id=i) for i, c, m in ROWS])
def test_malformed_input_is_refused_before_any_launch(call, message):
    with pytest.raises(RuntimeError) as e:
        call()
    assert type(e.value) is RuntimeError
    assert str(e.value) == message


def test_every_row_has_its_own_id():
    ids = [i for i, _, _ in ROWS]
    assert len(set(ids)) == len(ids)


# ------------------------------------------------------------------------------------------------------ well-formed calls
def test_gather_and_loss_at_one_centre_equal_the_definition():
    maps = [torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], device=DEV), torch.tensor([[[[-1.0, -2.0], [-3.0, -4.5]]]], device=DEV)]
    xy = torch.tensor([[[1, 0]]], dtype=I32, device=DEV)     # x = 1, y = 0
    c = RaggedBatch(xy, sample_sizes=torch.ones((1,), dtype=I64, device=DEV))
    rows = gather_at_centers(maps, c)
    assert rows.sample_sizes is c.sample_sizes and rows.tensor.tolist() == [[[2.0, -2.0]]]
    assert gather_at_centers(maps, torch.tensor([[3]], device=DEV)).tolist() == [[[4.0, -4.5]]]
    feats = [m.clone().requires_grad_() for m in maps]
    loss = center_regression_loss(feats, c, torch.tensor([[[0.5, 1.0]]], device=DEV))
    assert loss.item() == 1.5 + 3.0                         # |2 - 0.5| + |-2 - 1|, one valid object
    loss.backward()
    assert feats[0].grad.tolist() == [[[[0.0, 1.0], [0.0, 0.0]]]] and feats[1].grad.tolist() == [[[[0.0, -1.0], [0.0, 0.0]]]]


def on(dev, x):
    """a tensor, a HeatmapPeaks or a tuple of RaggedBatch objects on `dev`, the members sharing one sample_sizes again"""
    if isinstance(x, torch.Tensor):
        return x.to(dev)
    if isinstance(x, HeatmapPeaks):
        return HeatmapPeaks(*(t.to(dev) for t in x))
    sizes = x[0].sample_sizes.to(dev)
    return type(x)(*(RaggedBatch(m.tensor.to(dev), sample_sizes=sizes) for m in x))


def same(got, want, what):
    assert type(got) is type(want), what
    assert got[0].sample_sizes.cpu().tolist() == want[0].sample_sizes.tolist(), what
    for name, g, w in zip(type(got)._fields, got, want):
        assert g.sample_sizes is got[0].sample_sizes and g.tensor.device.type == "cuda", (what, name)
        if g.tensor.dtype == F32:
            torch.testing.assert_close(g.tensor.cpu(), w.tensor, **ULPS, msg=lambda m: f"{what}.{name}: {m}")
        else:
            assert torch.equal(g.tensor.cpu(), w.tensor), (what, name)


def test_every_detection_operator_equals_its_host_entry_at_the_smallest_shape():
    g = torch.Generator().manual_seed(7)
    idx = torch.tensor([[0, 3]])
    peaks = HeatmapPeaks(torch.tensor([[0.9, 0.8]]), idx, torch.zeros((1, 2), dtype=I64), idx // 2, idx % 2)
    feats3 = [torch.rand((1, 3, 2, 2), generator=g), torch.rand((1, 5, 2, 2), generator=g) - 0.5]
    kw3 = dict(pc_range=(-1.0, -1.0), voxel_size=(0.5, 0.5), out_size_factor=2, score_threshold=0.1, nms_threshold=0.01)
    cpu3 = center_point_decode(peaks, feats3, [[4]], **kw3)
    gpu3 = center_point_decode(on(DEV, peaks), [on(DEV, m) for m in feats3], [[4]], **kw3)
    assert cpu3[0].boxes.sample_sizes.tolist() == [2] and cpu3[0].labels.tensor.tolist() == [[4, 4]]
    same(gpu3[0], cpu3[0], "center_point_decode")

    feats2 = torch.rand((1, 5, 2, 2), generator=g) + 0.5
    kw2 = dict(image_hw=(8, 8), score_threshold=0.1, iou_threshold=0.99)
    cpu2 = box_heatmap_decode(peaks, feats2, **kw2)
    assert cpu2.boxes.sample_sizes.tolist() == [2] and tuple(cpu2.extras.tensor.shape) == (1, 2, 1)
    same(box_heatmap_decode(on(DEV, peaks), on(DEV, feats2), **kw2), cpu2, "box_heatmap_decode")

    d3 = CenterPointDetections(*(RaggedBatch(x, sample_sizes=cpu3[0].boxes.sample_sizes) for x in
                                 (torch.tensor([[[0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 0.3], [0.1, 0.0, 0.0, 2.0, 1.0, 1.0, 0.3]]]),
                                  cpu3[0].scores.tensor, cpu3[0].labels.tensor, cpu3[0].source.tensor)))
    cpu = rotated_nms_bev(d3, 0.5)
    assert cpu[0].boxes.sample_sizes.tolist() == [1]
    same(rotated_nms_bev(on(DEV, d3), 0.5)[0], cpu[0], "rotated_nms_bev")
    a = RaggedBatch(d3.boxes.tensor[:, :, [0, 1, 3, 4, 6]].contiguous(), sample_sizes=d3.boxes.sample_sizes)
    want = rotated_iou_bev(a, a)
    got = rotated_iou_bev(RaggedBatch(a.tensor.to(DEV), sample_sizes=a.sample_sizes.to(DEV)),
                          RaggedBatch(a.tensor.to(DEV), sample_sizes=a.sample_sizes.to(DEV)))
    assert want.tensor[0, 0, 0].item() == 1.0 and 0.5 < want.tensor[0, 0, 1].item() < 1.0
    torch.testing.assert_close(got.tensor.cpu(), want.tensor, **ULPS)

    d2 = BoxDetections(*(RaggedBatch(x, sample_sizes=cpu2.boxes.sample_sizes) for x in
                         (torch.tensor([[[0.0, 0.0, 4.0, 4.0], [0.0, 0.0, 4.0, 3.5]]]), cpu2.scores.tensor, cpu2.labels.tensor,
                          cpu2.source.tensor, cpu2.extras.tensor)))
    cpu = nms_boxes(d2, 0.5)
    assert cpu.boxes.sample_sizes.tolist() == [1]
    same(nms_boxes(on(DEV, d2), 0.5), cpu, "nms_boxes")

    cls = torch.tensor([[[0.2], [0.7]]])
    rows3 = torch.rand((1, 2, 8), generator=g) - 0.5
    cpu = query_box_decode_3d(cls, rows3, 2, score_threshold=0.5)
    assert cpu.boxes.sample_sizes.tolist() == [2] and cpu.source.tensor.tolist() == [[1, 0]]
    same(query_box_decode_3d(on(DEV, cls), on(DEV, rows3), 2, score_threshold=0.5), cpu, "query_box_decode_3d")
    rows2 = torch.tensor([[[0.5, 0.5, 0.25, 0.5], [0.25, 0.5, 0.5, 0.25]]])
    cpu = query_box_decode_2d(cls, rows2, 1, image_hw=(8, 16), scores_are_logits=False)
    assert cpu.boxes.tensor.tolist() == [[[0.0, 3.0, 8.0, 5.0]]] and cpu.source.tensor.tolist() == [[1]]
    same(query_box_decode_2d(on(DEV, cls), on(DEV, rows2), 1, image_hw=(8, 16), scores_are_logits=False), cpu, "query_box_decode_2d")
