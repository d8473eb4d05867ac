"""Float64 oracle and inputs of the matching-cost tests (test_matching_cost_cpu.py, test_matching_cost_gpu.py): the
per-pair formulas of accvlab.batching_helpers.batched_matching_cost written as torch broadcasts in float64."""
import torch

KINDS = ["one_minus_prob", "neg_prob", "focal"]
# box terms: (l1_weight, iou_weight, giou_weight, box_format, D)
BOX_TERMS = {
    "none": (0.0, 0.0, 0.0, "xyxy", 4),
    "l1": (0.7, 0.0, 0.0, "xyxy", 8),
    "iou": (0.0, 1.3, 0.0, "xyxy", 4),
    "giou": (0.0, 0.0, 2.0, "xyxy", 4),
    "l1_giou_cxcywh": (5.0, 0.0, 2.0, "cxcywh", 4),
    "l1_iou_giou_cxcywh": (1.0, 0.5, 2.0, "cxcywh", 4),
}
DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64]


def tolerance(dtype):
    return 1e-12 if dtype == torch.float64 else 1e-5


def ragged(tensor, sizes):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=torch.as_tensor(sizes, dtype=torch.int64, device=tensor.device))


def make_case(B, Q, C, sizes, kind, D, box_format, dtype, seed=0, label_dtype=torch.int64, device="cpu", width=None):
    """(pred_scores, gt_labels, pred_boxes, gt_boxes) in `dtype` on `device`; logits in [-30, 30] for the focal kind,
    probabilities otherwise; boxes in `box_format` with positive sizes.  `width` > D stores the predicted boxes in a wider
    tensor and returns the [..., :D] view."""
    g = torch.Generator().manual_seed(seed)
    G = max(sizes) if len(sizes) else 0
    if kind == "focal":
        scores = torch.rand(B, Q, C, generator=g, dtype=torch.float64) * 60.0 - 30.0
    else:
        scores = torch.softmax(torch.randn(B, Q, C, generator=g, dtype=torch.float64) * 2.0, -1)
    labels = torch.randint(0, max(C, 1), (B, G), generator=g).to(label_dtype)

    def boxes(*lead):
        lo = torch.rand(*lead, 2, generator=g, dtype=torch.float64) * 80.0
        wh = 4.0 + torch.rand(*lead, 2, generator=g, dtype=torch.float64) * 30.0
        box = torch.cat([lo + 0.5 * wh, wh], -1) if box_format == "cxcywh" else torch.cat([lo, lo + wh], -1)
        if D > 4:
            box = torch.cat([box, torch.randn(*lead, D - 4, generator=g, dtype=torch.float64) * 3.0], -1)
        return box

    pboxes = boxes(B, Q)
    gboxes = boxes(B, G)
    if width is not None and width > D:
        pboxes = torch.cat([pboxes, torch.randn(B, Q, width - D, generator=g, dtype=torch.float64)], -1)
    pboxes = pboxes.to(device=device, dtype=dtype)
    if width is not None and width > D:
        pboxes = pboxes[..., :D]
    return (scores.to(device=device, dtype=dtype), ragged(labels.to(device), sizes),
            pboxes, ragged(gboxes.to(device=device, dtype=dtype), sizes))


def _xyxy(b, box_format):
    if box_format == "cxcywh":
        cx, cy, w, h = b.unbind(-1)
        return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    return b


def _overlap(p, q):
    area_p = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
    area_g = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    iw = (torch.minimum(p[..., 2], q[..., 2]) - torch.maximum(p[..., 0], q[..., 0])).clamp(min=0.0)
    ih = (torch.minimum(p[..., 3], q[..., 3]) - torch.maximum(p[..., 1], q[..., 1])).clamp(min=0.0)
    inter = iw * ih
    return inter, area_g + area_p - inter


def _floor(x, eps):
    return torch.where(x < eps, torch.full_like(x, eps), x)   # NaN stays


def oracle(pred_scores, gt_labels, pred_boxes, gt_boxes, *, class_cost="one_minus_prob", class_weight=1.0,
           l1_weight=0.0, iou_weight=0.0, giou_weight=0.0, box_format="xyxy", focal_alpha=0.25, focal_gamma=2.0,
           focal_eps=1e-12, iou_eps=1e-6, filler=0.0):
    """([B, Q, G_max] float64 on the CPU, padded-column mask, sum of |weighted term| per pair).  The last one scales the
    tolerance of a float32 evaluation: a sum of large terms that cancel can only be as exact as its terms."""
    sizes_rb = gt_labels if class_weight != 0.0 else (gt_boxes if gt_boxes is not None else gt_labels)
    ref = pred_scores if pred_scores is not None else pred_boxes
    B, Q = ref.shape[0], ref.shape[1]
    G = sizes_rb.tensor.shape[1]
    acc = torch.zeros(B, Q, G, dtype=torch.float64)
    mag = torch.zeros(B, Q, G, dtype=torch.float64)

    def add(term, w):
        nonlocal acc, mag
        acc = acc + term * w
        mag = mag + (term * w).abs()
    if class_weight != 0.0:
        x = pred_scores.detach().cpu().double()
        C = x.shape[-1]
        lab = gt_labels.tensor.cpu().long()
        valid = (lab >= 0) & (lab < C)
        v = x.gather(2, lab.clamp(0, max(C - 1, 0)).unsqueeze(1).expand(B, Q, G)) if C else torch.zeros(B, Q, G,
                                                                                                         dtype=torch.float64)
        v = torch.where(valid.unsqueeze(1), v, torch.full_like(v, float("nan")))
        if class_cost == "one_minus_prob":
            cls = 1.0 - v
        elif class_cost == "neg_prob":
            cls = -v
        else:
            s, t = torch.sigmoid(v), torch.sigmoid(-v)
            cls = (-torch.log(s + focal_eps) * focal_alpha * t.pow(focal_gamma)
                   - (-torch.log(t + focal_eps) * (1.0 - focal_alpha) * s.pow(focal_gamma)))
        add(cls, class_weight)
    if l1_weight != 0.0 or iou_weight != 0.0 or giou_weight != 0.0:
        p = pred_boxes.detach().cpu().double().unsqueeze(2)
        q = gt_boxes.tensor.cpu().double().unsqueeze(1)
        if l1_weight != 0.0:
            add((p - q).abs().sum(-1), l1_weight)
        px, qx = _xyxy(p, box_format), _xyxy(q, box_format)
        if iou_weight != 0.0:
            inter, uni = _overlap(px, qx)
            add(1.0 - inter / _floor(uni, iou_eps), iou_weight)
        if giou_weight != 0.0:
            inter, uni = _overlap(px, qx)
            uni = _floor(uni, iou_eps)
            ew = (torch.maximum(px[..., 2], qx[..., 2]) - torch.minimum(px[..., 0], qx[..., 0])).clamp(min=0.0)
            eh = (torch.maximum(px[..., 3], qx[..., 3]) - torch.minimum(px[..., 1], qx[..., 1])).clamp(min=0.0)
            enclose = _floor(ew * eh, iou_eps)
            add(-(inter / uni - (enclose - uni) / enclose), giou_weight)
    sizes = sizes_rb.sample_sizes.cpu().long().clamp(0, G)
    pad = torch.arange(G).view(1, 1, G) >= sizes.view(B, 1, 1)
    return torch.where(pad, torch.full_like(acc, filler), acc), pad.expand(B, Q, G), mag.masked_fill(pad, 0.0)


def assert_close_nan_aware(got, want, rtol, what="", scale=None):
    """NaN and infinities where `want` has them, elsewhere |got - want| <= rtol * (1 + |want| + |scale|)"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape, what)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN masks differ at {int((gn ^ wn).sum())} entries"
    gi, wi = torch.isinf(got), torch.isinf(want)
    assert torch.equal(gi, wi) and torch.equal(got[gi], want[wi]), f"{what}: infinities differ"
    fin = ~(wn | wi)
    err = (got[fin] - want[fin]).abs()
    lim = rtol * (1.0 + want[fin].abs() + (0.0 if scale is None else scale.detach().cpu().double()[fin].abs()))
    if err.numel():
        k = int(torch.argmax(err / lim))
        assert bool((err <= lim).all()), f"{what}: error {float(err[k]):.3e} at |ref| {float(want[fin][k].abs()):.3e}"


def term_kwargs(kind, box_terms):
    l1, iou, giou, fmt, D = BOX_TERMS[box_terms]
    return dict(class_cost=kind, class_weight=1.0 if kind != "focal" else 2.0, l1_weight=l1, iou_weight=iou,
                giou_weight=giou, box_format=fmt), D
