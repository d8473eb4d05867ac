"""The float64 definition of ``matched_box_loss``, input generators and the comparison rules its CPU and GPU tests share.

Definition: the pair rule of ``matched_focal_loss`` (a slot ``j < clamp(n_b, 0, K)`` NAMES its query when both of its
indices are in range; the lowest slot that names a query is its pair) as a Python loop, mmdet's ``bbox_cxcywh_to_xyxy``,
IoU / GIoU as in ``matching_cost_cases.oracle`` (its ``_overlap`` and ``_floor``, ``torch.maximum`` / ``torch.minimum``), L1
with ``code_weights``, ``query_weights``, per-frame sums divided by the factor — evaluated in float64 on the dtype-rounded
inputs, the gradients by autograd.

Tolerances (those of ``matched_focal_loss_cases``): per-frame loss 1e-5 relative to the float64 value (float64: 1e-12);
float32 gradients ``|g - g64| <= 1e-4 |g64| + 1e-6 max|g64|`` (float64: 1e-12 / 1e-14); float16 / bfloat16 gradients within
one representable step of the float64 gradient rounded to the dtype OR within the float32 bound: a GIoU gradient
component is a signed sum, and a small one can sit more than a 16-bit step from the truth while its float32 error is
ordinary.  ``test_matched_box_loss_cpu.py::test_float32_torch_evaluation_of_the_definition_meets_the_bounds`` checks that
a plain float32 torch evaluation of the definition stays inside them on the inputs used here.
"""
import torch

from matched_focal_loss_cases import _ulp_steps, bits, check_loss, ragged  # noqa: F401
from matching_cost_cases import _floor, _overlap, _xyxy

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64]
SIZES = [0, 6, 3, 1, 6]   # ragged, an empty frame, full ones
PAIRS = [0, 6, 2, 1, 6]   # K = 6: frames 1 and 4 have n_b = K
name = lambda d: str(d).split(".")[-1]


def random_boxes(g, lead, D, box_format):
    """boxes in [0, 1] with sides >= 0.05 (the IoU arithmetic is well conditioned); coordinates past 4 are N(0, 1)"""
    wh = 0.05 + torch.rand(*lead, 2, generator=g, dtype=torch.float64) * 0.4
    lo = torch.rand(*lead, 2, generator=g, dtype=torch.float64) * (1.0 - wh)
    box = torch.cat([lo + 0.5 * wh, wh], -1) if box_format == "cxcywh" else torch.cat([lo, lo + wh], -1)
    if D > 4:
        box = torch.cat([box, torch.randn(*lead, D - 4, generator=g, dtype=torch.float64)], -1)
    return box[..., :D]


def make_case(B, Q, D, sizes, n_pairs, dtype, seed=0, box_format="xyxy", index_dtype=torch.int64, device="cpu", width=None,
              weights=False, offset=0):
    """-> (pred_boxes, gt_boxes, pred_ind, gt_ind, query_weights or None).  Frame b has sizes[b] objects and n_pairs[b]
    pairs (a random one-to-one matching); slots past n_pairs[b] hold zeros.  `width` > D stores the predictions in a wider
    tensor and returns the ``[..., :D]`` view; `offset` shifts their base by that many elements (off 16-byte alignment)."""
    g = torch.Generator().manual_seed(seed)
    G, K = max(list(sizes) + [0]), max(list(n_pairs) + [0])
    W = width or D
    pred = random_boxes(g, (B, Q), D, box_format)
    if W > D:
        pred = torch.cat([pred, torch.randn(B, Q, W - D, generator=g, dtype=torch.float64)], -1)
    flat = torch.zeros(B * Q * W + offset, dtype=dtype, device=device)
    flat[offset:] = pred.reshape(-1).to(dtype).to(device)
    store = flat[offset:].view(B, Q, W)
    boxes = store[..., :D] if W != D else store
    gt = random_boxes(g, (B, G), D, box_format).to(dtype).to(device)
    pind = torch.zeros(B, K, dtype=index_dtype)
    gind = torch.zeros(B, K, dtype=index_dtype)
    for b in range(B):
        n = n_pairs[b]
        assert n <= min(Q, sizes[b])
        pind[b, :n] = torch.randperm(Q, generator=g)[:n].to(index_dtype)
        gind[b, :n] = torch.randperm(sizes[b], generator=g)[:n].to(index_dtype)
    w = None
    if weights:
        w = (0.25 + torch.rand(B, Q, generator=g, dtype=torch.float64)).to(dtype).to(device)
    return boxes, ragged(gt, sizes), ragged(pind.to(device), n_pairs), ragged(gind.to(device), n_pairs), w


def shape_case(B, Q, D, max_objects, dtype, seed=0, device="cpu", **kw):
    """a case of a realistic shape: frame b has a random number of objects in [0, max_objects], all of them matched;
    frame 0 is empty and frame 1 full"""
    g = torch.Generator().manual_seed(seed + 1000)
    sizes = [int(v) for v in torch.randint(0, max_objects + 1, (B,), generator=g)]
    if B > 0:
        sizes[0] = 0
    if B > 1:
        sizes[1] = max_objects
    sizes = [min(s, Q) for s in sizes]
    return make_case(B, Q, D, sizes, sizes, dtype, seed=seed, device=device, **kw)


def pairs_of(Q, G, pred_ind, gt_ind):
    """[(b, q, g)] of the pair rule"""
    pi, gi, n = pred_ind.tensor.cpu(), gt_ind.tensor.cpu(), pred_ind.sample_sizes.cpu()
    K = pi.shape[1]
    out = []
    for b in range(pi.shape[0]):
        named = set()
        for j in range(max(0, min(int(n[b]), K))):
            q, g = int(pi[b, j]), int(gi[b, j])
            if 0 <= q < Q and 0 <= g < G and q not in named:
                named.add(q)
                out.append((b, q, g))
    return out


def pair_terms(p, t, box_format, iou_kind, iou_eps, code_weights):
    """(l1 [N], iou term [N]) of matched rows p, t [N, D] in their dtype"""
    diff = (p - t).abs()
    l1 = (diff * code_weights if code_weights is not None else diff).sum(-1)
    if iou_kind is None:
        return l1, torch.zeros_like(l1)
    px, tx = _xyxy(p, box_format), _xyxy(t, box_format)
    inter, uni = _overlap(px, tx)
    uni = _floor(uni, iou_eps)
    if iou_kind == "iou":
        return l1, 1.0 - inter / uni
    ew = (torch.maximum(px[..., 2], tx[..., 2]) - torch.minimum(px[..., 0], tx[..., 0])).clamp(min=0.0)
    eh = (torch.maximum(px[..., 3], tx[..., 3]) - torch.minimum(px[..., 1], tx[..., 1])).clamp(min=0.0)
    enclose = _floor(ew * eh, iou_eps)
    return l1, 1.0 - (inter / uni - (enclose - uni) / enclose)


def definition(boxes, gt_boxes, pred_ind, gt_ind, box_format="xyxy", iou_kind="giou", code_weights=None, query_weights=None,
               iou_eps=1e-6, avg_factor=None, grad_out=None, dtype=torch.float64):
    """-> (out [2, B], d sum(out * grad_out) / d boxes [B, Q, D], factor) on the CPU, evaluated in `dtype` (float64: the
    definition; float32: the plain torch evaluation the bounds are checked against)"""
    B, Q, D = boxes.shape
    gt = gt_boxes.tensor.detach().cpu().to(dtype)
    x = boxes.detach().cpu().to(dtype).clone().requires_grad_(True)
    pairs = pairs_of(Q, gt.shape[1], pred_ind, gt_ind)
    bs = torch.tensor([p[0] for p in pairs], dtype=torch.int64)
    qs = torch.tensor([p[1] for p in pairs], dtype=torch.int64)
    gs = torch.tensor([p[2] for p in pairs], dtype=torch.int64)
    cw = None
    if code_weights is not None:
        cw = code_weights if isinstance(code_weights, torch.Tensor) else torch.tensor(list(code_weights), dtype=torch.float64)
        cw = cw.detach().cpu().to(dtype)
    l1, iou = pair_terms(x[bs, qs], gt[bs, gs], box_format, iou_kind, iou_eps, cw)
    if query_weights is not None:
        w = query_weights.detach().cpu().to(dtype)[bs, qs]
        l1, iou = l1 * w, iou * w
    if avg_factor is None:
        K = pred_ind.tensor.shape[1]
        factor = max(float(pred_ind.sample_sizes.cpu().clamp(0, K).sum()), 1.0)
    else:
        factor = float(avg_factor)
    out = torch.stack([torch.zeros(B, dtype=dtype).index_add(0, bs, l1), torch.zeros(B, dtype=dtype).index_add(0, bs, iou)]) / factor
    go = torch.ones_like(out) if grad_out is None else grad_out.detach().cpu().to(dtype)
    grad = torch.zeros_like(x)
    if len(pairs):
        grad, = torch.autograd.grad((out * go).sum(), x)
    return out.detach(), grad, factor


def run(op, boxes, gt_boxes, pred_ind, gt_ind, grad_out=None, **kw):
    """-> (out [2, B], gradient) of the operator under test on a fresh leaf"""
    x = boxes.detach().requires_grad_(True)
    l1, iou = op(x, gt_boxes, pred_ind, gt_ind, **kw)
    out = torch.stack([l1, iou])
    go = torch.ones_like(out) if grad_out is None else grad_out.to(out.dtype).to(out.device)
    grad, = torch.autograd.grad(out, x, go)
    return out.detach(), grad


def grad_bound(want, dtype):
    if dtype == torch.float64:
        return 1e-12 * want.abs() + 1e-14 * want.abs().max()
    return 1e-4 * want.abs() + 1e-6 * want.abs().max()


def check_grad(grad, want, dtype, what=""):
    """`want`: the float64 gradient of the definition"""
    g, w = grad.detach().cpu(), want.double()
    assert g.dtype == dtype and g.shape == w.shape, (g.dtype, g.shape)
    if g.numel() == 0:
        return
    err = (g.double() - w).abs()
    bound = grad_bound(w, dtype)
    if dtype in (torch.float16, torch.bfloat16):
        steps = _ulp_steps(g, w.to(dtype))
        ok = (steps <= 1) | (err <= bound)
        print(f"{what} gradient: at most {int(steps.max())} steps from the rounded float64 gradient; "
              f"{int((steps > 1).sum())} elements rely on the float32 bound; worst excess {float((err - bound)[~ok].max()) if not bool(ok.all()) else 0.0:.3e}")
        assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside one step and the float32 bound"
        return
    print(f"{what} gradient: max error {float(err.max()):.3e}, max |g64| {float(w.abs().max()):.3e}, "
          f"smallest margin {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all()), f"{what}: gradient error {float((err - bound).max()):.3e} above the bound"


def check_losses(out, want, dtype, what=""):
    """both rows of [2, B]; a frame whose definition is exactly 0 must be exactly 0"""
    check_loss(out[0], want[0], dtype, what + " l1")
    check_loss(out[1], want[1], dtype, what + " iou")


def compare(op, inp, what="", grad_out=None, **kw):
    """the operator against the definition on one case; -> (out, grad)"""
    boxes, gt, pind, gind, w = inp
    kw = dict(kw, query_weights=w)
    out, grad = run(op, boxes, gt, pind, gind, grad_out=grad_out, **kw)
    ref = dict(kw)
    if isinstance(ref.get("avg_factor"), torch.Tensor):
        ref["avg_factor"] = float(ref["avg_factor"])
    want, gwant, _ = definition(boxes, gt, pind, gind, grad_out=grad_out, **ref)
    assert out.dtype == (torch.float64 if boxes.dtype == torch.float64 else torch.float32) and out.shape == want.shape
    assert grad.is_contiguous() and grad.device == boxes.device
    check_losses(out, want, boxes.dtype, what)
    check_grad(grad, gwant, boxes.dtype, what)
    return out, grad
