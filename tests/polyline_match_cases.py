"""The float64 definition of ``batched_polyline_matching_cost`` and ``matched_polyline_loss``, input builders and the
comparison rules their CPU and GPU tests share.

Definition: the equivalent orders of a ground-truth line are built explicitly as an index tensor ``[V, P]`` (``orders``),
the variants gathered as ``[V, P, D]``, the point-wise L1 distance summed and the LOWEST order of the minimum taken; the
loss evaluates its two terms on that order with autograd on the prediction.  Everything is float64 on the dtype-rounded
inputs.  The pair rule is ``matched_box_loss_cases.pairs_of``; the class term of the cost is ``matching_cost_cases.oracle``.

Tolerances are those of ``matching_cost_cases`` (costs: ``1e-5 * (1 + |ref| + sum of |weighted terms|)``, float64 1e-12) and
``matched_box_loss_cases`` (per-frame losses 1e-5 relative, float64 1e-12; float32 gradients ``1e-4 |g64| + 1e-6 max|g64|``,
float64 1e-12 / 1e-14, float16 / bfloat16 that file's rounding allowance).

A gradient comparison is meaningful only where float32 and float64 agree on the order, so ``definition`` also returns
the smallest relative margin between the best and the second best DISTINCT order over all pairs, and ``compare`` asserts
that it exceeds ``MARGIN`` (two orders with the same index vector — forward and reversed shifts of a closed line of two
points — are one order: they give the same loss and the same gradient).
"""
import math

import torch

from matched_box_loss_cases import check_grad, pairs_of  # noqa: F401
from matched_focal_loss_cases import bits, check_loss, ragged  # noqa: F401
from matching_cost_cases import assert_close_nan_aware, oracle as class_oracle, tolerance  # noqa: F401

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64]
SIZES = [3, 0, 5, 1, 4]
PAIRS = [3, 0, 0, 1, 4]    # K = 4: a frame without ground truth, one without pairs, a full one
MARGIN = 1e-3
name = lambda d: str(d).split(".")[-1]


def orders(P, closed, reversible):
    """index tensor [V, P] of the equivalent orders, in the order of the definition"""
    p = torch.arange(P)
    if not closed:
        rows = [p] + ([P - 1 - p] if reversible else [])
    else:
        rows = [(s + p) % P for s in range(P)] + ([(s - p) % P for s in range(P)] if reversible else [])
    return torch.stack(rows)


def random_line(g, P, D, closed):
    """an irregular line in about [0, 1]^D whose orders are well separated"""
    if closed:
        ang = (torch.arange(P, dtype=torch.float64) + 0.6 * torch.rand(P, generator=g, dtype=torch.float64)) * (2 * math.pi / P)
        ang = ang + 2 * math.pi * torch.rand((), generator=g, dtype=torch.float64)
        rad = 0.15 + 0.3 * torch.rand(P, generator=g, dtype=torch.float64)
        pts = torch.stack([0.5 + rad * torch.cos(ang), 0.5 + rad * torch.sin(ang)], -1)
    else:
        step = torch.stack([0.4 + torch.rand(P, generator=g, dtype=torch.float64),
                            0.6 * torch.randn(P, generator=g, dtype=torch.float64)], -1) / P
        pts = torch.rand(2, generator=g, dtype=torch.float64) * 0.2 + torch.cumsum(step, 0)
    if D == 3:
        pts = torch.cat([pts, 0.2 * torch.rand(P, 1, generator=g, dtype=torch.float64) + torch.linspace(0, 0.3, P)[:, None].double()], -1)
    return pts


def closed_flags(mode, B, G, g):
    if mode == "open":
        return None
    if mode == "closed":
        return torch.ones(B, G, dtype=torch.bool)
    return torch.rand(B, G, generator=g) < 0.5


def make_case(B, Q, P, D, sizes, n_pairs, dtype, seed=0, closed="mixed", reversible=True, index_dtype=torch.int64,
              closed_dtype=torch.bool, device="cpu", width=None, noise=0.05):
    """-> (pred_lines, gt_lines, pred_ind, gt_ind, gt_closed or None).  Frame b has sizes[b] lines and n_pairs[b] pairs (a
    random one-to-one matching); the prediction of a matched query is a random equivalent order of its line plus noise of
    `noise` x the line's extent, every other prediction a random line.  `width` > P * D stores the predictions in a wider
    tensor and returns a strided view."""
    g = torch.Generator().manual_seed(seed)
    G, K = max(list(sizes) + [0]), max(list(n_pairs) + [0])
    flags = closed_flags(closed, B, G, g)
    gt = torch.zeros(B, G, P, D, dtype=torch.float64)
    for b in range(B):
        for i in range(G):
            gt[b, i] = random_line(g, P, D, bool(flags[b, i]) if flags is not None else False)
    pred = torch.stack([torch.stack([random_line(g, P, D, False) for _ in range(Q)]) for _ in range(B)]) if B * Q else \
        torch.zeros(B, Q, P, D, dtype=torch.float64)
    pind = torch.zeros(B, K, dtype=index_dtype)
    gind = torch.zeros(B, K, dtype=index_dtype)
    for b in range(B):
        n = n_pairs[b]
        assert n <= min(Q, sizes[b])
        pind[b, :n] = torch.randperm(Q, generator=g)[:n].to(index_dtype)
        gind[b, :n] = torch.randperm(sizes[b], generator=g)[:n].to(index_dtype)
        for j in range(n):
            q, i = int(pind[b, j]), int(gind[b, j])
            o = orders(P, bool(flags[b, i]) if flags is not None else False, reversible)
            t = gt[b, i][o[int(torch.randint(0, o.shape[0], (1,), generator=g))]]
            extent = float((t.max(0).values - t.min(0).values).max())
            pred[b, q] = t + noise * extent * torch.randn(P, D, generator=g, dtype=torch.float64)
    W = width or P * D
    store = torch.zeros(B, Q, W, dtype=dtype)
    store[..., :P * D] = pred.reshape(B, Q, P * D).to(dtype)
    store = store.to(device)
    lines = store[..., :P * D].unflatten(-1, (P, D)) if W != P * D else store.view(B, Q, P, D)
    gt_rb = ragged(gt.to(dtype).to(device), sizes)
    closed_rb = None if flags is None else ragged(flags.to(closed_dtype).to(device), sizes)
    return lines, gt_rb, ragged(pind.to(device), n_pairs), ragged(gind.to(device), n_pairs), closed_rb


def _closed_at(gt_closed, b, i):
    return bool(gt_closed.tensor[b, i] != 0) if gt_closed is not None else False


def order_sums(x, t, closed, reversible):
    """x [..., P, D], t [P, D] -> (sums [..., V], index tensor [V, P])"""
    o = orders(t.shape[0], closed, reversible)
    return (x.unsqueeze(-3) - t[o]).abs().sum((-1, -2)), o


def lowest_argmin(sums):
    m = sums.min()
    return int((sums == m).nonzero()[0]) if not bool(torch.isnan(m)) else 0


def cost_definition(pred_lines, gt_lines, pred_scores=None, gt_labels=None, gt_closed=None, reversible=True, pts_weight=1.0,
                    class_cost="one_minus_prob", class_weight=0.0, focal_alpha=0.25, focal_gamma=2.0, focal_eps=1e-12,
                    filler=0.0):
    """-> ([B, Q, G_max] float64 on the CPU, padded-column mask, sum of |weighted term| per pair)"""
    sizes_rb = gt_lines if pts_weight != 0.0 else gt_labels
    G = sizes_rb.tensor.shape[1]
    ref = pred_lines if pts_weight != 0.0 else pred_scores
    B, Q = ref.shape[:2]
    acc = torch.zeros(B, Q, G, dtype=torch.float64)
    mag = torch.zeros(B, Q, G, dtype=torch.float64)
    if class_weight != 0.0:
        cls, _, cmag = class_oracle(pred_scores, gt_labels, None, None, class_cost=class_cost, class_weight=class_weight,
                                    focal_alpha=focal_alpha, focal_gamma=focal_gamma, focal_eps=focal_eps)
        acc, mag = acc + cls, mag + cmag
    sizes = sizes_rb.sample_sizes.cpu().long().clamp(0, G)
    if pts_weight != 0.0:
        x = pred_lines.detach().cpu().double()
        t = gt_lines.tensor.detach().cpu().double()
        closed = None if gt_closed is None else ragged(gt_closed.tensor.cpu(), [0] * B)
        for b in range(B):
            for i in range(int(sizes[b])):
                sums, _ = order_sums(x[b], t[b, i], _closed_at(closed, b, i), reversible)
                term = sums.min(-1).values * pts_weight
                term = torch.where(torch.isnan(sums).any(-1), torch.full_like(term, float("nan")), term)
                acc[b, :, i] += term
                mag[b, :, i] += term.abs()
    pad = torch.arange(G).view(1, 1, G) >= sizes.view(B, 1, 1)
    return torch.where(pad, torch.full_like(acc, filler), acc), pad.expand(B, Q, G), mag.masked_fill(pad, 0.0)


def pair_terms(x, t, closed, reversible, dir_eps):
    """x [P, D] (requires grad), t [P, D] -> (pts, dir, relative margin of the best distinct order)"""
    sums, o = order_sums(x.detach(), t, closed, reversible)
    v = lowest_argmin(sums)
    distinct = torch.tensor([not torch.equal(o[k], o[v]) for k in range(o.shape[0])])
    margin = float("inf")
    if bool(distinct.any()) and not bool(torch.isnan(sums).any()):
        margin = float((sums[distinct].min() - sums[v]) / sums[v].clamp_min(1e-300))
    ts = t[o[v]]
    pts = (x - ts).abs().sum()
    if closed:
        a, b = x.roll(-1, 0) - x, ts.roll(-1, 0) - ts
    else:
        a, b = x[1:] - x[:-1], ts[1:] - ts[:-1]
    cos = (a * b).sum(-1) / torch.sqrt(((a * a).sum(-1) + dir_eps) * ((b * b).sum(-1) + dir_eps))
    return pts, (1.0 - cos).sum(), margin


def definition(pred_lines, gt_lines, pred_ind, gt_ind, gt_closed=None, reversible=True, dir_loss=True, dir_eps=1e-12,
               avg_factor=None, grad_out=None):
    """-> (out [2, B], d sum(out * grad_out) / d pred_lines, factor, smallest order margin) in float64 on the CPU"""
    B, Q, P, D = pred_lines.shape
    t = gt_lines.tensor.detach().cpu().double()
    x = pred_lines.detach().cpu().double().clone().requires_grad_(True)
    closed = None if gt_closed is None else ragged(gt_closed.tensor.cpu(), [0] * B)
    if avg_factor is None:
        K = pred_ind.tensor.shape[1]
        factor = max(float(pred_ind.sample_sizes.cpu().clamp(0, K).sum()), 1.0)
    else:
        factor = float(avg_factor)
    rows = [[torch.zeros((), dtype=torch.float64) for _ in range(B)] for _ in range(2)]
    margin = float("inf")
    pairs = pairs_of(Q, t.shape[1], pred_ind, gt_ind)
    for b, q, i in pairs:
        pts, dr, m = pair_terms(x[b, q], t[b, i], _closed_at(closed, b, i), reversible, dir_eps)
        margin = min(margin, m)
        rows[0][b] = rows[0][b] + pts
        if dir_loss:
            rows[1][b] = rows[1][b] + dr
    out = torch.stack([torch.stack(r) for r in rows]) / factor if B else torch.zeros(2, 0, dtype=torch.float64)
    go = torch.ones_like(out) if grad_out is None else grad_out.detach().cpu().double()
    grad = torch.zeros_like(x)
    if len(pairs):
        grad, = torch.autograd.grad((out * go).sum(), x)
    return out.detach(), grad, factor, margin


def run(op, lines, gt, pind, gind, grad_out=None, **kw):
    """-> (out [2, B], gradient) of the operator under test on a fresh leaf"""
    x = lines.detach().requires_grad_(True)
    out = torch.stack(op(x, gt, pind, gind, **kw))
    go = torch.ones_like(out) if grad_out is None else grad_out.to(out.dtype).to(out.device)
    grad, = torch.autograd.grad(out, x, go)
    return out.detach(), grad


def check_losses(out, want, dtype, what=""):
    check_loss(out[0], want[0], dtype, what + " pts")
    check_loss(out[1], want[1], dtype, what + " dir")


def compare(op, inp, what="", grad_out=None, **kw):
    """the operator against the definition on one case, with the order margin asserted; -> (out, grad)"""
    lines, gt, pind, gind, closed = inp
    out, grad = run(op, lines, gt, pind, gind, grad_out=grad_out, gt_closed=closed, **kw)
    ref = dict(kw)
    if isinstance(ref.get("avg_factor"), torch.Tensor):
        ref["avg_factor"] = float(ref["avg_factor"])
    want, gwant, _, margin = definition(lines, gt, pind, gind, gt_closed=closed, grad_out=grad_out, **ref)
    print(f"{what}: smallest order margin {margin:.3e}")
    assert margin > MARGIN, f"{what}: the best order leads by {margin:.3e} only; pick another seed"
    assert out.dtype == (torch.float64 if lines.dtype == torch.float64 else torch.float32) and out.shape == want.shape
    assert grad.is_contiguous() and grad.device == lines.device and grad.shape == lines.shape
    check_losses(out, want, lines.dtype, what)
    check_grad(grad, gwant, lines.dtype, what)
    return out, grad


def check_cost(cost, inp, what="", scores=None, labels=None, **kw):
    """a cost RaggedBatch against the definition: values, bitwise filler, layout"""
    lines, gt, _, _, closed = inp
    want, pad, mag = cost_definition(lines, gt, scores, labels, gt_closed=closed, **kw)
    t = cost.tensor
    dtype = (lines if lines is not None else scores).dtype
    assert t.is_contiguous() and cost.non_uniform_dim == 2
    assert t.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert_close_nan_aware(t, want, tolerance(dtype), what, scale=mag)
    filler = torch.tensor(kw.get("filler", 0.0), dtype=t.dtype)
    assert torch.equal(bits(t.cpu()[pad]), bits(filler).expand(int(pad.sum()))), f"{what}: padded columns are not the filler"


def to_host(inp):
    cpu = lambda rb: None if rb is None else ragged(rb.tensor.cpu(), rb.sample_sizes.cpu().tolist())
    return (inp[0].cpu(),) + tuple(cpu(rb) for rb in inp[1:])


# ------------------------------------------------------------------------------------------------ the torch composition
# What a head writes without the fused operators, in the inputs' dtype on their device, for a batch whose lines are all
# open or all closed: the variants as one broadcast tensor.  scripts/bench_polyline_set_prediction.py times it.
def composed_cost(pred_lines, gt_lines, closed, reversible=True, filler=0.0):
    """[B, Q, G_max] through the [B, Q, G, V, P, D] broadcast"""
    t = gt_lines.tensor
    B, G, P, D = t.shape
    o = orders(P, closed, reversible).to(t.device)
    variants = t[:, :, o]                                                              # [B, G, V, P, D]
    cost = (pred_lines[:, :, None, None] - variants[:, None]).abs().sum((-1, -2)).min(-1).values
    pad = torch.arange(G, device=t.device)[None, None] >= gt_lines.sample_sizes[:, None, None]
    return cost.masked_fill(pad, filler)


def composed_loss(pred_lines, gt_lines, pred_ind, gt_ind, closed, reversible=True, dir_eps=1e-12):
    """(loss_pts [B], loss_dir [B]) through the [M, V, P, D] variants of the matched lines, the best gathered by index"""
    B, Q, P, D = pred_lines.shape
    K = pred_ind.tensor.shape[1]
    dev = pred_lines.device
    valid = torch.arange(K, device=dev)[None] < pred_ind.sample_sizes[:, None]
    frame = torch.arange(B, device=dev)[:, None].expand(B, K)[valid]
    x, t = pred_lines[frame, pred_ind.tensor[valid]], gt_lines.tensor[frame, gt_ind.tensor[valid]]
    variants = t[:, orders(P, closed, reversible).to(dev)]                             # [M, V, P, D]
    best = (x[:, None] - variants).abs().sum((-1, -2)).min(1).indices
    ts = variants[torch.arange(len(t), device=dev), best]
    pts = (x - ts).abs().sum((-1, -2))
    if closed:
        a, b = x.roll(-1, 1) - x, ts.roll(-1, 1) - ts
    else:
        a, b = x[:, 1:] - x[:, :-1], ts[:, 1:] - ts[:, :-1]
    cos = (a * b).sum(-1) / torch.sqrt(((a * a).sum(-1) + dir_eps) * ((b * b).sum(-1) + dir_eps))
    factor = pred_ind.sample_sizes.sum().clamp(min=1)
    zero = torch.zeros(B, dtype=pts.dtype, device=dev)
    return zero.index_add(0, frame, pts) / factor, zero.index_add(0, frame, (1.0 - cos).sum(-1)) / factor
