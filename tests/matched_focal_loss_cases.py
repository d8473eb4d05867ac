"""The float64 definition of ``matched_focal_loss``, input generators and the comparison rules its CPU and GPU tests
share.

Definition: torchvision's ``sigmoid_focal_loss`` / mmdet's ``py_sigmoid_focal_loss`` on one-hot targets built from the
matching, evaluated in float64 with autograd on the dtype-rounded inputs, in the cancellation-free form of
``elementwise_stable`` (the textbook spelling, ``definition_textbook``, loses the gradient's digits for |x| >~ 28).
A pair (slot ``j < clamp(n_b, 0, K)``) NAMES its query when both of its indices are in range; the lowest slot that names
a query decides its row, also when that slot's label is outside ``[0, C)`` (the row then stays all-background).

Tolerances: per-frame loss 1e-5 relative to the float64 value (float64: 1e-12); float32 gradients
``|g - g64| <= 1e-4 |g64| + 1e-6 max|g64|``; float16 / bfloat16 gradients within one unit in the last place of the float64
gradient rounded to the dtype.
"""
import torch

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64]


def ragged(tensor, sizes):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=torch.as_tensor(sizes, dtype=torch.int64, device=tensor.device))


def make_case(B, Q, C, sizes, n_pairs, dtype, seed=0, index_dtype=torch.int64, label_dtype=torch.int64, device="cpu",
              width=None, sigma=4.0, weights=False):
    """-> (pred_logits, gt_labels, pred_ind, gt_ind, query_weights or None).  Logits ~ N(0, sigma^2) rounded to `dtype`;
    frame b has sizes[b] objects and n_pairs[b] pairs (a random one-to-one matching: distinct queries, distinct
    objects); slots past n_pairs[b] hold zeros.  `width` > C stores the logits in a wider tensor and returns the
    ``[..., :C]`` view."""
    g = torch.Generator().manual_seed(seed)
    G, K = max(list(sizes) + [0]), max(list(n_pairs) + [0])
    W = width or C
    store = (torch.randn(B, Q, W, generator=g, dtype=torch.float64) * sigma).to(dtype).to(device)
    logits = store[..., :C] if W != C else store
    labels = torch.randint(0, max(C, 1), (B, G), generator=g).to(label_dtype)
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
    return (logits, ragged(labels.to(device), sizes), ragged(pind.to(device), n_pairs), ragged(gind.to(device), n_pairs), w)


def shape_case(B, Q, C, max_objects, dtype, seed=0, device="cpu", **kw):
    """a case of a realistic shape: frame b has a random number of objects in [0, max_objects], all of them matched;
    frame 0 is empty and frame 1 full"""
    g = torch.Generator().manual_seed(seed + 1000)
    sizes = [int(v) for v in torch.randint(0, max_objects + 1, (B,), generator=g)]
    if B > 0:
        sizes[0] = 0
    if B > 1:
        sizes[1] = max_objects
    sizes = [min(s, Q) for s in sizes]
    return make_case(B, Q, C, sizes, sizes, dtype, seed=seed, device=device, **kw)


TAIL_LOGITS = [33.0, 35.0, 37.0, 40.0, -33.0, -37.0]    # exact in every dtype; 1 - sigmoid loses 1 % .. 100 % in float64 there


def deep_tail_case(dtype, sigma, device="cpu", seed=21):
    """make_case(5, 100, 11) with logits ~ N(0, sigma^2) (sigma 8 or 16: most sigmoids saturated) and, so that the saturated
    tails are reached on both kinds of element whatever the draw, TAIL_LOGITS planted in frame 1 on its six matched
    (query, label) elements and on the next class of the same queries (background elements)"""
    sizes, pairs = [0, 6, 3, 1, 6], [0, 6, 2, 1, 6]
    inp = make_case(5, 100, 11, sizes, pairs, dtype, seed=seed, weights=True, sigma=sigma, device=device)
    logits, labels, pind, gind, _ = inp
    for j, v in enumerate(TAIL_LOGITS):
        q, c = int(pind.tensor[1, j]), int(labels.tensor[1, int(gind.tensor[1, j])])
        logits[1, q, c] = v
        logits[1, q, (c + 1) % 11] = v
    return inp


def targets(logits, gt_labels, pred_ind, gt_ind):
    """the one-hot target [B, Q, C] (float64, on the CPU) of the definition"""
    B, Q, C = logits.shape
    lab, pi, gi = gt_labels.tensor.cpu(), pred_ind.tensor.cpu(), gt_ind.tensor.cpu()
    n = pred_ind.sample_sizes.cpu()
    G, K = lab.shape[1], pi.shape[1]
    t = torch.zeros(B, Q, C, dtype=torch.float64)
    for b in range(B):
        named = set()
        for j in range(max(0, min(int(n[b]), K))):
            q, g = int(pi[b, j]), int(gi[b, j])
            if 0 <= q < Q and 0 <= g < G and q not in named:
                named.add(q)
                l = int(lab[b, g])
                if 0 <= l < C:
                    t[b, q, l] = 1.0
    return t


def elementwise_stable(x, t, alpha, gamma):
    """the focal term per element without a cancelling subtraction: ``softplus(-x) sigmoid(-x)^gamma`` where t = 1,
    ``softplus(x) sigmoid(x)^gamma`` where t = 0, with ``softplus(-z) = -logsigmoid(z)`` and
    ``sigmoid(z)^gamma = exp(gamma logsigmoid(z))``: every factor, and every factor of the autograd gradient, is a
    product of values that keep their relative precision however far the sigmoid saturates"""
    ls = torch.nn.functional.logsigmoid
    z = torch.where(t > 0.5, x, -x)                    # the logit seen from the element's own class
    loss = -ls(z) * torch.exp(gamma * ls(-z))
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def elementwise_textbook(x, t, alpha, gamma):
    """torchvision's ``sigmoid_focal_loss`` as written: ``1 - p_t`` cancels once ``1 - p`` is within a few units in the
    last place of 1 (float64: |x| >~ 28)"""
    p = x.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def definition_textbook(*args, **kw):
    """`definition` with the textbook form of the element term: accurate for |x| <= 20
    (test_matched_focal_loss_cpu.py::test_stable_and_textbook_definitions_agree_up_to_20), wrong in the deep tails"""
    return definition(*args, elementwise=elementwise_textbook, **kw)


def definition(logits, gt_labels, pred_ind, gt_ind, alpha=0.25, gamma=2.0, query_weights=None, avg_factor=None,
               grad_out=None, elementwise=elementwise_stable):
    """-> (out [B] float64, d sum(out * grad_out) / d logits [B, Q, C] float64, factor), on the CPU"""
    t = targets(logits, gt_labels, pred_ind, gt_ind)
    x = logits.detach().cpu().double().clone().requires_grad_(True)
    loss = elementwise(x, t, alpha, gamma)
    if query_weights is not None:
        loss = loss * query_weights.detach().cpu().double()[..., None]
    if avg_factor is None:
        K = pred_ind.tensor.shape[1]
        factor = max(float(pred_ind.sample_sizes.cpu().clamp(0, K).sum()), 1.0)
    else:
        factor = float(avg_factor)
    out = loss.sum((1, 2)) / factor
    go = torch.ones_like(out) if grad_out is None else grad_out.detach().cpu().double()
    grad, = torch.autograd.grad((out * go).sum(), x) if out.numel() else (torch.zeros_like(x),)
    return out.detach(), grad, factor


def run(op, logits, gt_labels, pred_ind, gt_ind, grad_out=None, **kw):
    """-> (out, gradient) of the operator under test on a fresh leaf"""
    x = logits.detach().requires_grad_(True)
    out = op(x, gt_labels, pred_ind, gt_ind, **kw)
    go = torch.ones_like(out) if grad_out is None else grad_out.to(out.dtype)
    grad, = torch.autograd.grad(out, x, go)
    return out.detach(), grad


def check_loss(out, want, dtype, what=""):
    rel = 1e-12 if dtype == torch.float64 else 1e-5
    o, w = out.detach().cpu().double(), want.double()
    err = (o - w).abs()
    worst = float((err / w.abs().clamp_min(1e-300)).max()) if o.numel() else 0.0
    print(f"{what} loss: worst relative error {worst:.3e} (bound {rel:g})")
    assert bool((err <= rel * w.abs()).all()), f"{what}: loss relative error {worst:.3e} above {rel:g}"


def _ulp_steps(a, b):
    """distance in representable values between two tensors of one 16-bit float dtype"""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (ordered(a) - ordered(b)).abs()


def check_grad(grad, want, dtype, what=""):
    g, w = grad.detach().cpu(), want
    assert g.dtype == dtype and g.shape == w.shape, (g.dtype, g.shape)
    if g.numel() == 0:
        return
    if dtype in (torch.float16, torch.bfloat16):
        steps = _ulp_steps(g, w.to(dtype))
        print(f"{what} gradient: at most {int(steps.max())} ulp from the rounded float64 gradient (bound 1)")
        assert int(steps.max()) <= 1, f"{what}: {int(steps.max())} ulp"
        return
    err = (g.double() - w).abs()
    if dtype == torch.float64:
        bound = 1e-12 * w.abs() + 1e-14 * w.abs().max()
    else:
        bound = 1e-4 * w.abs() + 1e-6 * w.abs().max()
    print(f"{what} gradient: max error {float(err.max()):.3e}, max |g64| {float(w.abs().max()):.3e}, "
          f"smallest margin {float((bound - err).min()):.3e}")
    assert bool((err <= bound).all()), f"{what}: gradient error {float((err - bound).max()):.3e} above the bound"


def bits(t):
    t = t.detach().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _focal_f32(x, t, alpha, gamma, num_pos):
    p = x.sigmoid()
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum((1, 2)) / num_pos


def end_to_end(device, ragged_ops):
    """batched_hungarian_match(class_cost="focal") -> matched_focal_loss + box L1 term against the composed class loss +
    the composed box term, on examples/matched_loss.py::make_inputs; values and both gradients.  ragged_ops: the
    composition is examples/matched_loss.py::focal_class_loss_composed and batched_indexing_access, the fused box term
    matched_pair_loss_sum (all three GPU-only, like the reference's indexed operators); otherwise the same composition is
    spelled with torch indexing, so that the chain is also checked where there is no GPU."""
    import matched_loss as ml
    import accvlab.batching_helpers as bh

    gt_boxes_l, gt_labels_l, _, pred_boxes, pred_scores, _ = ml.make_inputs(6, 40, 7, 9, device, seed=4)
    logits = (pred_scores.clamp_min(1e-6).log() * 3 + 4).detach()     # logits of some spread
    gt_boxes = bh.combine_data(gt_boxes_l)
    gt_labels = bh.combine_data(gt_labels_l, other_with_same_sample_sizes=gt_boxes)
    pred_ind, gt_ind = bh.batched_hungarian_match(logits, gt_labels, pred_boxes, gt_boxes, class_cost="focal",
                                                  l1_weight=0.05, iou_weight=1.0)
    B, Q, C = logits.shape
    K = pred_ind.tensor.shape[1]
    valid = torch.arange(K, device=logits.device)[None] < pred_ind.sample_sizes[:, None]
    frame = torch.arange(B, device=logits.device)[:, None].expand(B, K)[valid]
    qs, gs = pred_ind.tensor[valid], gt_ind.tensor[valid]

    def composed_box_term(boxes):
        if ragged_ops:
            box_g = bh.batched_indexing_access(gt_boxes, gt_ind)
            box_p = bh.batched_indexing_access(boxes, pred_ind)
            term = (box_g.tensor - box_p.tensor).abs().sum(-1)
            return bh.sum_over_targets(box_g.create_with_sample_sizes_like_self(term, non_uniform_dim=1))
        term = (gt_boxes.tensor[frame, gs] - boxes[frame, qs]).abs().sum(-1)
        return torch.zeros(B, device=boxes.device).index_add(0, frame, term)

    def composed_class_term(x):
        if ragged_ops:
            return ml.focal_class_loss_composed(x, gt_labels, pred_ind, gt_ind)
        query_labels = torch.full((B, Q), C, dtype=torch.int64, device=x.device)
        query_labels[frame, qs] = gt_labels.tensor[frame, gs]
        t = torch.nn.functional.one_hot(query_labels, C + 1)[..., :C].to(x.dtype)
        return _focal_f32(x, t, 0.25, 2.0, pred_ind.sample_sizes.sum().clamp(min=1))

    xa, ba = logits.clone().requires_grad_(True), pred_boxes.clone().requires_grad_(True)
    box = bh.matched_pair_loss_sum(gt_boxes, ba, gt_ind, pred_ind, kind="l1") if ragged_ops else composed_box_term(ba)
    fused = ml.focal_class_loss_fused(xa, gt_labels, pred_ind, gt_ind) + box
    xb, bb = logits.clone().requires_grad_(True), pred_boxes.clone().requires_grad_(True)
    composed = composed_class_term(xb) + composed_box_term(bb)
    torch.testing.assert_close(fused, composed, rtol=1e-5, atol=0)
    fused.sum().backward()
    composed.sum().backward()
    torch.testing.assert_close(ba.grad, bb.grad, rtol=1e-5, atol=1e-6)
    # both class terms against the float64 definition: the composition is an f32 evaluation with its own rounding
    want, gwant, _ = definition(logits, gt_labels, pred_ind, gt_ind)
    check_loss(ml.focal_class_loss_fused(logits, gt_labels, pred_ind, gt_ind), want, torch.float32, "fused")
    check_loss(composed_class_term(logits), want, torch.float32, "composed")
    check_grad(xa.grad, gwant, torch.float32, "fused")
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-3, atol=1e-6 * float(gwant.abs().max()))
