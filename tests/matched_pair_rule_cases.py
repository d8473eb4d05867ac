"""One hand-built index set for the three losses over matched pairs (matched_focal_loss, matched_box_loss,
matched_polyline_loss), whose docstrings promise that they always agree on which queries are matched.  Each loss gets inputs
from which the set of matched queries can be read off its gradient; the set must be the one of
matched_box_loss_cases.pairs_of.

The shapes are the smallest that cross every loop and workgroup edge of the pair rule's code (csrc/matched_pairs.h):
Q = 1025 is one past the focal kernel's 1024 queries per workgroup at C = 1 and crosses the box loss's 256 and the polyline
loss's 64 several times; K = 300 is more than the 256 threads of the scan, so its stride loop takes a second trip.
"""
import torch

from matched_box_loss_cases import pairs_of
from matched_focal_loss_cases import ragged

B, Q, K, G = 3, 1025, 300, 5
BOX_D = 4
LINE_P, LINE_D = 2, 2
COUNTS = [300, -4, 10 ** 6]   # frame 1 reads no slot although its slots hold valid indices, frame 2 is clamped to K
NAMED_0 = [0, 63, 64, 255, 256, 1023, 1024]   # the queries that frame 0 names with both indices in range
SKIPPED_0 = [100, 101]                        # named by slots of frame 0 whose g is out of range: they stay unmatched


def indices(index_dtype, device="cpu"):
    """-> (pred_ind, gt_ind) RaggedBatch [B, K]"""
    p = torch.full((B, K), -1, dtype=torch.int64)   # frame 0: every slot not set below has q = -1 and is skipped
    g = torch.zeros((B, K), dtype=torch.int64)
    slots = [(0, 0), (63, 1), (64, 2), (64, 3),     # query 64 twice within the first 64 slots
             (255, 4), (256, 0), (1023, 1), (1024, 2),
             (-1, 0), (Q, 0),                       # q out of range on either side: skipped, not wrapped to 1024 / 0
             (100, -1), (101, G)]                   # g out of range on either side: the query stays unmatched
    for j, (q, gi) in enumerate(slots):
        p[0, j], g[0, j] = q, gi
    p[0, K - 1], g[0, K - 1] = 256, 3               # query 256 again, with another g, in the scan's second trip
    j = torch.arange(K)
    p[1], g[1] = j, j % G                           # valid, but n = -4: never read
    p[2], g[2] = (j * 7) % Q, j % G                 # 300 distinct queries (7 and 1025 are coprime) all over the range
    return ragged(p.to(index_dtype).to(device), COUNTS), ragged(g.to(index_dtype).to(device), COUNTS)


def expected(pred_ind, gt_ind):
    """the matched (b, q) by the pair rule, and a check of the case itself"""
    want = {(b, q) for b, q, _ in pairs_of(Q, G, pred_ind, gt_ind)}
    assert {q for b, q in want if b == 0} == set(NAMED_0) and not any(b == 1 for b, _ in want)
    assert len({q for b, q in want if b == 2}) == K
    return want


def _matched(mask):
    return {(int(b), int(q)) for b, q in mask.nonzero().tolist()}


def matched_by_focal(op, pred_ind, gt_ind, dtype, device="cpu"):
    """C = 1, all labels 0, finite logits: the gradient of a matched query is negative (s - 1 times positive factors),
    of every other query positive"""
    gen = torch.Generator().manual_seed(0)
    logits = (torch.rand(B, Q, 1, generator=gen) * 4 - 2).to(dtype).to(device).requires_grad_()
    labels = ragged(torch.zeros(B, G, dtype=torch.int64, device=device), [G] * B)
    op(logits, labels, pred_ind, gt_ind).sum().backward()
    grad = logits.grad[:, :, 0]
    assert bool(((grad < 0) | (grad > 0)).all()), "a focal gradient is zero or NaN"
    return _matched(grad < 0)


def _matched_rows(grad):
    """predictions are ground truth + 1: every element of a matched row has a non-zero L1 gradient, an unmatched row is
    exactly +0"""
    rows = grad.reshape(B, Q, -1)
    any_nz, all_nz = (rows != 0).any(2), (rows != 0).all(2)
    assert torch.equal(any_nz, all_nz), "a row is written in part"
    zero_bits = rows.view(torch.int16 if rows.dtype == torch.float16 else torch.int32) == 0
    assert bool(zero_bits[~any_nz].all()), "an unmatched row is not +0"
    return _matched(any_nz)


def matched_by_box(op, pred_ind, gt_ind, dtype, device="cpu"):
    gen = torch.Generator().manual_seed(1)
    gt = torch.rand(B, G, BOX_D, generator=gen).to(dtype).to(device)
    boxes = (gt.max() + 1 + torch.zeros(B, Q, BOX_D, dtype=dtype, device=device)).requires_grad_()   # above every gt
    l1, _ = op(boxes, ragged(gt, [G] * B), pred_ind, gt_ind, iou_kind=None)
    l1.sum().backward()
    return _matched_rows(boxes.grad)


def matched_by_polyline(op, pred_ind, gt_ind, dtype, device="cpu"):
    gen = torch.Generator().manual_seed(2)
    gt = torch.rand(B, G, LINE_P, LINE_D, generator=gen).to(dtype).to(device)
    lines = (gt.max() + 1 + torch.zeros(B, Q, LINE_P, LINE_D, dtype=dtype, device=device)).requires_grad_()
    pts, _ = op(lines, ragged(gt, [G] * B), pred_ind, gt_ind, dir_loss=False)
    pts.sum().backward()
    return _matched_rows(lines.grad)
