"""What `box_heatmap_decode` and `nms_boxes` are measured against, and the inputs of their CPU and GPU tests.

`definition` restates the decoder as the per-peak Python loop it replaces (mmdet's CenterNetHead._decode_heatmap followed by
a greedy per-frame NMS; neither mmdet nor torchvision is imported) in numpy float32, one correctly rounded operation per
operator, parenthesised exactly as the comment of csrc/box_decode_arith.h has it.  `nms_definition` does the same for
`nms_boxes`.  The sigmoid is taken in float64 of the float32 input.  (The test of a box against the boxes kept so far runs
over float32 arrays: element-wise the same single roundings.)  `greedy_nms_f64` is the float64 greedy loop on given boxes,
with the smallest distance of a compared IoU from the threshold.

Acceptance (`check`):
  * sample_sizes, labels and source, padding slots included: bit-equal, no case excused.
  * boxes and extras: bit-equal (a NaN extra must meet a NaN); padding rows +0 bit for bit; raw scores bit-equal.
  * sigmoid scores: within BAR, the bar center_decode_cases.py holds the same expression to (imported, not copied).

The only inexact quantity that feeds a comparison is the sigmoid score against score_threshold: `assert_margin` (called by
`run`) requires that no float64 score of a case lies within MARGIN of the threshold used.
"""
import numpy as np
import torch

from center_decode_cases import BAR, MARGIN  # noqa: F401
from center_targets_cases import bits

F32 = np.float32
MAX_EXTENT = 1 << 24


def _np(t):
    return t.detach().cpu().float().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _finite(v):
    return bool(np.isfinite(v))


def _frame_hw(image_hw, f):
    if isinstance(image_hw, torch.Tensor):
        H, W = (int(v) for v in image_hw[f].tolist())
    else:
        H, W = image_hw
    return min(max(H, 0), MAX_EXTENT), min(max(W, 0), MAX_EXTENT)


def _suppressed(kept, box, cls, thr, agnostic):
    """kept: dict of float32 arrays x1, y1, x2, y2, area and int64 cls, ok of the boxes kept so far"""
    n = kept["n"]
    if n == 0:
        return False
    kx1, ky1, kx2, ky2, ka = (kept[k][:n] for k in ("x1", "y1", "x2", "y2", "area"))
    x1, y1, x2, y2, area = box
    lx, rx = np.where(kx1 > x1, kx1, x1), np.where(kx2 < x2, kx2, x2)
    ty, by = np.where(ky1 > y1, ky1, y1), np.where(ky2 < y2, ky2, y2)
    iw, ih = rx - lx, by - ty
    iw, ih = np.where(iw > 0, iw, F32(0)), np.where(ih > 0, ih, F32(0))
    inter = iw * ih
    iou = inter / ((ka + area) - inter)
    hit = kept["ok"][:n] & (iou > thr)
    if not agnostic:
        hit &= kept["cls"][:n] == cls
    return bool(hit.any())


def _new_kept(n):
    k = {name: np.zeros(n, np.float32) for name in ("x1", "y1", "x2", "y2", "area")}
    k["cls"], k["ok"], k["n"] = np.zeros(n, np.int64), np.zeros(n, bool), 0
    return k


def _keep(kept, box, cls, ok):
    n = kept["n"]
    for name, v in zip(("x1", "y1", "x2", "y2", "area"), box):
        kept[name][n] = v
    kept["cls"][n], kept["ok"][n] = cls, ok
    kept["n"] = n + 1


def _order(p, q):
    return (p, q) if p < q else (q, p)


def _to_source(m, order, x1, y1, x2, y2):
    a, b, tx, c, d, ty = (F32(v) for v in m.reshape(6))
    det = a * d - b * c
    ok = all(_finite(v) for v in (a, b, tx, c, d, ty, det)) and det != 0 and _finite(F32(1) / det)
    if not ok:
        return F32(0), F32(0), F32(0), F32(0)
    u1, v1, u2, v2 = x1 - tx, y1 - ty, x2 - tx, y2 - ty
    x1, y1 = (d * u1 - b * v1) / det, (a * v1 - c * u1) / det
    x2, y2 = (d * u2 - b * v2) / det, (a * v2 - c * u2) / det
    if order:
        (x1, x2), (y1, y2) = _order(x1, x2), _order(y1, y2)
    return x1, y1, x2, y2


def _empty(Fn, M, E):
    return dict(boxes=np.zeros((Fn, M, 4), np.float32), score_exact=np.zeros((Fn, M), np.float32),
                score_approx=np.zeros((Fn, M), np.float64), labels=np.zeros((Fn, M), np.int64),
                source=np.full((Fn, M), -1, np.int32), extras=np.zeros((Fn, M, E), np.float32), sizes=np.zeros((Fn,), np.int64))


def definition(peaks, feats, *, image_hw, image_matrices=None, score_threshold=None, scores_are_logits=False, min_size=None,
               clip=True, order_corners=True, iou_threshold=None, class_agnostic=False, post_max_size=None):
    """peaks: (scores, indices, classes); feats: a sequence of maps -> a dict of numpy arrays [F, M, ...]"""
    scores = _np(peaks[0]).astype(np.float32)
    indices, classes = peaks[1].cpu().numpy(), peaks[2].cpu().numpy()
    maps = np.concatenate([_np(m) for m in feats], 1).astype(np.float32)
    Fn, K = scores.shape
    _, C, Hm, Wm = maps.shape
    E = C - 4
    M = K if post_max_size is None else min(K, post_max_size)
    thr = None if score_threshold is None else F32(score_threshold)
    nthr = None if iou_threshold is None else F32(iou_threshold)
    if min_size is not None:
        min_h, min_w = (F32(v) for v in (min_size if isinstance(min_size, (list, tuple)) else (min_size, min_size)))
    mats = None if image_matrices is None else image_matrices.cpu().numpy()
    r = _empty(Fn, M, E)
    r.update(logits=scores_are_logits, all_scores=[], valid=np.zeros((Fn,), np.int64))
    with np.errstate(all="ignore"):
        for f in range(Fn):
            Hi, Wi = _frame_hw(image_hw, f)
            EW, EH = F32(Wi), F32(Hi)
            ux, uy = EW / F32(Wm), EH / F32(Hm)
            kept = _new_kept(K)
            for k in range(K):
                n = kept["n"]
                if n >= M:
                    break
                idx, cls = int(indices[f, k]), int(classes[f, k])
                if not (0 <= idx < Hm * Wm and cls >= 0):
                    continue
                ys, xs = idx // Wm, idx % Wm
                g = maps[f, :, ys, xs]
                cx, cy = F32(xs) + g[0], F32(ys) + g[1]
                hw, hh = F32(0.5) * g[3], F32(0.5) * g[2]
                x1, y1, x2, y2 = (cx - hw) * ux, (cy - hh) * uy, (cx + hw) * ux, (cy + hh) * uy
                if clip:
                    crop = lambda v, e: F32(0) if v < 0 else (e if v > e else v)   # noqa: E731
                    x1, y1, x2, y2 = crop(x1, EW), crop(y1, EH), crop(x2, EW), crop(y2, EH)
                s = scores[f, k]
                s64 = 1.0 / (1.0 + np.exp(-np.float64(s))) if scores_are_logits else np.float64(s)
                r["all_scores"].append(float(s64))
                if thr is not None and not ((s64 if scores_are_logits else s) > thr):
                    continue
                if min_size is not None and not ((y2 - y1) >= min_h and (x2 - x1) >= min_w):
                    continue
                if not all(_finite(v) for v in (x1, y1, x2, y2)):
                    continue
                r["valid"][f] += 1
                box = (x1, y1, x2, y2, (x2 - x1) * (y2 - y1))
                if nthr is not None and _suppressed(kept, box, cls, nthr, class_agnostic):
                    continue
                _keep(kept, box, cls, True)
                if mats is not None:
                    x1, y1, x2, y2 = _to_source(mats[f], order_corners, x1, y1, x2, y2)
                r["boxes"][f, n] = (x1, y1, x2, y2)
                r["score_approx" if scores_are_logits else "score_exact"][f, n] = s64 if scores_are_logits else s
                r["labels"][f, n], r["source"][f, n] = cls, k
                r["extras"][f, n] = g[4:]
            r["sizes"][f] = kept["n"]
    return r


def nms_definition(det, iou_threshold, *, class_agnostic=False, pre_max_size=None, post_max_size=None):
    """det: the five tensors and the sizes -> the dict of `definition`"""
    boxes, scores, labels, source, extras, sizes = (x.cpu().numpy() for x in det)
    Fn, N, E = boxes.shape[0], boxes.shape[1], extras.shape[2]
    M = min(v for v in (N, pre_max_size, post_max_size) if v is not None)
    nthr = None if iou_threshold is None else F32(iou_threshold)
    r = _empty(Fn, M, E)
    r.update(logits=False, all_scores=[])
    with np.errstate(all="ignore"):
        for f in range(Fn):
            n_in = min(max(int(sizes[f]), 0), N)
            n_in = n_in if pre_max_size is None else min(n_in, pre_max_size)
            kept = _new_kept(N)
            for k in range(n_in):
                n = kept["n"]
                if n >= M:
                    break
                x1, y1, x2, y2 = boxes[f, k]
                ok = all(_finite(v) for v in (x1, y1, x2, y2))
                box = (x1, y1, x2, y2, (x2 - x1) * (y2 - y1))
                if nthr is not None and ok and _suppressed(kept, box, int(labels[f, k]), nthr, class_agnostic):
                    continue
                _keep(kept, box, int(labels[f, k]), ok)
                r["boxes"][f, n], r["score_exact"][f, n] = boxes[f, k], scores[f, k]
                r["labels"][f, n], r["source"][f, n], r["extras"][f, n] = labels[f, k], source[f, k], extras[f, k]
            r["sizes"][f] = kept["n"]
    return r


def greedy_nms_f64(boxes, labels, thr, agnostic=False, limit=None):
    """The float64 greedy loop over the n boxes [n, 4] (float64 of the float32 values) in their order: (kept indices, the
    smallest |iou - thr| over every pair the loop compared)."""
    b = np.asarray(boxes, np.float64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept, gap = [], np.inf
    with np.errstate(all="ignore"):
        for k in range(len(b)):
            if limit is not None and len(kept) >= limit:
                break
            dead = False
            for j in kept:
                if not agnostic and labels[j] != labels[k]:
                    continue
                iw = max(0.0, min(b[j, 2], b[k, 2]) - max(b[j, 0], b[k, 0]))
                ih = max(0.0, min(b[j, 3], b[k, 3]) - max(b[j, 1], b[k, 1]))
                inter = iw * ih
                iou = inter / (area[j] + area[k] - inter)
                if np.isnan(iou):
                    continue
                gap = min(gap, abs(iou - thr))
                if iou > thr:
                    dead = True
                    break
            if not dead:
                kept.append(k)
    return kept, gap


def assert_margin(want, score_threshold):
    """no float64 score that was compared lies within MARGIN of the threshold (sigmoid scores are inexact)"""
    if score_threshold is None or not want["logits"] or not want["all_scores"]:
        return
    gap = np.abs(np.asarray(want["all_scores"]) - score_threshold).min()
    assert gap > MARGIN, f"a score lies {gap:.2e} from the threshold: regenerate the case with another seed"


def _close(g, a, tag, name):
    g, a = np.asarray(g, np.float64), np.asarray(a, np.float64)
    same = (np.isnan(g) & np.isnan(a)) | (g == a)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(g - a))
    err = np.where(np.isnan(err), np.inf, err)
    assert err.size == 0 or err.max() <= BAR, f"{tag}: {name} off by {err.max():.3e} (bar {BAR})"


def _same_bits_or_nan(g, a, tag, name):
    assert g.shape == a.shape, f"{tag}: {name} has shape {g.shape}, wanted {a.shape}"
    ok = (bits(g) == bits(a)) | (np.isnan(g) & np.isnan(a))
    assert ok.all(), f"{tag}: {name} differs at {np.argwhere(~ok)[:5].tolist()}: {g[~ok][:5]} vs {a[~ok][:5]}"


def check(result, want, what=""):
    """the acceptance of the module docstring: `result` is the operator's BoxDetections, `want` a definition's dict"""
    sizes = result.boxes.sample_sizes
    for name in ("scores", "labels", "source", "extras"):
        assert getattr(result, name).sample_sizes is sizes, f"{what}: {name} does not share the sample sizes"
    assert sizes.dtype == torch.int64 and np.array_equal(sizes.cpu().numpy(), want["sizes"]), \
        f"{what}: sizes {sizes.cpu().tolist()} vs {want['sizes'].tolist()}"
    for name, dtype in (("labels", torch.int64), ("source", torch.int32)):
        got = getattr(result, name).tensor
        assert got.dtype == dtype and got.is_contiguous(), f"{what}: {name} is {got.dtype}, contiguous {got.is_contiguous()}"
        got = got.cpu().numpy()
        assert got.shape == want[name].shape, f"{what}: {name} has shape {got.shape}, wanted {want[name].shape}"
        assert np.array_equal(got, want[name]), f"{what}: {name} differs at {np.argwhere(got != want[name])[:5].tolist()}"
    for name in ("boxes", "scores", "extras"):
        t = getattr(result, name).tensor
        assert t.dtype == torch.float32 and t.is_contiguous(), f"{what}: {name} is {t.dtype}, contiguous {t.is_contiguous()}"
    got, sc, ex = (getattr(result, n).tensor.cpu().numpy() for n in ("boxes", "scores", "extras"))
    _same_bits_or_nan(got, want["boxes"], what, "boxes")
    _same_bits_or_nan(ex, want["extras"], what, "extras")
    assert sc.shape == want["score_exact"].shape, f"{what}: scores have shape {sc.shape}"
    M = got.shape[1]
    pad = np.arange(M)[None, :] >= want["sizes"][:, None]
    assert not bits(got[pad]).any() and not bits(sc[pad]).any() and not bits(ex[pad]).any(), f"{what}: a padding slot is not +0"
    if want["logits"]:
        _close(sc, want["score_approx"], what, "sigmoid scores")
    else:
        _same_bits_or_nan(sc, want["score_exact"], what, "raw scores")


def check_device_against_host(dev, host, logits, what=""):
    """two results of the operator: everything bit-equal, the sigmoid scores within the bar"""
    assert torch.equal(dev.boxes.sample_sizes.cpu(), host.boxes.sample_sizes.cpu()), f"{what}: sizes"
    for name in ("labels", "source"):
        assert torch.equal(getattr(dev, name).tensor.cpu(), getattr(host, name).tensor.cpu()), f"{what}: {name}"
    for name in ("boxes", "extras"):
        _same_bits_or_nan(getattr(dev, name).tensor.cpu().numpy(), getattr(host, name).tensor.cpu().numpy(), what, name)
    gs, hs = dev.scores.tensor.cpu().numpy(), host.scores.tensor.cpu().numpy()
    if logits:
        _close(gs, hs, what, "sigmoid scores")
    else:
        _same_bits_or_nan(gs, hs, what, "raw scores")


class Case:
    """peaks (scores, indices, classes), feats (a tuple of maps) and the keyword operands that are tensors, on one device"""

    def __init__(self, peaks, feats, **tensors):
        self.peaks, self.feats, self.tensors = tuple(peaks), tuple(feats), tensors

    def to(self, device):
        return Case([x.to(device) for x in self.peaks], [m.to(device) for m in self.feats],
                    **{k: v.to(device) for k, v in self.tensors.items()})

    def clone(self):
        return Case([x.clone() for x in self.peaks], [m.clone() for m in self.feats], **{k: v.clone() for k, v in self.tensors.items()})

    def copy_(self, other):
        for a, b in zip(self.peaks + self.feats, other.peaks + other.feats):
            a.copy_(b)
        for k, v in self.tensors.items():
            v.copy_(other.tensors[k])

    def op_args(self):
        from accvlab.draw_heatmap import HeatmapPeaks

        s, i, c = self.peaks
        return HeatmapPeaks(s, i, c, i, i), list(self.feats)      # ys and xs are not read


SPLITS = {4: [(4,), (2, 2), (1, 1, 1, 1)], 5: [(5,), (2, 2, 1), (4, 1)], 6: [(6,), (2, 2, 2), (3, 3)], 8: [(8,), (2, 2, 4), (2, 1, 1, 2, 2), (1,) * 8]}


def make_case(Fn, K, grid=(64, 64), E=0, dtype=torch.float32, score_dtype=None, seed=0, logits=False, illegal=0.03, split=0,
              classes=3, size=(0.05, 0.3), cells=None, device="cpu"):
    """Random peaks and maps on a grid (W, H).  Scores descend per frame (in (0, 1), or logits in (-4, 4)); indices are random
    cells, of the first `cells` of the map if given (repeats included: identical boxes); classes lie in [0, classes); a
    fraction `illegal` of the peaks gets an index of -1 / H * W / 2^40 or a class of -1.  Maps: offsets in [0, 1), h and w
    between size[0] and size[1] of the map's extent, extras in [-10, 10]; split into maps by SPLITS[4 + E][split]."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    W, H = grid
    s = u(Fn, K).sort(1, descending=True).values
    s = (s * 8 - 4) if logits else s
    idx = torch.randint(0, cells or H * W, (Fn, K), generator=g)
    cls = torch.randint(0, classes, (Fn, K), generator=g)
    bad = u(Fn, K)
    for n, v in enumerate((-1, H * W, 2 ** 40)):
        idx[(bad >= n * illegal / 4) & (bad < (n + 1) * illegal / 4)] = v
    cls[(bad >= 3 * illegal / 4) & (bad < illegal)] = -1
    lo, hi = size
    full = torch.cat([u(Fn, 2, H, W), (lo + (hi - lo) * u(Fn, 1, H, W)) * H, (lo + (hi - lo) * u(Fn, 1, H, W)) * W,
                      u(Fn, 4, H, W) * 20 - 10], 1)[:, :4 + E]
    parts = SPLITS[4 + E][split % len(SPLITS[4 + E])]
    feats = [m.to(dtype).contiguous().to(device) for m in full.split(list(parts), 1)]
    return Case([s.to(score_dtype or dtype).contiguous().to(device), idx.to(device), cls.to(device)], feats)


def run(op, case, **kw):
    """the operator and the definition on the same inputs: (result, want); tensors of the case are keyword operands"""
    kw = dict(case.tensors, **kw)
    got = op(*case.op_args(), **kw)
    want = definition(case.peaks, case.feats, **kw)
    assert_margin(want, kw.get("score_threshold"))
    return got, want


# --------------------------------------------------------------------------------------------------------- placed boxes
def placed_case(K, placed, grid=(64, 64), E=0, scores=None, device="cpu"):
    """One frame on a grid (W, H) that is decoded with image_hw = (H, W), so that ux = uy = 1 and a box with corners on
    multiples of 1 / 4 comes back exactly.  `placed` maps a rank to (x1, y1, x2, y2) or (x1, y1, x2, y2, class): that peak
    sits in the cell of its centre with the offsets and sizes that give the box.  Every other rank is a filler of class 0:
    the box [xs, xs + 0.5] x [ys, ys + 0.5] of a cell of its own that no placed box (grown by a cell) touches.  Scores
    descend from 0.9 unless given."""
    W, H = grid
    maps = torch.zeros((1, 4 + E, H, W), dtype=torch.float32)
    idx = torch.zeros((1, K), dtype=torch.int64)
    cls = torch.zeros((1, K), dtype=torch.int64)
    taken = {}
    for k, p in placed.items():
        x1, y1, x2, y2 = (float(v) for v in p[:4])
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        xs, ys = int(cx), int(cy)
        assert 0 <= xs < W and 0 <= ys < H and (4 * cx).is_integer() and (4 * cy).is_integer()
        row = (cx - xs, cy - ys, y2 - y1, x2 - x1)
        cell = ys * W + xs
        assert taken.setdefault(cell, row) == row, "two placed boxes in one cell must be the same box"
        maps[0, :4, ys, xs] = torch.tensor(row)
        idx[0, k] = cell
        cls[0, k] = p[4] if len(p) > 4 else 0
    clear = lambda c: all(not (p[0] - 1 <= c % W + 1 and c % W <= p[2] + 1 and p[1] - 1 <= c // W + 1 and c // W <= p[3] + 1)   # noqa: E731
                          for p in placed.values())
    free = [c for c in range(H * W) if c not in taken and clear(c)]
    assert len(free) >= K - len(placed)
    n = 0
    for k in range(K):
        if k not in placed:
            c = free[n]
            maps[0, :4, c // W, c % W] = torch.tensor([0.25, 0.25, 0.5, 0.5])
            idx[0, k] = c
            n += 1
    s = torch.linspace(0.9, 0.2, K)[None] if scores is None else torch.as_tensor(scores, dtype=torch.float32)[None]
    return Case([s.clone().to(device), idx.to(device), cls.to(device)], [maps.to(device)])


def kept_ranks(result, f=0):
    n = int(result.source.sample_sizes[f])
    return result.source.tensor[f, :n].tolist()
