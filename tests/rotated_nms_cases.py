"""What `rotated_iou_bev` and `rotated_nms_bev` are measured against, and the inputs of their CPU and GPU tests.

`iou64` is an independent definition of the rotated BEV IoU in float64: A's corner polygon is clipped against the four edge
half-planes of B IN WORLD COORDINATES (a generic convex Sutherland-Hodgman clip against an arbitrarily oriented
quadrilateral, vectorised over the pairs) — deliberately not the operator's formulation, which moves A into B's frame
and clips against axis-aligned planes.  Pairs whose circumscribed circles are apart are not clipped: their IoU is 0
exactly.  A box whose five values are not all finite, or with dx <= 0 or dy <= 0, has IoU 0 with every box.

`definition` is the sequential NMS loop of mmcv's nms_rotated over that IoU: in slot order a box is kept iff no earlier kept
box has iou > threshold with it; degenerate boxes are kept and suppress nothing; only the first min(size, pre_max_size) slots
exist; the walk stops at post_max_size kept boxes.

Acceptance:
  * IoU values: within BAR = 1e-5 absolute of the float64 definition.  A float32 emulation of the operator's operation
    sequence stayed within 1.8e-7 on 3 302 overlapping nuScenes-like pairs; the bar leaves 50 x that for the platform's
    sinf / cosf and for thinner boxes.  What it leaves was measured off that range (yaws up to 650 turns from zero, strips
    with an aspect of thousands, quarter-turn and axis yaws, far centres): rotated_iou_hard_cases.py, for |yaw| <= 4096.
  * NMS: sizes, kept slots and every pass-through value (all D box columns, score, label, source) bit-equal to the input
    rows the definition keeps, padding +0 / source -1 — no case excused.
  * The margin condition: a keep decision is only comparable where no pair sits on the threshold.  `pick_threshold` takes the
    first of start, start + 0.001, ... for which no pair's float64 IoU of the case lies within MARGIN = 1e-5 of it, over ALL
    pairs of the case, and asserts that at most ten candidates were needed.
"""
import functools
import math

import numpy as np
import torch

BAR = 1e-5
MARGIN = 1e-5
BEV = (0, 1, 3, 4, 6)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- the IoU, float64
def _ok(b):
    return np.isfinite(b).all(-1) & (b[..., 2] > 0) & (b[..., 3] > 0)


def _corners(b):
    """[P, 5] -> [P, 4, 2] counter-clockwise, in world coordinates"""
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    hx, hy = b[:, 2] / 2, b[:, 3] / 2
    sx = np.array([1.0, -1.0, -1.0, 1.0])[None] * hx[:, None]
    sy = np.array([1.0, 1.0, -1.0, -1.0])[None] * hy[:, None]
    return np.stack([b[:, 0:1] + sx * c[:, None] - sy * s[:, None], b[:, 1:2] + sx * s[:, None] + sy * c[:, None]], -1)


def _clip_pairs(a, b):
    """intersection area of the boxes a[p] and b[p], [P, 5] each, all of them valid"""
    P = a.shape[0]
    V = 16
    poly = np.zeros((P, V, 2))
    poly[:, :4] = _corners(a)
    count = np.full(P, 4)
    cb = _corners(b)
    rows = np.arange(P)
    for e in range(4):
        e0, e1 = cb[:, e], cb[:, (e + 1) % 4]
        d = e1 - e0
        out, m = np.zeros((P, V, 2)), np.zeros(P, np.int64)
        for i in range(V - 1):
            act = i < count
            if not act.any():
                break
            S = poly[:, i]
            E = poly[rows, np.where(i + 1 < count, i + 1, 0)]
            dS = d[:, 0] * (S[:, 1] - e0[:, 1]) - d[:, 1] * (S[:, 0] - e0[:, 0])     # >= 0: on the inner side of the edge
            dE = d[:, 0] * (E[:, 1] - e0[:, 1]) - d[:, 1] * (E[:, 0] - e0[:, 0])
            inS, inE = dS >= 0, dE >= 0
            cross = act & (inS != inE)
            with np.errstate(all="ignore"):
                t = dS / (dS - dE)
                X = S + t[:, None] * (E - S)
            idx = np.nonzero(cross)[0]
            out[idx, m[idx]] = X[idx]
            m[idx] += 1
            idx = np.nonzero(act & inE)[0]
            out[idx, m[idx]] = E[idx]
            m[idx] += 1
        poly, count = out, m
        assert count.max(initial=0) <= 8
    pts = np.where((np.arange(V)[None] < count[:, None])[..., None], poly, poly[:, :1])
    rel = pts - pts[:, :1]
    nxt = np.roll(rel, -1, 1)
    return 0.5 * np.abs((rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]).sum(1))


def iou64(a, b):
    """a [Na, 5], b [Nb, 5] (any float dtype) -> float64 [Na, Nb]"""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    # repeated rows (a frame of identical boxes) are clipped once
    ua, ia = np.unique(a, axis=0, return_inverse=True)
    ub, ib = np.unique(b, axis=0, return_inverse=True)
    if len(ua) < len(a) or len(ub) < len(b):
        return iou64(ua, ub)[np.ravel(ia)[:, None], np.ravel(ib)[None, :]]
    out = np.zeros((a.shape[0], b.shape[0]))
    oka, okb = _ok(a), _ok(b)
    with np.errstate(all="ignore"):
        ra, rb = np.hypot(a[:, 2], a[:, 3]) / 2, np.hypot(b[:, 2], b[:, 3]) / 2
        d2 = (a[:, None, 0] - b[None, :, 0]) ** 2 + (a[:, None, 1] - b[None, :, 1]) ** 2
        near = oka[:, None] & okb[None, :] & (d2 <= (ra[:, None] + rb[None, :]) ** 2)
    i, j = np.nonzero(near)
    for lo in range(0, len(i), 1 << 16):
        ii, jj = i[lo:lo + (1 << 16)], j[lo:lo + (1 << 16)]
        inter = _clip_pairs(a[ii], b[jj])
        out[ii, jj] = inter / (a[ii, 2] * a[ii, 3] + b[jj, 2] * b[jj, 3] - inter)
    return out


# ------------------------------------------------------------------------------------------------------- the NMS loop
def nms_frame(iou, ok, n, thr, M):
    """the kept slots of one frame: iou [N, N] float64, ok [N], the first n slots exist, at most M are kept"""
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if len(keep) >= M:
            break
        if not alive[i]:
            continue
        keep.append(i)
        if thr is not None and ok[i]:
            alive[i + 1:] &= ~((iou[i, i + 1:n] > thr) & ok[i + 1:n])
    return keep


class Case:
    """per task boxes [B, N, D], scores, labels, source [B, N] and sizes [B], on one device; `ious` [T][B] float64 [N, N]"""

    def __init__(self, tasks, ious=None):
        self.tasks = tasks
        self.ious = ious if ious is not None else [[iou64(bx[b][:, BEV].cpu().numpy(), bx[b][:, BEV].cpu().numpy())
                                                    for b in range(bx.shape[0])] for bx, *_ in tasks]

    def to(self, device):
        return Case([tuple(x.to(device) for x in t) for t in self.tasks], self.ious)

    def clone(self):
        return Case([tuple(x.clone() for x in t) for t in self.tasks], self.ious)

    def copy_(self, other):
        for mine, theirs in zip(self.tasks, other.tasks):
            for a, b in zip(mine, theirs):
                a.copy_(b)
        self.ious = other.ious

    def detections(self):
        from accvlab.batching_helpers import RaggedBatch
        from accvlab.draw_heatmap import CenterPointDetections

        return [CenterPointDetections(*(RaggedBatch(x, sample_sizes=t[4]) for x in t[:4])) for t in self.tasks]

    def pairs(self, t):
        """the float64 IoU of every pair of existing slots of task t"""
        out = []
        for b, iou in enumerate(self.ious[t]):
            n = int(self.tasks[t][4][b])
            out.append(iou[:n, :n][np.triu_indices(n, 1)])
        return np.concatenate(out) if out else np.zeros(0)


def pick_threshold(case, t, start=0.2):
    """the first of start, start + 0.001, ... that no pair of task t comes within MARGIN of; at most ten candidates"""
    v = case.pairs(t)
    for n in range(10):
        thr = round(start + 0.001 * n, 3)
        if v.size == 0 or np.abs(v - np.float64(np.float32(thr))).min() > MARGIN:
            return thr
    raise AssertionError(f"ten threshold candidates from {start} all have a pair within {MARGIN}: the case is broken")


def assert_margin(case, thresholds):
    for t, thr in enumerate(thresholds):
        v = case.pairs(t)
        if thr is not None and v.size:
            gap = np.abs(v - np.float64(np.float32(thr))).min()
            assert gap > MARGIN, f"task {t}: a pair lies {gap:.2e} from the threshold {thr}"


def definition(case, thresholds, pre_max_size=None, post_max_size=None):
    """per task a dict: kept [B] lists of input slots, sizes [B], M"""
    out = []
    for t, (boxes, scores, labels, source, sizes) in enumerate(case.tasks):
        B, N, _ = boxes.shape
        M = min(v for v in (N, pre_max_size, post_max_size) if v is not None)
        bev = boxes[..., BEV].cpu().numpy().astype(np.float64)
        kept = []
        for b in range(B):
            n = min(max(int(sizes[b]), 0), N)
            n = n if pre_max_size is None else min(n, pre_max_size)
            thr = None if thresholds[t] is None else float(np.float32(thresholds[t]))      # the operator compares in float32
            kept.append(nms_frame(case.ious[t][b], _ok(bev[b]), n, thr, M))
        out.append(dict(kept=kept, sizes=np.array([len(k) for k in kept], np.int64), M=M))
    return out


def check(result, want, case, what=""):
    """sizes, kept rows bit-equal to the input rows the definition keeps, padding +0 / source -1, shapes and sharing"""
    assert len(result) == len(want), what
    for t, (r, w) in enumerate(zip(result, want)):
        tag = f"{what} task {t}"
        inputs = [x.cpu().numpy() for x in case.tasks[t][:4]]
        B, N, D = inputs[0].shape
        M = w["M"]
        sizes = r.boxes.sample_sizes
        for name in ("scores", "labels", "source"):
            assert getattr(r, name).sample_sizes is sizes, f"{tag}: {name} does not share the sample sizes"
        assert sizes.dtype == torch.int64 and tuple(sizes.shape) == (B,), tag
        assert np.array_equal(sizes.cpu().numpy(), w["sizes"]), f"{tag}: sizes {sizes.cpu().tolist()} vs {w['sizes'].tolist()}"
        for name, x, dtype, shape in zip(("boxes", "scores", "labels", "source"), r, (torch.float32, torch.float32, torch.int64, torch.int32),
                                         ((B, M, D), (B, M), (B, M), (B, M))):
            got = x.tensor
            assert got.dtype == dtype and got.is_contiguous() and tuple(got.shape) == shape, f"{tag}: {name} is {got.dtype} {tuple(got.shape)}"
        got = [x.tensor.cpu().numpy() for x in r]
        for b in range(B):
            k = w["kept"][b]
            for name, g, x in zip(("boxes", "scores", "labels", "source"), got, inputs):
                expect = np.zeros((M,) + x.shape[2:], x.dtype)
                if name == "source":
                    expect[:] = -1
                expect[:len(k)] = x[b, k]
                same = g[b].tobytes() == expect.tobytes()
                assert same, (f"{tag} frame {b}: {name} differs; kept by source {g[b][:int(w['sizes'][b])].tolist()[:12] if name == 'source' else ''} "
                              f"wanted slots {k[:12]}")


def share(want, case, thresholds):
    """(kept, suppressed, existing) summed over the tasks that have a threshold"""
    kept = sum(int(w["sizes"].sum()) for w, thr in zip(want, thresholds) if thr is not None)
    total = sum(int(t[4].clamp(0, t[0].shape[1]).sum()) for t, thr in zip(case.tasks, thresholds) if thr is not None)
    return kept, total - kept, total


# -------------------------------------------------------------------------------------------------------------- builders
# (dx, dy) and the scatter of the centres inside a cluster: cars, pedestrians, trucks
KINDS = ((4.5, 1.9, 0.7), (0.7, 0.7, 0.25), (10.0, 2.8, 1.2))


def random_boxes(rng, N, kind, bad=0.02):
    """[N, 5] float32 nuScenes-like BEV boxes in clusters of about three, so that many pairs overlap: centres within +-51.2 m,
    sizes within 20 % of the kind's, yaw close to the cluster's for two thirds and uniform for the rest; a fraction `bad`
    is degenerate (NaN, inf, zero or negative size)"""
    dx, dy, sigma = KINDS[kind % len(KINDS)]
    nc = max(1, N // 3)
    centre = rng.uniform(-50.0, 50.0, (nc, 2))
    cyaw = rng.uniform(-math.pi, math.pi, nc)
    which = rng.integers(0, nc, N)
    xy = np.clip(centre[which] + rng.normal(0, sigma, (N, 2)), -51.2, 51.2)
    size = np.array([dx, dy])[None] * rng.uniform(0.8, 1.2, (N, 2))
    yaw = np.where(rng.random(N) < 0.67, cyaw[which] + rng.normal(0, 0.15, N), rng.uniform(-math.pi, math.pi, N))
    out = np.concatenate([xy, size, yaw[:, None]], 1).astype(np.float32)
    u = rng.random(N)
    for n, (col, v) in enumerate(((0, np.nan), (2, np.inf), (2, 0.0), (3, -1.0), (4, np.nan))):
        out[(u >= n * bad / 5) & (u < (n + 1) * bad / 5), col] = v
    return out


def _task(bev, D, rng, sizes):
    """the five tensors of a task from BEV boxes [B, N, 5]: the other columns, scores, labels and source are random"""
    B, N, _ = bev.shape
    boxes = rng.uniform(-3, 3, (B, N, D)).astype(np.float32)
    boxes[..., BEV] = bev
    scores = -np.sort(-rng.random((B, N)).astype(np.float32), 1)
    labels = rng.integers(0, 10, (B, N)).astype(np.int64)
    source = (2 * np.arange(N, dtype=np.int32) + 5)[None].repeat(B, 0)      # distinct, and not the slot: passed through, not made
    return (torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(labels), torch.from_numpy(np.ascontiguousarray(source)),
            torch.tensor(sizes, dtype=torch.int64))


def frame_sizes(B, N):
    return [N, max(N - 7, 0), N // 2, N, 0][:B] if B <= 5 else [N] * B


@functools.lru_cache(maxsize=None)
def _frames(B, N, T, seed):
    """the BEV boxes [T] of [B, N, 5] and their float64 IoU matrices [T][B]: computed once per shape, shared by every D"""
    rng = np.random.default_rng(1000 * seed + N)
    bevs = [np.stack([random_boxes(rng, N, t) for _ in range(B)]) if B else np.zeros((0, N, 5), np.float32) for t in range(T)]
    return bevs, [[iou64(bev[b], bev[b]) for b in range(B)] for bev in bevs]


@functools.lru_cache(maxsize=None)
def make_case(B, N, T=3, D=9, seed=0):
    """T tasks of random clustered boxes (task t of kind t); frame sizes N, N - 7, N // 2.  Cached: treat as read-only."""
    bevs, ious = _frames(B, N, T, seed)
    rng = np.random.default_rng(seed + D)
    return Case([_task(bev, D, rng, frame_sizes(B, N)) for bev in bevs], ious)


FILL = (2.0, 2.0)


def placed_case(N, placed, T=1, D=7):
    """One frame; `placed` maps a slot to (x, y, dx, dy, yaw).  Every other slot is a 2 x 2 filler on a 20 m lattice with
    x, y >= 0; placed boxes belong at negative coordinates, far from all of them.  The same boxes go to every task;
    source is the slot."""
    bev = np.zeros((1, N, 5), np.float32)
    for k in range(N):
        bev[0, k] = placed[k] if k in placed else (20.0 * (k % 32), 20.0 * (k // 32), FILL[0], FILL[1], 0.0)
    for k, p in placed.items():
        assert p[0] < -10 and p[1] < -10 or not np.isfinite(p[0] + p[1]), "placed boxes sit at negative coordinates"
    rng = np.random.default_rng(N)
    tasks = []
    for _ in range(T):
        boxes, scores, labels, _, sizes = _task(bev, D, rng, [N])
        tasks.append((boxes, scores, labels, torch.arange(N, dtype=torch.int32)[None].contiguous(), sizes))
    return Case(tasks)


def kept_slots(result, t=0, b=0):
    """for placed cases, whose source is the slot"""
    n = int(result[t].source.sample_sizes[b])
    return result[t].source.tensor[b, :n].tolist()


def ragged5(boxes, sizes, device="cpu"):
    from accvlab.batching_helpers import RaggedBatch

    boxes = np.asarray(boxes, np.float32)
    boxes = boxes if boxes.ndim == 3 else boxes.reshape(len(sizes), -1, 5)
    return RaggedBatch(torch.from_numpy(np.ascontiguousarray(boxes)).to(device), sample_sizes=torch.tensor(sizes, dtype=torch.int64, device=device))


# boxes with closed forms: a 4 x 4 and a 2 x 2 box on one centre have IoU 4 / 16 = 0.25, every operation exact in float32
BIG, SMALL = (-100.0, -100.0, 4.0, 4.0, 0.0), (-100.0, -100.0, 2.0, 2.0, 0.0)
# a chain of 4 x 2 boxes 1.5 apart along x: neighbours 5 / 11 = 0.4545, the outer two 2 / 14 = 0.1429
CHAIN = ((-200.0, -100.0, 4.0, 2.0, 0.0), (-198.5, -100.0, 4.0, 2.0, 0.0), (-197.0, -100.0, 4.0, 2.0, 0.0))
CHAIN_THR = 0.3
