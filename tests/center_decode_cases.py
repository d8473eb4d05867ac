"""What `center_point_decode` is measured against, and the inputs of its CPU and GPU tests.

`definition` restates the operator as the per-peak Python loop it replaces (mmdet3d's CenterPointBBoxCoder.decode and the
`circle` branch of CenterHead.get_bboxes; neither mmdet3d nor mmcv is imported) in numpy float32 SCALARS, one correctly
rounded operation per operator, parenthesised exactly as the comment of csrc/center_decode_arith.h has it.  exp, atan2 and
the sigmoid are taken in float64 of the float32 inputs.  (The test of a peak against the centres kept so far runs over a
float32 array: element-wise the same single roundings.)

Acceptance (`check`):
  * sample_sizes, labels and source, padding slots included: bit-equal, no case excused.
  * x, y, z, velocity and raw-dims channels: bit-equal (a NaN computed from a NaN input must meet a NaN); padding rows +0
    bit for bit; raw scores bit-equal.
  * yaw, exp dims, sigmoid scores and z under bottom_center with norm_bbox: within BAR = 1e-5 absolute, the project's
    float32 bar (center_targets_cases.py).  The inputs keep d in [-1.6, 3]: exp(d) <= 20.1, where one float32 ulp is
    1.9e-6; |yaw| <= pi (ulp 2.4e-7), scores <= 1 (ulp 6e-8), |z| <= 5 + 10 (ulp 9.5e-7): the bar is at least 5 ulp of
    every value compared; NaN must meet NaN and an infinity the same infinity.

The only inexact quantity that feeds a comparison is the sigmoid score against score_threshold: `assert_margin` (called
by `run`) requires that no float64 score of a case lies within 1e-4 of the threshold used.
"""
import math

import numpy as np
import torch

from center_targets_cases import BAR, NUSC_TASKS, bits  # noqa: F401

F = np.float32
# 102.4 m x 102.4 m at 0.2 m voxels and stride 8: a 64 x 64 map
NUSC = dict(pc_range=[-51.2, -51.2], voxel_size=[0.2, 0.2], out_size_factor=8)
NUSC_GRID = (64, 64)      # (W, H)
NUSC_RANGE = [-45.0, -45.0, -4.0, 45.0, 45.0, 2.0]
# powers of two: x == xs + off_x and y == ys + off_y exactly, so a test can place a centre ON a face of the range and a
# pair of centres at a squared distance that EQUALS a threshold
UNIT = dict(pc_range=[0.0, 0.0], voxel_size=[0.5, 0.5], out_size_factor=2)
UNIT_GRID = (32, 24)
MARGIN = 1e-4


def _np(t):
    return t.detach().cpu().float().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def definition(peaks, feats, tasks, *, pc_range, voxel_size, out_size_factor, score_threshold=None, post_center_range=None,
               scores_are_logits=False, norm_bbox=True, nms_threshold=None, post_max_size=None, bottom_center=False):
    """peaks: per task (scores, indices, classes); feats: per task a sequence of maps -> per task a dict of numpy arrays
    [B, M, ...]: labels, source, sizes, `exact` (float32 boxes; the inexact channels hold 0 there) and `approx` (float64,
    those channels only), `approx_channels`, and the scores as `score_exact` (float32) or `score_approx` (float64)."""
    T = len(tasks)
    nms = list(nms_threshold) if isinstance(nms_threshold, (list, tuple)) else [nms_threshold] * T
    pc0, pc1, vs0, vs1, f = F(pc_range[0]), F(pc_range[1]), F(voxel_size[0]), F(voxel_size[1]), F(out_size_factor)
    thr = None if score_threshold is None else F(score_threshold)
    rng = None if post_center_range is None else [F(v) for v in post_center_range]
    out = []
    with np.errstate(all="ignore"):
        for t, ids in enumerate(tasks):
            scores = _np(peaks[t][0]).astype(np.float32)
            indices, classes = peaks[t][1].cpu().numpy(), peaks[t][2].cpu().numpy()
            maps = np.concatenate([_np(m) for m in feats[t]], 1).astype(np.float32)
            B, K = scores.shape
            _, C, H, W = maps.shape
            M = K if post_max_size is None else min(K, post_max_size)
            approx_channels = [6] + ([3, 4, 5] if norm_bbox else []) + ([2] if norm_bbox and bottom_center else [])
            r = dict(labels=np.zeros((B, M), np.int64), source=np.full((B, M), -1, np.int32), sizes=np.zeros((B,), np.int64),
                     exact=np.zeros((B, M, C - 1), np.float32), approx=np.zeros((B, M, C - 1), np.float64),
                     score_exact=np.zeros((B, M), np.float32), score_approx=np.zeros((B, M), np.float64),
                     approx_channels=sorted(approx_channels), logits=scores_are_logits, all_scores=[])
            nthr = None if nms[t] is None else F(nms[t])
            for b in range(B):
                kx, ky, kept = np.zeros(K, np.float32), np.zeros(K, np.float32), 0
                for k in range(K):
                    if kept >= M:
                        break
                    idx, pos = int(indices[b, k]), int(classes[b, k])
                    if not (0 <= idx < H * W and 0 <= pos < len(ids)):
                        continue
                    ys, xs = idx // W, idx % W
                    g = maps[b, :, ys, xs]
                    x = ((F(xs) + g[0]) * f) * vs0 + pc0
                    y = ((F(ys) + g[1]) * f) * vs1 + pc1
                    z = g[2]
                    s = scores[b, k]
                    s64 = 1.0 / (1.0 + np.exp(-np.float64(s))) if scores_are_logits else np.float64(s)
                    r["all_scores"].append(float(s64))
                    if thr is not None and not ((s64 if scores_are_logits else s) > thr):
                        continue
                    if rng is not None and not (rng[0] <= x <= rng[3] and rng[1] <= y <= rng[4] and rng[2] <= z <= rng[5]):
                        continue
                    if nthr is not None and kept:
                        dx, dy = x - kx[:kept], y - ky[:kept]
                        if bool((dx * dx + dy * dy <= nthr).any()):
                            continue
                    kx[kept], ky[kept] = x, y
                    e, a = r["exact"][b, kept], r["approx"][b, kept]
                    e[0], e[1] = x, y
                    if norm_bbox:
                        a[3:6] = np.exp(g[3:6].astype(np.float64))
                    else:
                        e[3:6] = g[3:6]
                    if not bottom_center:
                        e[2] = z
                    elif norm_bbox:
                        a[2] = np.float64(z) - a[5] * 0.5
                    else:
                        e[2] = z - g[5] * F(0.5)
                    a[6] = np.arctan2(np.float64(g[6]), np.float64(g[7]))
                    if C == 10:
                        e[7:9] = g[8:10]
                    if scores_are_logits:
                        r["score_approx"][b, kept] = s64
                    else:
                        r["score_exact"][b, kept] = s
                    r["labels"][b, kept] = ids[pos]
                    r["source"][b, kept] = k
                    kept += 1
                r["sizes"][b] = kept
            out.append(r)
    return out


def assert_margin(want, score_threshold):
    """no float64 score that was compared lies within MARGIN of the threshold (sigmoid scores are inexact)"""
    if score_threshold is None:
        return
    for w in want:
        if w["logits"] and w["all_scores"]:
            gap = np.abs(np.asarray(w["all_scores"]) - score_threshold).min()
            assert gap > MARGIN, f"a score lies {gap:.2e} from the threshold: regenerate the case with another seed"


def _close(g, a, tag, name):
    g, a = np.asarray(g, np.float64), np.asarray(a, np.float64)
    same = (np.isnan(g) & np.isnan(a)) | (g == a)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(g - a))
    err = np.where(np.isnan(err), np.inf, err)
    assert err.size == 0 or err.max() <= BAR, f"{tag}: {name} off by {err.max():.3e} (bar {BAR})"


def _same_bits_or_nan(g, a, tag, name):
    ok = (bits(g) == bits(a)) | (np.isnan(g) & np.isnan(a))
    assert ok.all(), f"{tag}: {name} differs at {np.argwhere(~ok)[:5].tolist()}"


def check(result, want, what=""):
    """the acceptance of the module docstring: `result` is the operator's list, `want` the definition's"""
    assert len(result) == len(want), what
    for t, (r, w) in enumerate(zip(result, want)):
        tag = f"{what} task {t}"
        sizes = r.boxes.sample_sizes
        for name in ("scores", "labels", "source"):
            assert getattr(r, name).sample_sizes is sizes, f"{tag}: {name} does not share the sample sizes"
        assert sizes.dtype == torch.int64 and np.array_equal(sizes.cpu().numpy(), w["sizes"]), \
            f"{tag}: sizes {sizes.cpu().tolist()} vs {w['sizes'].tolist()}"
        for name, dtype in (("labels", torch.int64), ("source", torch.int32)):
            got = getattr(r, name).tensor
            assert got.dtype == dtype and got.is_contiguous(), f"{tag}: {name} is {got.dtype}, contiguous {got.is_contiguous()}"
            got = got.cpu().numpy()
            assert got.shape == w[name].shape, f"{tag}: {name} has shape {got.shape}, wanted {w[name].shape}"
            assert np.array_equal(got, w[name]), f"{tag}: {name} differs at {np.argwhere(got != w[name])[:5].tolist()}"
        got, sc = r.boxes.tensor, r.scores.tensor
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == w["exact"].shape, tag
        assert sc.dtype == torch.float32 and sc.is_contiguous() and tuple(sc.shape) == w["score_exact"].shape, tag
        got, sc = got.cpu().numpy(), sc.cpu().numpy()
        approx = w["approx_channels"]
        computed = [c for c in (0, 1, 2) if c not in approx]
        copied = [c for c in range(3, got.shape[-1]) if c not in approx]
        _same_bits_or_nan(got[..., computed], w["exact"][..., computed], tag, "x / y / z")
        assert np.array_equal(bits(got[..., copied]), bits(w["exact"][..., copied])), f"{tag}: a copied channel differs"
        M = got.shape[1]
        pad = np.arange(M)[None, :] >= w["sizes"][:, None]
        assert not bits(got[pad]).any() and not bits(sc[pad]).any(), f"{tag}: a padding slot is not +0"
        _close(got[..., approx], w["approx"][..., approx], tag, "yaw / exp dims / bottom z")
        if w["logits"]:
            _close(sc, w["score_approx"], tag, "sigmoid scores")
        else:
            assert np.array_equal(bits(sc), bits(w["score_exact"])), f"{tag}: a raw score differs"


def check_device_against_host(dev, host, approx_channels, logits, what=""):
    """the same split between two results of the operator: integers and exact channels equal, the rest within the bar"""
    for t, (d, h) in enumerate(zip(dev, host)):
        tag = f"{what} task {t}"
        assert torch.equal(d.boxes.sample_sizes.cpu(), h.boxes.sample_sizes.cpu()), tag
        for name in ("labels", "source"):
            assert torch.equal(getattr(d, name).tensor.cpu(), getattr(h, name).tensor.cpu()), f"{tag}: {name}"
        g, a = d.boxes.tensor.cpu().numpy(), h.boxes.tensor.cpu().numpy()
        exact = [c for c in range(g.shape[-1]) if c not in approx_channels]
        _same_bits_or_nan(g[..., exact], a[..., exact], tag, "an exact channel")
        _close(g[..., approx_channels], a[..., approx_channels], tag, "yaw / exp dims / bottom z")
        gs, hs = d.scores.tensor.cpu().numpy(), h.scores.tensor.cpu().numpy()
        if logits:
            _close(gs, hs, tag, "sigmoid scores")
        else:
            assert np.array_equal(bits(gs), bits(hs)), f"{tag}: a raw score differs"


class Case:
    """peaks [T] of (scores, indices, classes) and feats [T] of map tuples, on one device"""

    def __init__(self, peaks, feats, tasks):
        self.peaks, self.feats, self.tasks = peaks, feats, tasks

    def to(self, device):
        return Case([tuple(x.to(device) for x in p) for p in self.peaks], [tuple(m.to(device) for m in f) for f in self.feats],
                    self.tasks)

    def clone(self):
        return Case([tuple(x.clone() for x in p) for p in self.peaks], [tuple(m.clone() for m in f) for f in self.feats], self.tasks)

    def copy_(self, other):
        for mine, theirs in zip(self.peaks + self.feats, other.peaks + other.feats):
            for a, b in zip(mine, theirs):
                a.copy_(b)

    def op_args(self):
        from accvlab.draw_heatmap import HeatmapPeaks

        peaks = [HeatmapPeaks(s, i, c, i, i) for s, i, c in self.peaks]      # ys and xs are not read
        return peaks, [list(f) for f in self.feats], self.tasks


SPLITS = {8: [(8,), (2, 1, 3, 2), (2, 6), (1, 1, 1, 3, 2), (3, 5)], 10: [(10,), (2, 1, 3, 2, 2), (2, 1, 5, 2), (4, 6), (2, 1, 3, 4)]}


def make_case(B, K, tasks=NUSC_TASKS, C=10, grid=NUSC_GRID, dtype=torch.float32, score_dtype=None, seed=0, logits=False,
              illegal=0.03, splits=None, device="cpu"):
    """Random peaks and maps.  Scores descend per frame (in (0, 1), or logits in (-4, 4)); indices are random cells (repeats
    included: identical centres); classes are positions inside the task; a fraction `illegal` of the peaks gets an index of
    -1 / H * W / 2^40 or a class position of -1 / len(task).  Maps: offsets in [0, 1), z in [-5, 3], d in [-1.6, 3], sin and
    cos of a random angle scaled by a random length, velocity in [-10, 10]; task t is split into maps by SPLITS (one to
    five maps)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    W, H = grid
    peaks, feats = [], []
    for t, ids in enumerate(tasks):
        s = u(B, K).sort(1, descending=True).values
        s = (s * 8 - 4) if logits else s
        idx = torch.randint(0, H * W, (B, K), generator=g)
        cls = torch.randint(0, len(ids), (B, K), generator=g)
        bad = u(B, K)
        for n, v in enumerate((-1, H * W, 2 ** 40)):
            idx[(bad >= n * illegal / 5) & (bad < (n + 1) * illegal / 5)] = v
        cls[(bad >= 3 * illegal / 5) & (bad < 4 * illegal / 5)] = -1
        cls[(bad >= 4 * illegal / 5) & (bad < illegal)] = len(ids)
        ang, length = (u(B, 1, H, W) * 2 - 1) * math.pi, 0.5 + u(B, 1, H, W)
        full = torch.cat([u(B, 2, H, W), u(B, 1, H, W) * 8 - 5, u(B, 3, H, W) * 4.6 - 1.6, length * ang.sin(), length * ang.cos(),
                          u(B, 2, H, W) * 20 - 10], 1)[:, :C]
        split = (splits or SPLITS[C])[t % len(splits or SPLITS[C])]
        assert sum(split) == C
        feats.append(tuple(m.to(dtype).contiguous().to(device) for m in full.split(list(split), 1)))
        peaks.append((s.to(score_dtype or dtype).contiguous().to(device), idx.to(device), cls.to(device)))
    return Case(peaks, feats, tasks)


def run(op, case, cfg, **kw):
    """the operator and the definition on the same inputs: (result, want)"""
    got = op(*case.op_args(), **cfg, **kw)
    want = definition(case.peaks, case.feats, case.tasks, **cfg, **kw)
    assert_margin(want, kw.get("score_threshold"))
    return got, want


# ------------------------------------------------------------------------------------------------------- placed centres
def split_cell(v):
    """(cell, offset) with float32(cell) + offset == v exactly, for a float32 v >= 0"""
    v = F(v)
    cell = int(math.floor(float(v)))
    off = F(v - F(cell))
    assert F(cell) + off == v and 0 <= off < 1
    return cell, off


def placed_case(K, placed, grid=UNIT_GRID, tasks=((0,),), C=8, scores=None, device="cpu"):
    """One frame, one map per task, on the UNIT geometry, where x = xs + off_x and y = ys + off_y exactly.  `placed` maps a
    rank to (x, y) or (x, y, z): that peak sits in a cell of its own with the offsets that put its centre there.  Every
    other rank is a filler on the integer corner of a cell of its own (offset 0, z 0), at least one cell away from every
    other filler and more than two cells away from every placed centre.  Scores descend from 0.9 unless given.  The same peaks and maps go to
    every task."""
    W, H = grid
    maps = torch.zeros((1, C, H, W), dtype=torch.float32)
    maps[0, 7] = 1.0
    idx = torch.zeros((1, K), dtype=torch.int64)
    taken = set()
    for k, p in placed.items():
        (xs, ox), (ys, oy) = split_cell(p[0]), split_cell(p[1])
        assert xs < W and ys < H
        cell = ys * W + xs
        if cell in taken:      # several placed peaks in one cell must agree on what the cell holds
            assert maps[0, 0, ys, xs].item() == float(ox) and maps[0, 1, ys, xs].item() == float(oy)
        taken.add(cell)
        maps[0, 0, ys, xs], maps[0, 1, ys, xs] = float(ox), float(oy)
        maps[0, 2, ys, xs] = p[2] if len(p) > 2 else 0.0
        idx[0, k] = cell
    far = lambda c: all((c % W - p[0]) ** 2 + (c // W - p[1]) ** 2 > 4.0 for p in placed.values())   # noqa: E731
    free = [c for c in range(H * W) if c not in taken and far(c)]
    assert len(free) >= K
    n = 0
    for k in range(K):
        if k not in placed:
            idx[0, k] = free[(n * 7) % len(free)] if math.gcd(7, len(free)) == 1 else free[n]
            n += 1
    s = torch.linspace(0.9, 0.2, K)[None] if scores is None else torch.as_tensor(scores, dtype=torch.float32)[None]
    cls = torch.zeros((1, K), dtype=torch.int64)
    peaks = [(s.clone().to(device), idx.clone().to(device), cls.clone().to(device)) for _ in tasks]
    feats = [(maps.clone().to(device),) for _ in tasks]
    return Case(peaks, feats, tasks)


def kept_ranks(result, t=0, b=0):
    n = int(result[t].source.sample_sizes[b])
    return result[t].source.tensor[b, :n].tolist()
