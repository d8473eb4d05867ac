"""What `query_box_decode_3d` / `query_box_decode_2d` are measured against, and the inputs of their CPU and GPU tests.

`definition_3d` and `definition_2d` restate the operators as the per-rank Python loop they replace (mmdet3d's
NMSFreeCoder.decode with denormalize_bbox, mmdet's DETRHead._predict_by_feat_single; neither is imported) in numpy float32
SCALARS, one correctly rounded operation per operator, parenthesised exactly as the comment of csrc/query_decode_arith.h has
it.  exp, atan2 and the sigmoid are taken in float64 of the float32 inputs.  The selection is np.argsort(kind="stable") on
the order-preserving key of the raw value (NaN above +inf, -0.0 == +0.0), which is torch.sort(descending=True, stable=True).

Acceptance (`check`), the split of center_decode_cases.py:
  * sample_sizes, labels and source, padding slots included: bit-equal, no case excused.
  * cx, cy, cz, the velocity, raw scores and all 2D coordinates: bit-equal (a NaN computed from a NaN input must meet a
    NaN); padding rows +0 bit for bit.
  * exp sizes, yaw, sigmoid scores and z under bottom_center: within BAR = 1e-5 absolute, the project's float32 bar
    (center_targets_cases.py).  The inputs keep the log-sizes in [-1.6, 3]: exp <= 20.1, where one float32 ulp is 1.9e-6;
    |yaw| <= pi (ulp 2.4e-7), scores <= 1 (ulp 6e-8), |z| <= 6 + 10.05 (ulp 9.5e-7): the bar is at least 5 ulp of every value
    compared; NaN must meet NaN and an infinity the same infinity.

The only inexact quantity that feeds a decision is the sigmoid score against score_threshold: `assert_margin` (called by
`run`) requires that no float64 score of a case lies within MARGIN = 1e-4 of the threshold used; `make_case` moves every
logit that would out of that band, so the definition alone satisfies it.
"""
import math

import numpy as np
import torch

from box_decode_cases import _frame_hw, _to_source
from center_decode_cases import MARGIN, _close, _same_bits_or_nan
from center_targets_cases import BAR, bits  # noqa: F401

F = np.float32
RANGE = [-48.0, -48.0, -4.0, 48.0, 48.0, 2.0]      # every face is a float16 / bfloat16 value too
THR = 0.3                                          # the score threshold of the cases that use one
HW = (96, 160)


def _np32(t):
    """float32 numpy values of a tensor, f16 / bf16 widened exactly.  float16 goes through numpy: torch's CPU cast turns every
    float16 NaN into 0x7FFFFFFF, while the operators (csrc/accv_numeric.h) and numpy keep its sign and payload, and a raw
    score is a copy of the value"""
    t = t.detach().cpu()
    if t.dtype == torch.float16:
        return t.contiguous().view(torch.int16).numpy().view(np.float16).astype(np.float32)
    return t.float().numpy()


def order_key(x):
    """uint32 keys of float32 values: larger = earlier; every NaN on top, -0.0 folded onto +0.0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = 0xFFFFFFFF
    return key


def select(x, k):
    """flat indices of the k first of torch.sort(x, descending=True, stable=True)"""
    return np.argsort(~order_key(x), kind="stable")[:k]


def _sigmoid64(s):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.float64(s)))


def _empty(B, M, W):
    return dict(labels=np.zeros((B, M), np.int64), source=np.full((B, M), -1, np.int32), sizes=np.zeros((B,), np.int64),
                exact=np.zeros((B, M, W), np.float32), approx=np.zeros((B, M, W), np.float64),
                score_exact=np.zeros((B, M), np.float32), score_approx=np.zeros((B, M), np.float64), all_scores=[])


def _score(r, s, logits, thr):
    """(float64 score or None, passes the threshold)"""
    s64 = _sigmoid64(s) if logits else None
    r["all_scores"].append(float(s64 if logits else s))
    return s64, thr is None or bool((s64 if logits else s) > thr)


def _put(r, b, slot, s, s64, q, label):
    if s64 is None:
        r["score_exact"][b, slot] = s
    else:
        r["score_approx"][b, slot] = s64
    r["labels"][b, slot], r["source"][b, slot] = label, q


def definition_3d(cls_scores, bbox_preds, max_num, *, score_threshold=None, post_center_range=None, scores_are_logits=True,
                  bottom_center=False):
    cls, rows = _np32(cls_scores), _np32(bbox_preds)
    B, Q, C = cls.shape
    D = rows.shape[2]
    thr = None if score_threshold is None else F(score_threshold)
    rng = None if post_center_range is None else [F(v) for v in post_center_range]
    r = _empty(B, max_num, D - 1)
    r.update(approx_channels=sorted([3, 4, 5, 6] + ([2] if bottom_center else [])), logits=scores_are_logits)
    with np.errstate(all="ignore"):
        for b in range(B):
            flat = cls[b].reshape(-1)
            kept = 0
            for idx in select(flat, max_num):
                q, label = int(idx) // C, int(idx) % C
                p = rows[b, q]
                cx, cy, cz = p[0], p[1], p[4]
                s64, ok = _score(r, flat[idx], scores_are_logits, thr)
                if not ok:
                    continue
                if rng is not None and not (rng[0] <= cx <= rng[3] and rng[1] <= cy <= rng[4] and rng[2] <= cz <= rng[5]):
                    continue
                e, a = r["exact"][b, kept], r["approx"][b, kept]
                e[0], e[1] = cx, cy
                a[3:6] = np.exp(np.float64(p[2])), np.exp(np.float64(p[3])), np.exp(np.float64(p[5]))
                if bottom_center:
                    a[2] = np.float64(cz) - a[5] * 0.5
                else:
                    e[2] = cz
                a[6] = np.arctan2(np.float64(p[6]), np.float64(p[7]))
                if D == 10:
                    e[7:9] = p[8:10]
                _put(r, b, kept, flat[idx], s64, q, label)
                kept += 1
            r["sizes"][b] = kept
    return r


def definition_2d(cls_scores, bbox_preds, max_num, *, image_hw, image_matrices=None, score_threshold=None, scores_are_logits=True,
                  box_format="cxcywh", normalized=True, clip=True, order_corners=True):
    cls, rows = _np32(cls_scores), _np32(bbox_preds)
    B, Q, C = cls.shape
    thr = None if score_threshold is None else F(score_threshold)
    mats = None if image_matrices is None else image_matrices.detach().cpu().numpy()
    r = _empty(B, max_num, 4)
    r.update(approx_channels=[], logits=scores_are_logits)
    crop = lambda v, E: F(0) if v < 0 else (E if v > E else v)   # noqa: E731
    with np.errstate(all="ignore"):
        for b in range(B):
            Hi, Wi = _frame_hw(image_hw, b)
            EW, EH = F(Wi), F(Hi)
            flat = cls[b].reshape(-1)
            kept = 0
            for idx in select(flat, max_num):
                q, label = int(idx) // C, int(idx) % C
                p = rows[b, q]
                x1, y1, x2, y2 = p[0], p[1], p[2], p[3]
                if box_format == "cxcywh":
                    hw, hh = F(0.5) * p[2], F(0.5) * p[3]
                    x1, y1, x2, y2 = p[0] - hw, p[1] - hh, p[0] + hw, p[1] + hh
                if normalized:
                    x1, y1, x2, y2 = x1 * EW, y1 * EH, x2 * EW, y2 * EH
                if clip:
                    x1, y1, x2, y2 = crop(x1, EW), crop(y1, EH), crop(x2, EW), crop(y2, EH)
                s64, ok = _score(r, flat[idx], scores_are_logits, thr)
                if not (ok and all(bool(np.isfinite(v)) for v in (x1, y1, x2, y2))):
                    continue
                if mats is not None:
                    x1, y1, x2, y2 = _to_source(mats[b], order_corners, x1, y1, x2, y2)
                r["exact"][b, kept] = (x1, y1, x2, y2)
                _put(r, b, kept, flat[idx], s64, q, label)
                kept += 1
            r["sizes"][b] = kept
    return r


def assert_margin(want, score_threshold):
    """no float64 sigmoid score that was compared lies within MARGIN of the threshold"""
    if score_threshold is None or not want["logits"] or not want["all_scores"]:
        return
    s = np.asarray(want["all_scores"])
    gap = np.abs(s[~np.isnan(s)] - score_threshold).min(initial=np.inf)
    assert gap > MARGIN, f"a score lies {gap:.2e} from the threshold: the case generator is wrong"


def check(result, want, what=""):
    """the acceptance of the module docstring: `result` is the operator's named tuple, `want` the definition's dict"""
    sizes = result.boxes.sample_sizes
    for name, member in zip(result._fields, result):
        assert member.sample_sizes is sizes, f"{what}: {name} does not share the sample sizes"
    assert sizes.dtype == torch.int64 and np.array_equal(sizes.cpu().numpy(), want["sizes"]), \
        f"{what}: sizes {sizes.cpu().tolist()} vs {want['sizes'].tolist()}"
    for name, dtype in (("labels", torch.int64), ("source", torch.int32)):
        got = getattr(result, name).tensor
        assert got.dtype == dtype and got.is_contiguous(), f"{what}: {name} is {got.dtype}"
        got = got.cpu().numpy()
        assert got.shape == want[name].shape, f"{what}: {name} has shape {got.shape}, wanted {want[name].shape}"
        assert np.array_equal(got, want[name]), f"{what}: {name} differs at {np.argwhere(got != want[name])[:5].tolist()}"
    got, sc = result.boxes.tensor, result.scores.tensor
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want["exact"].shape, what
    assert sc.dtype == torch.float32 and sc.is_contiguous() and tuple(sc.shape) == want["score_exact"].shape, what
    if hasattr(result, "extras"):
        ex = result.extras.tensor
        assert ex.dtype == torch.float32 and tuple(ex.shape) == tuple(got.shape[:2]) + (0,), f"{what}: extras is {tuple(ex.shape)}"
    got, sc = got.cpu().numpy(), sc.cpu().numpy()
    approx = want["approx_channels"]
    exact = [c for c in range(got.shape[-1]) if c not in approx]
    _same_bits_or_nan(got[..., exact], want["exact"][..., exact], what, "an exact channel")
    pad = np.arange(got.shape[1])[None, :] >= want["sizes"][:, None]
    assert not bits(got[pad]).any() and not bits(sc[pad]).any(), f"{what}: a padding slot is not +0"
    _close(got[..., approx], want["approx"][..., approx], what, "exp sizes / yaw / bottom z")
    if want["logits"]:
        _close(sc, want["score_approx"], what, "sigmoid scores")
    else:
        assert np.array_equal(bits(sc), bits(want["score_exact"])), f"{what}: a raw score differs"


def check_device_against_host(dev, host, approx_channels, logits, what=""):
    """integers and exact channels equal, exp / atan2 / sigmoid within the bar"""
    assert torch.equal(dev.boxes.sample_sizes.cpu(), host.boxes.sample_sizes.cpu()), what
    for name in ("labels", "source"):
        assert torch.equal(getattr(dev, name).tensor.cpu(), getattr(host, name).tensor.cpu()), f"{what}: {name}"
    g, a = dev.boxes.tensor.cpu().numpy(), host.boxes.tensor.cpu().numpy()
    exact = [c for c in range(g.shape[-1]) if c not in approx_channels]
    _same_bits_or_nan(g[..., exact], a[..., exact], what, "an exact channel")
    _close(g[..., approx_channels], a[..., approx_channels], what, "exp sizes / yaw / bottom z")
    gs, hs = dev.scores.tensor.cpu().numpy(), host.scores.tensor.cpu().numpy()
    if logits:
        _close(gs, hs, what, "sigmoid scores")
    else:
        assert np.array_equal(bits(gs), bits(hs)), f"{what}: a raw score differs"


# ------------------------------------------------------------------------------------------------------------- inputs
KINDS = ("distinct", "equal", "two", "special", "saturated")


def _avoid_threshold(x):
    """move every logit whose float64 sigmoid (of the value as stored) lies within 2 * MARGIN of THR"""
    near = (torch.sigmoid(x.double()) - THR).abs() <= 2 * MARGIN
    return torch.where(near, x + 0.01 * x.abs().clamp(min=1.0), x)


def logits(B, Q, C, kind="distinct", dtype=torch.float32, seed=0):
    """[B, Q, C] raw class logits:
    distinct   a random permutation of distinct values in (-7, 3) (ties remain after a cast to float16 / bfloat16)
    equal      one value everywhere: the select descends into the index bits
    two        two values at random: with k between the two counts the cut falls inside a tie group
    special    distinct, with NaN, +-inf and +-0.0 sprinkled over every frame
    saturated  distinct, with a block of distinct logits in [20, 40]: float32 sigmoid gives 1.0 for all of them"""
    g = torch.Generator().manual_seed(seed)
    N = Q * C
    if kind == "equal":
        x = torch.full((B, N), -1.25)
    elif kind == "two":
        x = torch.where(torch.rand(B, N, generator=g) < 0.4, 0.75, -0.5)
    else:
        base = torch.linspace(-7.0, 3.0, N + 2)[1:-1]
        x = torch.stack([base[torch.randperm(N, generator=g)] for _ in range(B)])
        if kind == "special":
            vals = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, float("nan"), 0.0, -0.0]
            for b in range(B):
                at = torch.randperm(N, generator=g)[: len(vals)]
                for i, v in zip(at.tolist(), vals):
                    x[b, i] = v
        if kind == "saturated":
            n = min(N, 24)
            for b in range(B):
                at = torch.randperm(N, generator=g)[:n]
                x[b, at] = torch.linspace(20.0, 40.0, n)[torch.randperm(n, generator=g)]
    x = _avoid_threshold(x.to(dtype))
    return x.view(B, Q, C).contiguous()


def rows_3d(B, Q, D=10, dtype=torch.float32, seed=0, special=False):
    """centres in [-60, 60]^2 x [-6, 4] (a share outside RANGE), log-sizes in [-1.6, 3], (sin, cos) of a random angle scaled by
    a random length, velocity in [-10, 10]; `special` puts NaN and +-inf into every column of some rows"""
    g = torch.Generator().manual_seed(seed + 1000)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    ang, length = (u(B, Q) * 2 - 1) * math.pi, 0.5 + u(B, Q)
    full = torch.stack([u(B, Q) * 120 - 60, u(B, Q) * 120 - 60, u(B, Q) * 4.6 - 1.6, u(B, Q) * 4.6 - 1.6, u(B, Q) * 10 - 6,
                        u(B, Q) * 4.6 - 1.6, length * ang.sin(), length * ang.cos(), u(B, Q) * 20 - 10, u(B, Q) * 20 - 10], 2)[..., :D]
    if special:
        n = 0
        for c in range(D):
            for v in (float("nan"), float("inf"), float("-inf")):
                full[n % B, (7 * n + 1) % Q, c] = v
                n += 1
    return full.to(dtype).contiguous()


def rows_2d(B, Q, box_format="cxcywh", normalized=True, dtype=torch.float32, seed=0, special=False):
    """boxes that partly leave the image: centres in [-0.1, 1.1], sizes in [0, 0.5] of it"""
    g = torch.Generator().manual_seed(seed + 2000)
    c = torch.rand(B, Q, 2, generator=g) * 1.2 - 0.1
    s = torch.rand(B, Q, 2, generator=g) * 0.5
    full = torch.cat([c, s], 2) if box_format == "cxcywh" else torch.cat([c - s / 2, c + s / 2], 2)
    if not normalized:
        full = full * torch.tensor([HW[1], HW[0], HW[1], HW[0]], dtype=torch.float32)
    if special:
        n = 0
        for col in range(4):
            for v in (float("nan"), float("inf"), float("-inf")):
                full[n % B, (5 * n + 2) % Q, col] = v
                n += 1
    return full.to(dtype).contiguous()


def matrices(B, seed=0, singular=()):
    """flip + scale + crop per frame: [[+-s, 0, tx], [0, t, ty]], and the frames of `singular` with a zero row"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros((B, 2, 3))
    for f in range(B):
        s, t = (0.4 + 0.9 * torch.rand(2, generator=g)).tolist()
        flip = f % 2 == 1
        m[f] = torch.tensor([[-s if flip else s, 0.0, (150.0 if flip else -13.5)], [0.0, t, -7.25 * f]])
        if f in singular:
            m[f, 1, :2] = 0.0
    return m


def run(op, definition, cls, rows, max_num, **kw):
    """the operator and its definition on the same inputs: (result, want)"""
    got = op(cls, rows, max_num, **kw)
    host = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    want = definition(cls, rows, max_num, **host)
    assert_margin(want, kw.get("score_threshold"))
    return got, want


def check_raw_half_nan(op3, op2, dev):
    """raw scores (scores_are_logits=False) of float16 / bfloat16 logits with NaNs of several signs and payloads, all of which
    rank first: the score is the value widened exactly, a NaN with its sign and payload.  (The sweeps of DESIGN §9zg found
    that `_np32` widened through torch's CPU cast, which gives 0x7FFFFFFF for every float16 NaN.)  Quiet NaNs only: a
    conversion instruction may quiet a signalling one."""
    B, Q, C = 2, 40, 3
    for dtype, quiet, widened in ((torch.float16, [0x7E00, 0x7E12, 0xFE01], [0x7FC00000, 0x7FC24000, 0xFFC02000]),
                                  (torch.bfloat16, [0x7FC0, 0x7FC1, 0xFFC3], [0x7FC00000, 0x7FC10000, 0xFFC30000])):
        cls = logits(B, Q, C, "distinct", dtype=dtype, seed=5)
        words = cls.view(torch.int16).view(B, -1)
        at = [7, 50, 119]
        words[:, at] = torch.tensor(quiet, dtype=torch.int32).to(torch.int16)
        cls = cls.to(dev)
        for M in (2, Q * C):
            got, want = run(op3, definition_3d, cls, rows_3d(B, Q, 10, seed=5).to(dev), M, scores_are_logits=False)
            check(got, want, f"3d raw {dtype} M={M}")
            assert want["score_exact"].view(np.uint32)[0, :min(M, 3)].tolist() == widened[:min(M, 3)], "the case holds no NaN payload"
            assert got.source.tensor[0, :min(M, 3)].tolist() == [a // C for a in at][:min(M, 3)]
            got, want = run(op2, definition_2d, cls, rows_2d(B, Q, seed=5).to(dev), M, image_hw=HW, scores_are_logits=False)
            check(got, want, f"2d raw {dtype} M={M}")


def max_nums(N, limit=1024):
    return sorted({m for m in (1, 2, 63, 64, 65, N, 1024) if m <= min(N, limit)})
