"""What `center_point_targets` is measured against, and the inputs of its CPU and GPU tests.

`definition` restates the operator as the per-object Python loop it replaces (mmdet3d's CenterHead.get_targets_single) in
numpy float32 SCALARS, one correctly rounded operation per operator, parenthesised exactly as the comment of
csrc/center_targets_arith.h has it.  log / sin / cos are taken in float64 of the float32 inputs.

Acceptance (`check`):
  * centers, radii, labels, indices, source and sample_sizes, padding slots included: bit-equal, no case excused.
  * offset, z, raw-dims and velocity channels: bit-equal.  log / sin / cos channels: within 1e-5 absolute, the project's
    float32 bar.  The inputs keep dims in [0.2, 20] (|log| <= 3, one float32 ulp there is 2.4e-7) and yaw in [-2 pi, 2 pi]
    (|sin|, |cos| <= 1, ulp 6e-8): the bar is more than 20 ulp of every value compared; NaN must meet NaN and an infinity
    the same infinity.
  * padding rows of the targets: +0 bit for bit in every channel.
"""
import math

import numpy as np
import torch

F = np.float32
BAR = 1e-5
NUSC_TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))      # the six nuScenes tasks of CenterPoint over ten classes
# 102.4 m x 102.4 m at 0.2 m voxels and stride 8: a 64 x 64 map
NUSC = dict(pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0], out_size_factor=8, grid_size=(64, 64))
# powers of two: cx == x and cy == y exactly, so a test can place a centre ON a boundary of the validity rule
UNIT = dict(pc_range=[0.0, 0.0, -5.0, 32.0, 24.0, 3.0], voxel_size=[0.5, 0.5, 8.0], out_size_factor=2, grid_size=(32, 24))


def to_int(v):
    """(int) of a float32 as the arithmetic header defines it: truncation, NaN -> 0, saturating"""
    if v >= F(2147483648.0):
        return 2 ** 31 - 1
    if v <= F(-2147483648.0):
        return -2 ** 31
    return int(v) if v == v else 0


def gaussian_radius(w, l, m, sqrt=np.sqrt):
    """CenterPoint's gaussian_radius((l, w), m) in float32 scalars; `sqrt` lets a test put a WRONG root in (one that is off
    by an ulp) to show that its cases would notice"""
    omm, opm = F(1) - m, F(1) + m
    s = l + w
    c1 = ((w * l) * omm) / opm
    sq1 = sqrt(s * s - F(4) * c1)
    r1 = (s + sq1) / F(2)
    b2 = F(2) * s
    c2 = (omm * w) * l
    sq2 = sqrt(b2 * b2 - F(16) * c2)
    r2 = (b2 + sq2) / F(2)
    a3 = F(4) * m
    b3 = (F(-2) * m) * s
    c3 = ((m - F(1)) * w) * l
    sq3 = sqrt(b3 * b3 - (F(4) * a3) * c3)
    r3 = (b3 + sq3) / F(2)
    rm = r1
    if r2 < rm:
        rm = r2
    if r3 < rm:
        rm = r3
    return rm


def definition(boxes, labels, sizes, tasks, *, pc_range, voxel_size, out_size_factor, grid_size, gaussian_overlap=0.1,
               min_radius=2, max_objs=500, norm_bbox=True):
    """boxes [B, N, D] float32, labels [B, N], sizes [B] (numpy or torch) -> per task a dict of numpy arrays [B, M, ...]:
    the integer outputs, `exact` (float32 targets; the log / sin / cos channels hold 0 there) and `approx` (float64, those
    channels only, elsewhere 0), plus `approx_channels` and `sizes`."""
    boxes, labels, sizes = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (boxes, labels, sizes))
    assert boxes.dtype == np.float32
    B, N, D = boxes.shape
    C, M = D + 1, min(max_objs, N)
    W, H = grid_size
    pc0, pc1, vs0, vs1, f, m = F(pc_range[0]), F(pc_range[1]), F(voxel_size[0]), F(voxel_size[1]), F(out_size_factor), F(gaussian_overlap)
    Wf, Hf = F(W), F(H)
    approx_channels = ([3, 4, 5] if norm_bbox else []) + [6, 7]
    out = []
    with np.errstate(all="ignore"):
        for ids in tasks:
            r = dict(centers=np.zeros((B, M, 2), np.int32), radii=np.zeros((B, M), np.int32), labels=np.zeros((B, M), np.int32),
                     indices=np.zeros((B, M), np.int64), source=np.full((B, M), -1, np.int32), exact=np.zeros((B, M, C), np.float32),
                     approx=np.zeros((B, M, C), np.float64), sizes=np.zeros((B,), np.int64), approx_channels=approx_channels)
            for b in range(B):
                cands = kept = 0
                for n in range(max(0, min(int(sizes[b]), N))):
                    if int(labels[b, n]) not in ids:
                        continue
                    cands += 1
                    if cands > max_objs:                      # min(num_objs, max_objs), before the validity test
                        break
                    x, y, z, dx, dy, dz, yaw = (boxes[b, n, i] for i in range(7))
                    w = (dx / vs0) / f
                    l = (dy / vs1) / f
                    cx = ((x - pc0) / vs0) / f
                    cy = ((y - pc1) / vs1) / f
                    if not (w > 0 and l > 0 and cx > -1 and cx < Wf and cy > -1 and cy < Hf):
                        continue
                    ix, iy = int(cx), int(cy)                 # truncation toward zero
                    r["centers"][b, kept] = (ix, iy)
                    r["radii"][b, kept] = max(min_radius, to_int(gaussian_radius(w, l, m)))
                    r["labels"][b, kept] = ids.index(int(labels[b, n]))
                    r["indices"][b, kept] = iy * W + ix
                    r["source"][b, kept] = n
                    e, a = r["exact"][b, kept], r["approx"][b, kept]
                    e[0], e[1], e[2] = cx - F(ix), cy - F(iy), z
                    if norm_bbox:
                        a[3:6] = [math.log(float(v)) if v > 0 else (-math.inf if v == 0 else math.nan) for v in (dx, dy, dz)]
                    else:
                        e[3:6] = (dx, dy, dz)
                    yaw64 = float(yaw)
                    a[6], a[7] = (math.sin(yaw64), math.cos(yaw64)) if math.isfinite(yaw64) else (math.nan, math.nan)
                    if D == 9:
                        e[8:10] = boxes[b, n, 7:9]
                    kept += 1
                r["sizes"][b] = kept
            out.append(r)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(result, want, what=""):
    """the acceptance of the module docstring: `result` is the operator's list, `want` the definition's"""
    assert len(result) == len(want), what
    for t, (r, w) in enumerate(zip(result, want)):
        tag = f"{what} task {t}"
        sizes = r.centers.sample_sizes
        for name in ("radii", "labels", "targets", "indices", "source"):
            assert getattr(r, name).sample_sizes is sizes, f"{tag}: {name} does not share the sample sizes"
        assert sizes.dtype == torch.int64 and np.array_equal(sizes.cpu().numpy(), w["sizes"]), \
            f"{tag}: sizes {sizes.cpu().tolist()} vs {w['sizes'].tolist()}"
        for name, dtype in (("centers", torch.int32), ("radii", torch.int32), ("labels", torch.int32), ("indices", torch.int64),
                            ("source", torch.int32)):
            got = getattr(r, name).tensor
            assert got.dtype == dtype and got.is_contiguous(), f"{tag}: {name} is {got.dtype}, contiguous {got.is_contiguous()}"
            got = got.cpu().numpy()
            assert got.shape == w[name].shape, f"{tag}: {name} has shape {got.shape}, wanted {w[name].shape}"
            assert np.array_equal(got, w[name]), f"{tag}: {name} differs at {np.argwhere(got != w[name])[:5].tolist()}"
        got = r.targets.tensor
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == w["exact"].shape, tag
        got = got.cpu().numpy()
        approx = w["approx_channels"]
        exact = [c for c in range(got.shape[-1]) if c not in approx]
        assert np.array_equal(bits(got[..., exact]), bits(w["exact"][..., exact])), f"{tag}: an exact target channel differs"
        B, M = got.shape[:2]
        pad = np.arange(M)[None, :] >= w["sizes"][:, None]
        assert not bits(got[pad]).any(), f"{tag}: a padding row of the targets is not +0"
        g, a = got[..., approx].astype(np.float64), w["approx"][..., approx]
        same = (np.isnan(g) & np.isnan(a)) | (g == a)
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(g - a))
        err = np.where(np.isnan(err), np.inf, err)
        assert err.size == 0 or err.max() <= BAR, f"{tag}: log / sin / cos channels off by {err.max():.3e} (bar {BAR})"


def check_device_against_host(dev, host, approx_channels, what=""):
    """the same split between two results of the operator: integers and exact channels equal, the rest within the bar"""
    for t, (d, h) in enumerate(zip(dev, host)):
        tag = f"{what} task {t}"
        assert torch.equal(d.centers.sample_sizes.cpu(), h.centers.sample_sizes.cpu()), tag
        for name in ("centers", "radii", "labels", "indices", "source"):
            assert torch.equal(getattr(d, name).tensor.cpu(), getattr(h, name).tensor.cpu()), f"{tag}: {name}"
        g, a = d.targets.tensor.cpu().numpy(), h.targets.tensor.cpu().numpy()
        exact = [c for c in range(g.shape[-1]) if c not in approx_channels]
        assert np.array_equal(bits(g[..., exact]), bits(a[..., exact])), f"{tag}: an exact target channel differs"
        g, a = g[..., approx_channels].astype(np.float64), a[..., approx_channels].astype(np.float64)
        same = (np.isnan(g) & np.isnan(a)) | (g == a)
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(g - a))
        err = np.where(np.isnan(err), np.inf, err)
        assert err.size == 0 or err.max() <= BAR, f"{tag}: log / sin / cos channels off by {err.max():.3e} (bar {BAR})"


def ragged(tensor, sizes, size_dtype=None):
    """a RaggedBatch over `tensor`; a tensor of sizes keeps its dtype unless one is asked for"""
    from accvlab.batching_helpers import RaggedBatch

    if not isinstance(sizes, torch.Tensor):
        sizes = torch.tensor(sizes, dtype=size_dtype or torch.int64)
    elif size_dtype is not None:
        sizes = sizes.to(size_dtype)
    return RaggedBatch(tensor, sample_sizes=sizes.to(tensor.device))


def make_case(B, N, sizes, D=9, seed=0, cfg=NUSC, classes=10, label_dtype=torch.int64, size_dtype=torch.int64, device="cpu"):
    """(boxes RaggedBatch, labels RaggedBatch): centres spread over 1.25 x the range (about a third fall outside), dims in
    [0.2, 20], yaw in [-2 pi, 2 pi], labels in [-1, classes] with class 63 and a zero-size box sprinkled in; padding slots
    hold NaN boxes and label 0, which must reach nothing."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    lo = torch.tensor(cfg["pc_range"][:2])
    span = torch.tensor(cfg["pc_range"][3:5]) - lo
    xy = lo + span * (u(B, N, 2) * 1.25 - 0.125)
    z = u(B, N, 1) * 8 - 5
    dims = 0.2 + u(B, N, 3) * 19.8
    yaw = (u(B, N, 1) * 2 - 1) * (2 * math.pi)
    vel = u(B, N, 2) * 20 - 10
    boxes = torch.cat([xy, z, dims, yaw, vel], -1)[..., :D].to(torch.float32).contiguous()
    labels = torch.randint(-1, classes + 1, (B, N), generator=g)
    labels[u(B, N) < 0.03] = 63
    boxes[..., 3][u(B, N) < 0.03] = 0.0
    slot = torch.arange(N)[None, :]
    pad = slot >= torch.as_tensor(sizes)[:, None].clamp(max=N)
    boxes[pad] = float("nan")
    labels[pad] = 0
    return ragged(boxes.to(device), sizes, size_dtype), ragged(labels.to(label_dtype).to(device), sizes, size_dtype)


def run(op, boxes, labels, tasks, cfg, **kw):
    """the operator and the definition on the same inputs: (result, want)"""
    got = op(boxes, labels, tasks, **cfg, **kw)
    want = definition(boxes.tensor, labels.tensor if hasattr(labels, "tensor") else labels, boxes.sample_sizes, tasks, **cfg, **kw)
    return got, want


# ------------------------------------------------------------------------------------------------------------ edge list
INF, NAN = float("inf"), float("nan")


def edge_case(D=9, device="cpu", label_dtype=torch.int32, size_dtype=torch.int32):
    """One frame on the UNIT grid (W, H = 32, 24; cx == x, cy == y; w == dx, l == dy), every object of class 0.  Returns
    (boxes, labels, kept): `kept` lists the input slots that survive, by the validity rule worked out here by hand.
      x in {-1, W}                 dropped (cx > -1 and cx < W are strict)
      x in {-0.5, 0, W-1, W-0.5}   kept; -0.5 lands in cell 0, W-0.5 in cell W-1
      the same six values in y     likewise against H
      x or y NaN / +inf / -inf     dropped (NaN fails the comparisons, the infinities the range)
      dx NaN / -inf / 0 / negative dropped (w > 0 fails); dx = +inf passes w > 0 and is KEPT with radius min_radius: its
                                   roots are inf - inf = NaN, which converts to 0
      vx NaN / +inf / -inf         kept; reaches only its own target row"""
    W, H = UNIT["grid_size"]
    base = [5.0, 6.0, -1.0, 4.0, 2.0, 1.5, 0.3, 1.0, -2.0]
    rows, kept = [], []

    def add(keep, **kw):
        b = list(base)
        for k, v in kw.items():
            b["x y z dx dy dz yaw vx vy".split().index(k)] = v
        if keep:
            kept.append(len(rows))
        rows.append(b)

    for v, keep in ((-1.0, False), (-0.5, True), (0.0, True), (W - 1.0, True), (W - 0.5, True), (float(W), False)):
        add(keep, x=v)
    for v, keep in ((-1.0, False), (-0.5, True), (0.0, True), (H - 1.0, True), (H - 0.5, True), (float(H), False)):
        add(keep, y=v)
    for v in (NAN, INF, -INF):
        add(False, x=v)
        add(False, y=v)
    for v, keep in ((NAN, False), (-INF, False), (0.0, False), (-3.0, False), (INF, True)):
        add(keep, dx=v)
    for v in (NAN, INF, -INF):
        add(True, vx=v)
    add(True, z=NAN, dz=-1.0, yaw=INF)      # non-finite / unloggable values pass into their own row
    add(True)
    boxes = torch.tensor(rows, dtype=torch.float32)[None, :, :D].contiguous().to(device)
    labels = torch.zeros((1, len(rows)), dtype=label_dtype, device=device)
    n = len(rows)
    return ragged(boxes, [n], size_dtype), ragged(labels, [n], size_dtype), kept


# ------------------------------------------------------------------------------------------- radii on an integer boundary
RADIUS_CFG = dict(UNIT, gaussian_overlap=0.5, min_radius=1, max_objs=4096)


def radius_boundary_case(device="cpu"):
    """One frame on the UNIT grid (w == dx, l == dy) with gaussian_overlap = 0.5, where the smallest root is
    r3 = (-s + sqrt(s * s + 4 w l)) / 2, s = w + l, built so that r3 sits ON an integer or within a few float32 steps of it:
    there a square root that is off by one ulp changes (int)r3, which the random cases almost never show.
      * w = 2 k, l = 3 k: s * s + 4 w l = 49 k * k is a perfect square, r3 = k exactly; with w and l also one float32 step
        up and down (nine boxes per k, k = 2 .. 40);
      * r3 = R solved for l = R (R + w) / (w - R) at three widths per R = 2 .. 40, l rounded to float32 and moved by
        -3 .. 3 steps: (int)r3 flips from R - 1 to R inside the seven neighbours.
    Returns (boxes, labels); every box is valid and of class 0."""
    rows = []
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    for k in range(2, 41):
        for w in (down(2 * k), F(2 * k), up(2 * k)):
            for l in (down(3 * k), F(3 * k), up(3 * k)):
                rows.append((w, l))
    for R in range(2, 41):
        for w in (1.5 * R, 2.0 * R + 0.37, 3.1 * R):
            l = F(R * (R + w) / (w - R))
            ls = [l]
            for _ in range(3):
                ls = [down(ls[0])] + ls + [up(ls[-1])]
            rows += [(F(w), v) for v in ls]
    boxes = torch.tensor([[5.0, 6.0, -1.0, float(w), float(l), 1.5, 0.3, 1.0, -2.0] for w, l in rows], dtype=torch.float32)[None]
    n = boxes.shape[1]
    return ragged(boxes.contiguous().to(device), [n]), ragged(torch.zeros((1, n), dtype=torch.int64, device=device), [n])


def radii_with_root_off_by_one_ulp(boxes, direction):
    """the radii of `radius_boundary_case` if every square root were one float32 step too high (+1) or too low (-1)"""
    m = F(RADIUS_CFG["gaussian_overlap"])
    off = lambda v: np.nextafter(np.sqrt(v), F(np.inf * direction))   # noqa: E731
    with np.errstate(all="ignore"):
        return [max(RADIUS_CFG["min_radius"], to_int(gaussian_radius(F(b[3]), F(b[4]), m, sqrt=off))) for b in boxes.tensor[0].cpu().numpy()]


# --------------------------------------------------------------------------------------------------------- pinned vector
# One frame, five objects, D = 7, raw dims (norm_bbox off), the UNIT grid (cx = x, cy = y, w = dx, l = dy),
# gaussian_overlap = 0.5 (omm = 0.5, opm = 1.5), min_radius = 1, max_objs = 3, tasks ((5, 2), (7,)).  In task 0:
#   slot 0  label 2  (10.25, 7.5) 40 x 20   kept: cell (10, 7), offset (0.25, 0.5), label position 1, index 7 * 32 + 10 = 234
#             s = 60; c1 = (800 * 0.5) / 1.5 = 266.67, sq1 = sqrt(3600 - 1066.67) = 50.33, r1 = 55.17
#             b2 = 120; c2 = (0.5 * 40) * 20 = 400, sq2 = sqrt(14400 - 6400) = 89.44, r2 = 104.72
#             a3 = 2, b3 = -60, c3 = (-0.5 * 40) * 20 = -400, sq3 = sqrt(3600 + 8 * 400) = 82.46, r3 = 11.23
#             radius = max(1, int(11.23)) = 11;  yaw = 0: sin 0, cos 1
#   slot 1  label 5  x = 32 = W             candidate 2, out of range: dropped
#   slot 2  label 9                          in no task
#   slot 3  label 2  dx = 0                  candidate 3, zero size: dropped
#   slot 4  label 5  (3.0, 4.0) 2 x 2        candidate 4 > max_objs = 3: cut although it is valid
# Task 1 (class 7) has no object.  M = min(3, 5) = 3.
PINNED_CFG = dict(UNIT, gaussian_overlap=0.5, min_radius=1, max_objs=3, norm_bbox=False)
PINNED_TASKS = ((5, 2), (7,))
PINNED_BOXES = [[10.25, 7.5, -1.0, 40.0, 20.0, 1.5, 0.0],
                [32.0, 7.5, -1.0, 4.0, 2.0, 1.5, 0.5],
                [5.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.5],
                [6.0, 6.0, -1.0, 0.0, 2.0, 1.5, 0.5],
                [3.0, 4.0, -1.0, 2.0, 2.0, 1.5, 0.5]]
PINNED_LABELS = [2, 5, 9, 2, 5]
PINNED_WANT = dict(sizes=[[1], [0]], centers=[[10, 7], [0, 0], [0, 0]], radii=[11, 0, 0], labels=[1, 0, 0], indices=[234, 0, 0],
                   source=[0, -1, -1], target=[0.25, 0.5, -1.0, 40.0, 20.0, 1.5, 0.0, 1.0])


def check_pinned(op, device):
    boxes = ragged(torch.tensor([PINNED_BOXES], dtype=torch.float32, device=device), [5])
    labels = ragged(torch.tensor([PINNED_LABELS], dtype=torch.int64, device=device), [5])
    r0, r1 = op(boxes, labels, PINNED_TASKS, **PINNED_CFG)
    w = PINNED_WANT
    assert r0.centers.sample_sizes.tolist() == w["sizes"][0] and r1.centers.sample_sizes.tolist() == w["sizes"][1]
    assert r0.centers.tensor.tolist() == [w["centers"]] and r0.radii.tensor.tolist() == [w["radii"]]
    assert r0.labels.tensor.tolist() == [w["labels"]] and r0.indices.tensor.tolist() == [w["indices"]]
    assert r0.source.tensor.tolist() == [w["source"]]
    assert r0.targets.tensor.tolist() == [[w["target"], [0.0] * 8, [0.0] * 8]]      # sin 0 and cos 0 are exact everywhere
    assert r1.source.tensor.tolist() == [[-1, -1, -1]] and not r1.targets.tensor.any() and not r1.centers.tensor.any()
    assert not r1.radii.tensor.any() and not r1.labels.tensor.any() and not r1.indices.tensor.any()
    # and the definition computes the same vector
    check([r0, r1], definition(boxes.tensor, labels.tensor, boxes.sample_sizes, PINNED_TASKS, **PINNED_CFG), "pinned")
