"""Cases and oracles of lidar_depth_targets, shared by test_depth_targets_cpu.py and test_depth_targets_gpu.py.

Two oracles:
  (a) `definition`: numpy float32, restating csrc/depth_targets_arith.h operation by operation (numpy rounds every float32
      operation once and contracts nothing).  The operator must be torch.equal to it.
  (b) `definition_f64`: the same quantities in float64 on the float32-rounded inputs.  Bars: depth within
      6 * 2^-24 * (the largest float64 intermediate of the p_2 chain among the points of the cell) — six roundings feed d —
      cells and bins equal.

`placed_case` builds the inputs of (b): it chooses (u, v, d) per point and back-projects through the float64 inverse of the
float32 matrix, with u, v at least 0.01 px from every integer (so from every cell and image edge for every stride), d at
least 1e-3 from the range ends and 0.01 * step from every bin edge.  Its cameras share the lidar origin, look 360 / C degrees
apart and see less than that (53 degrees), so a point placed for one camera is far outside every other: no point has to be
left out of the float64 comparison.  `random_case` scatters points with overlapping cameras and hostile values; it is
compared against (a) only.
"""
import functools

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import lidar_depth_targets

f32 = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
RAGGED_P = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
DEPTH_RANGE = (2.0, 58.0)
BINS = (2.0, 0.5, 112)


# ------------------------------------------------------------------------------------------------------------ oracle (a)
def fold(proj, affine):
    """rows 0 and 1 of [R, 4] float32 through the image matrix [2, 3] float32: matrix_element of camera_boxes_arith.h"""
    a, b, tx, c, d, ty = (affine.reshape(6)[i] for i in range(6))
    out = proj.copy()
    with np.errstate(all="ignore"):
        out[0] = (a * proj[0] + b * proj[1]) + tx * proj[2]
        out[1] = (c * proj[0] + d * proj[1]) + ty * proj[2]
    return out


def definition(points, sizes, projection, *, image_hw, downsample=16, depth_range, depth_bins=None, image_transforms=None):
    """(depth float32 [B, C, h, w], bins int32 or None) from numpy inputs, in float32"""
    points, projection = np.asarray(points, f32), np.asarray(projection, f32)
    B, P, _ = points.shape
    C = projection.shape[1]
    H, W = image_hw
    h, w = -(-H // downsample), -(-W // downsample)
    d_min, d_max, Wf, Hf = f32(depth_range[0]), f32(depth_range[1]), f32(W), f32(H)
    keys = np.full((B, C, h * w), EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        for b in range(B):
            n = int(min(max(int(sizes[b]), 0), P))
            x, y, z = (points[b, :n, i] for i in range(3))
            for c in range(C):
                m = projection[b, c]
                if image_transforms is not None:
                    m = fold(m, np.asarray(image_transforms, f32)[b, c])
                p = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
                d = p[2]
                u, v = p[0] / d, p[1] / d
                ok = (d >= d_min) & (d < d_max) & (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
                cx = u[ok].astype(np.int32) // downsample
                cy = v[ok].astype(np.int32) // downsample
                np.minimum.at(keys[b, c], cy * w + cx, d[ok].view(np.uint32))
        has = keys != EMPTY
        depth = np.where(has, keys, np.uint32(0)).view(f32).reshape(B, C, h, w)
        bins = None
        if depth_bins is not None:
            lo, step, count = f32(depth_bins[0]), f32(depth_bins[1]), depth_bins[2]
            t = (depth - lo) / step
            ok = has.reshape(depth.shape) & (t >= 0) & (t < f32(count))
            bins = np.where(ok, np.where(ok, t, 0).astype(np.int32), np.int32(-1)).astype(np.int32)
    return depth, bins


# ------------------------------------------------------------------------------------------------------------ oracle (b)
def definition_f64(points, sizes, projection, *, image_hw, downsample=16, depth_range, depth_bins=None):
    """(depth float64, bins or None, bar [B, C, h, w]): the definition in float64 on the float32 inputs; bar is
    6 * 2^-24 * the largest intermediate of the p_2 chain among the points of the cell"""
    pts, proj = np.asarray(points, f32).astype(np.float64), np.asarray(projection, f32).astype(np.float64)
    B, P, _ = pts.shape
    C = proj.shape[1]
    H, W = image_hw
    h, w = -(-H // downsample), -(-W // downsample)
    d_min, d_max = float(f32(depth_range[0])), float(f32(depth_range[1]))
    depth = np.full((B, C, h * w), np.inf)
    big = np.zeros((B, C, h * w))
    for b in range(B):
        n = int(min(max(int(sizes[b]), 0), P))
        x, y, z = (pts[b, :n, i] for i in range(3))
        for c in range(C):
            m = proj[b, c]
            p = [m[k, 0] * x + m[k, 1] * y + m[k, 2] * z + m[k, 3] for k in range(3)]
            d = p[2]
            with np.errstate(all="ignore"):
                u, v = p[0] / d, p[1] / d
            ok = (d >= d_min) & (d < d_max) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            cell = (np.floor(v[ok]).astype(np.int64) // downsample) * w + np.floor(u[ok]).astype(np.int64) // downsample
            np.minimum.at(depth[b, c], cell, d[ok])
            t1, t2, t3 = m[2, 0] * x, m[2, 1] * y, m[2, 2] * z
            chain = np.max(np.abs(np.stack([t1, t2, t1 + t2, t3, t1 + t2 + t3, d])), axis=0)
            np.maximum.at(big[b, c], cell, chain[ok])
    has = np.isfinite(depth)
    depth = np.where(has, depth, 0.0).reshape(B, C, h, w)
    bins = None
    if depth_bins is not None:
        lo, step, count = float(f32(depth_bins[0])), float(f32(depth_bins[1])), depth_bins[2]
        t = np.floor((depth - lo) / step)
        bins = np.where(has.reshape(depth.shape) & (t >= 0) & (t < count), t, -1).astype(np.int32)
    return depth, bins, (6 * 2.0 ** -24 * big).reshape(B, C, h, w)


# ----------------------------------------------------------------------------------------------------------------- cases
def cameras(rng, B, C, R, image_hw, *, shared_origin):
    """float32 [B, C, R, 4] lidar-to-pixel matrices: a pinhole (focal 1 .. 1.3 W, so at most 53 degrees wide, flipped at
    random, principal point off centre) looking 360 / C degrees apart from any first yaw; row 3, where there is one, is NaN:
    it is never read"""
    H, W = image_hw
    out = np.full((B, C, R, 4), np.nan, np.float64)
    for b in range(B):
        yaw0 = rng.uniform(0, 2 * np.pi)
        for c in range(C):
            yaw = yaw0 + 2 * np.pi * c / C + (0 if shared_origin else rng.uniform(-0.3, 0.3))
            fx = W * rng.uniform(1.0, 1.3) * rng.choice([-1.0, 1.0])
            fy = W * rng.uniform(1.0, 1.3)
            K = np.array([[fx, 0, W * rng.uniform(0.45, 0.55)], [0, fy, H * rng.uniform(0.45, 0.55)], [0, 0, 1]])
            # camera axes in lidar coordinates: z forward along the yaw, x to the right, y down
            fwd = np.array([np.cos(yaw), np.sin(yaw), 0.0])
            right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
            Rm = np.stack([right, np.array([0, 0, -1.0]), fwd])
            t = np.zeros(3) if shared_origin else rng.uniform(-1, 1, 3)
            out[b, c, :3, :3] = K @ Rm
            out[b, c, :3, 3] = K @ t
    return out.astype(f32)


def hostile(rng, points, sizes):
    """NaN and huge values in the ignored channels and in every slot beyond sample_sizes"""
    points[:, :, 3:] = rng.choice(np.array([np.nan, 3e38, -3e38, np.inf], f32), points[:, :, 3:].shape)
    for b, n in enumerate(sizes):
        points[b, n:] = rng.choice(np.array([np.nan, 3e38, -1e30, np.inf], f32), points[b, n:].shape)
    return points


def placed_case(seed, sizes, C, D, R, image_hw, depth_bins=BINS, depth_range=DEPTH_RANGE):
    """inputs of the float64 comparison (see the module's docstring): dict(points, sizes, projection)"""
    rng = np.random.default_rng(seed)
    H, W = image_hw
    B, P = len(sizes), max(max(sizes), 1)
    proj = cameras(rng, B, C, R, image_hw, shared_origin=True)
    points = np.zeros((B, P, D), f32)
    for b, n in enumerate(sizes):
        cam = rng.integers(0, C, n)
        u = rng.integers(0, W, n) + rng.uniform(0.01, 0.99, n)
        v = rng.integers(0, H, n) + rng.uniform(0.01, 0.99, n)
        if depth_bins is not None:
            lo, step, count = depth_bins
            d = lo + (rng.integers(0, count, n) + rng.uniform(0.01, 0.99, n)) * step
            d = np.clip(d, depth_range[0] + 1e-3, depth_range[1] - 1e-3)
        else:
            d = rng.uniform(depth_range[0] + 1e-3, depth_range[1] - 1e-3, n)
        for i in range(n):
            m = proj[b, cam[i]].astype(np.float64)
            points[b, i, :3] = np.linalg.solve(m[:3, :3], d[i] * np.array([u[i], v[i], 1.0]) - m[:3, 3])
    return dict(points=hostile(rng, points, sizes), sizes=np.asarray(sizes), projection=proj)


def random_case(seed, sizes, C, D, R, image_hw):
    """points scattered around overlapping cameras; compared against the float32 definition only"""
    rng = np.random.default_rng(seed)
    B, P = len(sizes), max(max(sizes), 1)
    proj = cameras(rng, B, C, R, image_hw, shared_origin=False)
    points = rng.uniform(-40, 40, (B, P, D)).astype(f32)
    points[:, :, 2] = rng.uniform(-3, 3, (B, P)).astype(f32)
    return dict(points=hostile(rng, points, sizes), sizes=np.asarray(sizes), projection=proj)


def transforms(seed, B, C):
    """float32 [B, C, 2, 3] image matrices: scale 0.3 .. 0.6 (here on an image already small: 0.6 .. 1.2), a small rotation,
    a flip at random, a shift"""
    rng = np.random.default_rng(seed)
    s, r = rng.uniform(0.6, 1.2, (B, C)), rng.uniform(-0.1, 0.1, (B, C))
    flip = rng.choice([-1.0, 1.0], (B, C))
    t = np.zeros((B, C, 2, 3))
    t[..., 0, 0], t[..., 0, 1], t[..., 0, 2] = s * np.cos(r) * flip, -s * np.sin(r), rng.uniform(-3, 3, (B, C)) + (flip < 0) * 40
    t[..., 1, 0], t[..., 1, 1], t[..., 1, 2] = s * np.sin(r) * flip, s * np.cos(r), rng.uniform(-3, 3, (B, C))
    return t.astype(f32)


# ------------------------------------------------------------------------------------------------------------- running
def ragged(points, sizes, dev, size_dtype=torch.int64):
    return RaggedBatch(torch.from_numpy(np.ascontiguousarray(points)).to(dev),
                       sample_sizes=torch.from_numpy(np.asarray(sizes)).to(size_dtype).to(dev))


def run(case, dev, size_dtype=torch.int64, image_transforms=None, **kw):
    """the operator on a case's numpy inputs moved to `dev`"""
    tr = None if image_transforms is None else torch.from_numpy(image_transforms).to(dev)
    return lidar_depth_targets(ragged(case["points"], case["sizes"], dev, size_dtype), torch.from_numpy(case["projection"]).to(dev),
                               image_transforms=tr, **kw)


def check_equal(got, want, what=""):
    """torch.equal against oracle (a), NaN-free by construction; +0 and -0 compare equal, so the bits are compared"""
    depth, bins = want
    g = got.depth.cpu().numpy()
    assert g.dtype == f32 and g.shape == depth.shape, f"{what}: depth is {g.dtype} {g.shape}, expected {depth.shape}"
    diff = g.view(np.uint32) != depth.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} depth cells differ, first at {tuple(np.argwhere(diff)[0])}"
    if bins is None:
        assert got.bins is None, f"{what}: bins without depth_bins"
    else:
        assert got.bins.dtype == torch.int32
        assert torch.equal(got.bins.cpu(), torch.from_numpy(bins)), f"{what}: bins differ"


def check_f64(got, case, what="", **kw):
    """oracle (b): the same cells are filled, depth within the bar, bins equal"""
    depth, bins, bar = definition_f64(case["points"], case["sizes"], case["projection"], **kw)
    g = got.depth.cpu().numpy().astype(np.float64)
    assert ((g != 0) == (depth != 0)).all(), f"{what}: {int(((g != 0) != (depth != 0)).sum())} cells filled on one side only"
    err = np.abs(g - depth)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    assert (err <= bar).all(), f"{what}: depth error {err[worst]:.3e} over its bar {bar[worst]:.3e} at {worst}"
    if bins is not None:
        assert torch.equal(got.bins.cpu(), torch.from_numpy(bins)), f"{what}: bins differ from float64"
    return float((err / np.where(bar > 0, bar, 1)).max())   # the largest error in units of the bar


# ---------------------------------------------------------------------------------------- the checks both test files run
# B, C, D, R, dtype of sample_sizes, image_hw, downsample: B in {1, 3}, C in {1, 2, 6}, D in {3, 4, 5}, R in {3, 4}, both extents
# (neither a multiple of 16, 30 x 44 of no stride but 1 and 2), every stride; w = 44, 22, 11, 3 are no multiples of 4 but the first
CONFIGS = [(1, 1, 3, 3, torch.int32, (32, 48), 1), (3, 2, 4, 4, torch.int64, (30, 44), 2), (3, 6, 5, 3, torch.int32, (32, 48), 4),
           (1, 6, 4, 3, torch.int64, (30, 44), 16), (3, 1, 4, 4, torch.int32, (30, 44), 4), (1, 2, 5, 4, torch.int64, (32, 48), 16),
           (3, 2, 3, 3, torch.int64, (30, 44), 1)]
SIZES = {1: [(1025,), (65,)], 3: [(0, 65, 1025), (1, 64, 257), (63, 255, 256)]}
assert {n for s in SIZES[3] for n in s} == set(RAGGED_P)


def check_config(dev, B, C, D, R, size_dtype, image_hw, downsample):
    kw = dict(image_hw=image_hw, downsample=downsample, depth_range=DEPTH_RANGE, depth_bins=BINS)
    worst = 0.0
    for n, sizes in enumerate(SIZES[B]):
        case = placed_case(100 * B + 10 * C + n, sizes, C, D, R, image_hw)
        got = run(case, dev, size_dtype, **kw)
        assert got.depth.device.type == torch.device(dev).type
        check_equal(got, definition(case["points"], case["sizes"], case["projection"], **kw), f"placed {sizes}")
        if sum(sizes):
            assert int((got.depth != 0).sum()) > 0, "the case places no point"
        worst = max(worst, check_f64(got, case, f"placed {sizes}", **kw))
        case = random_case(200 * B + 10 * C + n, sizes, C, D, R, image_hw)
        check_equal(run(case, dev, size_dtype, **kw), definition(case["points"], case["sizes"], case["projection"], **kw), f"random {sizes}")
    print(f"largest depth error against float64: {worst:.3f} of the bar")


def check_misaligned_points(dev):
    """D == 4 with the first point 4 bytes off a 16-byte boundary: the kernel's 4-byte loads"""
    case = random_case(5, (300, 77), 2, 4, 3, (32, 48))
    kw = dict(image_hw=(32, 48), downsample=4, depth_range=DEPTH_RANGE, depth_bins=BINS)
    flat = torch.zeros(case["points"].size + 1, dtype=torch.float32, device=dev)
    view = flat[1:].view(case["points"].shape)
    view.copy_(torch.from_numpy(case["points"]))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    pts = RaggedBatch(view, sample_sizes=torch.tensor(case["sizes"], device=dev))
    got = lidar_depth_targets(pts, torch.from_numpy(case["projection"]).to(dev), **kw)
    check_equal(got, definition(case["points"], case["sizes"], case["projection"], **kw), "misaligned")


def check_band_splits(dev):
    """every split of a tiny map gives the bits of the automatic one"""
    for image_hw, downsample in (((32, 48), 4), ((30, 44), 2), ((30, 44), 1)):
        case = random_case(7, (1025, 64, 257), 2, 4, 3, image_hw)
        kw = dict(image_hw=image_hw, downsample=downsample, depth_range=DEPTH_RANGE, depth_bins=BINS)
        want = definition(case["points"], case["sizes"], case["projection"], **kw)
        h = -(-image_hw[0] // downsample)
        for rows in (0, 1, 2, h - 1, h):
            check_equal(run(case, dev, _band_rows=rows, **kw), want, f"{image_hw} / {downsample}, band_rows {rows}")


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)    # u = x / z, v = y / z, d = z


def uvd(rows):
    """points (x, y, z) of (u, v, d) under IDENTITY; exact where u * d and v * d are"""
    a = np.asarray(rows, np.float64)
    return np.stack([a[:, 0] * a[:, 2], a[:, 1] * a[:, 2], a[:, 2]], axis=1).astype(f32)


def auto_band_rows(h, w, maps, band_cells):
    """the library's band rule (choose_band_rows of csrc/depth_targets.hip), restated"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd", "csrc", "depth_targets.hip")).read()
    target = int(re.search(r"constexpr int kTargetWorkgroups = (\d+);", src).group(1))
    most = band_cells // w
    bands = max(-(-h // most), min(h, target // maps))
    return -(-h // bands)


def check_multi_band(dev, band_cells):
    """maps of limit - w, limit and limit + w cells: the last is the smallest extent of this width that no single band holds.
    Points sit in the last row of a band and the first of the next for the automatic split of one map, for the automatic
    split of so many maps that only the limit splits them (two bands), and for forced splits; every split gives the same bits"""
    w = 64
    limit = band_cells // w
    assert limit * w == band_cells
    for h in (limit - 1, limit, limit + 1):
        few, many = auto_band_rows(h, w, 1, band_cells), auto_band_rows(h, w, 64, band_cells)
        assert few < many and many == (h if h <= limit else -(-h // 2))
        edges = sorted({r for k in (few, many, 64, limit) for r in (k - 1, k) if 0 <= r < h} | {0, h - 1})
        rng = np.random.default_rng(h)
        rows = [(rng.integers(0, w) + 0.5, r + 0.5, float(2 ** rng.integers(1, 6))) for r in edges for _ in range(3)]
        pts = np.concatenate([uvd(rows), np.zeros((len(rows), 1), f32)], axis=1)[None]
        sizes = np.array([len(rows)])
        proj = IDENTITY[None, None]
        kw = dict(image_hw=(h, w), downsample=1, depth_range=(1.0, 100.0), depth_bins=(1.0, 1.0, 64))
        want = definition(pts, sizes, proj, **kw)
        assert {int(r) for r in np.argwhere(want[0][0, 0] != 0)[:, 0]} == set(edges)
        case = dict(points=pts, sizes=sizes, projection=proj)
        for rows_forced in (0, 1, 64, few, many, limit):
            check_equal(run(case, dev, _band_rows=rows_forced, **kw), want, f"h {h}, band_rows {rows_forced}")
        # 4 frames x 16 cameras: the automatic split is the limit's alone
        case = dict(points=pts.repeat(4, 0), sizes=sizes.repeat(4), projection=np.ascontiguousarray(np.broadcast_to(proj, (4, 16, 3, 4))))
        got = run(case, dev, **kw)
        assert tuple(got.depth.shape) == (4, 16, h, w)
        for b in range(4):
            for c in range(16):
                check_equal(DepthPair(got.depth[b:b + 1, c:c + 1], got.bins[b:b + 1, c:c + 1]), want, f"h {h}, map ({b}, {c})")


class DepthPair:
    def __init__(self, depth, bins):
        self.depth, self.bins = depth, bins


def check_hand_placed(dev):
    H, W, s = 32, 48, 4
    below_w = float(np.nextafter(f32(W), f32(0)))
    rows = [(0.0, 1.5, 4.0),                    # 0: u exactly 0 counts: cell (0, 0) = 4
            (-0.5, 1.5, 2.0),                   # 1: u in (-1, 0) does not count, though int(u) == 0 and it is nearer
            (below_w, 5.5, 8.0),                # 2: the largest u below W counts: cell (1, 11) = 8
            (float(W), 9.5, 4.0),               # 3: u == W does not count (cell (2, 12) does not exist)
            (9.5, 9.5, 2.0),                    # 4: d == d_min counts: cell (2, 2) = 2
            (13.5, 9.5, 58.0),                  # 5: d == d_max does not count: cell (2, 3) stays empty
            (17.5, 17.5, 8.0), (18.5, 18.5, 8.0),     # 6, 7: equal depths in cell (4, 4) = 8
            (21.5, 17.5, 16.0), (22.5, 17.5, 8.0),    # 8, 9: the later is nearer: cell (4, 5) = 8
            (25.5, 17.5, 4.0), (26.5, 17.5, 16.0),    # 10, 11: the earlier is nearer: cell (4, 6) = 4
            (29.5, 17.5, 10.0),                 # 12: cell (4, 7) = 10, t == count
            (33.5, 17.5, 16.0)]                 # 13: cell (4, 8) = 16, int(t) > count
    xyz = uvd(rows)
    nan, inf = np.nan, np.inf
    xyz = np.concatenate([xyz, np.array([[1, 1, 0], [-8, 8, -4],                     # d = 0; behind the camera with u = 2 in range
                                         [nan, 8, 4], [8, nan, 4], [8, 8, nan], [inf, 8, 4], [8, -inf, 4], [8, 8, inf]], f32)])
    assert np.array_equal(xyz[:14, 0] / xyz[:14, 2], np.array([r[0] for r in rows], f32))   # the placements are exact
    pts = np.zeros((1, len(xyz) + 2, 4), f32)
    pts[0, :len(xyz), :3] = xyz
    pts[0, len(xyz):, :3] = uvd([(40.5, 29.5, 4.0), (41.5, 29.5, 4.0)])              # beyond sample_sizes: never read
    proj = np.stack([IDENTITY, IDENTITY])[None].copy()
    proj[0, 1, 1, 2] = np.nan                                                         # camera 1 only: its v is NaN for every point
    case = dict(points=pts, sizes=np.array([len(xyz)]), projection=proj)
    kw = dict(image_hw=(H, W), downsample=s, depth_range=(2.0, 58.0), depth_bins=(4.0, 2.0, 3))
    got = run(case, dev, **kw)
    check_equal(got, definition(pts, case["sizes"], proj, **kw), "hand-placed")
    d, b = got.depth.cpu().numpy(), got.bins.cpu().numpy()
    expect = {(0, 0): (4.0, 0), (1, 11): (8.0, 2), (2, 2): (2.0, -1), (2, 3): (0.0, -1), (4, 4): (8.0, 2), (4, 5): (8.0, 2),
              (4, 6): (4.0, 0), (4, 7): (10.0, -1), (4, 8): (16.0, -1), (7, 10): (0.0, -1), (7, 11): (0.0, -1)}
    for (cy, cx), (depth, bin_) in expect.items():
        assert (d[0, 0, cy, cx], b[0, 0, cy, cx]) == (depth, bin_), f"cell ({cy}, {cx}): {d[0, 0, cy, cx]}, {b[0, 0, cy, cx]}"
    assert int((d[0, 0] != 0).sum()) == 8
    assert not d[0, 1].any() and (b[0, 1] == -1).all(), "a NaN in camera 1's matrix leaves camera 1 empty and camera 0 alone"
    none = run(case, dev, **dict(kw, depth_bins=None))
    assert none.bins is None and torch.equal(none.depth, got.depth)


def check_image_transforms(dev):
    """image_transforms folded inside against the matrices camera_augment_boxes returns: bit for bit"""
    from accvlab.draw_heatmap import camera_augment_boxes

    B, C, image_hw = 3, 2, (32, 48)
    kw = dict(image_hw=image_hw, downsample=4, depth_range=DEPTH_RANGE, depth_bins=BINS)
    for R in (3, 4):
        case = random_case(11 + R, (257, 64, 1025), C, 4, R, image_hw)
        tr = transforms(3, B, C)
        inside = run(case, dev, image_transforms=tr, **kw)
        check_equal(inside, definition(case["points"], case["sizes"], case["projection"], image_transforms=tr, **kw), "folded inside")
        boxes = RaggedBatch(torch.zeros((B * C, 1, 4), device=dev), sample_sizes=torch.zeros((B * C,), dtype=torch.int64, device=dev))
        aug = camera_augment_boxes(boxes, torch.from_numpy(tr).to(dev).view(B * C, 2, 3), image_hw=image_hw, check_occlusion=False,
                                   projection_matrices=[torch.from_numpy(case["projection"]).to(dev).view(B * C, R, 4)])
        outside = lidar_depth_targets(ragged(case["points"], case["sizes"], dev), aug.projection_matrices[0].view(B, C, R, 4), **kw)
        assert torch.equal(inside.depth, outside.depth) and torch.equal(inside.bins, outside.bins)
        assert int((inside.depth != 0).sum()) > 0 and not torch.equal(inside.depth, run(case, dev, **kw).depth)


def check_reproducible_and_inputs_untouched(dev):
    case = random_case(21, (1025, 257, 65), 6, 4, 3, (32, 48))
    kw = dict(image_hw=(32, 48), downsample=4, depth_range=DEPTH_RANGE, depth_bins=BINS)
    pts, proj = ragged(case["points"], case["sizes"], dev), torch.from_numpy(case["projection"]).to(dev)
    before = (pts.tensor.clone(), pts.sample_sizes.clone(), proj.clone())
    one, two = lidar_depth_targets(pts, proj, **kw), lidar_depth_targets(pts, proj, **kw)
    assert torch.equal(one.depth, two.depth) and torch.equal(one.bins, two.bins)
    assert not one.depth.requires_grad
    for now, then in zip((pts.tensor, pts.sample_sizes, proj), before):
        assert torch.equal(now.view(torch.uint8 if now.dtype == torch.float32 else now.dtype), then.view_as(now).view(
            torch.uint8 if now.dtype == torch.float32 else now.dtype))


def check_empty(dev):
    kw = dict(image_hw=(32, 48), downsample=4, depth_range=DEPTH_RANGE, depth_bins=BINS)
    got = lidar_depth_targets(RaggedBatch(torch.zeros((0, 5, 4), device=dev), sample_sizes=torch.zeros((0,), dtype=torch.int64, device=dev)),
                              torch.zeros((0, 6, 3, 4), device=dev), **kw)
    assert tuple(got.depth.shape) == tuple(got.bins.shape) == (0, 6, 8, 12)
    for P in (0, 9):      # P == 0, and slots that no frame uses: the launch still writes every cell
        pts = RaggedBatch(torch.full((2, P, 4), float("nan"), device=dev), sample_sizes=torch.zeros((2,), dtype=torch.int32, device=dev))
        got = lidar_depth_targets(pts, torch.from_numpy(np.stack([IDENTITY] * 3)[None].repeat(2, 0)).to(dev), **kw)
        assert tuple(got.depth.shape) == (2, 3, 8, 12) and not got.depth.any() and bool((got.bins == -1).all())
        assert got.depth.dtype == torch.float32 and got.bins.dtype == torch.int32
    # sample_sizes beyond P and below 0 are clamped
    case = random_case(31, (300, 300), 2, 3, 3, (32, 48))
    want = definition(case["points"], [300, 0], case["projection"], **kw)
    check_equal(run(dict(case, sizes=np.array([10 ** 6, -5])), dev, **kw), want, "clamped sizes")


@functools.lru_cache(maxsize=None)
def most_frames_case():
    """B = 65535 frames of at most two points, one camera, 2 x 2 maps: (case, kw, want), built once for both test files and
    never written to.  Under IDENTITY d is z itself, so every frame has depths of its own"""
    B = 65535
    rng = np.random.default_rng(71)
    rows = np.stack([rng.uniform(-1, 5, 2 * B), rng.uniform(-1, 5, 2 * B), rng.uniform(1, 64, 2 * B)], axis=1)
    case = dict(points=uvd(rows).reshape(B, 2, 3), sizes=rng.integers(0, 3, B),
                projection=np.ascontiguousarray(np.broadcast_to(IDENTITY[None, None], (B, 1, 3, 4))))
    kw = dict(image_hw=(4, 4), downsample=2, depth_range=DEPTH_RANGE, depth_bins=BINS)
    want = definition(case["points"], case["sizes"], case["projection"], **kw)
    filled = (want[0] != 0).reshape(B, -1).sum(1)
    assert sorted(np.unique(filled).tolist()) == [0, 1, 2] and filled[0] > 0 and filled[-1] > 0 and (filled <= case["sizes"]).all()
    assert sorted(np.unique(case["sizes"]).tolist()) == [0, 1, 2]
    return case, kw, want


def check_most_frames(dev, other_dev=None):
    """B = 65535 frames, the most a launch takes in its grid's z extent; no map holds anything but depths of its own frame"""
    case, kw, want = most_frames_case()
    got = run(case, dev, **kw)
    check_equal(got, want, "65535 frames")
    depth, z = got.depth.cpu().numpy().reshape(-1, 4), case["points"][:, :, 2]
    own = (depth == 0) | ((depth[:, :, None] == z[:, None, :]) & (np.arange(2) < case["sizes"][:, None])[:, None, :]).any(2)
    assert own.all() and bool((got.bins.cpu().numpy().reshape(-1, 4)[depth == 0] == -1).all())
    if other_dev is not None:
        other = run(case, other_dev, **kw)
        assert torch.equal(got.depth.cpu().view(torch.int32), other.depth.cpu().view(torch.int32)) and torch.equal(got.bins.cpu(), other.bins.cpu())


def check_guard_bands(dev, band_cells):
    """the C entry alone writes [B, C, h, w] of both outputs completely and nothing outside, for outputs on a 16-byte boundary
    (16-byte stores) and 4 bytes off it (4-byte stores)"""
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    cuda = torch.device(dev).type == "cuda"
    for image_hw, downsample, pad in (((32, 48), 4, 512), ((30, 44), 2, 516), ((30, 44), 16, 512), ((band_cells // 64 + 1, 64), 1, 516)):
        case = random_case(41, (257, 1025), 2, 4, 3, image_hw)
        kw = dict(image_hw=image_hw, downsample=downsample, depth_range=DEPTH_RANGE, depth_bins=BINS)
        pts, proj = ragged(case["points"], case["sizes"], dev), torch.from_numpy(case["projection"]).to(dev)
        h, w = -(-image_hw[0] // downsample), -(-image_hw[1] // downsample)
        nbytes = 2 * 2 * h * w * 4
        bufs = [torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2)]
        depth = bufs[0][pad: pad + nbytes].view(torch.float32).view(2, 2, h, w)
        bins = bufs[1][pad: pad + nbytes].view(torch.int32).view(2, 2, h, w)
        assert depth.data_ptr() % 16 == pad % 16
        p = nat.DepthTargetsParams()
        p.points, p.sample_sizes, p.projection = pts.tensor.data_ptr(), pts.sample_sizes.data_ptr(), proj.data_ptr()
        p.image_h, p.image_w, p.downsample = image_hw[0], image_hw[1], downsample
        p.depth_min, p.depth_max, p.bin_lo, p.bin_step, p.bin_count, p.sizes_i64 = *DEPTH_RANGE, *BINS, 1
        args = (ctypes.addressof(p), 2, pts.tensor.shape[1], 4, 2, 3, depth.data_ptr(), bins.data_ptr())
        if cuda:
            status = lib.accv_depth_targets(*args, nat.stream_ptr(torch.device(dev, torch.cuda.current_device())))
            torch.cuda.synchronize()
        else:
            status = lib.accv_depth_targets_cpu(*args)
        assert status == 0, lib.accv_last_error()
        for buf in bufs:
            assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + nbytes:] == 0xA5).all()), "wrote outside its buffer"
        # the sentinel inside is gone wherever the definition has a value, which is everywhere
        check_equal(DepthPair(depth.clone(), bins.clone()), definition(
            case["points"], case["sizes"], case["projection"], **kw), f"banded {image_hw} / {downsample}")


def check_errors(dev, band_cells, other_dev=None):
    """every documented error is raised by the Python layer or the entry's own checks, before a launch"""
    import pytest

    case = random_case(51, (20, 30), 2, 4, 3, (32, 48))
    good = dict(image_hw=(32, 48), downsample=4, depth_range=DEPTH_RANGE, depth_bins=BINS)
    pts = lambda: ragged(case["points"], case["sizes"], dev)                            # noqa: E731
    proj = lambda: torch.from_numpy(case["projection"]).to(dev)                         # noqa: E731
    call = lambda p=None, m=None, **kw: lidar_depth_targets(p if p is not None else pts(), m if m is not None else proj(),  # noqa: E731
                                                            **dict(good, **kw))
    call()
    for bad in ((0.0, 58.0), (-1.0, 58.0), (58.0, 2.0), (2.0, 2.0), (2.0, float("inf")), (float("nan"), 58.0), (1e-60, 58.0)):
        with pytest.raises(RuntimeError, match="depth_range"):
            call(depth_range=bad)
    with pytest.raises(RuntimeError, match="cameras"):
        call(m=torch.zeros((2, 17, 3, 4), device=dev))
    with pytest.raises(RuntimeError, match="cameras"):
        call(m=torch.zeros((2, 0, 3, 4), device=dev))
    with pytest.raises(RuntimeError, match="DT_BAND_CELLS"):
        call(image_hw=(4, band_cells + 1), downsample=1)
    call(image_hw=(4, band_cells), downsample=1)
    with pytest.raises(RuntimeError, match="DT_BAND_CELLS"):
        call(_band_rows=band_cells // 12 + 1)
    wide = torch.zeros((2, 30, 8), device=dev)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(p=RaggedBatch(wide[:, :, :4], sample_sizes=torch.tensor([20, 30], device=dev)))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(m=torch.zeros((2, 2, 4, 3), device=dev).transpose(2, 3))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(image_transforms=torch.zeros((2, 2, 3, 2), device=dev).transpose(2, 3))
    with pytest.raises(TypeError, match="float32"):
        call(p=RaggedBatch(pts().tensor.double(), sample_sizes=pts().sample_sizes))
    with pytest.raises(TypeError, match="float32"):
        call(m=proj().half())
    with pytest.raises(TypeError, match="float32"):
        call(image_transforms=torch.zeros((2, 2, 2, 3), dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="sample_sizes"):
        call(p=RaggedBatch(pts().tensor, sample_sizes=torch.tensor([20, 30], dtype=torch.int16, device=dev)))
    with pytest.raises(RuntimeError, match="image_hw"):
        call(image_hw=torch.tensor([32, 48], device=dev))
    for bad in ((0, 48), (32, 48.0), (32,), 32):
        with pytest.raises(RuntimeError, match="image_hw"):
            call(image_hw=bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(RuntimeError, match="downsample"):
            call(downsample=bad)
    for bad in ((2.0, 0.0, 4), (2.0, -1.0, 4), (2.0, 0.5, 0), (2.0, 0.5, 2 ** 15 + 1), (2.0, 0.5, 4.0), (float("nan"), 0.5, 4), (2.0, 0.5)):
        with pytest.raises(RuntimeError, match="depth_bins"):
            call(depth_bins=bad)
    call(depth_bins=(2.0, 0.5, 2 ** 15))
    for bad in (torch.zeros((2, 2, 2, 4), device=dev), torch.zeros((2, 2, 3, 3), device=dev), torch.zeros((3, 2, 3, 4), device=dev),
                torch.zeros((2, 3, 4), device=dev)):
        with pytest.raises(RuntimeError, match="projection"):
            call(m=bad)
    with pytest.raises(RuntimeError, match="image_transforms"):
        call(image_transforms=torch.zeros((2, 2, 3, 3), device=dev))
    with pytest.raises(RuntimeError, match="points"):
        call(p=RaggedBatch(torch.zeros((2, 30, 2), device=dev), sample_sizes=torch.tensor([20, 30], device=dev)))
    with pytest.raises(RuntimeError, match="points"):
        call(p=pts().tensor)
    if other_dev is not None:       # mixed devices
        with pytest.raises(RuntimeError, match="device"):
            call(m=proj().to(other_dev))
        with pytest.raises(RuntimeError, match="device"):
            call(image_transforms=torch.zeros((2, 2, 2, 3), device=other_dev))
        with pytest.raises(RuntimeError, match="device"):
            call(p=RaggedBatch(pts().tensor, sample_sizes=pts().sample_sizes.to(other_dev)))
