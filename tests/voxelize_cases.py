"""Cases and the definition of voxelize_points, shared by test_voxelize_cpu.py and test_voxelize_gpu.py.

`definition` is mmcv's hard_voxelize_forward_cpu, the sequential loop, restated in numpy float32 operation by operation
(numpy rounds every float32 operation once and contracts nothing): the keys of all points at once, then one pass over the
points in slot order with a dict from key to voxel number.  `stop_when_full=True` gives the older mmcv rule (`break` where
the current one has `continue`), which the truncation test asserts to differ.  `augment` restates augment_center of
csrc/bev_augment_arith.h.  Nothing in the operator is approximate: every comparison is bit for bit, floats as int32 views, so
that NaN payloads and the sign of zero count.

The second half of the checks enters the launch regimes of csrc/voxelize.hip (DESIGN, "Launch regimes and the tests that
enter them"); the constants of the device's work partition are arguments, which the GPU file reads from the source.
"""
import functools

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.point_cloud import Voxels, concatenate_voxels, voxelize_points

f32 = np.float32
FIELDS = ("voxels", "coors", "num_points", "voxel_counts", "point_voxel")

# 16 x 16 pillars and 16 x 16 x 4 voxels over the same range; the random points overshoot it on every side
RANGE = (-4.0, -4.0, -2.0, 4.0, 4.0, 2.0)
PILLARS = dict(voxel_size=(0.5, 0.5, 4.0), point_cloud_range=RANGE)
VOXELS3D = dict(voxel_size=(0.5, 0.5, 1.0), point_cloud_range=RANGE)
FINE = dict(voxel_size=(0.125, 0.125, 4.0), point_cloud_range=RANGE)     # 64 x 64 pillars: most points alone in theirs


# ------------------------------------------------------------------------------------------------------- the definition
def grid_of(voxel_size, point_cloud_range):
    v = np.asarray(voxel_size, f32)
    lo, hi = np.asarray(point_cloud_range[:3], f32), np.asarray(point_cloud_range[3:], f32)
    return v, lo, np.rint((hi - lo) / v).astype(f32)


def augment(rows, points):
    """points [B, P, D] with x, y, z through the rows [B, 7]: augment_center in float32, operation by operation"""
    rows, out = np.asarray(rows, f32), np.array(points, f32, copy=True)
    with np.errstate(all="ignore"):
        c, s, k, tx, ty, tz = (rows[:, i, None] for i in range(1, 7))
        x, y, z = points[:, :, 0], points[:, :, 1], points[:, :, 2]
        out[:, :, 0] = ((c * x - s * y) * k) + tx
        out[:, :, 1] = ((s * x + c * y) * k) + ty
        out[:, :, 2] = (z * k) + tz
    return out


def definition(points, sizes, *, voxel_size, point_cloud_range, max_points, max_voxels, augmentation=None, stop_when_full=False):
    """dict of the five outputs as numpy arrays (voxels float32 [B, V, T, D], the others int32)"""
    points = np.asarray(points, f32)
    B, P, D = points.shape
    T, V = max_points, max_voxels
    placed = points if augmentation is None else augment(augmentation, points)
    v, lo, g = grid_of(voxel_size, point_cloud_range)
    with np.errstate(all="ignore"):
        t = np.floor((placed[:, :, :3] - lo) / v)
        ok = ((t >= 0) & (t < g)).all(axis=2)
        c = np.where(ok[:, :, None], t, 0).astype(np.int64)
    gi = g.astype(np.int64)
    keys = (c[:, :, 2] * gi[1] + c[:, :, 1]) * gi[0] + c[:, :, 0]
    voxels = np.zeros((B, V, T, D), f32)
    coors = np.full((B, V, 3), -1, np.int32)
    num = np.zeros((B, V), np.int32)
    counts = np.zeros((B,), np.int32)
    pv = np.full((B, P), -1, np.int32)
    bits, out_bits = placed.view(np.uint32), voxels.view(np.uint32)
    for b in range(B):
        n = int(min(max(int(sizes[b]), 0), P))
        number = {}
        for p in range(n):
            if not ok[b, p]:
                continue
            key = int(keys[b, p])
            vox = number.get(key)
            if vox is None:
                if len(number) == V:
                    if stop_when_full:
                        break
                    continue
                vox = number[key] = len(number)
                coors[b, vox] = (c[b, p, 2], c[b, p, 1], c[b, p, 0])
            pv[b, p] = vox
            if num[b, vox] < T:
                out_bits[b, vox, num[b, vox]] = bits[b, p]
                num[b, vox] += 1
        counts[b] = len(number)
    return dict(voxels=voxels, coors=coors, num_points=num, voxel_counts=counts, point_voxel=pv)


# ----------------------------------------------------------------------------------------------------------------- cases
def random_points(seed, sizes, D, P=None, spread=4.5):
    """float32 [B, P, D]: x, y in [-spread, spread], z in [-2.3, 2.3], passthrough channels with NaNs of several payloads, and
    in-range garbage in the slots beyond the sizes"""
    rng = np.random.default_rng(seed)
    B, P = len(sizes), max(max(sizes), 1) if P is None else P
    pts = rng.uniform(-spread, spread, (B, P, D)).astype(f32)
    pts[:, :, 2] = rng.uniform(-2.3, 2.3, (B, P)).astype(f32)
    if D > 3:
        extra = pts[:, :, 3:].view(np.uint32)
        hit = rng.random(extra.shape) < 0.1
        extra[hit] = rng.choice(np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000], np.uint32), int(hit.sum()))
    return pts


def ragged(points, sizes, dev, size_dtype=torch.int64):
    return RaggedBatch(torch.from_numpy(np.ascontiguousarray(points)).to(dev),
                       sample_sizes=torch.from_numpy(np.asarray(sizes, np.int64)).to(size_dtype).to(dev))


def run(points, sizes, dev, size_dtype=torch.int64, augmentation=None, **kw):
    aug = None if augmentation is None else torch.from_numpy(np.asarray(augmentation, f32)).to(dev)
    return voxelize_points(ragged(points, sizes, dev, size_dtype), augmentation=aug, return_point_voxel=True, **kw)


def bits_of(t):
    t = t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check_equal(got, want, what=""):
    """all five outputs bit for bit; `want` is a Voxels or the dict of `definition`"""
    if isinstance(want, Voxels):
        want = want._asdict()
    for name in FIELDS:
        g, w = getattr(got, name), want[name]
        assert g.dtype == (torch.float32 if name == "voxels" else torch.int32), f"{what}: {name} is {g.dtype}"
        g, w = bits_of(g), bits_of(w)
        assert tuple(g.shape) == tuple(w.shape), f"{what}: {name} is {tuple(g.shape)}, expected {tuple(w.shape)}"
        if not torch.equal(g, w):
            first = tuple(int(i) for i in torch.nonzero(g != w)[0])
            raise AssertionError(f"{what}: {name} differs in {int((g != w).sum())} elements, first at {first}: "
                                 f"{int(g[first])} for {int(w[first])}")


def rows(seed, B):
    """augmentation rows [B, 7]: a rotation, a scale near 1 and a shift of about a voxel"""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.4, 0.4, B)
    return np.stack([th, np.cos(th), np.sin(th), rng.uniform(0.95, 1.05, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B),
                     rng.uniform(-0.2, 0.2, B)], axis=1).astype(f32)


IDENTITY_ROW = np.array([0, 1, 0, 1, 0, 0, 0], f32)

# B, D, dtype of sample_sizes, grid, T, V, whether V is below the occupied voxels of a 1500-point frame (all 256 pillars,
# about 680 of the 1024 voxels): B in {1, 3}, D in {3, 4, 5, 8}, both dtypes, pillars and 3D grids, T in {1, 3, 10}
CONFIGS = [(1, 3, torch.int32, PILLARS, 3, 400, False), (3, 4, torch.int64, VOXELS3D, 10, 150, True),
           (3, 5, torch.int32, PILLARS, 1, 64, True), (1, 8, torch.int64, VOXELS3D, 3, 1100, False),
           (3, 8, torch.int32, PILLARS, 10, 100, True), (1, 4, torch.int64, PILLARS, 1, 400, False),
           (3, 3, torch.int64, VOXELS3D, 3, 300, True), (1, 5, torch.int32, VOXELS3D, 10, 200, True)]
SIZES = {1: [(1500,), (65,)], 3: [(0, 65, 1500), (1, 64, 700), (63, 255, 256)]}


# ---------------------------------------------------------------------------------------- the checks both test files run
def check_config(dev, B, D, size_dtype, grid, T, V, below):
    kw = dict(max_points=T, max_voxels=V, **grid)
    for n, sizes in enumerate(SIZES[B]):
        pts = random_points(100 * B + 10 * D + n, sizes, D)
        got = run(pts, sizes, dev, size_dtype, **kw)
        assert got.voxels.device.type == torch.device(dev).type
        want = definition(pts, sizes, **kw)
        check_equal(got, want, f"random {sizes}")
        if max(sizes) == 1500:      # the case is what its comment says
            occupied = int(definition(pts, sizes, **dict(kw, max_voxels=4096))["voxel_counts"][-1])
            assert (occupied > V) == below and int(want["voxel_counts"][-1]) == min(occupied, V)
            assert T > 3 or int((want["point_voxel"] >= 0).sum()) > int(want["num_points"].sum()), "no voxel overflows max_points"


def check_partition(dev, threads, scan_points):
    """P at one chunk of the count and number kernels' workgroups (scan_points = lanes x points a lane) - 1, at it, + 1 and
    at two chunks + 1, with ragged sizes that straddle the per-point kernels' workgroup (threads) and the step; 4096 and 8192 are powers of
    two and 4097, 8193 just past one: the table-size rule on both sides"""
    kw = dict(max_points=3, max_voxels=5000, **FINE)
    for P, sizes in ((scan_points - 1, (scan_points - 1, threads - 1, threads)), (scan_points, (threads + 1, scan_points, 2 * threads + 1)),
                     (scan_points + 1, (scan_points + 1, scan_points, scan_points - 1)),
                     (2 * scan_points + 1, (2 * scan_points + 1, 2 * scan_points, scan_points + threads))):
        for D in (4, 5):
            pts = random_points(P + D, sizes, D, P=P, spread=4.2)
            got = run(pts, sizes, dev, **kw)
            check_equal(got, definition(pts, sizes, **kw), f"P {P}, D {D}")
            assert int(got.voxel_counts.max()) > 1000


def check_truncation(dev):
    # every point of a frame in one voxel, P > 4 T: the cascade under the most contention
    T, P = 10, 700
    rng = np.random.default_rng(3)
    pts = np.zeros((2, P, 4), f32)
    pts[:, :, :2] = rng.uniform(0.51, 0.99, (2, P, 2))
    pts[:, :, 3] = np.arange(2 * P, dtype=f32).reshape(2, P)
    kw = dict(max_points=T, max_voxels=7, **PILLARS)
    got = run(pts, (P, P - 13), dev, **kw)
    check_equal(got, definition(pts, (P, P - 13), **kw), "one voxel")
    assert got.voxel_counts.tolist() == [1, 1] and got.num_points[:, 0].tolist() == [T, T]
    assert got.voxels[0, 0, :, 3].tolist() == list(range(T)) and bool((got.point_voxel[0] == 0).all())
    # every point in a voxel of its own and more of them than V: every refusal
    side = 40
    xy = (np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2) * 0.125 - 3.9375).astype(f32)
    pts = np.zeros((1, side * side, 3), f32)
    pts[0, :, :2] = xy[np.random.default_rng(4).permutation(side * side)]
    kw = dict(max_points=3, max_voxels=1000, **FINE)
    got = run(pts, (side * side,), dev, **kw)
    check_equal(got, definition(pts, (side * side,), **kw), "distinct voxels")
    assert int(got.voxel_counts[0]) == 1000 and int((got.point_voxel[0] == -1).sum()) == side * side - 1000
    assert got.point_voxel[0, :1000].tolist() == list(range(1000))
    # points of an accepted voxel that arrive after V is reached are still stored: mmcv's `continue`
    pts = random_points(5, (900,), 4)
    kw = dict(max_points=10, max_voxels=50, **PILLARS)
    want, stop = definition(pts, (900,), **kw), definition(pts, (900,), stop_when_full=True, **kw)
    assert not np.array_equal(want["num_points"], stop["num_points"]) and not np.array_equal(want["point_voxel"], stop["point_voxel"])
    check_equal(run(pts, (900,), dev, **kw), want, "late points of accepted voxels")


def check_table_pressure(dev):
    """the smallest legal table (one slot more than points: probe chains through most of it), the default and 8 x the
    default give the same bits; so do two consecutive calls; no input is modified"""
    P = 1023
    sizes = (P, 600, P)
    pts = random_points(7, sizes, 4, P=P, spread=3.99)
    pts[:, :, 2] = 0.0          # every point in range: about 900 keys in the 1024 slots of the smallest table
    kw = dict(max_points=2, max_voxels=600, **FINE)
    want = definition(pts, sizes, **kw)
    assert int(want["voxel_counts"][0]) == 600 and 400 < int(want["voxel_counts"][1]) < 600
    assert int(definition(pts, sizes, **dict(kw, max_voxels=1024))["voxel_counts"][0]) > 850
    for slots in (1024, 0, 2048, 8 * 2048):
        check_equal(run(pts, sizes, dev, _table_slots=slots, **kw), want, f"table_slots {slots}")
    rb = ragged(pts, sizes, dev)
    aug = torch.from_numpy(rows(1, 3)).to(dev)
    before = (rb.tensor.clone(), rb.sample_sizes.clone(), aug.clone())
    one = voxelize_points(rb, augmentation=aug, return_point_voxel=True, **kw)
    two = voxelize_points(rb, augmentation=aug, return_point_voxel=True, **kw)
    check_equal(one, two, "second call")
    assert not one.voxels.requires_grad
    for now, then in zip((rb.tensor, rb.sample_sizes, aug), before):
        assert torch.equal(bits_of(now), bits_of(then))
    none = voxelize_points(rb, augmentation=aug, **kw)
    assert none.point_voxel is None and torch.equal(bits_of(none.voxels), bits_of(one.voxels))


def check_hand_placed(dev):
    nan, inf = np.nan, np.inf
    lo, hi = f32(-4.0), f32(4.0)
    up, down = (lambda v: np.nextafter(f32(v), f32(inf))), (lambda v: np.nextafter(f32(v), f32(-inf)))
    near = lambda v: down(down(v))        # noqa: E731  (two ulp inside hi: the last value whose distance from lo is not rounded up)
    assert near(hi) - lo == down(hi - lo) and near(2.0) + f32(2.0) == down(f32(4.0)) and down(hi) - lo == hi - lo
    xyz = [(lo, 0.1, 0.0),              # 0: exactly on lo_x: in, cell x = 0
           (hi, 0.1, 0.0),              # 1: exactly on hi_x: out
           (near(hi), 0.1, 0.0),        # 2: the largest x whose x - lo_x is below hi_x - lo_x: in, cell x = 15
           (down(lo), 0.1, 0.0),        # 3: one ulp outside lo_x: out
           (up(lo), 0.1, 0.0),          # 4: one ulp inside lo_x: the voxel of point 0
           (0.1, lo, 0.0), (0.1, hi, 0.0), (0.1, near(hi), 0.0),            # 5 in, 6 out, 7 in: the same along y
           (0.6, 0.6, -2.0), (0.6, 0.6, 2.0), (0.6, 0.6, near(2.0)),        # 8 in, 9 out, 10 in (the voxel of 8): along z
           (nan, 0.1, 0.0), (0.1, nan, 0.0), (0.1, 0.1, nan),               # 11..13: dropped
           (inf, 0.1, 0.0), (0.1, -inf, 0.0), (0.1, 0.1, inf), (-inf, 0.1, 0.0),   # 14..17: dropped
           (-0.0, -0.0, -0.0),          # 18: cell (8, 8), stored with its sign bits
           (0.0, 0.0, 0.0),             # 19: the same voxel, other bits
           (1.3, 1.3, 0.5), (1.3, 1.3, 0.5), (1.3, 1.3, 0.5),               # 20..22: duplicates, all stored
           (2.3, 2.3, 0.5),             # 23: NaN in its passthrough channel: kept, payload preserved
           (down(hi), 0.1, 0.0)]        # 24: one ulp inside hi_x: OUT, as x - lo_x rounds to hi_x - lo_x (float32, as in mmcv)
    n = len(xyz)
    pts = np.zeros((1, n + 3, 5), f32)
    pts[0, :n, :3] = np.asarray(xyz, f32)
    pts[0, :, 3] = np.arange(n + 3)
    pts.view(np.uint32)[0, 23, 4] = 0x7FC0BEEF
    pts[0, n:, :3] = [(3.1, 3.1, 0.0), (3.2, -3.1, 0.0), (-3.1, 3.1, 0.0)]        # beyond sample_sizes, in range: never read
    kw = dict(max_points=4, max_voxels=32, **PILLARS)
    got = run(pts, (n,), dev, **kw)
    check_equal(got, definition(pts, (n,), **kw), "hand-placed")
    pv = got.point_voxel[0].tolist()
    dropped = {1, 3, 6, 9, 24} | set(range(11, 18)) | {n, n + 1, n + 2}
    assert {i for i, v in enumerate(pv) if v == -1} == dropped, pv
    assert pv[4] == pv[0] and pv[10] == pv[8] and pv[19] == pv[18] and pv[20] == pv[21] == pv[22]
    assert got.coors[0, pv[0]].tolist() == [0, 8, 0] and got.coors[0, pv[2]].tolist() == [0, 8, 15]
    assert got.coors[0, pv[5]].tolist() == [0, 0, 8] and got.coors[0, pv[7]].tolist() == [0, 15, 8]
    assert got.coors[0, pv[18]].tolist() == [0, 8, 8] and int(got.num_points[0, pv[20]]) == 3
    v = bits_of(got.voxels)[0]
    assert v[pv[18], 0, :3].tolist() == [-2 ** 31] * 3 and v[pv[18], 1, :3].tolist() == [0, 0, 0]
    assert int(v[pv[23], 0, 4]) == 0x7FC0BEEF
    # sizes above P and below 0 are clamped
    pts = random_points(9, (300, 300), 4)
    kw = dict(max_points=3, max_voxels=100, **PILLARS)
    check_equal(run(pts, (10 ** 6, -5), dev, **kw), definition(pts, (300, 0), **kw), "clamped sizes")


def check_augmentation(dev):
    sizes = (700, 0, 1500)
    for D, grid in ((4, PILLARS), (5, VOXELS3D)):
        pts = random_points(20 + D, sizes, D)
        r = rows(D, 3)
        kw = dict(max_points=5, max_voxels=200, **grid)
        inside = run(pts, sizes, dev, augmentation=r, **kw)
        check_equal(inside, definition(pts, sizes, augmentation=r, **kw), "rows inside")
        check_equal(inside, run(augment(r, pts), sizes, dev, **kw), "rows inside against augmented points")
        plain = run(pts, sizes, dev, **kw)
        assert not torch.equal(inside.coors, plain.coors)
        check_equal(run(pts, sizes, dev, augmentation=np.stack([IDENTITY_ROW] * 3), **kw), plain, "identity rows")


def check_concatenate(dev):
    sizes = (100, 0, 1500)
    pts = random_points(31, sizes, 5)
    vox = run(pts, sizes, dev, max_points=3, max_voxels=150, **VOXELS3D)
    counts = vox.voxel_counts.tolist()
    assert counts[1] == 0 and counts[0] < 150 == counts[2]
    voxels, coors, num = concatenate_voxels(vox)
    want_c = torch.cat([torch.cat([torch.full((n, 1), b, dtype=torch.int32, device=vox.coors.device), vox.coors[b, :n]], dim=1)
                        for b, n in enumerate(counts)])
    assert torch.equal(bits_of(voxels), bits_of(torch.cat([vox.voxels[b, :n] for b, n in enumerate(counts)])))
    assert torch.equal(coors, want_c) and coors.dtype == torch.int32 and tuple(coors.shape) == (sum(counts), 4)
    assert torch.equal(num, torch.cat([vox.num_points[b, :n] for b, n in enumerate(counts)])) and num.dtype == torch.int32
    for rb, t in zip(vox.ragged(), (vox.voxels, vox.coors, vox.num_points)):
        assert rb.tensor is t and rb.sample_sizes is vox.voxel_counts
    empty = run(np.zeros((2, 4, 3), f32), (0, 0), dev, max_points=3, max_voxels=5, **PILLARS)
    assert [tuple(t.shape) for t in concatenate_voxels(empty)] == [(0, 3, 3), (0, 4), (0,)]


def check_empty(dev):
    kw = dict(max_points=3, max_voxels=5, **PILLARS)
    got = voxelize_points(RaggedBatch(torch.zeros((0, 6, 4), device=dev), sample_sizes=torch.zeros((0,), dtype=torch.int64, device=dev)),
                          return_point_voxel=True, **kw)
    assert [tuple(t.shape) for t in got] == [(0, 5, 3, 4), (0, 5, 3), (0, 5), (0,), (0, 6)]
    for P in (0, 9):       # P == 0, and slots that no frame uses: all padding is still written
        rb = RaggedBatch(torch.full((2, P, 4), 0.25, device=dev), sample_sizes=torch.zeros((2,), dtype=torch.int32, device=dev))
        got = voxelize_points(rb, return_point_voxel=True, **kw)
        check_equal(got, definition(np.full((2, P, 4), 0.25, f32), (0, 0), **kw), f"P {P}, sizes 0")
        assert not bits_of(got.voxels).any() and bool((got.coors == -1).all()) and not got.num_points.any()


def misaligned_points(dev):
    """D == 4 with the first point 4 bytes off a 16-byte boundary: 4-byte loads and stores"""
    sizes = (300, 77)
    pts = random_points(41, sizes, 4)
    flat = torch.zeros(pts.size + 1, dtype=torch.float32, device=dev)
    view = flat[1:].view(pts.shape)
    view.copy_(torch.from_numpy(pts))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    kw = dict(max_points=3, max_voxels=100, **PILLARS)
    got = voxelize_points(RaggedBatch(view, sample_sizes=torch.tensor(sizes, device=dev)), return_point_voxel=True, **kw)
    check_equal(got, definition(pts, sizes, **kw), "misaligned points")


def check_guard_bands(dev):
    """the C entry alone writes all of the five outputs and nothing outside them, nor outside its workspace, for 16-byte rows
    (D = 4, everything aligned) and 4-byte rows (D = 5)"""
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    cuda = torch.device(dev).type == "cuda"
    sizes, T, V, pad = (700, 1500), 3, 120, 512
    for D in (4, 5):
        pts = random_points(50 + D, sizes, D)
        rb = ragged(pts, sizes, dev)
        B, P = 2, rb.tensor.shape[1]
        shapes = dict(voxels=(B, V, T, D), coors=(B, V, 3), num_points=(B, V), voxel_counts=(B,), point_voxel=(B, P))
        bufs, outs = {}, {}
        for name, shape in shapes.items():
            nbytes = 4 * int(np.prod(shape))
            bufs[name] = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
            outs[name] = bufs[name][pad: pad + nbytes].view(torch.float32 if name == "voxels" else torch.int32).view(shape)
        p = nat.VoxelizeParams()
        p.points, p.sample_sizes, p.sizes_i64 = rb.tensor.data_ptr(), rb.sample_sizes.data_ptr(), 1
        p.voxel_size[:], p.range_min[:], p.range_max[:] = VOXELS3D["voxel_size"], RANGE[:3], RANGE[3:]
        p.max_points, p.max_voxels = T, V
        args = (ctypes.addressof(p), B, P, D) + tuple(outs[name].data_ptr() for name in FIELDS)
        if cuda:
            need = lib.accv_voxelize_workspace_bytes(B, P, V, T, 0)
            assert need > 0 and need % 16 == 0
            bufs["workspace"] = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device=dev)
            ws = bufs["workspace"].data_ptr() + pad
            stream = nat.stream_ptr(torch.device(dev, torch.cuda.current_device()))
            assert lib.accv_voxelize(*args, ws, need - 1, stream) == -3, "a workspace one byte short is ACCV_EWORKSPACE"
            assert lib.accv_voxelize(*args, ws + 4, need, stream) == -3, "a workspace off a 16-byte boundary is ACCV_EWORKSPACE"
            for name in FIELDS:
                assert bool((bufs[name] == 0xA5).all()), "a refused call wrote"
            status = lib.accv_voxelize(*args, ws, need, stream)
            torch.cuda.synchronize()
        else:
            status = lib.accv_voxelize_cpu(*args)
        assert status == 0, lib.accv_last_error()
        for name, buf in bufs.items():
            inner = buf.numel() - 2 * pad
            assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + inner:] == 0xA5).all()), f"wrote outside {name}"
        # the sentinel inside is gone wherever the definition has a value, which is everywhere
        check_equal(Voxels(**{name: outs[name].clone() for name in FIELDS}),
                    definition(pts, sizes, max_points=T, max_voxels=V, **VOXELS3D), f"banded D {D}")


def check_errors(dev, other_dev=None):
    """every documented error is raised by the Python layer, before a launch"""
    import pytest

    sizes = (20, 30)
    pts = random_points(61, sizes, 4)
    good = dict(max_points=3, max_voxels=50, **PILLARS)
    rb = lambda: ragged(pts, sizes, dev)                                                # noqa: E731
    call = lambda p=None, **kw: voxelize_points(p if p is not None else rb(), **dict(good, **kw))        # noqa: E731
    call()
    with pytest.raises(TypeError, match="float32"):
        call(p=RaggedBatch(rb().tensor.double(), sample_sizes=rb().sample_sizes))
    with pytest.raises(TypeError, match="float32"):
        call(augmentation=torch.zeros((2, 7), dtype=torch.float16, device=dev))
    for bad in (torch.zeros((2, 30, 2), device=dev), torch.zeros((2, 30, 17), device=dev), torch.zeros((2, 30), device=dev),
                torch.zeros((2, 30, 4), dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match="points"):
            call(p=RaggedBatch(bad, sample_sizes=torch.tensor([20, 30], device=dev)))
    with pytest.raises(RuntimeError, match="points"):
        call(p=rb().tensor)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(p=RaggedBatch(torch.zeros((2, 30, 8), device=dev)[:, :, :4], sample_sizes=torch.tensor([20, 30], device=dev)))
    with pytest.raises(RuntimeError, match="sample_sizes"):
        call(p=RaggedBatch(rb().tensor, sample_sizes=torch.tensor([20, 30], dtype=torch.int16, device=dev)))
    for bad in (0, 129, 3.0, True):
        with pytest.raises(RuntimeError, match="max_points"):
            call(max_points=bad)
    for bad in (0, 2 ** 20 + 1, 50.0):
        with pytest.raises(RuntimeError, match="max_voxels"):
            call(max_voxels=bad)
    call(max_points=128, max_voxels=2)
    for bad in ((0.5, 0.5), (0.5, 0.0, 4.0), (0.5, -0.5, 4.0), (0.5, float("nan"), 4.0), (0.5, float("inf"), 4.0), (1e-60, 0.5, 4.0),
                (0.5, 0.5, "4"), 0.5):
        with pytest.raises(RuntimeError, match="voxel_size"):
            call(voxel_size=bad)
    for bad in ((-4.0, -4.0, -2.0, 4.0, 4.0), (4.0, -4.0, -2.0, -4.0, 4.0, 2.0), (-4.0, -4.0, 2.0, 4.0, 4.0, 2.0),
                (-4.0, float("nan"), -2.0, 4.0, 4.0, 2.0), (-4.0, -4.0, -2.0, float("inf"), 4.0, 2.0)):
        with pytest.raises(RuntimeError, match="point_cloud_range"):
            call(point_cloud_range=bad)
    with pytest.raises(RuntimeError, match="grid"):      # 0.4 cells along z rounds to none
        call(voxel_size=(0.5, 0.5, 10.0))
    with pytest.raises(RuntimeError, match="grid"):      # 2^32 cells along x
        call(voxel_size=(2.0 ** -29, 0.5, 4.0))
    with pytest.raises(RuntimeError, match="2\\^31"):    # 2048 x 1024 x 1024 cells = 2^31
        call(voxel_size=(2.0 ** -8, 2.0 ** -7, 2.0 ** -8))
    call(voxel_size=(2.0 ** -8, 2.0 ** -7, 2.0 ** -7))   # 2^30
    for bad in (torch.zeros((2, 6), device=dev), torch.zeros((3, 7), device=dev), torch.zeros((2, 7, 1), device=dev)):
        with pytest.raises(RuntimeError, match="augmentation"):
            call(augmentation=bad)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(augmentation=torch.zeros((7, 2), device=dev).t())
    for bad in (16, 30, 48, 2 ** 32, -64, 64.0):         # P = 30: not above P, no power of two, too large, no int
        with pytest.raises(RuntimeError, match="_table_slots"):
            call(_table_slots=bad)
    call(_table_slots=32)
    if other_dev is not None:
        with pytest.raises(RuntimeError, match="device"):
            call(augmentation=torch.zeros((2, 7), device=other_dev))
        with pytest.raises(RuntimeError, match="device"):
            call(p=RaggedBatch(rb().tensor, sample_sizes=rb().sample_sizes.to(other_dev)))


# ------------------------------------------------------------------- the launch regimes of the device's work partition
# Each check below enters a regime of csrc/voxelize.hip that the checks above leave alone, and asserts through the
# definition alone that it does: a seed edited later cannot quietly empty the case.
WAVE = 64


def cell_centres(cells, side, cell):
    """float32 [n, 2]: the centres of the cells (index c_y * side + c_x) of a side x side grid over RANGE; exact in float32"""
    cells = np.asarray(cells)
    return ((np.stack([cells % side, cells // side], axis=1) + 0.5) * cell - 4.0).astype(f32)


@functools.lru_cache(maxsize=None)
def many_chunks_case(chunks, scan_points, seed):
    """one frame of chunks * scan_points + 1 points in which few points open a voxel, so that the voxel number of an opener
    is the prefix over the chunks before its own: about 70 % of the points are out of range (z = 5), the others sit in 8
    pillars of row 0 of FINE that the frame's first 8 points open, but for k_c in {0, 1, 2, 3} points of chunk c and the
    single point of the last chunk, each alone in a cell of rows 1..63.  max_voxels refuses the last five of them; `free`
    is the definition of the same frame with room for all.
    Returns (points, sizes, kw, want, free, openers per chunk): built once for both test files, never written to"""
    rng = np.random.default_rng(seed)
    P = chunks * scan_points + 1
    k = rng.integers(0, 4, chunks + 1)
    k[-1] = 1
    total = int(k.sum())
    assert total <= 63 * 64, "more openers than cells in rows 1..63"
    pts = np.zeros((1, P, 3), f32)
    pts[0, :, :2] = cell_centres(rng.integers(0, 8, P), 64, 0.125)
    pts[0, :, 2] = np.where(rng.random(P) < 0.7, f32(5.0), f32(0.0))
    pts[0, :8, :2], pts[0, :8, 2] = cell_centres(np.arange(8), 64, 0.125), 0.0
    where = np.concatenate([c * scan_points + 8 + np.sort(rng.choice(scan_points - 8, int(k[c]), replace=False)) for c in range(chunks)]
                           + [np.array([P - 1])]).astype(np.int64)
    pts[0, where, :2], pts[0, where, 2] = cell_centres(64 + rng.permutation(63 * 64)[:total], 64, 0.125), 0.0
    kw = dict(max_points=3, max_voxels=total + 8 - 5, **FINE)
    want, free = definition(pts, (P,), **kw), definition(pts, (P,), **dict(kw, max_voxels=total + 8))
    # the case is what its comment says, by the definition alone
    pv, pv_free = want["point_voxel"][0], free["point_voxel"][0]
    assert int(free["voxel_counts"][0]) == total + 8 and int(want["voxel_counts"][0]) == total + 3
    assert np.array_equal(pv_free[where], 8 + np.arange(total)), "an opener's number is not 8 + the openers before it"
    assert np.array_equal(pv[where[:-5]], 8 + np.arange(total - 5)) and (pv[where[-5:]] == -1).all()
    refused = np.flatnonzero((pv_free >= 0) & (pv < 0))
    assert refused.size == 5 and (refused // scan_points >= chunks - 4).all(), "the refusals are not five points of the last chunks"
    per_chunk = np.bincount(where // scan_points, minlength=chunks + 1)
    assert np.array_equal(per_chunk, k) and (k == 0).any() and (k == 3).any()
    return pts, (P,), kw, want, free, per_chunk


MANY_CHUNKS_SEEDS = {130: 1, 1025: 5}


def check_many_chunks(dev, chunks, scan_threads, unroll):
    """the numbering workgroup's sum over the chunks before its own: lane i reads the counts of chunks i, i + scan_threads,
    ...; a wave's lanes are added by shuffles and the waves' sums through LDS.  With more than 2 * 64 chunks in front of
    the last workgroup waves 1 and 2 carry a value; with more than scan_threads, lane 0 takes a second trip.

    Only the last workgroup (one point, the last opener) reads the count of chunk scan_threads, and a chunk opens at most 3
    voxels: with the last five openers refused, a sum that misses that count still refuses the last opener and still
    reports max_voxels voxels.  So the frame is also run with room for every voxel, where the last opener's number and
    voxel_counts are the whole sum"""
    pts, sizes, kw, want, free, per_chunk = many_chunks_case(chunks, scan_threads * unroll, MANY_CHUNKS_SEEDS[chunks])
    assert chunks > 2 * WAVE
    for w in range(1, -(-chunks // WAVE)):
        if w * WAVE < scan_threads:
            assert per_chunk[w * WAVE: min((w + 1) * WAVE, chunks, scan_threads)].sum() > 0, f"wave {w} of the last workgroup carries nothing"
    if chunks > scan_threads:        # the counts that only a second trip reads: those of chunks scan_threads .. chunks - 1
        assert per_chunk[scan_threads: chunks].sum() > 0 and per_chunk[scan_threads:].sum() > 1, "the second trip carries nothing"
    check_equal(run(pts, sizes, dev, **kw), want, f"{chunks} chunks")
    roomy = dict(kw, max_voxels=int(free["voxel_counts"][0]))
    assert roomy["max_voxels"] == kw["max_voxels"] + 5 == 8 + int(per_chunk.sum())
    check_equal(run(pts, sizes, dev, **roomy), free, f"{chunks} chunks, room for all")


LIST_FILL_SIZES = (1500, 0, 700)


def list_fill_cases(list_words, fill_blocks_max):
    """(V, T) with more than one list-filling workgroup a frame (list_words index words each), and the workgroups each takes"""
    out = [(list_words // 3 + 1, 3), (list_words + 1, 1), (2 * list_words // 128 + 1, 128)]
    blocks = [-(-V * T // list_words) for V, T in out]
    B = len(LIST_FILL_SIZES)
    assert blocks == [2, 2, 3] and max(blocks) < fill_blocks_max and [B * V * T % 4 for V, T in out] == [2, 3, 0]
    return out


def list_fill_points(seed, V, T):
    pts = random_points(seed, LIST_FILL_SIZES, 5)
    kw = dict(max_points=T, max_voxels=V, **FINE)
    want = definition(pts, LIST_FILL_SIZES, **kw)
    counts = want["voxel_counts"].tolist()
    assert 800 < counts[0] < min(V, 1000) and counts[1] == 0 and 400 < counts[2] < 500, counts
    assert 4 * int(want["num_points"].sum()) < V * T, "most list words are not left empty"
    return pts, kw, want


def check_padding(got, sizes):
    """the padding of every output, spelled out: rows from num_points on are +0.0, voxels from voxel_counts on have +0.0
    rows, coors of -1 and no points, points from sample_sizes on have no voxel"""
    voxels, coors, num = bits_of(got.voxels), got.coors.cpu(), got.num_points.cpu()
    B, V, T, _ = voxels.shape
    for b, n in enumerate(got.voxel_counts.tolist()):
        assert not voxels[b, n:].any() and bool((coors[b, n:] == -1).all()) and not num[b, n:].any(), f"padding of frame {b}"
        assert bool((coors[b, :n] >= 0).all()) and bool((num[b, :n] >= 1).all())
        assert bool((got.point_voxel[b, sizes[b]:] == -1).all())
    beyond = torch.arange(T).view(1, 1, T) >= num.view(B, V, 1)
    assert not voxels[beyond].any(), "a row from num_points on is not +0.0"


def check_list_fill(dev, list_words, fill_blocks_max):
    """V * T above the index words one list-filling workgroup takes: two and three of them a frame, dealt over all frames'
    lists as one range, with the 4-byte tail of that range (B * V * T no multiple of 4)"""
    for n, (V, T) in enumerate(list_fill_cases(list_words, fill_blocks_max)):
        pts, kw, want = list_fill_points(300 + n, V, T)
        got = run(pts, LIST_FILL_SIZES, dev, **kw)
        check_equal(got, want, f"V {V}, T {T}")
        check_padding(got, LIST_FILL_SIZES)


def check_list_fill_workspace(dev, list_words, fill_blocks_max):
    """the same through the C entry alone, twice into one workspace of the test's own that starts as zero bytes: a list word
    that the fill leaves out then reads as point 0, a valid index, and shows as a mismatch; the second call (other points)
    finds the lists of the first"""
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    assert torch.device(dev).type == "cuda"
    B, D = len(LIST_FILL_SIZES), 5
    for n, (V, T) in enumerate(list_fill_cases(list_words, fill_blocks_max)):
        P = max(LIST_FILL_SIZES)
        need = lib.accv_voxelize_workspace_bytes(B, P, V, T, 0)
        assert need > 0 and need % 16 == 0
        workspace = torch.zeros((need,), dtype=torch.uint8, device=dev)
        assert workspace.data_ptr() % 16 == 0
        stream = nat.stream_ptr(torch.device(dev, torch.cuda.current_device()))
        for call, seed in enumerate((300 + n, 310 + n)):
            pts, kw, want = list_fill_points(seed, V, T)
            rb = ragged(pts, LIST_FILL_SIZES, dev)
            shapes = dict(voxels=(B, V, T, D), coors=(B, V, 3), num_points=(B, V), voxel_counts=(B,), point_voxel=(B, P))
            outs = {name: torch.full((4 * int(np.prod(shape)),), 0xA5, dtype=torch.uint8, device=dev)
                    .view(torch.float32 if name == "voxels" else torch.int32).view(shape) for name, shape in shapes.items()}
            p = nat.VoxelizeParams()
            p.points, p.sample_sizes, p.sizes_i64 = rb.tensor.data_ptr(), rb.sample_sizes.data_ptr(), 1
            p.voxel_size[:], p.range_min[:], p.range_max[:] = FINE["voxel_size"], RANGE[:3], RANGE[3:]
            p.max_points, p.max_voxels = T, V
            status = lib.accv_voxelize(ctypes.addressof(p), B, P, D, *(outs[name].data_ptr() for name in FIELDS),
                                       workspace.data_ptr(), need, stream)
            torch.cuda.synchronize()
            assert status == 0, lib.accv_last_error()
            got = Voxels(**outs)
            check_equal(got, want, f"V {V}, T {T}, call {call} into a workspace of zero bytes")
            check_padding(got, LIST_FILL_SIZES)


def check_budget_crossings(dev, unroll, scan_points):
    """max_voxels reached inside a lane's `unroll` consecutive points, between two lanes, between two waves and between
    two chunks of the numbering launch: every point of frame 0 opens a voxel, so voxel V is refused at point V"""
    side, extra = 128, 300
    P = scan_points + extra
    rng = np.random.default_rng(12)
    pts = np.zeros((2, P, 3), f32)
    pts[0, :, :2] = cell_centres(rng.permutation(side * side)[:P], side, 0.0625)
    pts[1, :extra, :2] = cell_centres(rng.permutation(side * side)[:extra], side, 0.0625)
    sizes = (P, extra)
    budgets = sorted(set(range(1, unroll + 2)) | {n + d for n in (WAVE * unroll, scan_points) for d in (-1, 0, 1)})
    assert len(budgets) == unroll + 7 and budgets[-1] < P
    for V in budgets:
        kw = dict(max_points=1, max_voxels=V, voxel_size=(0.0625, 0.0625, 4.0), point_cloud_range=RANGE)
        want = definition(pts, sizes, **kw)
        assert want["voxel_counts"].tolist() == [V, min(V, extra)]
        assert np.array_equal(want["point_voxel"][0, :V], np.arange(V)) and (want["point_voxel"][0, V:] == -1).all()
        check_equal(run(pts, sizes, dev, **kw), want, f"max_voxels {V}")


def check_point_budget(dev, T):
    """voxels that receive T - 1, T, T + 1 and 8 T points and one point, interleaved, in one frame and in its reverse: the
    end of the rank cascade and the rule that finds a voxel's last row"""
    groups = ([T - 1] if T > 1 else []) + [T, T + 1, 8 * T, 1]
    rng = np.random.default_rng(40 + T)
    label = rng.permutation(np.repeat(np.arange(len(groups)), groups))
    P = label.size
    cells = rng.permutation(256)[:len(groups)]
    pts = np.zeros((2, P, 4), f32)
    pts[0, :, :2] = cell_centres(cells[label], 16, 0.5) + rng.uniform(-0.2, 0.2, (P, 2)).astype(f32)
    pts[0, :, 2] = rng.uniform(-1.9, 1.9, P)
    pts[1] = pts[0, ::-1]
    pts[:, :, 3] = np.arange(P)
    kw = dict(max_points=T, max_voxels=2 * len(groups), **PILLARS)
    want = definition(pts, (P, P), **kw)
    assert want["voxel_counts"].tolist() == [len(groups)] * 2
    for b, lab in enumerate((label, label[::-1])):
        for g, n in enumerate(groups):
            idx = np.flatnonzero(lab == g)
            assert idx.size == n and (n < 2 or int(np.diff(idx).max()) > 1), "the points of a voxel are contiguous"
            v = int(want["point_voxel"][b, idx[0]])
            kept = min(n, T)
            assert v >= 0 and (want["point_voxel"][b, idx] == v).all(), "a point beyond max_points lost its voxel"
            assert int(want["num_points"][b, v]) == kept
            assert want["voxels"][b, v, :kept, 3].tolist() == idx[:kept].tolist(), "not the T lowest indices in ascending order"
            assert not want["voxels"][b, v, kept:].view(np.uint32).any()
    check_equal(run(pts, (P, P), dev, **kw), want, f"max_points {T}")


def run_misaligned(pts, sizes, dev, augmentation=None, **kw):
    """`run` with the first point 4 bytes off a 16-byte boundary"""
    flat = torch.zeros(pts.size + 1, dtype=torch.float32, device=dev)
    view = flat[1:].view(pts.shape)
    view.copy_(torch.from_numpy(pts))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    aug = None if augmentation is None else torch.from_numpy(np.asarray(augmentation, f32)).to(dev)
    return voxelize_points(RaggedBatch(view, sample_sizes=torch.tensor(sizes, device=dev)), augmentation=aug, return_point_voxel=True, **kw)


def check_row_widths(dev, D):
    """rows of 6, 8, 12, 15 and 16 channels, with and without augmentation rows; the multiples of 4 also off a 16-byte
    boundary, where the gather goes element by element"""
    sizes = (700, 257)
    pts = random_points(500 + D, sizes, D)
    kw = dict(max_points=3, max_voxels=150, **VOXELS3D)
    for aug in (None, rows(D, 2)):
        what = f"D {D}, {'rows' if aug is not None else 'no rows'}"
        want = definition(pts, sizes, augmentation=aug, **kw)
        assert int(want["voxel_counts"][0]) == 150 and 100 < int(want["voxel_counts"][1]) <= 150
        stored = want["voxels"][want["num_points"] > 0][:, 0]
        assert np.isnan(stored[:, -1]).any() and np.isnan(stored[:, 3]).any(), "no NaN payload rides in a stored row's last channel"
        check_equal(run(pts, sizes, dev, augmentation=aug, **kw), want, what)
        if D % 4 == 0:
            check_equal(run_misaligned(pts, sizes, dev, augmentation=aug, **kw), want, what + ", misaligned")


def check_large_keys(dev):
    """a grid of 2^30 cells (2048 x 1024 x 512): keys, probe starts and coors near the largest key"""
    kw = dict(max_points=3, max_voxels=2000, voxel_size=(2.0 ** -8, 2.0 ** -7, 2.0 ** -7), point_cloud_range=RANGE)
    rng = np.random.default_rng(60)
    sizes = (1500,)
    pts = random_points(61, sizes, 4, spread=4.2)
    pts[0, :, 2] = rng.uniform(-2.1, 2.1, 1500)
    pts[0, :40, :3] = np.array([4.0, 4.0, 2.0]) - rng.uniform(0.0, 0.02, (40, 3))
    pts[0, 0, :3] = (4.0 - 2.0 ** -9, 4.0 - 2.0 ** -8, 2.0 - 2.0 ** -8)        # the centre of the last cell
    want = definition(pts, sizes, **kw)
    n = int(want["voxel_counts"][0])
    c = want["coors"][0, :n].astype(np.int64)
    keys = (c[:, 0] * 1024 + c[:, 1]) * 2048 + c[:, 2]
    assert 1000 < n < 1500 and tuple(c.max(0)) == (511, 1023, 2047)
    assert int(keys.max()) == 2 ** 30 - 1 and int((keys > 2 ** 29).sum()) > 100 and int(np.unique(keys).size) == n
    check_equal(run(pts, sizes, dev, **kw), want, "2^30 cells")


@functools.lru_cache(maxsize=None)
def most_frames_case():
    B = 65535
    sizes = np.random.default_rng(70).integers(0, 3, B)
    pts = random_points(71, (2,) * B, 3, spread=4.2)
    kw = dict(max_points=1, max_voxels=2, **PILLARS)
    want = definition(pts, sizes, **kw)
    assert sorted(np.unique(want["voxel_counts"]).tolist()) == [0, 1, 2] and int(want["voxel_counts"][-1]) > 0
    assert sorted(np.unique(sizes).tolist()) == [0, 1, 2]
    return pts, sizes, kw, want


def check_most_frames(dev):
    """B = 65535 frames, the most a launch takes in its grid's y extent"""
    pts, sizes, kw, want = most_frames_case()
    check_equal(run(pts, sizes, dev, **kw), want, "65535 frames")
