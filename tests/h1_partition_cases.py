"""Inputs at the edges of the heat-map rasteriser's own work partition, shared by test_h1_partition_edges_cpu.py (regime
assertions, the oracle's sensitivity to every named hit, the host rules) and test_h1_partition_edges_gpu.py (the kernels).
DESIGN.md §9r has the table.  Every shape is derived from a constant read from the source text of the rasteriser
(`csrc/draw_heatmap.hip`, `splat_common.h`, `splat_small.h`, `heatmap_prep.h`) or of `accvlab/draw_heatmap/ops.py`; no
shape and no input is random.

A case proves from outside that it is in the regime it names.  The cull of the tile kernels is restated here in numpy
(`cull`, the rule of `cull_test`; `clipped_boxes`, the box of `make_hit`), so that a case can count the hits of a tile per
cull round of `kCand` candidates, the height of the tallest clipped box of a round (the small-splat kernel's `rows_hint`)
and the box a hit packs into `Hit::box`; `expected_dispatch` restates `dispatch_splat` / `launch_splat`, and the GPU tests
compare it with what `accv_draw_heatmap_last_dispatch` reports (kernel, PX, R, CLEAR, SM, grid, block)."""
import math
import os
import re
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "accv-lab_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _constant(text, ident):
    """the initialiser of `constexpr <type> ... ident = value` (also the second name of one declaration)"""
    return re.search(rf"\b{ident} = ([^,;]+)[,;]", text).group(1).strip()


def _int(expr):
    if "<<" in expr:
        a, b = expr.split("<<")
        return int(a) << int(b)
    return int(expr)


_HIP = _read(_CSRC, "draw_heatmap.hip")
_COMMON = _read(_CSRC, "splat_common.h")
_SMALL = _read(_CSRC, "splat_small.h")
_PREP = _read(_CSRC, "heatmap_prep.h")
_OPS = _read(ROOT, "accv-lab_amd", "accvlab", "draw_heatmap", "ops.py")

KCAND = _int(_constant(_COMMON, "kCand"))                       # candidates per cull round
WPG = _int(_constant(_COMMON, "kWavesPerGroup"))                # tile waves per workgroup of splat_kernel
MAX_SCALES = _int(_constant(_COMMON, "kMaxScales"))
BOX_TILE_R = _int(_constant(_COMMON, "kBoxTileR"))
STORE_PLAIN = _int(_constant(_COMMON, "kStorePlain"))
STORE_WT = _int(_constant(_COMMON, "kStoreWriteThrough"))
STORE_ADAPTIVE = _int(_constant(_COMMON, "kStoreAdaptive"))
CLAMP_XY = _int(re.search(r"kClampXY = ([^,;]+)[,;]", _COMMON).group(1))
CLAMP_R = _int(re.search(r"kClampR = ([^,;]+)[,;]", _COMMON).group(1))
SMALL_TW = _int(_constant(_SMALL, "kSmallTW"))
SMALL_TH = _int(_constant(_SMALL, "kSmallTH"))
SMALL_FETCH = _int(re.search(r"constexpr int kFetch = (\d+);\s+for \(int base = 0; base < t\.n", _SMALL).group(1))
BIN_SMALL_PLANES = _int(_constant(_PREP, "kBinSmallPlanes"))
BIN_SMALL_OBJECTS = _int(_constant(_PREP, "kBinSmallObjects"))
assert "num_planes <= kBinSmallPlanes && num_objects <= kBinSmallObjects" in _HIP      # the rule the binning cases sit around
# the 3-D grid is taken while planes and tile rows fit a grid dimension (both launchers state the same limits)
_g = set(re.findall(r"p\.grid3d = \(planes <= (\d+) && p\.tiles_y <= (\d+)\) \? 1 : 0;", _HIP))
assert len(_g) == 1
GRID_Z, GRID_Y = (int(v) for v in _g.pop())
# bin_count_kernel / bin_fill_kernel: min(ceil(N / threads), cap) workgroups, a grid-stride loop behind them
_m = re.search(r"min\(\(num_objects \+ (\d+)\) / (\d+), (\d+)\)", _HIP)
BIN_THREADS, BIN_GRID_CAP = int(_m.group(2)), int(_m.group(3))
assert int(_m.group(1)) == BIN_THREADS - 1
BIN_WG = _int(re.search(r"for \(int i = t; i < planes; i \+= (\d+)\) s_cnt\[i\] = 0;", _PREP).group(1))   # bin_small / bin_scan
# targets_from_*: min(ceil(n / 256), cap) workgroups
_t = set(re.findall(r"std::min<long long>\(\(num_\w+ \+ 255\) / 256, (\d+)\)", _HIP))
assert len(_t) == 1
TARGETS_GRID_CAP, TARGETS_THREADS = int(_t.pop()), 256
FLAT_DIRECT_MAX_OBJECTS = int(re.search(r"_FLAT_DIRECT_MAX_OBJECTS = ([\d_]+)", _OPS).group(1))
FLAT_DIRECT_MAX_ROUNDS = int(re.search(r"_FLAT_DIRECT_MAX_ROUNDS = ([\d_]+)", _OPS).group(1))
FLAT_DIRECT_MAX_PLANES = int(re.search(r"0 < planes <= (\d+)", _OPS).group(1))
assert (KCAND, WPG, SMALL_TW, SMALL_TH, GRID_Z, GRID_Y) == (64, 1, 128, 16, 65535, 65535)
assert FLAT_DIRECT_MAX_PLANES == GRID_Z


# ------------------------------------------------------------------------------------------- the cull, restated in numpy
def tile_bounds(tx, ty, TW, TH, H, W):
    """pixel bounds (tx0, ty0, tx1, ty1) of tile (tx, ty), clipped to the map: locate_tile"""
    return tx * TW, ty * TH, min(tx * TW + TW, W), min(ty * TH + TH, H)


def cull(centers, radii, n, tile, labels=None, cls=-1):
    """bool [N]: the objects of one plane that pass cull_test for `tile` (first `n` slots are valid)"""
    c, r = np.asarray(centers, dtype=np.int64).reshape(-1, 2), np.asarray(radii, dtype=np.int64).reshape(-1)
    tx0, ty0, tx1, ty1 = tile
    xc, yc = np.clip(c[:, 0], -CLAMP_XY, CLAMP_XY), np.clip(c[:, 1], -CLAMP_XY, CLAMP_XY)
    rc = np.minimum(r, CLAMP_R)
    hit = (np.arange(r.size) < n) & (r >= 0) & (xc - rc < tx1) & (xc + rc >= tx0) & (yc - rc < ty1) & (yc + rc >= ty0)
    if cls >= 0:
        hit &= np.asarray(labels, dtype=np.int64).reshape(-1) == cls
    return hit


def per_round(hit, rounds=None):
    """hits of every cull round of KCAND candidates"""
    rounds = -(-hit.size // KCAND) if rounds is None else rounds
    padded = np.zeros(rounds * KCAND, dtype=bool)
    padded[:hit.size] = hit
    return tuple(int(v) for v in padded.reshape(rounds, KCAND).sum(1))


def clipped_boxes(centers, radii, tile, H, W):
    """make_hit: columns [xlo, xhi) and rows [ylo, yhi) of the tile, int64 [N, 4]; an empty exact box is all zero"""
    c, r = np.asarray(centers, dtype=np.int64).reshape(-1, 2), np.asarray(radii, dtype=np.int64).reshape(-1)
    x, y = c[:, 0], c[:, 1]
    tx0, ty0, tx1, ty1 = tile
    x0, x1 = x - np.minimum(x, r), x + np.minimum(W - x, r + 1)
    y0, y1 = y - np.minimum(y, r), y + np.minimum(H - y, r + 1)
    box = np.stack([np.maximum(x0, tx0) - tx0, np.minimum(x1, tx1) - tx0, np.maximum(y0, ty0) - ty0, np.minimum(y1, ty1) - ty0], 1)
    box[(box[:, 1] <= box[:, 0]) | (box[:, 3] <= box[:, 2])] = 0
    return box


def tile_rounds(case, plane, tile_xy, TW, TH):
    """per-round hit counts of tile (tx, ty) of `plane`"""
    tile = tile_bounds(tile_xy[0], tile_xy[1], TW, TH, case.H, case.W)
    return per_round(cull(case.centers[plane], case.radii[plane], int(case.counts[plane]), tile))


def round_rows(case, plane, tile_xy, TW, TH, rnd=0):
    """(hits, tallest clipped box) of cull round `rnd` in a tile: what splat_round hands to walk_hits as (nh, rows_hint)"""
    tile = tile_bounds(tile_xy[0], tile_xy[1], TW, TH, case.H, case.W)
    hit = cull(case.centers[plane], case.radii[plane], int(case.counts[plane]), tile)
    hit[:rnd * KCAND] = False
    hit[(rnd + 1) * KCAND:] = False
    box = clipped_boxes(case.centers[plane], case.radii[plane], tile, case.H, case.W)[hit]
    return int(hit.sum()), max(1, int((box[:, 3] - box[:, 2]).max())) if len(box) else 1


# ------------------------------------------------------------------------------------------- the dispatch, restated
# every instantiation dispatch_splat can reach.  `odd`: the case is built with a width that is no multiple of 4 (PX == 1)
Variant = namedtuple("Variant", "name kernel PX R clear sm TW TH odd kwargs")


def _variants():
    out = []
    for rows in (8, 16):
        for clear, wt, sm in ((True, False, STORE_PLAIN), (True, True, STORE_WT), (False, False, STORE_PLAIN),
                              (False, True, STORE_WT), (False, None, STORE_ADAPTIVE)):
            out.append(Variant(f"px4_r{rows}_{'clear' if clear else 'inplace'}_sm{sm}", "splat_kernel", 4, rows, clear, sm, 128,
                               2 * rows, False, dict(tile_rows=rows, write_through=wt)))
    for clear in (True, False):   # PX == 1 has plain stores and R == 8, whatever the hints say
        out.append(Variant(f"px1_{'clear' if clear else 'inplace'}", "splat_kernel", 1, 8, clear, STORE_PLAIN, 32, 16, True,
                           dict(tile_rows=16, write_through=None if clear else True)))
    for clear in (True, False):   # the small-splat kernel reports PX=4,R=8 (note_dispatch); adaptive means plain there
        for wt, sm in ((None, STORE_PLAIN), (True, STORE_WT)):
            out.append(Variant(f"small_{'clear' if clear else 'inplace'}_sm{sm}", "splat_small_kernel", 4, 8, clear, sm, SMALL_TW,
                               SMALL_TH, False, dict(small_radii=True, write_through=wt)))
    return out


VARIANTS = _variants()
SMALL_VARIANTS = [v for v in VARIANTS if v.kernel == "splat_small_kernel"]


def family_reference(v):
    """the variant whose map `v`'s must equal bit for bit (the equalities the suite already holds: R = 16 against R = 8,
    write-through and adaptive against plain stores), or None"""
    if v.PX == 1 or (v.sm == STORE_PLAIN and (v.R == 8 or v.kernel == "splat_small_kernel")):
        return None
    return next(u for u in VARIANTS if u.kernel == v.kernel and u.PX == v.PX and u.clear == v.clear and u.sm == STORE_PLAIN and u.R == 8)


def expected_grid(kernel, PX, R, planes, H, W):
    """(grid, block) of launch_splat / launch_splat_small"""
    TW, TH = (SMALL_TW, SMALL_TH) if kernel == "splat_small_kernel" else (32 * PX, 2 * R)
    wpg = 1 if kernel == "splat_small_kernel" else WPG
    tiles_x, tiles_y = -(-W // TW), -(-H // TH)
    if planes <= GRID_Z and tiles_y <= GRID_Y:
        return (-(-tiles_x // wpg), tiles_y, planes), 64 * wpg
    return (-(-(planes * tiles_x * tiles_y) // wpg), 1, 1), 64 * wpg


def expected_dispatch(v, planes, H, W):
    (gx, gy, gz), block = expected_grid(v.kernel, v.PX, v.R, planes, H, W)
    return f"{v.kernel}<PX={v.PX},R={v.R},CLEAR={int(v.clear)},SM={v.sm}> grid({gx},{gy},{gz}) block({block})"


def is_linear(dispatch):
    """a linear launch shows a one-dimensional grid"""
    gx, gy, gz = (int(g) for g in re.search(r"grid\((\d+),(\d+),(\d+)\)", dispatch).groups())
    return gy == 1 and gz == 1, gx


def base_map(shape, k=1.0):
    """distinct non-zero values in (-0.25, 1.25) — for a negative k in (-1.25, 0.25): some above and some below anything a
    draw with |k| <= 1 writes"""
    n = int(np.prod(shape))
    v = ((np.arange(n, dtype=np.float64) * 0.6180339887 + 0.137) % 1.0) * 1.5 - 0.25
    return (v - (1.0 if k < 0 else 0.0)).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------- structural cases (batched API)
# Every case is built for a tile geometry (TW x TH pixels).  The map has 3 x 3 tiles, the last column and row partial:
# W = 2 TW + 8 (2 TW + 5 for the PX = 1 instantiations, which a width off 4 selects), H = 2 TH + 3.
def _map_shape(TW, TH, odd):
    return 2 * TH + 3, 2 * TW + (5 if odd else 8)


def _pack(objs_per_plane, counts=None):
    """[[(x, y, r), ...], ...] -> centers [B, N, 2], radii [B, N], counts [B]; padded slots hold a large object"""
    n_max = max(len(o) for o in objs_per_plane)
    B = len(objs_per_plane)
    c = np.zeros((B, n_max, 2), dtype=np.int64)
    r = np.full((B, n_max), 50, dtype=np.int64)
    c[:, :, 0], c[:, :, 1] = 9, 7
    for b, objs in enumerate(objs_per_plane):
        for i, (x, y, rad) in enumerate(objs):
            c[b, i] = (x, y)
            r[b, i] = rad
    counts = [len(o) for o in objs_per_plane] if counts is None else counts
    return c, r, np.asarray(counts, dtype=np.int64)


# (hits of the target tile in cull round 1, 2, 3; valid objects of the plane)
ROUND_SPLITS = [((3, 0, 0), 130), ((0, 4, 0), 130), ((0, 0, 1), 130), ((0, 0, 2), 130), ((5, 0, 2), 130), ((64, 0, 0), 130),
                ((64, 64, 2), 130), ((1, 1, 1), 130), ((2, 3, 0), 130), ((0, 64, 1), 130), ((64, 64, 2), 0), ((64, 64, 2), 1),
                ((64, 64, 2), 64), ((64, 64, 2), 65), ((7, 0, 0), 64), ((2, 0, 0), 130)]
TARGET_TILE, FILLER_TILE = (1, 0), (0, 1)


def round_splits(TW, TH, odd, k=0.8):
    """130 slots per plane = cull rounds of 64, 64 and 2.  Tile (1, 0) gets the named number of hits in each round (first
    touched in round 1, 2 or 3; a round without hits between two with hits; 64 hits in a round; odd and even counts; one to
    three rounds by the plane's count 0 / 1 / 64 / 65 / 130); all other slots sit in tile (0, 1) and reach no other tile"""
    H, W = _map_shape(TW, TH, odd)
    N = 2 * KCAND + 2
    sizes = (KCAND, KCAND, 2)
    planes, named, target = [], [], []
    for b, (split, count) in enumerate(ROUND_SPLITS):
        j = np.arange(N)
        objs = [(8 + (i * 5) % (TW - 16), TH + 4 + (i * 3) % (TH - 8), i % 3) for i in j]
        mask = np.zeros(N, dtype=bool)
        for q, h in enumerate(split):
            for i in range(h):
                s = KCAND * q + (i * 37) % sizes[q]
                objs[s] = (TW + 4 + (s * 11) % (TW - 8), 2 + (s * 5) % (TH - 4), 1 + s % 6)
                mask[s] = True
        planes.append(objs)
        target.append(mask)
        named.append((b, TARGET_TILE, tuple(min(h, max(0, min(count - KCAND * q, sizes[q]))) for q, h in enumerate(split))))
    c, r, _ = _pack(planes)
    return SimpleNamespace(name="round_splits", H=H, W=W, centers=c, radii=r, counts=np.array([n for _, n in ROUND_SPLITS]),
                           k=k, named=named, target=np.array(target))


def box_edges(TW, TH, odd, k=1.0):
    """clipped boxes whose left / right edges fall at x % 4 = 1, 2, 3 (inside the four columns of a lane), boxes whose last
    row is R - 1 or whose first row is R of tile row 0 (the half-wave boundary), in three pairings; plane 2 adds an object
    whose clipped box is the whole of tile (1, 0): xhi == TW and yhi == TH in the byte packing of Hit::box"""
    H, W = _map_shape(TW, TH, odd)
    R = TH // 2
    objs = []
    for left in (1, 2, 3):
        for right in (1, 2, 3):
            for r in range(2, R):
                xs = [x for x in range(r, TW - r) if (x - r) % 4 == left and (x + r + 1) % 4 == right]
                if not xs:
                    continue
                objs.append((xs[0] + TW * (left % 2), R - 1 - r, r))       # last row R - 1
                objs.append((xs[0] + TW * (right % 2), R + r, r))          # first row R
                break
    objs += [(TW + 2, R - 1, 0), (TW + 3, R, 0), (TW + 1, R - 3, 2), (2 * TW - 1, R + 5, 5), (W - 2, H - 2, 3), (TW - 1, TH - 1, 7)]
    assert any((x - r) % 4 == 1 for x, _, r in objs) and any((x + r + 1) % 4 == 3 for x, _, r in objs)
    n = len(objs)
    perm = [(i * 7 + 3) % n for i in range(n)] if math.gcd(7, n) == 1 else [(i * 5 + 3) % n for i in range(n)]
    assert sorted(perm) == list(range(n))
    whole = (TW + TW // 2, TH // 2, TW)
    c, r, counts = _pack([objs, [objs[i] for i in perm], [whole] + objs[:5]], counts=[n, n - 1, 6])
    return SimpleNamespace(name="box_edges", H=H, W=W, centers=c, radii=r, counts=counts, k=k, whole=(2, 0, TARGET_TILE),
                           named=[], target=np.arange(c.shape[1])[None, :] < counts[:, None])


def off_map(TW, TH, odd, k=1.0):
    """radius 0, centres on the corners and off the map on every side (boxes that reach in and boxes that stop one pixel
    short), a negative radius, and an object beyond the clamps of the cull whose exact box is empty (it passes cull_test in
    every tile and packs box = 0)"""
    H, W = _map_shape(TW, TH, odd)
    R = TH // 2
    reach = [(0, 0, 0), (W - 1, H - 1, 0), (W, H, 1), (-1, -1, 1), (-30, R, 30), (W + 29, R - 1, 30), (TW, -20, 20), (TW + 1, H + 19, 20),
             (TW + 5, TH + 1, 0), (3, TH - 1, 0)]
    short = [(-31, 5, 30), (W + 30, 5, 30), (TW, -21, 20), (TW, H + 20, 20), (10, 10, -1), (1 << 30, 5, (1 << 29) + 5)]
    c, r, counts = _pack([reach + short, short, reach])
    mask = np.zeros(r.shape, dtype=bool)
    mask[0, :len(reach)] = True
    mask[2, :len(reach)] = True
    return SimpleNamespace(name="off_map", H=H, W=W, centers=c, radii=r, counts=counts, k=k, named=[], target=mask,
                           empty_box=(0, len(reach) + len(short) - 1), drawn_by_none=1)


def _odd_squares(total, terms=16):
    """odd d_i with sum d_i^2 == total"""
    def rec(rem, dmax, left):
        if rem == 0:
            return []
        if left == 0:
            return None
        d = min(dmax, math.isqrt(rem))
        d -= (d + 1) % 2
        while d >= 1 and d * d * left >= rem:
            sub = rec(rem - d * d, d, left - 1)
            if sub is not None:
                return [d] + sub
            d -= 2
        return None
    return rec(total, 1 << 20, terms)


def cover(TW, TH, odd, k=0.9):
    """in-place launches with the adaptive store policy choose per plane: sum (2r + 1)^2 of the plane's objects against
    dense_area = 0.75 H W.  Plane 0 is below it by the smallest object, plane 1 EQUAL to it, plane 2 above by one pixel,
    plane 3 far below, plane 4 far above.  Only value neutrality can be seen from outside; the sums are asserted here"""
    H, W = _map_shape(TW, TH, odd)
    dense = 3 * H * W // 4 if (H * W) % 4 == 0 else None
    ds = _odd_squares(dense if dense is not None else 3 * (H * W // 4))
    assert ds is not None
    objs = [((17 * i + 5) % W, (11 * i + 3) % H, (d - 1) // 2) for i, d in enumerate(ds)]
    planes = [objs[:-1], objs, objs + [(W // 2, H // 2, 0)], [(5, 5, 1)], objs + objs]
    c, r, counts = _pack(planes)
    cov = [sum((2 * rad + 1) ** 2 for _, _, rad in p) for p in planes]
    return SimpleNamespace(name="cover", H=H, W=W, centers=c, radii=r, counts=counts, k=k, named=[], cover=cov,
                           dense_area=0.75 * H * W, target=np.arange(c.shape[1])[None, :] < counts[:, None])


STRUCTURAL = {"round_splits": round_splits, "round_splits_kneg": lambda TW, TH, odd: round_splits(TW, TH, odd, k=-0.75),
              "box_edges": box_edges, "off_map": off_map, "off_map_kneg": lambda TW, TH, odd: off_map(TW, TH, odd, k=-1.0),
              "cover": cover}


# ------------------------------------------------------------------------------------------- the small-splat kernel
SMALL_H, SMALL_W = 2 * SMALL_TH + 9, 2 * SMALL_TW + 8       # 41 x 264: tile row 2 has nine rows


def rows_hint_planes():
    """(rows, where) of every plane of small_rows(): one plane per height 1..7 of the tallest clipped box of the round;
    even heights come from radii 1..3 clipped by the top edge (tile (1, 0)) or by the bottom edge (tile (1, 2))"""
    out = []
    for rows in range(1, 8):
        out += [(rows, "inside")] if rows % 2 else [(rows, "top"), (rows, "bottom")]
    return out


def small_rows():
    """walk_hits' row walk (rows_hint 1..7): 64 objects per plane, all in one tile and one cull round, the tallest clipped
    box `rows` high, so that the tile has more hits than one pass of 64 / rows takes (rows == 1: 64 hits are one pass — more
    cannot be: a round has 64 candidates)"""
    planes, named = [], []
    for b, (rows, where) in enumerate(rows_hint_planes()):
        r = rows // 2
        if where == "inside":
            objs = [(SMALL_TW + 3 + i, r + i % (SMALL_TH - 2 * r), r) for i in range(KCAND)]
            tile = (1, 0)
        elif where == "top":
            objs = [(SMALL_TW + 3 + i, r - 1, r) for i in range(KCAND)]                  # rows [0, 2r)
            tile = (1, 0)
        else:
            objs = [(SMALL_TW + 3 + i, SMALL_H - r, r) for i in range(KCAND)]            # rows [H - 2r, H)
            tile = (1, 2)
        planes.append(objs)
        named.append((b, tile, rows))
    c, r, counts = _pack(planes)
    return SimpleNamespace(name="small_rows", H=SMALL_H, W=SMALL_W, centers=c, radii=r, counts=counts, k=0.9, named=named,
                           target=np.ones(r.shape, dtype=bool))


def small_walk():
    """walk_hits' 16-lane walk (tallest box of the round 8 rows or more).  Plane 0: boxes 8, 11 and 15 rows high, one 128
    wide and 16 high (the whole of tile (1, 1); tile (2, 1) sees it 8 wide), single pixels, and the empty box beyond the
    clamps — nine hits in tile (1, 0), which the large one reaches 16 rows high: three trips of `h0 += 4`.  Plane 1: six boxes exactly 8 rows high (just past the row
    walk); plane 2: six boxes exactly 7 rows high (the row walk's last height, one pass)"""
    X = SMALL_TW
    p0 = [(X + 12, 3, 4), (X + 22, 8, 5), (X + 42, 7, 7), (X + 64, SMALL_TH + 8, 72), (X + 72, 2, 0), (X + 80, 12, 1), (X + 90, 5, 4),
          (X + 100, 9, 5), (1 << 30, 5, (1 << 29) + 5)]
    p1 = [(X + 5 + 13 * i, 3, 4) for i in range(6)]
    p2 = [(X + 5 + 13 * i, 3 + i, 3) for i in range(6)]
    c, r, counts = _pack([p0, p1, p2])
    return SimpleNamespace(name="small_walk", H=SMALL_H, W=SMALL_W, centers=c, radii=r, counts=counts, k=0.9,
                           named=[(0, (1, 0), 9, 16), (0, (1, 1), 2, 16), (1, (1, 0), 6, 8), (2, (1, 0), 6, 7)],
                           whole=(0, 3, (1, 1)), target=np.arange(c.shape[1])[None, :] < counts[:, None])


def small_fetch():
    """small_body's candidate loop `base += kFetch * kCand`: 300 objects, so a second trip of 256; the first 256 and the last
    12 sit in tile (0, 0), slots 256..287 in tile (1, 1)"""
    n = SMALL_FETCH * KCAND + 44
    objs = [(4 + (i * 7) % 100, 2 + i % 12, i % 3) for i in range(n)]
    for i in range(SMALL_FETCH * KCAND, SMALL_FETCH * KCAND + 32):
        objs[i] = (SMALL_TW + 6 + 3 * (i - SMALL_FETCH * KCAND), SMALL_TH + 2 + i % 12, 1 + i % 2)
    c, r, counts = _pack([objs])
    mask = np.zeros(r.shape, dtype=bool)
    mask[0, SMALL_FETCH * KCAND:SMALL_FETCH * KCAND + 32] = True
    return SimpleNamespace(name="small_fetch", H=SMALL_H, W=SMALL_W, centers=c, radii=r, counts=counts, k=0.9,
                           named=[(0, (1, 1), (0, 0, 0, 0, 32))], target=mask)


SMALL = {"small_rows": small_rows, "small_walk": small_walk, "small_fetch": small_fetch}


# ------------------------------------------------------------------------------------------- linear grids
def many_planes_flat(P=70000, H=8, W=16):
    """flat API, more planes than a grid dimension holds: splat_kernel on a linear grid of P tiles, the three-kernel binning
    with ceil(P / 1024) planes per thread of bin_scan_kernel.  Objects in the planes around every boundary (0, 1023 / 1024 of
    the scan, GRID_Z - 1 / GRID_Z / GRID_Z + 1, the last) and every 23rd in between; plane indices -1 and P among them"""
    assert P > GRID_Z and P > BIN_SMALL_PLANES
    marks = [0, 1, BIN_WG - 1, BIN_WG, GRID_Z - 1, GRID_Z, GRID_Z + 1, P - 2, P - 1]
    idx = marks + list(range(7, P, 23)) + [-1, P, P + 5, -7]
    n = len(idx)
    i = np.arange(n)
    c = np.stack([(i * 5) % (W + 4) - 2, (i * 3) % (H + 4) - 2], 1)
    r = i % 4
    m = np.arange(len(marks))
    c[m, 0], c[m, 1], r[m] = 2 + m, 1 + m % 6, 1                      # the marked planes' objects lie on the map
    return SimpleNamespace(P=P, H=H, W=W, centers=c.astype(np.int32), radii=r.astype(np.int32), idx=np.asarray(idx, dtype=np.int32),
                           marks=marks)


def many_planes_classwise(B=7, C=10000, H=4, W=8, n_max=40):
    """class-wise batched call with B C > GRID_Z planes: the plane of a linear tile splits into (sample, class) by a
    division.  Labels include -1 and C (drawn nowhere), class 0 and class C - 1 of the first and the last sample"""
    assert B * C > GRID_Z
    b, i = np.meshgrid(np.arange(B), np.arange(n_max), indexing="ij")
    labels = (i * 251 + b * 977) % C
    labels[:, 0], labels[:, 1], labels[:, 2], labels[:, 3] = 0, C - 1, -1, C
    c = np.stack([(i * 3 + b) % (W + 2) - 1, (i + 2 * b) % (H + 2) - 1], -1)
    r = (i + b) % 3
    c[:, :4], r[:, :4] = [(2, 1), (5, 2), (3, 3), (6, 0)], 1            # the four named labels' objects lie on the map
    counts = np.array([n_max, n_max - 1, 0, 5, n_max + 3, 17, n_max][:B], dtype=np.int64)     # one above n_max: clamped
    return SimpleNamespace(B=B, C=C, H=H, W=W, centers=c.astype(np.int32), radii=r.astype(np.int32), labels=labels.astype(np.int32),
                           counts=counts)


def many_tile_rows(tile_rows, B=1, W=4, TH=16):
    """a map of `tile_rows` rows of 16-pixel tiles plus one row, W = 4: objects in the first, a middle and the last tile row
    (the last is the single row H - 1), and across the border of two tile rows"""
    H = TH * tile_rows + 1
    mid = TH * (tile_rows // 2)
    objs = [(1, 0, 1), (2, 9, 3), (0, mid + 3, 2), (3, mid + TH - 1, 4), (2, H - 1, 0), (1, H - 3, 2), (0, H - 1 - TH, 1), (2, TH * (tile_rows - 1), 6)]
    c, r, counts = _pack([objs] * B, counts=[len(objs) - b for b in range(B)])
    return SimpleNamespace(H=H, W=W, centers=c, radii=r, counts=counts, rows=[0, mid // TH, tile_rows])


# ------------------------------------------------------------------------------------------- flat-API binning
def flat_binning(P, N, H=8, W=16):
    """N objects for P planes.  Every object crosses the binning loops; one in `keep` names a plane in range (the others -1 or P,
    ignored), so that the planes stay sparse and each drawn object shows.  Radius 0 or 1; no object but the last — the only one
    in the last trip of every object loop — reaches column W - 1, and the last draws pixel (W - 1, H - 1) of plane P // 2.
    Objects 2, 3, 4 go to the last plane and to the planes on either side of the zeroing loop's first trip"""
    keep = max(1, N // 300)
    i = np.arange(N, dtype=np.int64)
    j = i // keep
    idx = np.where(i % keep == 0, (j * 7919) % P, np.where(i % 2 == 0, -1, P))
    c = np.stack([i % (W - 1), (i // (W - 1)) % H], 1)
    r = ((i % 5 == 0) & (c[:, 0] + 1 < W - 1)).astype(np.int64)
    idx[0], idx[1], idx[2], idx[3], idx[4] = -1, P, P - 1, min(BIN_WG, P - 1), min(BIN_WG, P) - 1
    c[N - 1], r[N - 1], idx[N - 1] = (W - 1, H - 1), 0, P // 2
    return SimpleNamespace(P=P, H=H, W=W, centers=c.astype(np.int32), radii=r.astype(np.int32), idx=idx.astype(np.int32),
                           last=(P // 2, H - 1, W - 1))


def bin_path(P, N):
    """which binning the flat entry point runs: the host rule of accv_draw_heatmap_flat_f32"""
    return "bin_small" if P <= BIN_SMALL_PLANES and N <= BIN_SMALL_OBJECTS else "three_kernels"


# name -> (planes, objects, path, what the shape crosses)
BINNING = {
    "planes_1025": (BIN_WG + 1, 3000, "bin_small"),                         # per == 2; the zeroing loop's second trip
    "planes_8192": (BIN_SMALL_PLANES, 3000, "bin_small"),                   # the last plane count of the single launch
    "planes_8193": (BIN_SMALL_PLANES + 1, 3000, "three_kernels"),
    "objects_65536": (5, BIN_SMALL_OBJECTS, "bin_small"),                   # 64 trips of the object loops
    "objects_65537": (5, BIN_SMALL_OBJECTS + 1, "three_kernels"),
    "objects_262145": (5, BIN_GRID_CAP * BIN_THREADS + 1, "three_kernels"),  # grid-stride second trip of count and fill
}


def flat_direct(planes, height, width, n):
    """ops._flat_direct, restated from the constants of ops.py"""
    if not (0 < n <= FLAT_DIRECT_MAX_OBJECTS and 0 < planes <= FLAT_DIRECT_MAX_PLANES and height > 0 and width > 0):
        return False
    tiles = planes * -(-width // SMALL_TW) * -(-height // SMALL_TH)
    return tiles * -(-n // KCAND) <= FLAT_DIRECT_MAX_ROUNDS


# (planes, H, W, objects) on either side of every threshold of _flat_direct: (direct, not direct)
FLAT_DIRECT_EDGES = {
    "objects": ((2, 8, 16, FLAT_DIRECT_MAX_OBJECTS), (2, 8, 16, FLAT_DIRECT_MAX_OBJECTS + 1)),
    "planes": ((FLAT_DIRECT_MAX_PLANES, 4, 8, 40), (FLAT_DIRECT_MAX_PLANES + 1, 4, 8, 40)),
    "rounds": ((FLAT_DIRECT_MAX_ROUNDS // 4, 4, 8, 4 * KCAND), (FLAT_DIRECT_MAX_ROUNDS // 4, 4, 8, 4 * KCAND + 1)),
}


def flat_objects(P, H, W, N):
    """deterministic flat objects for the threshold calls: every plane index in [-1, P] appears when N allows"""
    i = np.arange(N, dtype=np.int64)
    idx = (i * 7919) % (P + 2) - 1
    idx[N - 1] = P - 1
    c = np.stack([(i * 5) % (W + 2) - 1, (i * 3) % (H + 2) - 1], 1)
    return c.astype(np.int32), (i % 3).astype(np.int32), idx.astype(np.int32)


# ------------------------------------------------------------------------------------------- the reference
def oracle_batched(case, clear, base=None, radii=None, labels=None):
    """the CPU oracle (float64 inside) on a case of the batched API; in place it starts from `base`"""
    from oracle import h1 as oracle

    B = len(case.counts)
    ref = np.full((B, case.H, case.W), 55.0, dtype=np.float32) if clear else np.array(base, dtype=np.float32, copy=True)
    oracle.draw_heatmap_batched(ref, np.asarray(case.centers, dtype=np.int32), np.asarray(case.radii if radii is None else radii, dtype=np.int32),
                                np.asarray(case.counts, dtype=np.int64), labels=labels, k=case.k, clear=clear)
    return ref


def without(case, mask):
    """the case's radii with the objects of `mask` taken out (radius -1: drawn by nothing)"""
    r = np.array(case.radii, copy=True)
    r[mask] = -1
    return r


GEOMETRIES = sorted({(v.TW, v.TH, v.odd) for v in VARIANTS})
