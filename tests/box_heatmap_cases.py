"""Cases and the oracle of the box-to-heat-map tests (test_box_heatmap_cpu.py, test_box_heatmap_gpu.py).

The oracle is written here in numpy from the docstring of accvlab.draw_heatmap.boxes_to_heatmap and shares no code with the
library: the per-object outputs with float32 numpy scalars, one operation per step of the definition; the map painted object
by object in float64 from the float32 radius and the float32 factors.

Bars (the project's, see the README): integer, bool and float per-object outputs bitwise equal to the oracle and between
device and host entry; map values within 1e-5 x max(1, max k) absolute of the float64 oracle; map elements outside every
active object's patch exactly 0.0.  No case and no element is excluded from any comparison.
"""
import functools
import json
import os

import numpy as np
import torch

from accvlab import _amd_native as nat
from accvlab.batching_helpers import RaggedBatch

F = np.float32
NAN, INF = float("nan"), float("inf")
TW, TH = nat.BH_TILE_W, nat.BH_TILE_H
MAX_BOXES, MAX_CATEGORIES = nat.BH_MAX_BOXES, nat.BH_MAX_CATEGORIES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_heatmap_reference_case.json")

DEFAULTS = dict(num_categories=None, min_object_size=None, per_category_min_object_sizes=None, use_per_category_heatmap=True,
                min_fraction_area_clipping=0.25, min_radius=0.5, max_radius=10.0, radius_scaling_factor=0.8,
                radius_to_sigma_factor=1.0 / 3.0, k_for_classes=None)
FLOAT_FIELDS = ("center_offset", "height_width", "bboxes_heatmap", "radii")


class Case:
    """frames: a list of dicts with `boxes` [n, 4] and, the same keys in every frame, `centers` [n, 2], `cats` [n], `valid`
    [n]; image_hw: one (H, W) or one per frame; kw: the operator's keyword arguments"""

    def __init__(self, name, frames, image_hw, heatmap_hw, G=None, cat_dtype=torch.int32, hw_dtype=None, **kw):
        self.name, self.frames, self.heatmap_hw, self.kw = name, frames, tuple(heatmap_hw), kw
        self.per_frame_hw = len(image_hw) > 0 and not isinstance(image_hw[0], int)
        self.image_hw = [tuple(v) for v in image_hw] if self.per_frame_hw else [tuple(image_hw)] * len(frames)
        self.G = max([len(f["boxes"]) for f in frames] + [0]) if G is None else G
        self.cat_dtype, self.hw_dtype = cat_dtype, hw_dtype
        for f in frames:
            f["boxes"] = np.asarray(f["boxes"], F).reshape(-1, 4)
            assert set(f) == set(frames[0]) and len(f["boxes"]) <= self.G

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------- oracle
def _clip(v, m):
    return F(0) if v < F(0) else (m if v > m else v)


def _object(box, centre, sx, sy, xm, ym, p):
    """steps 1 to 7 for one object: (finite, bboxes_heatmap, (h, w), fraction, (ix, iy), (ox, oy), radius)"""
    b = [F(v) for v in box]
    with np.errstate(all="ignore"):
        c0, c1 = ((b[0] + b[2]) / F(2), (b[1] + b[3]) / F(2)) if centre is None else (F(centre[0]), F(centre[1]))
        X1, Y1, X2, Y2, CX, CY = sx * b[0], sy * b[1], sx * b[2], sy * b[3], sx * c0, sy * c1
        if not all(np.isfinite(v) for v in (X1, Y1, X2, Y2, CX, CY)):
            return False, [F(0)] * 4, (F(0), F(0)), F(0), (0, 0), (F(0), F(0)), F(0)
        x1, y1, x2, y2 = _clip(X1, xm), _clip(Y1, ym), _clip(X2, xm), _clip(Y2, ym)
        h, w = np.abs(y2 - y1), np.abs(x2 - x1)
        ho, wo = np.abs(Y2 - Y1), np.abs(X2 - X1)
        fraction = (h * w) / (ho * wo)
        cx, cy = _clip(CX, xm), _clip(CY, ym)
        fx, fy = np.floor(cx), np.floor(cy)
        l, r = (x1, x2) if x1 <= x2 else (x2, x1)
        t, bt = (y1, y2) if y1 <= y2 else (y2, y1)
        d = min(cx - l, cy - t, r - cx, bt - cy)
        d = F(0) if d < F(0) else d
        q = d * F(p["radius_scaling_factor"])
        lo = max(F(0.5), F(p["min_radius"]))
        q = lo if q < lo else q
        radius = F(p["max_radius"]) if q > F(p["max_radius"]) else q
    for v in (h, w, fraction, cx - fx, radius):
        assert v.dtype == F
    return True, [x1, y1, x2, y2], (h, w), fraction, (int(fx), int(fy)), (cx - fx, cy - fy), radius


def _oracle(case):
    p = dict(DEFAULTS, **case.kw)
    B, G, (Hm, Wm) = len(case.frames), case.G, case.heatmap_hw
    C = p["num_categories"]
    planes = C if p["use_per_category_heatmap"] else 1
    k = [1.0] * planes if p["k_for_classes"] is None else [float(F(v)) for v in p["k_for_classes"]]
    out = dict(heatmap=np.zeros((B, planes, Hm, Wm), np.float64), patches=np.zeros((B, planes, Hm, Wm), bool),
               is_active=np.zeros((B, G), bool), center=np.zeros((B, G, 2), np.int32), center_offset=np.zeros((B, G, 2), F),
               height_width=np.zeros((B, G, 2), F), bboxes_heatmap=np.zeros((B, G, 4), F), radii=np.zeros((B, G), F),
               max_k=max([1.0] + [abs(v) for v in k]))
    for b, (f, (Hi, Wi)) in enumerate(zip(case.frames, case.image_hw)):
        Hi, Wi = (min(max(int(v), 0), 1 << 24) for v in (Hi, Wi))
        with np.errstate(all="ignore"):
            sx, sy = F(Wm) / F(Wi), F(Hm) / F(Hi)
        for i, box in enumerate(f["boxes"]):
            centre = f["centers"][i] if "centers" in f else None
            finite, bb, (h, w), fraction, (ix, iy), off, radius = _object(box, centre, sx, sy, F(Wm - 1), F(Hm - 1), p)
            out["bboxes_heatmap"][b, i], out["height_width"][b, i] = bb, (h, w)
            out["center"][b, i], out["center_offset"][b, i], out["radii"][b, i] = (ix, iy), off, radius
            active, cat = finite and bool(fraction >= F(p["min_fraction_area_clipping"])), 0
            if C is not None:
                cat = int(f["cats"][i])
                active = active and 0 <= cat < C
            if p["per_category_min_object_sizes"] is not None and 0 <= cat < C:
                mh, mw = p["per_category_min_object_sizes"][cat]
                active = active and bool(h >= F(mh)) and bool(w >= F(mw))
            if p["min_object_size"] is not None:
                active = active and bool(h >= F(p["min_object_size"][0])) and bool(w >= F(p["min_object_size"][1]))
            if "valid" in f:
                active = active and bool(f["valid"][i])
            out["is_active"][b, i] = active
            if not active:
                continue
            plane = cat if p["use_per_category_heatmap"] else 0
            R = int(np.ceil(radius))
            sigma = float(radius) * float(F(p["radius_to_sigma_factor"]))
            ya, yb, xa, xb = max(iy - R, 0), min(iy + R, Hm - 1), max(ix - R, 0), min(ix + R, Wm - 1)
            yy, xx = np.ogrid[ya:yb + 1, xa:xb + 1]
            val = k[plane] * np.exp(-((yy - iy) ** 2 + (xx - ix) ** 2).astype(np.float64) / (2.0 * sigma * sigma))
            view = out["heatmap"][b, plane, ya:yb + 1, xa:xb + 1]
            np.maximum(view, val, out=view)
            out["patches"][b, plane, ya:yb + 1, xa:xb + 1] = True
    if not p["use_per_category_heatmap"]:
        out["heatmap"], out["patches"] = out["heatmap"][:, 0], out["patches"][:, 0]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_of(case):
    """the oracle of any Case, a drawn one included; not cached by name, read-only"""
    return _oracle(case)


_ORACLES = {}


def oracle(case):
    """computed once per case and shared, read-only"""
    if case.name not in _ORACLES:
        _ORACLES[case.name] = (case, _oracle(case))
    assert _ORACLES[case.name][0] is case, f"two cases are called {case.name}"
    return _ORACLES[case.name][1]


# ------------------------------------------------------------------------------------------------------ inputs and checks
def batch(case, device, size_dtype=torch.int64):
    """(bboxes, keyword arguments) of the operator for a case.  Padding slots are hostile: NaN, 1e30 and inf coordinates,
    categories out of range and inside it, is_valid true"""
    B, G = len(case.frames), case.G
    boxes = np.empty((B, G, 4), F)
    boxes[...] = np.array([NAN, 1e30, -INF, 3.0], F)
    boxes[:, 1::2] = np.array([5.0, 7.0, 25.0, 30.0], F)          # every other padding slot is a well-formed box
    centers = np.full((B, G, 2), NAN, F)
    centers[:, 1::2] = np.array([12.0, 15.0], F)
    cats = np.zeros((B, G), np.int64)
    cats[:, 0::3], cats[:, 1::3] = 2 ** 31 - 1, -5
    valid = np.ones((B, G), bool)
    for b, f in enumerate(case.frames):
        n = len(f["boxes"])
        boxes[b, :n] = f["boxes"]
        if "centers" in f:
            centers[b, :n] = np.asarray(f["centers"], F).reshape(-1, 2)
        if "cats" in f:
            cats[b, :n] = f["cats"]
        if "valid" in f:
            valid[b, :n] = f["valid"]
    sizes = torch.tensor([len(f["boxes"]) for f in case.frames], dtype=size_dtype, device=device)
    kw = dict(case.kw, heatmap_hw=case.heatmap_hw)
    first = case.frames[0] if case.frames else {}
    if "centers" in first:
        kw["centers"] = RaggedBatch(torch.from_numpy(centers).to(device), sample_sizes=sizes)
    if "cats" in first:
        kw["categories"] = torch.from_numpy(cats).to(case.cat_dtype).to(device)     # int32: the low 32 bits
    if "valid" in first:
        kw["is_valid"] = torch.from_numpy(valid).to(device)
    if case.per_frame_hw or case.hw_dtype is not None:
        kw["image_hw"] = torch.tensor(case.image_hw, dtype=case.hw_dtype or torch.int32, device=device).reshape(B, 2)
    else:
        kw["image_hw"] = case.image_hw[0] if case.image_hw else (1, 1)
    return RaggedBatch(torch.from_numpy(boxes).to(device), sample_sizes=sizes), kw


def run(op, case, device, **more):
    bboxes, kw = batch(case, device)
    return op(bboxes, **dict(kw, **more))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_objects(got, want, what):
    """the per-object outputs of a BoxHeatmapTargets against the oracle (or another run's numpy dict), bit for bit"""
    a = got.is_active.tensor.cpu().numpy()
    assert a.dtype == np.bool_ and np.array_equal(a, want["is_active"]), f"{what}: is_active"
    c = got.center.tensor.cpu().numpy()
    assert c.dtype == np.int32 and np.array_equal(c, want["center"]), f"{what}: center"
    for name in FLOAT_FIELDS:
        g = getattr(got, name).tensor.cpu().numpy()
        assert g.dtype == F and g.shape == want[name].shape, f"{what}: {name}"
        assert np.array_equal(_bits(g), _bits(want[name])), f"{what}: {name} differs in {(_bits(g) != _bits(want[name])).sum()} elements"


def check_map(heatmap, want, what):
    g = heatmap.detach().cpu().numpy()
    assert g.dtype == F and g.shape == want["heatmap"].shape, f"{what}: map shape {g.shape}"
    err = np.abs(g.astype(np.float64) - want["heatmap"])
    bar = 1e-5 * want["max_k"]
    assert np.all(err <= bar), f"{what}: map error {np.nanmax(err):.3g} above {bar:.3g} (or NaN)"
    assert np.all(_bits(g)[~want["patches"]] == 0), f"{what}: a pixel outside every patch is not +0.0"


def check(got, case, what=None):
    want = oracle(case)
    check_objects(got, want, what or case.name)
    check_map(got.heatmap, want, what or case.name)
    for r in got[1:]:
        assert torch.equal(r.sample_sizes.cpu(), torch.tensor([len(f["boxes"]) for f in case.frames]))


def as_numpy(got):
    """a run's outputs in the oracle's layout, for comparing two runs bit for bit"""
    out = {n: getattr(got, n).tensor.cpu().numpy() for n in ("is_active", "center") + FLOAT_FIELDS}
    out["heatmap"] = got.heatmap.cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------- the reference's test
@functools.lru_cache(None)
def reference_cases():
    """bounding_box_to_heatmap_converter_test.py of the reference: the eight parametrisations of :288-295 and the two
    single-map configurations of :446-483, from the data-only fixture; every one expects the same is_active.  Built once:
    the CPU and the GPU module of one pytest process share the cases, as `oracle` demands of cases with one name."""
    g = json.load(open(GOLDEN))
    canon = np.array(g["bboxes"], F)
    common = dict(radius_scaling_factor=g["radius_scaling_factor"])
    cases = []
    for q in g["parametrisations"]:
        x1, y1, x2, y2 = canon.T
        if q["use_other_diagonal"]:
            y1, y2 = y2, y1
        if q["reverse_point_order"]:
            x1, y1, x2, y2 = x2, y2, x1, y1
        f = dict(boxes=np.stack([x1, y1, x2, y2], 1), cats=g["categories"], valid=g["is_valid"])
        if q["use_centers"]:
            f["centers"] = g["centers"]
        cases.append(Case("reference_" + q["id"], [f], g["image_hw"], q["heatmap_hw"], num_categories=g["num_categories"],
                          per_category_min_object_sizes=g["per_category_min_object_sizes"], **common))
    for s in g["single_heatmap"]:
        f = dict(boxes=canon.copy(), centers=g["centers"], valid=g["is_valid"])
        kw = dict(common, use_per_category_heatmap=False)
        if s["min_object_size"] is not None:
            kw["min_object_size"] = s["min_object_size"]
        else:
            f["cats"] = g["categories"]
            kw.update(num_categories=g["num_categories"], per_category_min_object_sizes=s["per_category_min_object_sizes"])
        cases.append(Case("reference_single_" + s["id"], [f], g["image_hw"], s["heatmap_hw"], **kw))
    return cases, g


# -------------------------------------------------------------------------------------------------------- random frames
def random_frame(rng, n, image_hw, C=None, centers=True, valid=True, wild=0.0):
    """n objects of an H x W image: small and large boxes inside and across the border, corners in any order; given
    centres mostly inside the box; categories from -1 to C; `wild`: the share of objects with a non-finite value"""
    H, W = image_hw
    c = rng.uniform(-0.1, 1.1, (n, 2)) * [W, H]
    half = 0.3 + rng.uniform(0, 1, (n, 2)) ** 1.5 * [W / 3.0, H / 3.0]
    boxes = np.concatenate([c - half, c + half], 1)
    swap = rng.random((n, 2)) < 0.4
    for axis in (0, 1):
        s = swap[:, axis]
        boxes[s, axis], boxes[s, axis + 2] = boxes[s, axis + 2], boxes[s, axis].copy()
    f = dict(boxes=boxes.astype(F))
    if centers:
        f["centers"] = (c + rng.uniform(-1.2, 1.2, (n, 2)) * half).astype(F)
    if C is not None:
        f["cats"] = rng.integers(-1, C + 1, n)
        f["cats"][rng.random(n) < 0.7] %= C
    if valid:
        f["valid"] = rng.random(n) < 0.85
    for i in np.nonzero(rng.random(n) < wild)[0]:
        v = rng.choice([NAN, INF, -INF, 3e38])
        if centers and rng.random() < 0.4:
            f["centers"][i, rng.integers(2)] = v
        else:
            f["boxes"][i, rng.integers(4)] = v
    return f


def random_case(name, seed, sizes, heatmap_hw, image_hw, C=None, single=False, G=None, centers=True, valid=True, wild=0.0,
                sized=None, **kw):
    """sizes: objects per frame; C: categories (None: not used, then one map); single: one map although categories are used;
    sized: None, "global" or "per_category" minimum sizes"""
    rng = np.random.default_rng(seed)
    hws = image_hw if isinstance(image_hw, list) else [image_hw] * len(sizes)
    frames = [random_frame(rng, n, hw if min(hw) > 0 else (50, 50), C, centers, valid, wild) for n, hw in zip(sizes, hws)]
    if C is not None:
        kw["num_categories"] = C
    if C is None or single:
        kw["use_per_category_heatmap"] = False
    if sized == "global":
        kw["min_object_size"] = (1.5, 2.0)
    elif sized == "per_category":
        kw["per_category_min_object_sizes"] = [(float(c % 3), 1.0 + c % 2) for c in range(C)]
    return Case(name, frames, image_hw, heatmap_hw, G=G, **kw)


def centred(cx, cy, r):
    """a box whose centre lands in pixel (cx, cy) and whose radius is r at scale 1 and radius_scaling_factor 1"""
    return [cx + 0.5 - r, cy + 0.5 - r, cx + 0.5 + r, cy + 0.5 + r]


@functools.lru_cache(None)
def cases():
    """every case of the tests by name (built once: the oracle results are cached by name)"""
    out = []
    # batch and box counts; map widths with and without W % 4 == 0, heights below, above and far below a tile
    widths, heights = (TW - 1, TW, TW + 1, 2 * TW + 3), (TH - 1, TH + 1, 1)
    counts = (1, 63, 64, 65, MAX_BOXES)
    classes = (1, 2, 3, None, 2)
    for j, (Wm, Hm) in enumerate((w, h) for w in widths for h in heights):
        G = counts[j % 5]
        sizes = [G] if j % 2 == 0 else [min(G, 1 + j), 0, G]
        C = classes[j % 5]
        out.append(random_case(f"shape_{Hm}x{Wm}_G{G}_B{len(sizes)}_C{C}", 100 + j, sizes, (Hm, Wm), (max(Hm, 8) * 2, Wm * 3),
                               C=C, single=(j == 4), G=G, centers=j % 3 != 0, valid=j % 4 != 1, wild=0.05,
                               sized=None if Hm == 1 else (None, "global", "per_category")[j % 3] if C else (None, "global")[j % 2],
                               radius_scaling_factor=(0.8, 2.0)[j % 2],
                               # a map of one row clips every height to 0: only a threshold of 0 lets anything be drawn
                               min_fraction_area_clipping=0.0 if Hm == 1 else 0.25))
    out.append(random_case("sizes_0_1_G_in_one_batch", 120, [0, 1, 9], (TH + 1, TW + 1), (40, 130), C=2, G=9))
    out.append(random_case("every_frame_empty", 121, [0, 0], (TH + 1, TW + 4), (40, 130), C=3, G=5))
    out.append(random_case("no_slots_at_all", 122, [0, 0], (3, 7), (40, 130), C=2, G=0))
    out.append(random_case("max_categories", 123, [40, 3], (TH + 3, TW + 8), (60, 200), C=MAX_CATEGORIES, sized="per_category",
                           k_for_classes=[0.5 + (c % 4) * 0.5 for c in range(MAX_CATEGORIES)]))
    out.append(random_case("max_categories_one_map", 124, [40], (TH + 3, TW + 8), (60, 200), C=MAX_CATEGORIES, single=True,
                           sized="per_category", k_for_classes=[2.0]))

    # object placement: both sides of every tile edge of a 3 x 3 tile map, radius 0.5 (3 x 3), 2.5 and 10 (three tiles),
    # a plane per radius
    Hm, Wm = 3 * TH, 3 * TW
    boxes, cats = [], []
    for c, r in enumerate((0.5, 2.5, 10.0)):
        for x in (TW - 1, TW, 2 * TW - 1, 2 * TW):
            for y in (TH - 1, TH, 2 * TH - 1, 2 * TH):
                boxes.append(centred(x, y, r))
                cats.append(c)
    out.append(Case("tile_edges", [dict(boxes=boxes, cats=cats)], (Hm, Wm), (Hm, Wm), num_categories=3, radius_scaling_factor=1.0,
                    k_for_classes=[1.0, 0.5, 2.0]))
    # the same objects on one plane: far ones win pixels of near ones
    out.append(Case("tile_edges_one_map", [dict(boxes=boxes)], (Hm, Wm), (Hm, Wm), use_per_category_heatmap=False,
                    radius_scaling_factor=1.0))
    # the four map corners: a clipped centre on the border has distance 0 to it, so min_radius sets the patch
    Hm, Wm = TH + 1, TW + 1
    corner = [[-6, -6, 6, 6], [Wm - 7, -6, Wm + 5, 6], [-6, Hm - 7, 6, Hm + 5], [Wm - 7, Hm - 7, Wm + 5, Hm + 5]]
    ccent = [[-1, -1], [Wm + 3, -2], [-4, Hm], [Wm, Hm]]
    out.append(Case("map_corners", [dict(boxes=corner, centers=ccent)], (Hm, Wm), (Hm, Wm), use_per_category_heatmap=False,
                    min_radius=3.0))
    # two overlapping objects on one plane, the far one wins some pixels; two classes at the same pixel; k of 0.5 and 2.0
    two = [centred(20, 8, 2.5), centred(26, 9, 10.0), centred(40, 5, 4.0), centred(40, 5, 4.0)]
    out.append(Case("overlap_and_same_pixel", [dict(boxes=two, cats=[0, 0, 0, 1])], (TH + 4, TW), (TH + 4, TW), num_categories=2,
                    radius_scaling_factor=1.0, k_for_classes=[0.5, 2.0]))

    # decision edges.  Area fraction: 9 * 10 / (40 * 10) after clipping x to [0, W - 1] = [0, 9]
    frac = [dict(boxes=[[-30, 0, 10, 10]])]
    f32 = F(90) / F(400)
    for tag, thr in (("at", f32), ("above", np.nextafter(f32, F(1))), ("below", np.nextafter(f32, F(0)))):
        out.append(Case(f"fraction_threshold_{tag}", frac, (16, 10), (16, 10), use_per_category_heatmap=False,
                        min_fraction_area_clipping=float(thr)))
    # size: clipped height 3 and width 4 against minima at them and one ulp above (the object is one ulp below)
    size = [dict(boxes=[[2, 2, 6, 5], [9, 5, 5, 2]])]
    up = lambda v: float(np.nextafter(F(v), F(100)))   # noqa: E731
    for tag, mn in (("at", (3.0, 4.0)), ("h_one_ulp_below", (up(3), 4.0)), ("w_one_ulp_below", (3.0, up(4)))):
        out.append(Case(f"size_minimum_{tag}", size, (16, 20), (16, 20), use_per_category_heatmap=False, min_object_size=mn))
    # categories: -1, num_categories, far outside int32 (low 32 bits 0 and 1), and the two valid ones
    cat = [dict(boxes=[centred(5 + 6 * i, 6, 2.0) for i in range(6)], cats=[-1, 2, 1 << 40, (1 << 32) + 1, 0, 1])]
    out.append(Case("category_range_int64", cat, (14, 48), (14, 48), cat_dtype=torch.int64, num_categories=2))
    cat32 = [dict(boxes=[centred(5 + 6 * i, 6, 2.0) for i in range(4)], cats=[-1, 2, 0, 1])]
    out.append(Case("category_range_int32", cat32, (14, 48), (14, 48), num_categories=2,
                    per_category_min_object_sizes=[(1.0, 1.0), (50.0, 1.0)]))
    out.append(Case("category_range_one_map", cat32, (14, 48), (14, 48), num_categories=2, use_per_category_heatmap=False))
    out.append(Case("is_valid_all_false", [dict(boxes=[centred(5, 6, 2.0), centred(9, 3, 1.0)], valid=[False, False])],
                    (14, 48), (14, 48), use_per_category_heatmap=False))

    # degenerate and non-finite inputs
    out.append(Case("centre_outside_its_box", [dict(boxes=[[10, 4, 20, 12], [30, 4, 40, 12]], centers=[[25, 8], [35, 30]])],
                    (16, 48), (16, 48), use_per_category_heatmap=False, min_radius=1.5))
    out.append(Case("zero_area_boxes", [dict(boxes=[[10, 4, 10, 12], [20, 6, 30, 6], [5, 5, 5, 5], [10, 4, 20, 12]])], (16, 48),
                    (16, 48), use_per_category_heatmap=False, min_fraction_area_clipping=0.0))
    bad = [[NAN, 4, 20, 12], [10, INF, 20, 12], [10, 4, -INF, 12], [10, 4, 20, NAN], [10, 4, 20, 12], [10, 4, 20, 12],
           [10, 4, 20, 12], [3e38, 4, 20, 12], [10, 4, 20, 12]]
    badc = [[15, 8], [15, 8], [15, 8], [15, 8], [NAN, 8], [15, -INF], [INF, INF], [15, 8], [15, 8]]
    out.append(Case("non_finite_box_and_centre", [dict(boxes=bad, centers=badc)], (32, 96), (16, 48),
                    use_per_category_heatmap=False))
    out.append(Case("non_finite_box_default_centre", [dict(boxes=bad[:4] + [[3e38, 4, 3e38, 12], [10, 4, 20, 12]])], (32, 96),
                    (16, 48), use_per_category_heatmap=False))
    for dt in (torch.int32, torch.int64):
        hws = [(32, 96), (16, 48), (0, 48), (64, 0), (16, 200)]
        out.append(random_case(f"image_hw_per_frame_{str(dt)[6:]}", 130, [6, 5, 4, 3, 7], (16, 48), hws, C=2, hw_dtype=dt))
    out.append(random_case("image_hw_negative_and_huge", 131, [4, 4], (16, 48), [(-5, 48), (1 << 40, 1 << 40)], C=2,
                           hw_dtype=torch.int64))

    # seeded sweep: three tiles each way at the most
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        B, C = int(rng.integers(1, 5)), (None, 1, 2, 3, 4)[seed % 5]
        Hm, Wm = int(rng.integers(1, 6 * TH + 1)), int(rng.integers(1, 2 * TW + TW // 2 + 1))
        hw = (int(Hm * rng.uniform(0.7, 4)) + 1, int(Wm * rng.uniform(0.7, 4)) + 1)
        out.append(random_case(f"sweep_{seed}", 2000 + seed, [int(v) for v in rng.integers(0, 65, B)], (Hm, Wm), hw, C=C,
                               single=seed % 7 == 3, centers=seed % 3 != 1, valid=seed % 4 != 2, wild=0.04,
                               sized=(None, "global", "per_category")[seed % 3] if C else (None, "global")[seed % 2],
                               radius_scaling_factor=float(rng.choice([0.5, 0.8, 1.5])),
                               max_radius=float(rng.choice([10.0, 6.0])),
                               k_for_classes=None if seed % 2 else [0.5 + 0.5 * c for c in range(1 if C is None or seed % 7 == 3 else C)]))
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def case_names():
    return list(cases())
