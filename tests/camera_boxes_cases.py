"""Cases and the two oracles of camera_augment_boxes, shared by test_camera_boxes_cpu.py (the host entry) and
test_camera_boxes_gpu.py (the kernel).  Both oracles are numpy restatements of the definition in
accv-lab_amd/csrc/camera_boxes_arith.h and share no code with the library.

Oracle (a), `oracle_a`: the float32 operation sequence of the warp, the matrices and the crop, one IEEE operation per numpy
operator; the visibility of the warped boxes from the canvas painter of visible_boxes_cases.py (imported, not edited); the
compaction as a Python loop.  The operator must equal it exactly on every output tensor, padding and sizes included
(`assert_same`; NaN counts as equal to NaN at the same place).

Oracle (b), `oracle_b`: the warp, the crop and the matrices in float64, for coordinates and matrices only.  The bar per
element is n * 2^-24 * (the largest magnitude among that element's float64 intermediates, inputs included), n = the
roundings that feed the element: 4 for a point coordinate, 5 for an element of a matrix row (the header derives the same
numbers; test_camera_boxes_cpu.py checks that they agree).  Each rounding adds at most 2^-24 times what it rounds, the crop
is a clamp and widens no difference.  Decisions (visible, keep, source, counts) are compared with oracle (a) only: a
float64 warp may round an edge to the other side of an integer.  The cases named `exact` use matrices and coordinates whose
products are exact in float32, so both oracles warp alike; `built` asserts that they do.
"""
import numpy as np
import torch

import visible_boxes_cases as vb
from bev_augment_cases import same

N_POINT, N_MATRIX = 4, 5
U = 2.0 ** -24
F32 = np.float32
NAN, INF = float("nan"), float("inf")
HW = (40, 56)
IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


def hflip(W):
    return [[-1.0, 0.0, float(W)], [0.0, 1.0, 0.0]]


# ------------------------------------------------------------------------------------------------------------- inputs
class Case:
    """the inputs of one call, as numpy arrays; `hw` is (H, W) or an integer array [F, 2]; `kw` the keyword switches"""

    def __init__(self, boxes, sizes, transforms, hw=HW, centers=None, depths=None, categories=None, valid=None, mats=(),
                 sizes_dtype=np.int64, exact=False, **kw):
        self.boxes = np.ascontiguousarray(boxes, F32)
        self.sizes = np.asarray(sizes).astype(sizes_dtype)
        self.transforms = np.ascontiguousarray(transforms, F32)
        self.hw = hw
        self.centers = None if centers is None else np.ascontiguousarray(centers, F32)
        self.depths = None if depths is None else np.ascontiguousarray(depths, F32)
        self.categories, self.valid = categories, valid
        self.mats = [np.ascontiguousarray(m, F32) for m in mats]
        self.exact = exact
        self.kw = dict(check_occlusion=depths is not None, minimum_size=None, shrink_to_int=False, crop=True, order_corners=False)
        self.kw.update(kw)
        assert self.boxes.ndim == 3 and self.transforms.shape == (self.boxes.shape[0], 2, 3)

    def frame_hw(self, f):
        return tuple(int(v) for v in (self.hw if isinstance(self.hw, tuple) else self.hw[f]))

    def count(self, f):
        return int(min(max(int(self.sizes[f]), 0), self.boxes.shape[1]))


def from_frames(frames, transforms, G=None, hostile=True, **kw):
    """a Case from a list of (boxes, depths) frames; with `hostile` the padding slots hold drawable boxes that cover the
    image at depth -1 (on top of every real box), category 0 and valid, in turn with NaN and 1e30"""
    Fr = len(frames)
    G = max([len(f[0]) for f in frames] + [0]) if G is None else G
    boxes, depths = np.zeros((Fr, G, 4), F32), np.zeros((Fr, G), F32)
    if hostile and G:
        fill = np.array([[-5.0, -5.0, 4e3, 4e3], [NAN, NAN, NAN, NAN], [-1e30, -1e30, 1e30, 1e30], [0.0, 0.0, 30.0, 30.0]], F32)
        boxes[:] = fill[np.arange(G) % 4]
        depths[:] = -1.0
    for f, (bx, dp) in enumerate(frames):
        n = len(bx)
        if n:
            boxes[f, :n] = np.asarray(bx, F32).reshape(-1, 4)
            depths[f, :n] = np.asarray(dp, F32)
    return Case(boxes, [len(f[0]) for f in frames], transforms, depths=depths, **kw)


# ----------------------------------------------------------------------------------------------------------- oracle (a)
def _warp32(t, x, y):
    a, b, tx, c, d, ty = (F32(v) for v in t.reshape(-1))
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    ox = (a * x + b * y) + tx
    oy = (c * x + d * y) + ty
    assert ox.dtype == F32 and oy.dtype == F32
    return ox, oy


def _crop(v, E):
    E = v.dtype.type(E)
    return np.where(v < 0, v.dtype.type(0), np.where(v > E, E, v))


def _order(p, q):
    lt = p < q
    return np.where(lt, p, q), np.where(lt, q, p)


def _warp_frame(case, f, warp, dtype):
    """warped boxes [n, 4] and centres [n, 2] (or None) of the real slots of frame f"""
    n = case.count(f)
    bx = case.boxes[f, :n].astype(dtype)
    x1, y1 = warp(case.transforms[f], bx[:, 0], bx[:, 1])
    x2, y2 = warp(case.transforms[f], bx[:, 2], bx[:, 3])
    if case.kw["order_corners"]:
        (x1, x2), (y1, y2) = _order(x1, x2), _order(y1, y2)
    ctr = None
    if case.centers is not None:
        ctr = np.stack(warp(case.transforms[f], case.centers[f, :n, 0].astype(dtype), case.centers[f, :n, 1].astype(dtype)), 1)
    return np.stack([x1, y1, x2, y2], 1), ctr


def _matrix32(t, m):
    a, b, tx, c, d, ty = (F32(v) for v in t.reshape(-1))
    out = m.copy()
    out[..., 0, :] = (a * m[..., 0, :] + b * m[..., 1, :]) + tx * m[..., 2, :]
    out[..., 1, :] = (c * m[..., 0, :] + d * m[..., 1, :]) + ty * m[..., 2, :]
    return out


def oracle_a(case):
    Fr, G = case.boxes.shape[:2]
    out = dict(bboxes=np.zeros((Fr, G, 4), F32), source=np.full((Fr, G), -1, np.int32), keep=np.zeros((Fr, G), bool),
               visible=np.zeros((Fr, G), bool), sizes=np.zeros((Fr,), np.int64), mats=[np.zeros_like(m) for m in case.mats],
               centers=None if case.centers is None else np.zeros((Fr, G, 2), F32),
               depths=None if case.depths is None else np.zeros((Fr, G), F32),
               categories=None if case.categories is None else np.zeros_like(case.categories))
    kw = case.kw
    with np.errstate(all="ignore"):
        for f in range(Fr):
            n, (H, W) = case.count(f), (int(np.clip(v, 0, 1 << 24)) for v in case.frame_hw(f))
            warped, ctr = _warp_frame(case, f, _warp32, F32)
            vis = np.ones(n, bool)
            if n and (kw["check_occlusion"] or kw["minimum_size"] is not None):
                vis = vb.oracle_frame(warped, case.depths[f, :n] if kw["check_occlusion"] else None, (H, W),
                                      check_occlusion=kw["check_occlusion"], minimum_size=kw["minimum_size"],
                                      shrink_to_int=kw["shrink_to_int"])
            on = vis.copy()
            if case.categories is not None:
                on &= case.categories[f, :n] >= 0
            if case.valid is not None:
                on &= case.valid[f, :n] != 0
            out["visible"][f, :n], out["keep"][f, :n] = vis, on
            if kw["crop"]:
                warped = np.stack([_crop(warped[:, 0], W), _crop(warped[:, 1], H), _crop(warped[:, 2], W), _crop(warped[:, 3], H)], 1)
                if ctr is not None:
                    ctr = np.stack([_crop(ctr[:, 0], W), _crop(ctr[:, 1], H)], 1)
            kept = 0
            for g in range(n):             # the compaction, in slot order
                if on[g]:
                    out["bboxes"][f, kept] = warped[g]
                    out["source"][f, kept] = g
                    if ctr is not None:
                        out["centers"][f, kept] = ctr[g]
                    if case.depths is not None:
                        out["depths"][f, kept] = case.depths[f, g]
                    if case.categories is not None:
                        out["categories"][f, kept] = case.categories[f, g]
                    kept += 1
            out["sizes"][f] = kept
            for m_in, m_out in zip(case.mats, out["mats"]):
                m_out[f] = _matrix32(case.transforms[f], m_in[f])
    return out


# ----------------------------------------------------------------------------------------------------------- oracle (b)
def _warp64(t, x, y, mags=None):
    a, b, tx, c, d, ty = (float(v) for v in t.reshape(-1))
    ox, oy = (a * x + b * y) + tx, (c * x + d * y) + ty
    if mags is not None:
        mags.append(np.max(np.abs([x, y, a * x, b * y, a * x + b * y, np.full_like(x, tx), ox]), 0))
        mags.append(np.max(np.abs([x, y, c * x, d * y, c * x + d * y, np.full_like(x, ty), oy]), 0))
    return ox, oy


def oracle_b(case):
    """float64 values of EVERY real input slot (no compaction; the caller gathers by oracle (a)'s source), cropped like the
    operator's, and of every matrix, each with the per-element largest magnitude among its intermediates"""
    Fr, G = case.boxes.shape[:2]
    boxes, bmag = np.full((Fr, G, 4), np.nan), np.zeros((Fr, G, 4))
    ctrs, cmag = np.full((Fr, G, 2), np.nan), np.zeros((Fr, G, 2))
    raw = np.full((Fr, G, 4), np.nan)
    mats, mmag = [], []
    with np.errstate(all="ignore"):
        for f in range(Fr):
            n, (H, W) = case.count(f), case.frame_hw(f)
            mg = []
            warped, ctr = _warp_frame(case, f, lambda t, x, y: _warp64(t, x, y, mg), np.float64)
            if case.kw["order_corners"]:    # either corner may land in either place: the larger magnitude of the pair
                mg[0] = mg[2] = np.maximum(mg[0], mg[2])
                mg[1] = mg[3] = np.maximum(mg[1], mg[3])
            raw[f, :n] = warped
            if case.kw["crop"]:
                warped = np.stack([_crop(warped[:, 0], W), _crop(warped[:, 1], H), _crop(warped[:, 2], W), _crop(warped[:, 3], H)], 1)
                if ctr is not None:
                    ctr = np.stack([_crop(ctr[:, 0], W), _crop(ctr[:, 1], H)], 1)
            boxes[f, :n] = warped
            bmag[f, :n] = np.stack(mg[:4], 1) if n else 0
            if ctr is not None:
                ctrs[f, :n], cmag[f, :n] = ctr, (np.stack(mg[4:6], 1) if n else 0)
        for m_in in case.mats:
            m = m_in.astype(np.float64)
            out, mag = m.copy(), np.abs(m)
            for f in range(Fr):
                a, b, tx, c, d, ty = (float(v) for v in case.transforms[f].reshape(-1))
                m0, m1, m2 = m[f][..., 0, :], m[f][..., 1, :], m[f][..., 2, :]
                for row, (p, q, s) in enumerate(((a, b, tx), (c, d, ty))):
                    out[f][..., row, :] = (p * m0 + q * m1) + s * m2
                    mag[f][..., row, :] = np.max(np.abs([m0, m1, m2, p * m0, q * m1, p * m0 + q * m1, s * m2, out[f][..., row, :]]), 0)
            mats.append(out)
            mmag.append(mag)
    return dict(bboxes=boxes, bboxes_mag=bmag, centers=ctrs, centers_mag=cmag, mats=mats, mats_mag=mmag, raw=raw)


# ------------------------------------------------------------------------------------------------------ run and compare
def to_torch(case, device, categories_dtype=torch.int64, valid_dtype=torch.bool, hw_dtype=torch.int32, offset=False,
             ragged_fields=False):
    """(bboxes, transforms, kw) of camera_augment_boxes on `device`; with `offset`, boxes, transforms, centres and the first
    matrix tensor are contiguous views that start one element into their storage"""
    from accvlab.batching_helpers import RaggedBatch

    def place(a, shifted=False):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not shifted:
            return t.to(device)
        buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device=device)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.storage_offset() == 1 and view.is_contiguous()
        return view

    sizes = torch.from_numpy(case.sizes).to(device)
    rag = (lambda t: RaggedBatch(t, sample_sizes=sizes)) if ragged_fields else (lambda t: t)
    kw = dict(case.kw)
    kw["image_hw"] = case.hw if isinstance(case.hw, tuple) else torch.as_tensor(np.asarray(case.hw)).to(hw_dtype).to(device)
    kw["projection_matrices"] = tuple(place(m, offset and i == 0) for i, m in enumerate(case.mats))
    if case.centers is not None:
        kw["centers"] = rag(place(case.centers, offset))
    if case.depths is not None:
        kw["depths"] = rag(place(case.depths))
    if case.categories is not None:
        kw["categories"] = rag(torch.from_numpy(np.asarray(case.categories)).to(categories_dtype).to(device))
    if case.valid is not None:
        kw["valid"] = rag(torch.from_numpy(np.asarray(case.valid).astype(np.uint8)).to(valid_dtype).to(device))
    return RaggedBatch(place(case.boxes, offset), sample_sizes=sizes), place(case.transforms, offset), kw


def _inputs(boxes, transforms, kw):
    ts = [boxes.tensor, boxes.sample_sizes, transforms, *kw["projection_matrices"]]
    ts += [getattr(kw[k], "tensor", kw[k]) for k in ("centers", "depths", "categories", "valid") if k in kw]
    return ts + ([kw["image_hw"]] if isinstance(kw["image_hw"], torch.Tensor) else [])


def run(case, device, **how):
    """the operator's outputs as CPU tensors, in oracle (a)'s layout; the inputs must come back bit for bit"""
    from accvlab.draw_heatmap import camera_augment_boxes

    boxes, transforms, kw = to_torch(case, device, **how)
    before = [t.clone() for t in _inputs(boxes, transforms, kw)]
    out = camera_augment_boxes(boxes, transforms, **kw)
    for a, b in zip(before, _inputs(boxes, transforms, kw)):
        assert a.shape == b.shape and (a.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))), \
            "an input was modified"
    return flatten(out, case)


def flatten(out, case):
    shared = out.bboxes.sample_sizes
    assert shared.dtype == torch.int64 and out.source.sample_sizes is shared
    for name, given in (("centers", case.centers), ("depths", case.depths), ("categories", case.categories)):
        got = getattr(out, name)
        assert (got is None) == (given is None), name
        assert got is None or got.sample_sizes is shared
    assert out.keep.tensor.dtype == torch.bool and out.visible.tensor.dtype == torch.bool and out.source.tensor.dtype == torch.int32
    assert torch.equal(out.keep.sample_sizes.cpu().to(torch.int64), torch.from_numpy(case.sizes.astype(np.int64)))
    cpu = lambda r: None if r is None else r.tensor.cpu()   # noqa: E731
    return dict(bboxes=cpu(out.bboxes), centers=cpu(out.centers), depths=cpu(out.depths), categories=cpu(out.categories),
                source=cpu(out.source), keep=cpu(out.keep), visible=cpu(out.visible), sizes=shared.cpu(),
                mats=[t.cpu() for t in out.projection_matrices])


def _pairs(got, want):
    for name in ("bboxes", "source", "keep", "visible", "sizes", "centers", "depths", "categories"):
        if want[name] is not None:
            yield name, got[name], want[name]
    assert len(got["mats"]) == len(want["mats"])
    for i, (g, w) in enumerate(zip(got["mats"], want["mats"])):
        yield f"projection_matrices[{i}]", g, w


def differing(got, want):
    """the names of the output tensors of `got` that differ from `want` (oracle (a) as numpy, or another run)"""
    names = []
    for name, g, w in _pairs(got, want):
        w = torch.from_numpy(np.ascontiguousarray(w)) if isinstance(w, np.ndarray) else w
        if name == "categories":
            w = w.to(g.dtype)
        if not same(g, w):
            names.append(name)
    return names


def assert_same(got, want, what=""):
    names = differing(got, want)
    assert not names, f"{what} {', '.join(names)} differ"


def _ratio(got, ref, mag):
    """max |got - ref| / (2^-24 * mag) over the elements where ref is finite; got must be finite exactly where ref is, and
    equal to it where it is infinite"""
    with np.errstate(invalid="ignore"):     # a signalling NaN widens with a flag raised
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN where the float64 evaluation has none, or the reverse"
        assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "infinities differ"
        diff = np.abs(np.where(fin, got - ref, 0.0))
    exact = fin & (mag == 0)
    assert not diff[exact].any()
    live = fin & (mag > 0)
    return float((diff[live] / (U * mag[live])).max()) if live.any() else 0.0


def check_against_b(got, case, a, report=None, what=""):
    """`got` against the float64 evaluation within n * 2^-24 * the element's largest intermediate; the kept slots are found
    through oracle (a)'s source.  Returns the ratios error / (2^-24 * magnitude)."""
    ref = oracle_b(case)
    ratios = {}
    for name in ("bboxes", "centers"):
        if a[name] is None:
            continue
        g, r, m = [], [], []
        for f in range(case.boxes.shape[0]):
            for j in range(int(a["sizes"][f])):
                g.append(got[name][f, j].numpy()), r.append(ref[name][f, a["source"][f, j]]), m.append(ref[name + "_mag"][f, a["source"][f, j]])
        if g:
            ratios[name] = (_ratio(np.stack(g), np.stack(r), np.stack(m)), N_POINT)
    for i, (g, r, m) in enumerate(zip(got["mats"], ref["mats"], ref["mats_mag"])):
        if g.numel():
            ratios[f"projection_matrices[{i}]"] = (_ratio(g.numpy(), r, m), N_MATRIX)
    for name, (ratio, n) in ratios.items():
        line = f"{what} {name}: max error {ratio:.3f} x 2^-24 x largest intermediate (bar {n})"
        print(line)
        if report is not None:
            report.append(line)
    for name, (ratio, n) in ratios.items():
        assert ratio <= n, f"{what} {name}: {ratio:.3f} x 2^-24 x largest intermediate exceeds the bar of {n}"
    return ratios


# --------------------------------------------------------------------------------------------------------------- cases
def identity_case():
    """the partition frames of the visible-box tests under the identity matrix, uncropped, without categories"""
    frames = [(f[0], f[1]) for f in vb.partition_frames()[:8]] + [(f[0], f[1]) for f in vb.sweep_frames(5, 6)]
    # one image extent for all: the sweep frames bring their own, which only changes what is inside
    return from_frames(frames, [IDENTITY] * len(frames), crop=False, exact=True)


H0, W0 = HW
# slot 0 lies behind slot 1; slot 2 stands alone on the right and lands on the left; slot 3 is flipped on input
FLIP_BOXES = [[10, 10, 30, 30], [8, 8, 32, 32], [40, 5, 50, 15], [30.5, 20.25, 20.125, 38]]
FLIP_DEPTHS = [5, 1, 3, 0.5]


def flip_case(order_corners=False):
    ctr = np.array([[[(b[0] + b[2]) / 2, (b[1] + b[3]) / 2] for b in FLIP_BOXES]], F32)
    return from_frames([(FLIP_BOXES, FLIP_DEPTHS)], [hflip(W0)], centers=ctr, order_corners=order_corners, exact=True,
                       mats=[np.arange(12, dtype=F32).reshape(1, 3, 4)])


def border_case():
    """x' = 2x - 40, y' = 2y - 20 on a 40 x 56 image: slot 0 ends up left of the image, slot 1 half outside, slot 2 inside,
    slot 3 below the image, slot 4 reaches over the lower right corner"""
    boxes = [[2, 12, 10, 20], [15, 12, 25, 20], [30, 15, 40, 25], [25, 31, 30, 36], [44.5, 25.25, 50, 32]]
    ctr = np.array([[[6, 16], [20, 16], [35, 20], [27.5, 33.5], [47.25, 28.625]]], F32)
    return from_frames([(boxes, [1, 2, 3, 4, 5])], [[[2.0, 0.0, -40.0], [0.0, 2.0, -20.0]]], centers=ctr, minimum_size=2, exact=True)


def condition_case():
    """frame 0: a box of category -1 in front of a valid one; frame 1: the same with valid = False; frame 2: both wanted"""
    boxes, depths = [[8, 8, 32, 32], [10, 10, 30, 30], [40, 20, 50, 30]], [1, 5, 2]
    cats = np.array([[-1, 3, 2], [4, 3, -7], [4, 3, 2]], np.int64)
    valid = np.array([[1, 1, 1], [0, 1, 1], [1, 1, 1]], bool)
    c = from_frames([(boxes, depths)] * 3, [IDENTITY, hflip(W0), IDENTITY], categories=cats, valid=valid, exact=True)
    return c


def _ulp(v, up):
    return float(np.nextafter(F32(v), F32(INF if up else -INF)))


def crop_case(crop=True):
    """frame 0 under the identity: coordinates one ulp inside and outside 0, W and H, and NaN; frame 1 under x' = 2x: 3e38
    overflows to +-inf without a NaN beside it.  No check: every real slot is visible and kept."""
    f0 = [[_ulp(0, False), _ulp(0, True), _ulp(W0, False), _ulp(W0, True)],
          [_ulp(0, True), _ulp(0, False), _ulp(W0, True), _ulp(H0, True)],
          [5, _ulp(H0, False), NAN, 7], [NAN, NAN, NAN, NAN], [-0.0, -0.0, W0, H0], [-3, -4, 100, 90]]
    f1 = [[-3e38, 5, 3e38, 7], [3e38, 50, -3e38, -9], [1, 2, 3, 4], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    boxes = np.array([f0, f1], F32)
    ctr = boxes[:, :, [0, 3]].copy()
    return Case(boxes, [6, 3], [IDENTITY, [[2.0, 0.0, 0.0], [0.0, 1.0, 0.0]]], centers=ctr, crop=crop)


SNAN = np.array([0x7FA00001, 0xFFC12345, 0x7F800000, 0x80000000], np.uint32).view(F32)   # NaN payloads, inf, -0.0


def _general(rng, shape):
    return rng.uniform(-900, 900, shape).astype(F32)


def matrices_case(which, seed=9):
    """`which`: "shapes" (3 x 3 as [F, 3, 3], 3 x 4 as [F, 1, 3, 4], 4 x 4 as [F, 6, 4, 4], K = 0) or "big" ([F, 20, 4, 4]:
    320 elements per frame, and [F, 4, 4]); frame 1 has NaN and inf in its transform; rows 2 and 3 hold NaN payloads"""
    rng = np.random.default_rng(seed)
    Fr = 3
    t = np.array([[[0.44, 0.0, -12.5], [0.0, 0.44, -3.25]], [[NAN, 1.0, INF], [0.5, NAN, 2.0]], [[-0.5, 0.125, 700.0], [0.25, 1.5, -8.0]]], F32)
    if which == "shapes":
        mats = [_general(rng, (Fr, 3, 3)), _general(rng, (Fr, 1, 3, 4)), _general(rng, (Fr, 6, 4, 4)), np.zeros((Fr, 0, 4, 4), F32)]
    else:
        mats = [_general(rng, (Fr, 20, 4, 4)), _general(rng, (Fr, 4, 4))]
    for m in mats:
        if m.size:
            m[..., 2, :] = np.resize(SNAN, m[..., 2, :].shape) if m.shape[-2] == 3 else m[..., 2, :]
            if m.shape[-2] == 4:
                m[..., 3, :] = np.resize(SNAN, m[..., 3, :].shape)
                m[:, ..., 2, 0] = SNAN[0]
    boxes = np.zeros((Fr, 2, 4), F32)
    boxes[:, 0] = (3, 4, 20, 30)
    return Case(boxes, [1, 0, 1], t, mats=mats)


PARTITION = {1: [1, 0, 1], 64: [63, 64, 0, 1, 64], 65: [65, 64, 63], 256: [128, 129, 255, 256, 0]}


def partition_case(G, seed=13):
    """frames of the counts of PARTITION[G] on a flipped, scaled image, every field given, hostile padding"""
    rng = np.random.default_rng(seed + G)
    counts = PARTITION[G]
    frames = [vb.random_frame(rng, n, HW, depth_values=24)[:2] for n in counts]
    Fr = len(counts)
    t = [[[-0.875, 0.0, 52.5], [0.0, 0.875, 2.25]], hflip(W0), IDENTITY, [[1.25, 0.0, -6.0], [0.0, 1.25, -4.5]], hflip(W0)][:Fr]
    ctr = rng.integers(-8, 2 * W0, (Fr, G, 2)).astype(F32) / 2
    return from_frames(frames, t, G=G, centers=ctr, categories=rng.integers(-1, 6, (Fr, G)), valid=rng.random((Fr, G)) < 0.8,
                       minimum_size=2, mats=[_general(rng, (Fr, 2, 3, 4))])


def clamped_case(seed=17):
    rng = np.random.default_rng(seed)
    frames = [vb.random_frame(rng, 70, HW)[:2] for _ in range(3)]
    c = from_frames(frames, [hflip(W0), IDENTITY, hflip(W0)], categories=rng.integers(-1, 6, (3, 70)), minimum_size=2)
    c.sizes = np.array([1000, -5, 41], np.int64)
    return c


def dtypes_case(seed=19):
    """per-frame image extents, every optional field"""
    rng = np.random.default_rng(seed)
    hw = np.array([[40, 56], [24, 30], [12, 20]])
    frames = [vb.random_frame(rng, n, tuple(hw[i]))[:2] for i, n in enumerate((30, 17, 0))]
    ctr = rng.integers(0, 100, (3, 30, 2)).astype(F32) / 2
    return from_frames(frames, [hflip(56), IDENTITY, IDENTITY], hw=hw, centers=ctr, categories=rng.integers(-1, 6, (3, 30)),
                       valid=rng.random((3, 30)) < 0.8, minimum_size=1.5, mats=[_general(rng, (3, 3, 3))])


def sweep_case(seed, shrink=False):
    """dataset-like frames: 900 x 1600 boxes brought to 256 x 704 by flip, scale and crop matrices whose products are not
    exact; lidar2img as [F, 4, 4], intrinsics as [F, 3, 3]"""
    rng = np.random.default_rng(seed)
    Fr, G = 6, 48
    counts = rng.integers(0, G + 1, Fr)
    frames, t = [], []
    for n in counts:
        bx, dp, _ = vb.random_frame(rng, int(n), (900, 1600))
        frames.append((bx + rng.uniform(-0.5, 0.5, bx.shape), dp + 1))
        s = rng.uniform(0.40, 0.48)
        flip = rng.random() < 0.5
        t.append([[-s if flip else s, 0.0, (704 + rng.uniform(-30, 30)) if flip else rng.uniform(-30, 30)], [0.0, s, 256 - 900 * s]])
    ctr = np.stack([rng.uniform(0, 1600, (Fr, G)), rng.uniform(0, 900, (Fr, G))], -1)
    return from_frames(frames, t, G=G, hw=(64, 96) if shrink else (256, 704), centers=ctr, categories=rng.integers(-1, 10, (Fr, G)),
                       valid=rng.random((Fr, G)) < 0.9, minimum_size=2, shrink_to_int=shrink,
                       mats=[_general(rng, (Fr, 4, 4)), _general(rng, (Fr, 3, 3))])


def empty_case(which):
    if which == "F0":
        return Case(np.zeros((0, 4, 4), F32), [], np.zeros((0, 2, 3), F32), depths=np.zeros((0, 4), F32), centers=np.zeros((0, 4, 2), F32),
                    categories=np.zeros((0, 4), np.int64), mats=[np.zeros((0, 4, 4), F32)])
    return Case(np.zeros((2, 0, 4), F32), [0, 0], [IDENTITY, hflip(W0)], depths=np.zeros((2, 0), F32), categories=np.zeros((2, 0), np.int64),
                mats=[np.arange(24, dtype=F32).reshape(2, 3, 4)] if which == "G0-matrices" else [])


CASES = {
    "identity": identity_case,
    "flip": flip_case,
    "flip-ordered": lambda: flip_case(order_corners=True),
    "border": border_case,
    "condition": condition_case,
    "crop": crop_case,
    "crop-off": lambda: crop_case(crop=False),
    "matrices-shapes": lambda: matrices_case("shapes"),
    "matrices-big": lambda: matrices_case("big"),
    **{f"partition-G{G}": (lambda G=G: partition_case(G)) for G in PARTITION},
    "clamped": clamped_case,
    "dtypes": dtypes_case,
    "sweep-1": lambda: sweep_case(1),
    "sweep-2-shrink": lambda: sweep_case(2, shrink=True),
    "empty-F0": lambda: empty_case("F0"),
    "empty-G0": lambda: empty_case("G0"),
    "empty-G0-matrices": lambda: empty_case("G0-matrices"),
}
# the cases whose real coordinates and matrices are numbers of ordinary size: compared with oracle (b) too (it handles NaN
# and inf where they stand, but "crop" holds subnormals, whose rounding is absolute, not relative)
B_CASES = {n for n in CASES if not n.startswith(("crop", "empty"))}
_BUILT = {}


def built(name):
    """(case, oracle (a)) of a named case, computed once per process and never modified"""
    if name not in _BUILT:
        case = CASES[name]()
        a = oracle_a(case)
        if case.exact:                      # both oracles warp alike, so they decide alike
            raw = oracle_b(case)["raw"]
            for f in range(case.boxes.shape[0]):
                w32, _ = _warp_frame(case, f, _warp32, F32)
                assert np.array_equal(w32.astype(np.float64), raw[f, :case.count(f)], equal_nan=True), f"{name}: the warp is not exact"
        _BUILT[name] = (case, a)
    return _BUILT[name]


def check_case(name, device, report=None, **how):
    """the operator on `device` equals oracle (a) on every output, and lies within the bar of oracle (b)"""
    case, a = built(name)
    got = run(case, device, **how)
    assert_same(got, a, f"{name} on {device}:")
    if name in B_CASES:
        check_against_b(got, case, a, report=report, what=f"{name} on {device}:")
    return case, a, got


def c_entry_args(case, device, bands=None):
    """(args, params, outputs) of the C entries for a case: outputs are fresh tensors, or the inner views of `bands`"""
    import ctypes

    from accvlab import _amd_native as nat

    boxes, transforms, kw = to_torch(case, device)
    Fr, G = case.boxes.shape[:2]
    shapes = dict(bboxes=((Fr, G, 4), torch.float32), source=((Fr, G), torch.int32), keep=((Fr, G), torch.bool),
                  visible=((Fr, G), torch.bool), sizes=((Fr,), torch.int64))
    if case.centers is not None:
        shapes["centers"] = ((Fr, G, 2), torch.float32)
    if case.depths is not None:
        shapes["depths"] = ((Fr, G), torch.float32)
    if case.categories is not None:
        shapes["categories"] = ((Fr, G), torch.int64)
    for i, m in enumerate(case.mats):
        shapes[f"mats{i}"] = (tuple(m.shape), torch.float32)
    make = bands if bands is not None else (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device))
    out = {k: make(*v) for k, v in shapes.items()}
    inner = (lambda k: out[k][1]) if bands is not None else (lambda k: out[k])
    p = nat.CameraBoxesParams()
    p.minimum_size = float(case.kw["minimum_size"] or 0.0)
    hw = kw["image_hw"]
    if isinstance(hw, torch.Tensor):
        p.image_hw = hw.data_ptr()
    else:
        p.image_h, p.image_w = hw
    for i, m in enumerate(kw["projection_matrices"]):
        p.mat_in[i], p.mat_out[i] = m.data_ptr(), inner(f"mats{i}").data_ptr()
        p.mat_count[i], p.mat_rows[i], p.mat_cols[i] = (m.shape[1] if m.dim() == 4 else 1), m.shape[-2], m.shape[-1]
    p.num_matrices = len(case.mats)
    p.check_occlusion, p.check_size = int(case.kw["check_occlusion"]), int(case.kw["minimum_size"] is not None)
    p.shrink_to_int, p.crop, p.order_corners = int(case.kw["shrink_to_int"]), int(case.kw["crop"]), int(case.kw["order_corners"])
    flags = (nat.CB_COUNTS_I64 if case.sizes.dtype == np.int64 else 0) | (nat.CB_CATEGORIES_I64 if case.categories is not None else 0)
    ptr = lambda k, src: (src[k].data_ptr() if k in src else None)   # noqa: E731
    optr = lambda k: (inner(k).data_ptr() if k in out else None)   # noqa: E731
    args = [boxes.tensor.data_ptr(), transforms.data_ptr(), ptr("centers", kw), ptr("depths", kw), ptr("categories", kw),
            ptr("valid", kw), boxes.sample_sizes.data_ptr(), flags, Fr, G, ctypes.addressof(p), optr("bboxes"), optr("centers"),
            optr("depths"), optr("categories"), optr("source"), optr("keep"), optr("visible"), optr("sizes")]
    return args, p, out, (boxes, transforms, kw)


def call_c_entry(args, device, trampoline=False):
    from accvlab import _amd_native as nat

    lib = nat.lib() if trampoline else nat.ctypes_lib()
    if torch.device(device).type == "cuda":
        status = lib.accv_camera_boxes(*args, nat.stream_ptr(torch.device("cuda", torch.cuda.current_device())))
        torch.cuda.synchronize()
        return status
    return lib.accv_camera_boxes_host(*args)


def check_guard_bands(name, device, trampoline=False):
    """the C entry alone on sentinel-filled outputs between guard bands: nothing outside is touched, and everything inside
    is written (it equals oracle (a), padding included)"""
    from accvlab import _amd_native as nat

    case, a = built(name)
    pad = 512

    def banded(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=device)   # the sentinel fills the inside too
        return buf, buf[pad: pad + nbytes].view(dtype).view(shape)

    args, p, out, keepalive = c_entry_args(case, device, bands=banded)
    status = call_c_entry(args, device, trampoline)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    for key, (buf, inner) in out.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{key}: wrote outside its buffer"
    got = {k: (out[k][1].cpu() if k in out else None) for k in ("bboxes", "centers", "depths", "categories", "source", "keep",
                                                                 "visible", "sizes")}
    got["mats"] = [out[f"mats{i}"][1].cpu() for i in range(len(case.mats))]
    assert_same(got, a, f"{name} banded:")
