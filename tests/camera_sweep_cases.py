"""Seeded random draws for the sweeps of the camera-side and augmentation operators (test_camera_sweeps_cpu.py,
test_camera_sweeps_gpu.py), in the form of operator_sweep_cases.py (§9q), whose helpers it reuses.

One function per operator: ``draw_<operator>(rng, device="cpu") -> (inputs, kwargs, description)``.  Every draw is a pure
function of the numpy generator: the seed of the generator and the number of draws taken from it reproduce a case, and
`description` names every drawn parameter for the failure message.  The inputs come from the builders of the operators' own
``*_cases.py`` modules (seeded from `rng`); what is drawn here is what those builders take as arguments.

Every value list straddles a constant of the operator's kernel: wave 64, workgroup or chunk 256 (MAX_BOXES of the visible-box
and heat-map kernels), the 64 x 16 output tile and the four pixels a lane of image_prep.hip stores, the even / odd chroma
positions of nv12.hip, 1024 peaks of box_decode.hip.  Where a definition is a Python loop, the batch size or frame count is
cut so that a case stays within a fraction of a second on the CPU; the cut keeps the drawn edge (G, N, K).

All operators here have a host entry that the device is held bit-equal to, and all comparisons with a definition are exact
or have a derived bar; the only margins are the decoder's score threshold under sigmoid scores and the IoU threshold where
the float64 greedy loop is consulted (see `draw_box_heatmap_decode`).
"""
import math

import numpy as np
import torch

from operator_sweep_cases import FLOATS3, INTS, Worst, name, pick, ragged_sizes, seed_of  # noqa: F401

F32 = np.float32
NAN, INF = float("nan"), float("inf")
FLAGS = [torch.bool, torch.uint8]
BOX_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256]      # one lane per slot, 256 slots, wave ranks
MINIMUM_SIZES = [None, 1.5, 2]
# redraws of a case whose comparison sat on a threshold, per operator (the tests assert their share)
REDRAWS = {"box_heatmap_decode": 0, "nms_boxes": 0}


def _hw(rng, lo=(1, 1), hi=(64, 96)):
    return int(rng.integers(lo[0], hi[0] + 1)), int(rng.integers(lo[1], hi[1] + 1))


# ------------------------------------------------------------------------------------------------------- visible boxes
def draw_visible_boxes(rng, device="cpu"):
    """inputs: (frames, G, (bboxes, depths, image_hw)) with the frames as numpy for visible_boxes_cases.oracle and the
    batch on `device`; image_hw is a tuple (one extent for every frame) or a tensor [B, 2].  kwargs: the operator's
    switches.  The canvas oracle paints H x W per frame: extents stay at or below 64 x 96."""
    import visible_boxes_cases as vb

    G = pick(rng, BOX_COUNTS)
    B = int(rng.integers(1, 7))
    sizes = ragged_sizes(rng, B, G)
    common = bool(rng.integers(0, 2))
    hws = [_hw(rng)] * B if common else [_hw(rng) for _ in range(B)]
    kw = dict(check_occlusion=bool(rng.integers(0, 4) > 0), minimum_size=pick(rng, MINIMUM_SIZES), shrink_to_int=bool(rng.integers(0, 2)))
    if not kw["check_occlusion"] and kw["minimum_size"] is None:      # the operator wants one check at least
        kw["minimum_size"] = 1.5
    depth_values = pick(rng, [2, 8, 24])
    hostile = bool(rng.integers(0, 4) > 0)
    size_dtype, hw_dtype = pick(rng, INTS), pick(rng, INTS)
    seed = seed_of(rng)
    frng = np.random.default_rng(seed)
    frames = [vb.random_frame(frng, n, hw, depth_values=depth_values) for n, hw in zip(sizes, hws)]
    boxes, depths, hw = vb.batch(frames, G, device, hostile_padding=hostile, size_dtype=size_dtype, hw_dtype=hw_dtype)
    what = (f"visible_boxes G {G} sizes {sizes} image_hw {'common ' + str(hws[0]) if common else hws} depth values {depth_values} "
            f"hostile padding {hostile} sizes as {name(size_dtype)} hw as {name(hw_dtype)} builder seed {seed} {kw}")
    return (frames, G, (boxes, depths, hws[0] if common else hw)), kw, what


# ---------------------------------------------------------------------------------------------------- boxes_to_heatmap
def draw_boxes_to_heatmap(rng, device="cpu"):
    """inputs: a box_heatmap_cases.Case named by its description (its oracle comes from box_heatmap_cases.oracle_of, not
    from the module's cache by name: the CPU and the GPU file draw two objects of one name); kwargs: size_dtype for
    box_heatmap_cases.batch"""
    import box_heatmap_cases as bc

    G = pick(rng, [0, 1, 63, 64, 65, 255, 256])                 # records per workgroup; MAX_BOXES
    Wm, Hm = pick(rng, [1, 3, 4, 5, 63, 64, 65, 131]), pick(rng, [1, 15, 16, 17, 33])      # 64 x 16 tiles, 16-byte stores
    B = int(rng.integers(1, 5))
    sizes = ragged_sizes(rng, B, G)
    per_frame = bool(rng.integers(0, 2))
    scale = lambda: (int(Hm * rng.uniform(0.7, 4)) + 1, int(Wm * rng.uniform(0.7, 4)) + 1)   # noqa: E731  non-integer image-to-map scale
    image_hw = [scale() for _ in range(B)] if per_frame else scale()
    C = pick(rng, [None, 1, 3, 10, 128])
    single = bool(C is not None and rng.integers(0, 3) == 0)
    centers, valid = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    wild = pick(rng, [0.0, 0.05])
    sized = pick(rng, [None, "global", "per_category"] if C is not None else [None, "global"])
    cat_dtype, hw_dtype, size_dtype = pick(rng, INTS), pick(rng, [None] + INTS), pick(rng, INTS)
    planes = 1 if C is None or single else C
    kw = dict(radius_scaling_factor=pick(rng, [0.5, 0.8, 1.5, 2.0]), max_radius=pick(rng, [10.0, 6.0]),
              # a map of one row or column clips every extent to 0: only a threshold of 0 lets anything be drawn
              min_fraction_area_clipping=0.0 if min(Hm, Wm) == 1 else pick(rng, [0.25, 0.0]))
    if rng.integers(0, 2):
        kw["k_for_classes"] = [0.5 + 0.5 * (c % 4) for c in range(planes)]
    seed = seed_of(rng)
    what = (f"boxes_to_heatmap G {G} sizes {sizes} map {Hm} x {Wm} image_hw {image_hw} C {C} single {single} centres {centers} "
            f"valid {valid} wild {wild} sized {sized} categories {name(cat_dtype)} hw {name(hw_dtype) if hw_dtype else 'as given'} "
            f"sizes as {name(size_dtype)} builder seed {seed} {kw}")
    case = bc.random_case(what, seed, sizes, (Hm, Wm), image_hw, C=C, single=single, G=G, centers=centers, valid=valid, wild=wild,
                          sized=sized, cat_dtype=cat_dtype, hw_dtype=hw_dtype, **kw)
    return case, dict(size_dtype=size_dtype), what


# ------------------------------------------------------------------------------------------------------ prepare_images
SOURCE_H, SOURCE_W = [1, 2, 7, 20, 33], [1, 3, 4, 5, 27, 64, 65]
MATRIX_KINDS = ["none", "identity", "output_size", "x_flip", "rotation"]


def _matrix(rng, kind, src, dst):
    import image_prep_cases as ic

    if kind == "identity":
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], "identity"
    if kind == "output_size":
        mode, anchor = pick(rng, ["stretch", "pad", "crop"]), pick(rng, ["top_or_left", "center", "bottom_or_right"])
        return ic.output_size_transform(src, dst, mode, anchor), f"{mode}/{anchor}"
    if kind == "x_flip":
        s, t = dst[1] / src[1], dst[0] / src[0]
        return [[-s, 0.0, float(dst[1])], [0.0, t, 0.0]], f"flip {s:.3f} {t:.3f}"
    angle, scale, shear = float(rng.uniform(-math.pi, math.pi)), float(rng.uniform(0.4, 2.5)), float(rng.uniform(-0.3, 0.3))
    c, s = math.cos(angle) * scale, math.sin(angle) * scale
    lin = ((c, c * shear - s), (s, s * shear + c))                        # rotation x scale x shear
    return ic._about_centre(lin, src, dst), f"angle {angle:.3f} scale {scale:.3f} shear {shear:.3f}"


BROKEN = {"zero": [[0, 0, 0], [0, 0, 0]], "rank_1": [[1, 2, 0], [2, 4, 1]], "nan": [[1, 0, NAN], [0, 1, 0]], "inf": [[INF, 0, 0], [0, 1, 0]]}


def draw_prepare_case(rng, tag="prepare_images"):
    """the geometry, colour and normalisation part of a prepare_images draw, shared with prepare_images_nv12:
    (image_prep_cases.Case with seeded noise images, dict(source_hw dtype), description)"""
    import image_prep_cases as ic

    B = int(rng.integers(1, 4))
    Hs, Ws = pick(rng, SOURCE_H), pick(rng, SOURCE_W)
    kind = pick(rng, MATRIX_KINDS)
    Ho, Wo = (Hs, Ws) if kind == "none" else (pick(rng, list(ic.PARTITION_HEIGHTS)), pick(rng, list(ic.PARTITION_WIDTHS)))
    mats, mat_what = None, []
    if kind != "none":
        mats = []
        for _ in range(B):
            m, w = _matrix(rng, kind, (Hs, Ws), (Ho, Wo))
            mats.append(m), mat_what.append(w)
        if rng.integers(0, 5) == 0:                                  # one image of the batch without an inverse
            b, how = int(rng.integers(0, B)), pick(rng, sorted(BROKEN))
            mats[b], mat_what[b] = BROKEN[how], how
        mats = np.asarray(mats, F32).reshape(B, 2, 3)
    source_hw, src_dtype = None, pick(rng, INTS)
    if rng.integers(0, 2):
        source_hw = np.stack([rng.integers(0, Hs + 2, B), rng.integers(0, Ws + 2, B)], 1)     # [0, extent + 1]: clamped
    photometric = None
    if rng.integers(0, 3) > 0:
        rows = []
        for b in range(B):
            on = rng.integers(0, 3, 6) > 0                           # each stage off in a third of the rows: the skips
            row = [rng.uniform(-0.3, 0.3) if on[0] else 0.0, rng.uniform(0.5, 1.5) if on[1] else 1.0,
                   rng.uniform(0.5, 2.0) if on[2] else 1.0, rng.uniform(-180, 180) if on[3] else 0.0,
                   rng.uniform(0.5, 1.5) if on[4] else 1.0, float(rng.integers(0, 6)) if on[5] else 0.0]
            rows.append(row)
        if rng.integers(0, 4) == 0:
            rows[int(rng.integers(0, B))][5] = pick(rng, [7.0, 2.5, -1.0])       # an invalid index is permutation 0
        photometric = np.asarray(rows, F32)
    kw = dict(is_bgr=bool(rng.integers(0, 2)), pad_before_normalize=bool(rng.integers(0, 2)))
    kw.update(pick(rng, [{}, ic.NORM, dict(mean=0.0, std=255.0)]))
    tile = pick(rng, [1, 4, (8, 32), 32, "larger"])
    kw["tile_hw"] = (Ho + 3, Wo + 5) if tile == "larger" else tile
    seed = seed_of(rng)
    images = np.random.default_rng(seed).integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    what = (f"{tag} B {B} source {Hs} x {Ws} output {Ho} x {Wo} matrix {kind} {mat_what} source_hw "
            f"{None if source_hw is None else source_hw.tolist()} as {name(src_dtype)} photometric "
            f"{None if photometric is None else np.round(photometric, 3).tolist()} builder seed {seed} {kw}")
    case = ic.Case(what, images, output_hw=None if kind == "none" else (Ho, Wo), transforms=mats, source_hw=source_hw,
                   photometric=photometric, kw=kw)
    return case, src_dtype, what


def prepare_tensors(case, src_dtype, device):
    """the tensor keyword arguments of prepare_images / prepare_images_nv12 for a drawn case (without the images)"""
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)   # noqa: E731
    return dict(transforms=t(case.transforms, torch.float32), source_hw=t(case.source_hw, src_dtype),
                photometric=t(case.photometric, torch.float32), output_hw=case.output_hw, **case.kw)


def draw_store(rng):
    """how the result is stored: layout, dtype, and `out=` absent, aligned, or 1 or 3 elements off alignment"""
    return dict(layout=pick(rng, ["CHW", "HWC"]), dtype=pick(rng, FLOATS3), out=pick(rng, [None, 0, 1, 3]))


BAND, SENTINEL = 64, -7.0


def banded_out(shape, dtype, shift, device):
    """(buffer, view): a view of `shape` full of NaN, `shift` elements off a 16-byte base, inside a buffer of sentinels"""
    n = int(np.prod(shape))
    buf = torch.full((BAND + shift + n + BAND,), SENTINEL, dtype=dtype, device=device)
    out = buf[BAND + shift: BAND + shift + n].view(shape)
    out.fill_(NAN)
    assert out.data_ptr() % 16 == (shift * out.element_size()) % 16
    return buf, out


def bands_intact(buf, shift, n):
    return bool((buf[:BAND + shift] == SENTINEL).all()) and bool((buf[BAND + shift + n:] == SENTINEL).all())


def draw_prepare_images(rng, device="cpu"):
    """inputs: (image_prep_cases.Case, images uint8 on `device`); kwargs: `tensors` (the operator's keyword arguments on
    `device`) and `store` (draw_store)"""
    case, src_dtype, what = draw_prepare_case(rng)
    store = draw_store(rng)
    images = torch.from_numpy(case.images).to(device)
    what += f" store {store['layout']} {name(store['dtype'])} out {store['out']}"
    return (case, images), dict(tensors=prepare_tensors(case, src_dtype, device), store=store), what


# ---------------------------------------------------------------------------------------------------------------- NV12
def draw_format(rng):
    return dict(full_range=bool(rng.integers(0, 2)), as_bgr=bool(rng.integers(0, 2)), chroma_order=pick(rng, ["uv", "vu"]))


def _planes(rng, B, H, W, device):
    """pitched plane views of drawn surfaces and what was drawn for them"""
    import nv12_cases as nc
    from accvlab.image_prep import nv12_planes

    extra, gap, fill, seed = int(rng.integers(0, 14)), int(rng.integers(0, 4)), pick(rng, [0, 255, 77]), seed_of(rng)
    s, uv_row = nc.surfaces(B, H, W, seed, fill=fill, extra_pitch=extra, uv_gap=gap, device=device)
    return nv12_planes(s, (H, W), uv_row=uv_row), f"extra pitch {extra} plane gap {gap} fill {fill} surface seed {seed}"


def draw_nv12_to_rgb(rng, device="cpu"):
    """inputs: (y, uv) plane views on `device`; kwargs: the format"""
    import nv12_cases as nc

    B = int(rng.integers(1, 4))
    H, W = pick(rng, list(nc.GRID_H) + [15, 16, 17, 33]), pick(rng, list(nc.GRID_W))
    fmt = draw_format(rng)
    planes, how = _planes(rng, B, H, W, device)
    return planes, fmt, f"nv12_to_rgb B {B} {H} x {W} {fmt} {how}"


def draw_prepare_images_nv12(rng, device="cpu"):
    """inputs: (y, uv) plane views of the case's source extent on `device`; kwargs: `format`, `tensors`, `store`.  The
    contract is bit-equality with prepare_images(nv12_to_rgb(...)), which has no bar: `is_bgr` follows `as_bgr`."""
    case, src_dtype, what = draw_prepare_case(rng, "prepare_images_nv12")
    store = draw_store(rng)
    fmt = draw_format(rng)
    B, Hs, Ws = case.images.shape[:3]
    planes, how = _planes(rng, B, Hs, Ws, device)
    tensors = prepare_tensors(case, src_dtype, device)
    tensors.pop("is_bgr")
    what += f" store {store['layout']} {name(store['dtype'])} out {store['out']} {fmt} {how}"
    return planes, dict(format=fmt, tensors=tensors, store=store), what


# --------------------------------------------------------------------------------------------------- bev_augment_boxes
def draw_bev_augment_boxes(rng, device="cpu"):
    """inputs: a bev_augment_cases.Case (numpy); kwargs: `how` for bev_augment_cases.run (dtypes, offset views) and
    `ordinary` (whether oracle (b) applies).  The module's rule for oracle (b): real boxes and matrices finite and of
    ordinary size, which every draw here is (padding slots are hostile, but oracle (b) reads real slots only)."""
    import bev_augment_cases as ba

    N = pick(rng, list(ba.FRAME_SIZES) + [513])                  # chunks of 256 with the alternating LDS row
    D = pick(rng, [7, 9])
    B = int(rng.integers(1, 7))
    counts = ragged_sizes(rng, B, N)
    if rng.integers(0, 2):                                       # counts outside [0, N] are clamped
        counts[int(rng.integers(0, B))] = N + int(rng.integers(1, 1000))
        if B > 1:
            counts[int(rng.integers(0, B))] = -int(rng.integers(1, 1000))
    seed = seed_of(rng)
    brng = np.random.default_rng(seed)
    boxes = ba.fill_padding(ba.random_boxes(brng, B, N, D), [min(max(c, 0), N) for c in counts])
    params = ba.random_params(brng, B)
    params[int(rng.integers(0, B))] = ba.IDENTITY
    rng_mode = pick(rng, ["off", "input", "output"])
    valid = (brng.random((B, N)) < 0.8) if rng.integers(0, 2) else None
    labels = brng.integers(-1, 10, (B, N)) if rng.integers(0, 2) else None
    pts, pt_what = [], []
    for _ in range(int(rng.integers(0, 5))):
        K, rows = pick(rng, [0, 1, 63, 65, 300]), pick(rng, [3, 4])      # 16-byte matrix rows against four floats
        pts.append(ba.random_poses(brng, B, K, rows=rows) if K else np.zeros((B, 0, rows, 4), F32)), pt_what.append((K, rows))
    frs, fr_what = [], []
    for _ in range(int(rng.integers(0, 3))):
        K = pick(rng, [0, 1, 65])
        frs.append(ba.random_poses(brng, B, K) if K else np.zeros((B, 0, 4, 4), F32)), fr_what.append(K)
    how = dict(labels_dtype=pick(rng, INTS), valid_dtype=pick(rng, FLAGS), offset=bool(rng.integers(0, 2)))
    sizes_dtype = pick(rng, [np.int32, np.int64])
    case = ba.Case(boxes, counts, ba.make_rows(params), labels=labels, valid=valid,
                   point_range=None if rng_mode == "off" else ba.SWEEP_RANGE, on="input" if rng_mode == "off" else rng_mode,
                   pts=pts, frs=frs, sizes_dtype=sizes_dtype)
    what = (f"bev_augment_boxes N {N} D {D} B {B} counts {counts} range {rng_mode} valid {valid is not None} as {name(how['valid_dtype'])} "
            f"labels {labels is not None} as {name(how['labels_dtype'])} counts as {np.dtype(sizes_dtype).name} point transforms (K, rows) "
            f"{pt_what} frame transforms K {fr_what} offset {how['offset']} builder seed {seed}")
    return case, dict(how=how, ordinary=True), what


# ------------------------------------------------------------------------------------------------ camera_augment_boxes
def _camera_matrix(rng, kind, hw):
    H, W = hw
    if kind == "identity":
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    if kind == "hflip":
        return [[-1.0, 0.0, float(W)], [0.0, 1.0, 0.0]]
    if kind == "flip_scale_crop":                                # camera_boxes_cases.sweep_case: products that are not exact
        s, flip = rng.uniform(0.40, 1.3), rng.random() < 0.5
        return [[-s if flip else s, 0.0, (W + rng.uniform(-8, 8)) if flip else rng.uniform(-8, 8)], [0.0, s, H * (1 - s) * rng.uniform(0, 1)]]
    if kind == "affine":
        a, s, sh = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 1.5), rng.uniform(-0.3, 0.3)
        c, d = math.cos(a) * s, math.sin(a) * s
        lin = ((c, c * sh - d), (d, d * sh + c))
        return [[lin[0][0], lin[0][1], W / 2 - lin[0][0] * W / 2 - lin[0][1] * H / 2],      # about the image's centre
                [lin[1][0], lin[1][1], H / 2 - lin[1][0] * W / 2 - lin[1][1] * H / 2]]
    m = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    m[int(rng.integers(0, 2))][int(rng.integers(0, 3))] = pick(rng, [NAN, INF, -INF])
    return m


CAMERA_KINDS = ["identity", "hflip", "flip_scale_crop", "affine", "nonfinite"]


def draw_camera_augment_boxes(rng, device="cpu"):
    """inputs: a camera_boxes_cases.Case (numpy); kwargs: `how` for camera_boxes_cases.run and `ordinary`: oracle (b)
    applies where no matrix holds a NaN or inf (the module's rule: numbers of ordinary size, no subnormals; the builders
    draw none)."""
    import camera_boxes_cases as cb
    import visible_boxes_cases as vb

    G = pick(rng, BOX_COUNTS)
    Fr = int(rng.integers(1, 7))
    sizes = ragged_sizes(rng, Fr, G)
    common = bool(rng.integers(0, 2))
    hws = [_hw(rng, lo=(4, 4))] * Fr if common else [_hw(rng, lo=(4, 4)) for _ in range(Fr)]
    kinds = [pick(rng, CAMERA_KINDS) for _ in range(Fr)]
    seed = seed_of(rng)
    brng = np.random.default_rng(seed)
    transforms = [_camera_matrix(brng, k, hw) for k, hw in zip(kinds, hws)]
    depth_values = pick(rng, [2, 8, 24])
    frames = [vb.random_frame(brng, n, hw, depth_values=depth_values)[:2] for n, hw in zip(sizes, hws)]
    kw = dict(check_occlusion=bool(rng.integers(0, 4) > 0), minimum_size=pick(rng, MINIMUM_SIZES), shrink_to_int=bool(rng.integers(0, 2)),
              crop=bool(rng.integers(0, 2)), order_corners=bool(rng.integers(0, 2)))
    Wmax, Hmax = max(h[1] for h in hws), max(h[0] for h in hws)
    centers = np.stack([brng.integers(-8, 2 * Wmax + 8, (Fr, G)), brng.integers(-8, 2 * Hmax + 8, (Fr, G))], -1).astype(F32) / 2 \
        if rng.integers(0, 2) else None
    categories = brng.integers(-1, 6, (Fr, G)) if rng.integers(0, 2) else None
    valid = (brng.random((Fr, G)) < 0.8) if rng.integers(0, 2) else None
    mats, mat_what = [], []
    for _ in range(int(rng.integers(0, 5))):
        shape = pick(rng, ["3x3", "Kx3x4", "Kx4x4"])
        K = pick(rng, [0, 1, 6, 20])
        full = (Fr, 3, 3) if shape == "3x3" else (Fr, K, 3, 4) if shape == "Kx3x4" else (Fr, K, 4, 4)
        mats.append(cb._general(brng, full)), mat_what.append(full[1:])
    how = dict(categories_dtype=pick(rng, INTS), valid_dtype=pick(rng, FLAGS), hw_dtype=pick(rng, INTS), offset=bool(rng.integers(0, 2)),
               ragged_fields=bool(rng.integers(0, 2)))
    case = cb.from_frames(frames, transforms, G=G, hostile=bool(rng.integers(0, 4) > 0), hw=hws[0] if common else np.asarray(hws),
                          centers=centers, categories=categories, valid=valid, mats=mats, sizes_dtype=pick(rng, [np.int32, np.int64]), **kw)
    what = (f"camera_augment_boxes G {G} sizes {sizes} image_hw {'common ' + str(hws[0]) if common else hws} matrices {kinds} "
            f"depth values {depth_values} centres {centers is not None} categories {categories is not None} valid {valid is not None} "
            f"projection matrices {mat_what} counts as {case.sizes.dtype.name} {how} builder seed {seed} {kw}")
    return case, dict(how=how, ordinary="nonfinite" not in kinds), what


# -------------------------------------------------------------------------------------- box_heatmap_decode, nms_boxes
IOU_MARGIN = 1e-5        # tests/test_box_decode_cpu.py: no compared pair within 1e-5 of the threshold
POST_MAX = [None, 1, 40, 83, 300]


def _off_the_score_threshold(case, threshold):
    """operator_sweep_cases._off_the_score_threshold for the one score tensor of a box_decode_cases.Case"""
    from box_decode_cases import MARGIN

    s = case.peaks[0]
    near = (torch.sigmoid(s.double()) - threshold).abs() <= 2 * MARGIN
    if bool(near.any()):
        s.copy_(torch.where(near, (s.double() + 0.02).to(s.dtype), s))       # logits lie in (-4, 4): spacing <= 0.0157
    return not bool(((torch.sigmoid(s.double()) - threshold).abs() <= 2 * MARGIN).any())


def iou_gap(frames, thr, agnostic):
    """the smallest distance of a compared IoU from `thr` over the float64 greedy loops of `frames`: (boxes, labels) each"""
    from box_decode_cases import greedy_nms_f64

    return min([greedy_nms_f64(b, l, thr, agnostic)[1] for b, l in frames if len(b)] + [np.inf])


def pick_iou_threshold(frames, start, agnostic):
    """the first of start, start + 0.001, ... whose float64 greedy loop compares no pair within IOU_MARGIN of it; ten
    candidates at the most, as rotated_nms_cases.pick_threshold; None when none is clear"""
    for step in range(10):
        thr = round(start + 0.001 * step, 3)
        if iou_gap(frames, thr, agnostic) > IOU_MARGIN:
            return thr
    return None


def _valid_frames(want):
    """(boxes float64 [n, 4], labels) per frame of a definition's result without NMS, matrices and cut: the boxes the
    greedy walk sees, in rank order"""
    out = []
    for f, n in enumerate(want["sizes"]):
        out.append((want["boxes"][f, :n].astype(np.float64), want["labels"][f, :n].tolist()))
    return out


def _image_matrices(rng, Fn, hw):
    m = torch.zeros((Fn, 2, 3))
    for f in range(Fn):
        s, t, flip = float(rng.uniform(0.4, 1.3)), float(rng.uniform(0.4, 1.3)), bool(rng.integers(0, 2))
        m[f] = torch.tensor([[-s if flip else s, 0.0, float(hw[1]) - 10.0 if flip else -13.5], [0.0, t, -7.25 * f]])
    if rng.integers(0, 2):
        m[int(rng.integers(0, Fn)), 1, :2] = 0.0                                   # singular: zero boxes, the count kept
    return m


def draw_box_heatmap_decode(rng, device="cpu"):
    """inputs: a box_decode_cases.Case on the host (the GPU test moves it); kwargs: the operator's options, tensors among
    them.  Two margins: (1) with logit scores and a score threshold the draw moves the logits whose float64 sigmoid lies
    within 2 MARGIN of the threshold, and only then builds again from the next builder seed (REDRAWS); (2) the IoU
    threshold is the first of the drawn value + 0.001 j that the float64 greedy loop over the decoded boxes clears by
    IOU_MARGIN (a case without such a value among ten is built again and counted too)."""
    import box_decode_cases as bd

    K = pick(rng, [1, 63, 64, 65, 255, 256, 257, 500, 1024])     # wave blocks of 64, chunks of 256, the cap
    grid = pick(rng, [(1, 1), (5, 3), (64, 64), (130, 17)])
    E = pick(rng, [0, 1, 2, 4])                                  # the channel counts box_decode_cases.SPLITS has
    split = int(rng.integers(0, len(bd.SPLITS[4 + E])))
    Fn = max(1, min(int(rng.integers(1, 5)), 2048 // K))          # the definition is a loop over frames x K peaks
    dtype = pick(rng, FLOATS3)
    score_dtype = pick(rng, [None, torch.float32])
    logits = bool(rng.integers(0, 2))
    illegal, cells = pick(rng, [0.0, 0.03, 0.3]), pick(rng, [None, 4])
    opt = dict(clip=bool(rng.integers(0, 2)), order_corners=bool(rng.integers(0, 2)), class_agnostic=bool(rng.integers(0, 2)))
    if logits:
        opt["scores_are_logits"] = True
    thr = pick(rng, [None, 0.1, 0.3])
    if thr is not None:
        opt["score_threshold"] = thr
    if rng.integers(0, 2):
        opt["min_size"] = pick(rng, [2.0, (2.0, 3.0)])
    post = pick(rng, POST_MAX)
    if post is not None:
        opt["post_max_size"] = post
    iou = pick(rng, [None, 0.3, 0.5, 0.7])
    hw = (int(rng.integers(1, 200)), int(rng.integers(1, 300)))
    per_frame, hw_dtype = bool(rng.integers(0, 2)), pick(rng, INTS)
    with_matrices = bool(rng.integers(0, 2))
    nms = None
    if rng.integers(0, 2):                 # nms_boxes on the decode result: rows are copied and the IoU sequence is the
        nms = dict(iou_threshold=pick(rng, [None, 0.3, 0.5, 0.7]), class_agnostic=bool(rng.integers(0, 2)))    # definition's, exactly
        for key, v in (("pre_max_size", pick(rng, [None, 1, 64, 100, 500])), ("post_max_size", pick(rng, POST_MAX))):
            if v is not None:
                nms[key] = v
    seed = seed_of(rng)
    mrng = np.random.default_rng(seed)
    tensors = {}
    if per_frame:
        rows = [[int(mrng.integers(0, 200)), int(mrng.integers(0, 300))] for _ in range(Fn)]
        rows[0] = list(hw)
        tensors["image_hw"] = torch.tensor(rows, dtype=hw_dtype)
    else:
        opt["image_hw"] = hw
    if with_matrices:
        tensors["image_matrices"] = _image_matrices(mrng, Fn, hw)
    for attempt in range(10):
        case = bd.make_case(Fn, K, grid, E=E, dtype=dtype, score_dtype=score_dtype, seed=seed + attempt, logits=logits, illegal=illegal,
                            split=split, cells=cells)
        case.tensors.update(tensors)
        ok = not (logits and thr is not None) or _off_the_score_threshold(case, thr)
        if ok and iou is not None:
            plain = {k: v for k, v in dict(case.tensors, **opt).items()
                     if k not in ("image_matrices", "post_max_size", "class_agnostic", "iou_threshold")}
            picked = pick_iou_threshold(_valid_frames(bd.definition(case.peaks, case.feats, **plain)), iou, opt["class_agnostic"])
            ok = picked is not None
            if ok:
                opt["iou_threshold"] = picked
        if ok:
            break
        REDRAWS["box_heatmap_decode"] += 1
    else:
        raise AssertionError("ten builder seeds in a row left a score or an IoU on its threshold: the draw is broken")
    what = (f"box_heatmap_decode K {K} frames {Fn} grid {grid} E {E} split {split} maps {name(dtype)} scores {name(score_dtype or dtype)} "
            f"illegal {illegal} cells {cells} image_hw {'per frame ' + name(hw_dtype) if per_frame else hw} matrices {with_matrices} "
            f"iou drawn {iou} builder seed {seed + attempt} {opt} then nms_boxes {nms}")
    return case, dict(options=opt, nms=nms), what


def f64_kept_ranks(case, opt):
    """per frame, the source ranks that the float64 greedy loop keeps among the valid decoded boxes of a drawn decoder
    case (None without an IoU threshold): what the operator's `source` must hold, since the draw cleared the threshold"""
    import box_decode_cases as bd

    if opt.get("iou_threshold") is None:
        return None
    plain = {k: v for k, v in dict(case.tensors, **opt).items() if k not in ("image_matrices", "post_max_size", "class_agnostic", "iou_threshold")}
    want = bd.definition(case.peaks, case.feats, **plain)
    K = case.peaks[0].shape[1]
    M = K if opt.get("post_max_size") is None else min(K, opt["post_max_size"])
    out = []
    for f, (boxes, labels) in enumerate(_valid_frames(want)):
        keep, gap = bd.greedy_nms_f64(boxes, labels, opt["iou_threshold"], opt["class_agnostic"], limit=M)
        assert gap > IOU_MARGIN
        out.append(want["source"][f, keep].tolist())
    return out


def draw_nms_boxes(rng, device="cpu"):
    """inputs: the six tensors (boxes, scores, labels, source, extras, sizes) of a ragged BoxDetections on the host, built
    from the decoded-box geometry of box_decode_cases.make_case (the definition's boxes without any filter, so that the
    draw uses no operator); kwargs: iou_threshold (picked as in draw_box_heatmap_decode), class_agnostic, pre / post max"""
    import box_decode_cases as bd

    N = pick(rng, [1, 63, 65, 200, 257, 1024])
    Fn = max(1, min(int(rng.integers(1, 5)), 2048 // N))
    E = pick(rng, [0, 1, 2])
    sizes = ragged_sizes(rng, Fn, N)
    cells = pick(rng, [None, 4])
    agnostic = bool(rng.integers(0, 2))
    pre, post = pick(rng, [None, 1, 64, 100, 500]), pick(rng, POST_MAX)
    iou = pick(rng, [None, 0.3, 0.5, 0.7])
    seed = seed_of(rng)
    kw = dict(class_agnostic=agnostic)
    if pre is not None:
        kw["pre_max_size"] = pre
    if post is not None:
        kw["post_max_size"] = post
    for attempt in range(10):
        case = bd.make_case(Fn, N, (64, 64), E=E, seed=seed + attempt, illegal=0.0, cells=cells)
        want = bd.definition(case.peaks, case.feats, image_hw=(96, 160))         # every peak is valid: N rows per frame
        assert want["sizes"].tolist() == [N] * Fn
        boxes = torch.from_numpy(want["boxes"].copy())
        nrng = np.random.default_rng(seed + attempt)
        for f in range(Fn):                                                      # a few rows that are not finite: kept, suppress nothing
            for k in nrng.integers(0, N, 2 if N > 2 else 0):
                boxes[f, int(k), int(nrng.integers(0, 4))] = pick(nrng, [NAN, INF, -INF])
        det = (boxes, torch.from_numpy(want["score_exact"].copy()), torch.from_numpy(want["labels"].copy()),
               torch.from_numpy(want["source"].copy()), torch.from_numpy(want["extras"].copy()),
               torch.tensor(sizes, dtype=torch.int64))                           # the operator takes int64 sizes alone
        if iou is None:
            kw["iou_threshold"] = None
            break
        frames = []
        for f, n in enumerate(sizes):
            n = n if pre is None else min(n, pre)
            b = boxes[f, :n].double().numpy()
            fin = np.isfinite(b).all(1)                                          # rows that are not finite meet no comparison
            frames.append((b[fin], np.asarray(want["labels"][f, :n])[fin].tolist()))
        picked = pick_iou_threshold(frames, iou, agnostic)
        if picked is not None:
            kw["iou_threshold"] = picked
            break
        REDRAWS["nms_boxes"] += 1
    else:
        raise AssertionError("ten builder seeds in a row left an IoU on its threshold: the draw is broken")
    what = (f"nms_boxes N {N} frames {Fn} E {E} sizes {sizes} cells {cells} iou drawn {iou} "
            f"builder seed {seed + attempt} {kw}")
    return det, kw, what


def detections(det, device="cpu"):
    """a BoxDetections on `device` from the six tensors of draw_nms_boxes"""
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import BoxDetections

    sizes = det[5].to(device)
    return BoxDetections(*(RaggedBatch(x.to(device), sample_sizes=sizes) for x in det[:5]))


def detection_tensors(d):
    return tuple(x.tensor for x in d) + (d.boxes.sample_sizes,)


# (seed base, seeds at ACCV_FUZZ_SCALE = 1, cases per seed): shared by the CPU and the GPU sweep, which draw the same cases.
# Measured seconds per seed (the slowest seed of each sweep): host entries alone in the CPU file / the GPU file on the MI355X,
# where every case runs on the device and on the host.  The Python definitions dominate both; the CPU file takes 9 s, the
# GPU file 6 s, the existing CPU sweep file 10 s.
SWEEPS = {
    "visible_boxes": (820000, 4, 12),             # 0.3 / 0.5 s
    "boxes_to_heatmap": (830000, 4, 8),           # 0.4 / 0.2 s
    "prepare_images": (840000, 6, 16),            # 0.1 / 0.05 s
    "nv12_to_rgb": (850000, 4, 16),               # 0.01 / 0.01 s
    "prepare_images_nv12": (860000, 6, 16),       # 0.02 / 0.02 s
    "bev_augment_boxes": (870000, 4, 10),         # 0.4 / 0.2 s
    "camera_augment_boxes": (880000, 4, 10),      # 0.1 / 0.05 s
    "box_heatmap_decode": (890000, 4, 10),        # 0.6 / 0.2 s
    "nms_boxes": (900000, 4, 8),                  # 1.9 / 1.3 s: the float64 greedy loop over 1024 + 577 rows at 0.7
}


def sweep(op, seed, device="cpu"):
    """yields (tag, inputs, kwargs) of the cases of one seed of an operator's sweep"""
    base, _, cases = SWEEPS[op]
    rng = np.random.default_rng(base + seed)
    draw = globals()["draw_" + op]
    for case in range(cases):
        inp, kw, what = draw(rng, device)
        yield f"seed {seed} case {case}: {what}", inp, kw
