"""Cases and an independent oracle for accvlab.image_prep.prepare_images, shared by test_image_prep_cpu.py and
test_image_prep_gpu.py.

The oracle is written from the operator's docstring, not from the library: numpy in float64, bilinear sampling with zero
outside the valid region, the stdlib's ``colorsys.rgb_to_hsv`` / ``hsv_to_rgb`` for the HSV stage, plain formulas for
the rest.  Everything in the chain is continuous in the pixel value, so ONE tolerance holds for every element and no
element is excluded.  The sample position is the exception: under a general matrix the float32 rounding of (sx, sy) moves
the weights by far more than the value arithmetic does.  The oracle therefore takes (x0, y0, wx, wy) from
``positions_f32``, a numpy-float32 restatement of the coordinate sequence of the docstring; the CPU tests hold it
bit-equal to what the library's host entry reports for every case with a matrix (``sample_positions``).

Tolerance (derived, not tuned).  K counts the rounded float32 operations on the longest chain from the four source bytes
to an output value in csrc/image_prep_arith.h, every stage active: the blend 5 (1 - wx, two products and sums on the way
through top and the value), 1/255 and its product 2, delta 1, alpha_pre 1, the HSV stage 9 (max - min, the division, the
sector offset, the hue shift, the wrap, 1 - f, s * (1 - f), 1 - (.), max * (.); floor, f, max and min are exact),
alpha_post 1, scale and its product 2, bias and its sum 2: K = 23.  Each rounds a value of magnitude at most
(1 + saturation) in [0, 1] units by 2^-24 of it, and a [0, 1] unit is 255 / std at the output:

    bar = K * 2^-24 * (1 + max saturation used) * 255 / min(std)

which is 23 * 2^-24 * 2 * 255 = 6.99e-4 for an identity saturation and std = 1, and 1.05e-3 with saturation 2.  f16 / bf16
results are held bit-equal to the float32 result's ``.to(dtype)``, and the device is held bit-equal to the host entry.
"""
import colorsys
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from accvlab import _amd_native as nat
from accvlab.image_prep import CHANNEL_PERMUTATIONS, IDENTITY_PHOTOMETRIC, output_size_transform, padded_hw, prepare_images

TW, TH = nat.IP_TILE_W, nat.IP_TILE_H
K_ROUNDED_OPS = 23
F32 = np.float32


@dataclass
class Case:
    name: str
    images: np.ndarray                      # uint8 [B, Hs, Ws, 3]
    output_hw: tuple = None
    transforms: np.ndarray = None           # float32 [B, 2, 3]
    source_hw: np.ndarray = None            # int [B, 2]
    photometric: np.ndarray = None          # float32 [B, 6]
    kw: dict = field(default_factory=dict)  # is_bgr, mean, std, tile_hw, pad_before_normalize

    def __repr__(self):
        return self.name


def bar(case) -> float:
    sat = 1.0 if case.photometric is None or not len(case.photometric) else max(1.0, float(np.max(case.photometric[:, 2])))
    std = case.kw.get("std", 1.0)
    min_std = min(std) if isinstance(std, (tuple, list)) else std
    return K_ROUNDED_OPS * 2.0 ** -24 * (1.0 + sat) * 255.0 / min_std


# ------------------------------------------------------------------------------------------------------------- oracle
def positions_f32(m, Ho, Wo, Wv, Hv):
    """(x0, y0, wx, wy, inside) per output pixel from one 2x3 float32 matrix: the docstring's sequence, one float32
    operation per step.  Outside pixels are (-2, -2, 0, 0)."""
    x0 = np.full((Ho, Wo), -2, np.int64)
    y0 = np.full((Ho, Wo), -2, np.int64)
    wx = np.zeros((Ho, Wo), F32)
    wy = np.zeros((Ho, Wo), F32)
    inside = np.zeros((Ho, Wo), bool)
    m = np.asarray(m, F32)
    a, b, tx, c, d, ty = (m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2])
    with np.errstate(all="ignore"):
        det = F32(F32(a * d) - F32(b * c))
        ok = bool(np.all(np.isfinite(m))) and bool(np.isfinite(det)) and det != 0 and bool(np.isfinite(F32(1) / det))
        if not ok:
            return x0, y0, wx, wy, inside
        X = np.arange(Wo, dtype=F32)[None, :].repeat(Ho, 0)
        Y = np.arange(Ho, dtype=F32)[:, None].repeat(Wo, 1)
        u = (X + F32(0.5)) - tx
        v = (Y + F32(0.5)) - ty
        sx = (d * u - b * v) / det - F32(0.5)
        sy = (a * v - c * u) / det - F32(0.5)
        assert sx.dtype == F32 and sy.dtype == F32
        inside = (sx > F32(-1)) & (sx < F32(Wv)) & (sy > F32(-1)) & (sy < F32(Hv))
        fx, fy = np.floor(sx), np.floor(sy)
        x0 = np.where(inside, fx, F32(-2)).astype(np.int64)
        y0 = np.where(inside, fy, F32(-2)).astype(np.int64)
        wx = np.where(inside, sx - fx, F32(0)).astype(F32)
        wy = np.where(inside, sy - fy, F32(0)).astype(F32)
    return x0, y0, wx, wy, inside


def _tap(img, x, y, Wv, Hv):
    """float64 [Ho, Wo, 3]: the source pixel at integer (x, y), 0 outside [0, Wv) x [0, Hv)"""
    ok = (x >= 0) & (x < Wv) & (y >= 0) & (y < Hv)
    px = img[np.clip(y, 0, img.shape[0] - 1), np.clip(x, 0, img.shape[1] - 1)].astype(np.float64)
    return np.where(ok[..., None], px, 0.0)


def _sampled(img, m, Ho, Wo, Wv, Hv):
    if m is None:
        X, Y = np.meshgrid(np.arange(Wo), np.arange(Ho))
        return _tap(img, X, Y, Wv, Hv)
    x0, y0, wx, wy, inside = positions_f32(m, Ho, Wo, Wv, Hv)
    wx, wy = wx.astype(np.float64)[..., None], wy.astype(np.float64)[..., None]
    top = _tap(img, x0, y0, Wv, Hv) * (1 - wx) + _tap(img, x0 + 1, y0, Wv, Hv) * wx
    bot = _tap(img, x0, y0 + 1, Wv, Hv) * (1 - wx) + _tap(img, x0 + 1, y0 + 1, Wv, Hv) * wx
    return np.where(inside[..., None], top * (1 - wy) + bot * wy, 0.0)


def _colour(v, row, is_bgr):
    """v: float64 [H, W, 3] in [0, 1]; row: the six float32 values, taken exactly"""
    delta, alpha_pre, sat, hue, alpha_post, index = (float(x) for x in row)
    if delta != 0:
        v = np.clip(v + delta, 0, 1)
    if alpha_pre != 1:
        v = np.clip(v * alpha_pre, 0, 1)
    if not (sat == 1 and hue == 0):
        flat = v.reshape(-1, 3)
        res = np.empty_like(flat)
        for i, px in enumerate(flat):
            r, g, b = (px[2], px[1], px[0]) if is_bgr else px
            h, s, val = colorsys.rgb_to_hsv(r, g, b)
            r, g, b = colorsys.hsv_to_rgb((h + hue / 360.0) % 1.0, s * sat, val)
            res[i] = (b, g, r) if is_bgr else (r, g, b)
        v = res.reshape(v.shape)
    if alpha_post != 1:
        v = np.clip(v * alpha_post, 0, 1)
    perm = CHANNEL_PERMUTATIONS[int(index)] if index in (0, 1, 2, 3, 4, 5) else (0, 1, 2)
    return np.clip(v[..., list(perm)], 0, 1)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """float64 [B, 3, Hp, Wp] of case `name`; computed once, shared and never written to"""
    return oracle_of(cases()[name])


def oracle_of(case):
    """float64 [B, 3, Hp, Wp] of any Case, a drawn one included; not cached, read-only"""
    B, Hs, Ws = case.images.shape[:3]
    Ho, Wo = case.output_hw or (Hs, Ws)
    kw = case.kw
    mean, std = (np.broadcast_to(np.asarray(kw.get(k, d), np.float64), (3,)) for k, d in (("mean", 0.0), ("std", 1.0)))
    Hp, Wp = padded_hw((Ho, Wo), kw.get("tile_hw", 1))
    pad = (0.0 - mean) / std if kw.get("pad_before_normalize", True) else np.zeros(3)
    out = np.empty((B, Hp, Wp, 3), np.float64)
    out[:] = pad
    for b in range(B):
        Hv, Wv = (Hs, Ws) if case.source_hw is None else (int(np.clip(case.source_hw[b, 0], 0, Hs)),
                                                          int(np.clip(case.source_hw[b, 1], 0, Ws)))
        m = None if case.transforms is None else case.transforms[b]
        v = _sampled(case.images[b], m, Ho, Wo, Wv, Hv) / 255.0
        v = _colour(v, IDENTITY_PHOTOMETRIC if case.photometric is None else case.photometric[b], kw.get("is_bgr", False))
        out[b, :Ho, :Wo] = (255.0 * v - mean) / std
    out = np.ascontiguousarray(out.transpose(0, 3, 1, 2))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------ running
def tensors(case, device):
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)   # noqa: E731
    src_dt = torch.int32 if case.name.endswith("int32") else torch.int64
    return dict(images=t(case.images, torch.uint8), transforms=t(case.transforms, torch.float32),
                source_hw=t(case.source_hw, src_dt), photometric=t(case.photometric, torch.float32))


def run(case, device, **over):
    """prepare_images on the case's inputs; `over` replaces keyword arguments (layout, dtype, out, ...)"""
    t = tensors(case, device)
    images = t.pop("images")
    return prepare_images(images, **{**t, **case.kw, "output_hw": case.output_hw, **over})


def as_chw64(result, layout="CHW"):
    a = result.detach().cpu().to(torch.float64).numpy()
    return a.transpose(0, 3, 1, 2) if layout == "HWC" else a


def max_error(result, case, layout="CHW"):
    want = oracle(case.name)
    got = as_chw64(result, layout)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{case.name}: an element is not finite (not written?)"
    return float(np.abs(got - want).max()) if want.size else 0.0


def check(result, case, layout="CHW"):
    """every element within the derived bar; returns the largest error"""
    err, limit = max_error(result, case, layout), bar(case)
    print(f"{case.name}: max abs error {err:.3e}, bar {limit:.3e}")
    assert err <= limit, f"{case.name}: max abs error {err:.3e} above the bar {limit:.3e}"
    return err


# -------------------------------------------------------------------------------------------------------------- cases
def _noise(rng, B, H, W):
    return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def lattice():
    """64 x 64: every combination of 16 levels per channel (greys, black, white, primaries, hue-sector boundaries)"""
    lv = (np.arange(16) * 17).astype(np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing="ij")
    return np.stack([r, g, b], -1).reshape(1, 64, 64, 3)


def _rows(*rows):
    return np.asarray(rows, F32).reshape(-1, 6)


def _row(delta=0.0, alpha_pre=1.0, saturation=1.0, hue=0.0, alpha_post=1.0, index=0.0):
    return (delta, alpha_pre, saturation, hue, alpha_post, index)


def _mats(*ms):
    return np.asarray(ms, F32).reshape(-1, 2, 3)


def _about_centre(lin, src_hw, out_hw):
    """the matrix with linear part `lin` that takes the source's centre to the output's centre"""
    (a, b), (c, d) = lin
    cx, cy, ox, oy = src_hw[1] / 2, src_hw[0] / 2, out_hw[1] / 2, out_hw[0] / 2
    return [[a, b, ox - a * cx - b * cy], [c, d, oy - c * cx - d * cy]]


PARTITION_WIDTHS = (1, 3, 4, 5, TW - 1, TW, TW + 1, 2 * TW + 3)
PARTITION_HEIGHTS = (1, TH - 1, TH, TH + 1)
NORM = dict(mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375))


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    out = {}

    def add(name, images, **kw):
        fields = {k: kw.pop(k) for k in ("output_hw", "transforms", "source_hw", "photometric") if k in kw}
        assert name not in out
        out[name] = Case(name, images, kw=kw, **fields)

    # partition: every width against every height, two images with different matrices and colour rows
    for w in PARTITION_WIDTHS:
        for h in PARTITION_HEIGHTS:
            src = (11, 14)
            add(f"partition_{h}x{w}", _noise(rng, 2, *src), output_hw=(h, w),
                transforms=_mats(output_size_transform(src, (h, w), "stretch"),
                                 _about_centre(((0.9, 0.2), (-0.1, 1.1)), src, (h, w))),
                photometric=_rows(_row(delta=0.1, alpha_pre=1.2, index=4), _row(alpha_post=0.8, index=1)), **NORM)
    add("batch_0", _noise(rng, 0, 5, 6), output_hw=(4, 7), transforms=np.zeros((0, 2, 3), F32),
        photometric=np.zeros((0, 6), F32), source_hw=np.zeros((0, 2), np.int64), tile_hw=4)
    add("batch_1_no_arguments", _noise(rng, 1, 9, 13))
    ang = [math.radians(a) for a in (0, 10, 30, 90, 135, 180, 270)]
    src, dst = (20, 27), (TH + 3, TW + 9)
    add("batch_7_parameters_per_image", _noise(rng, 7, *src), output_hw=dst,
        transforms=_mats(*[_about_centre(((s * math.cos(t), -s * math.sin(t)), (s * math.sin(t), s * math.cos(t))), src, dst)
                           for t, s in zip(ang, (1.0, 0.8, 1.5, 2.0, 3.0, 0.6, 1.1))]),
        source_hw=np.asarray([(20, 27), (19, 27), (20, 5), (1, 1), (0, 9), (25, 40), (13, 17)]),
        photometric=_rows(IDENTITY_PHOTOMETRIC, _row(0.1, 1.1, 1.3, 40.0, 1.0, 3), _row(-0.2, 1.0, 0.5, -100.0, 0.9, 5),
                          _row(saturation=2.0), _row(hue=200.0, index=2), _row(delta=0.3, index=9), _row(0.05, 0.7, 1.7, 300.0, 1.0, 1)),
        is_bgr=True, tile_hw=(8, 32), **NORM)

    # padding
    pad_norm = dict(mean=(10.0, 20.0, 30.0), std=(2.0, 4.0, 8.0))
    for name, hw, tile in (("tile_1", (9, 10), 1), ("tile_32_exact_multiple", (32, 64), 32), ("tile_32_multiple_plus_1", (33, 65), 32),
                           ("tile_8x32", (TH + 1, 40), (8, 32)), ("tile_larger_than_the_image", (3, 5), (TH + 4, TW + 8))):
        for before in (True, False):
            add(f"pad_{name}_{'before' if before else 'after'}_normalize", _noise(rng, 2, *hw), tile_hw=tile,
                pad_before_normalize=before, **pad_norm)

    # warp
    src = (12, 20)
    img = _noise(rng, 1, *src)
    ident = [[1, 0, 0], [0, 1, 0]]
    add("warp_none", img)
    add("warp_identity", img, transforms=_mats(ident))
    add("warp_integer_translation", img, transforms=_mats([[1, 0, 3], [0, 1, -2]]))
    add("warp_half_pixel_translation", img, transforms=_mats([[1, 0, 0.5], [0, 1, 0.5]]))
    add("warp_x_flip", img, transforms=_mats([[-1, 0, 20], [0, 1, 0]]))
    add("warp_y_flip", img, transforms=_mats([[1, 0, 0], [0, -1, 12]]))
    add("warp_scale_half", img, output_hw=(6, 10), transforms=_mats([[0.5, 0, 0], [0, 0.5, 0]]))
    add("warp_scale_2", img, output_hw=(24, 40), transforms=_mats([[2, 0, 0], [0, 2, 0]]))
    big = _noise(rng, 1, 45, 80)     # 900 x 1600 -> 256 x 704 at a twentieth
    for mode, anchors in (("stretch", ("center",)), ("pad", ("top_or_left", "center", "bottom_or_right")),
                          ("crop", ("top_or_left", "center", "bottom_or_right"))):
        for anchor in anchors:
            add(f"warp_output_size_{mode}_{anchor}", big, output_hw=(13, 35),
                transforms=_mats(output_size_transform((45, 80), (13, 35), mode, anchor)))
    c30, s30 = math.cos(math.radians(30)), math.sin(math.radians(30))
    add("warp_rotation_30", img, output_hw=(16, 22), transforms=_mats(_about_centre(((c30, -s30), (s30, c30)), src, (16, 22))))
    add("warp_shear", img, output_hw=(12, 26), transforms=_mats([[1, 0.4, 0], [0.15, 1, -1]]))
    add("warp_singular_zero", img, transforms=_mats(np.zeros((2, 3))), photometric=_rows(_row(delta=0.25)), **NORM)
    add("warp_singular_rank_1", img, transforms=_mats([[1, 2, 0], [2, 4, 1]]), photometric=_rows(_row(delta=0.25)), **NORM)
    add("warp_nan_entry", img, transforms=_mats([[1, 0, float("nan")], [0, 1, 0]]), **NORM)
    add("warp_inf_entry", img, transforms=_mats([[float("inf"), 0, 0], [0, 1, 0]]), **NORM)
    add("warp_det_underflows", img, transforms=_mats([[1e-30, 0, 0], [0, 1e-30, 0]]), **NORM)
    add("warp_fully_outside", img, transforms=_mats([[1, 0, 1000], [0, 1, 0]]), **NORM)
    add("warp_source_1x1", np.full((1, 1, 1, 3), 200, np.uint8), output_hw=(4, 4), transforms=_mats([[4, 0, 0], [0, 4, 0]]))
    add("warp_source_1x1_none", np.asarray([[[[9, 100, 255]]]], np.uint8))
    add("source_hw_zero", img, source_hw=np.asarray([(0, 0)]), transforms=_mats(ident), photometric=_rows(_row(delta=0.5)))
    add("source_hw_zero_none_int32", img, source_hw=np.asarray([(0, 20)]))

    # colour, on the lattice
    lat = lattice()
    colour = dict(identity_row=IDENTITY_PHOTOMETRIC, delta_up=_row(delta=0.2), delta_down=_row(delta=-0.2), delta_plus_1=_row(delta=1.0),
                  delta_minus_1=_row(delta=-1.0), contrast_pre=_row(alpha_pre=1.3), contrast_post=_row(alpha_post=0.7),
                  saturation_0=_row(saturation=0.0), saturation_2=_row(saturation=2.0), saturation_1_5=_row(saturation=1.5),
                  hue_30=_row(hue=30.0), hue_plus_180=_row(hue=180.0), hue_minus_180=_row(hue=-180.0), hue_360=_row(hue=360.0),
                  hue_minus_77_5=_row(hue=-77.5), all_contrast_pre=_row(0.1, 1.2, 1.4, 50.0, 1.0, 4),
                  all_contrast_post=_row(-0.1, 1.0, 0.6, -130.0, 1.25, 5), permutation_7=_row(index=7.0),
                  permutation_2_5=_row(index=2.5), permutation_minus_1=_row(index=-1.0))
    for i in range(6):
        colour[f"permutation_{i}"] = _row(index=float(i))
    for name, row in colour.items():
        add(f"colour_{name}", lat, photometric=_rows(row), **NORM)
    add("colour_none", lat, **NORM)
    add("colour_bgr_hue_saturation", lat, photometric=_rows(_row(saturation=1.5, hue=70.0, index=3)), is_bgr=True, **NORM)
    add("colour_all_with_a_warp", lat, output_hw=(40, 50), photometric=_rows(_row(0.1, 1.2, 1.4, 50.0, 1.0, 4)),
        transforms=_mats(_about_centre(((0.7, 0.1), (-0.2, 0.8)), (64, 64), (40, 50))), tile_hw=16, **NORM)
    add("colour_range_0_1_normalizer", lat, photometric=_rows(_row(saturation=2.0, hue=10.0)), mean=0.0, std=255.0)
    return out


def case_names():
    return sorted(cases())
