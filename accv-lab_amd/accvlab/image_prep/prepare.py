"""(extension) Decoded camera images -> network input in one launch: the image side of the reference's camera pipeline
(packages/dali_pipeline_framework, processing_steps/affine_transformer.py through ``fn.warp_affine``,
photo_metric_distorter.py, image_to_tile_size_padder.py and image_mean_std_dev_normalizer.py / image_range_0_1_normalizer.py,
wired up in examples/pipeline_setup/stream_petr_pipeline.py).

The reference runs four DALI operators, each its own pass over the image.  Here one HIP kernel reads the uint8 HWC source
where it is sampled and writes the final float tensor once (``csrc/image_prep.hip``; the per-pixel arithmetic is
``csrc/image_prep_arith.h``).
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from .._amd_native.operands import is_int, is_number

MAX_EXTENT = _nat.IP_MAX_EXTENT
TILE_W = _nat.IP_TILE_W
TILE_H = _nat.IP_TILE_H
_WHO = "prepare_images"
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_LAYOUTS = {"CHW": _nat.IP_LAYOUT_CHW, "HWC": _nat.IP_LAYOUT_HWC}
# get_color_channel_permutation of the reference: output channel k takes input channel CHANNEL_PERMUTATIONS[index][k]
CHANNEL_PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 1, 0), (2, 0, 1), (1, 2, 0))
# the photometric row that changes nothing: (delta, alpha_pre, saturation, hue_degrees, alpha_post, permutation_index)
IDENTITY_PHOTOMETRIC = (0.0, 1.0, 1.0, 0.0, 1.0, 0.0)


def _hw(name, v, who=_WHO):
    if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(is_int(x) for x in v):
        raise RuntimeError(f"{who}: {name} must be (height, width) Python ints, got {v!r}")
    return int(v[0]), int(v[1])


def _tile(tile_hw, who=_WHO):
    t = (tile_hw, tile_hw) if is_int(tile_hw) else _hw("tile_hw", tile_hw, who)
    if not all(1 <= x <= MAX_EXTENT for x in t):
        raise RuntimeError(f"{who}: tile_hw must be at least 1 and at most {MAX_EXTENT}, got {tile_hw!r}")
    return t


def padded_hw(hw, tile_hw):
    """``(Hp, Wp)``: ``hw`` rounded up to multiples of ``tile_hw``, an int or ``(tile_h, tile_w)``.  The reference's
    ``ImageToTileSizePadder`` orders its ``tile_size_to_pad_to`` as (x, y); this one is (h, w), as its name says."""
    h, w = _hw("hw", hw, "padded_hw")
    th, tw = _tile(tile_hw, "padded_hw")
    if h < 0 or w < 0:
        raise RuntimeError(f"padded_hw: hw must not be negative, got {hw!r}")
    return -(-h // th) * th, -(-w // tw) * tw


def output_size_transform(source_hw, output_hw, mode="stretch", anchor="center"):
    """The 2x3 forward matrix (source -> output coordinates, nested lists of Python floats) that brings an image of
    ``source_hw`` to ``output_hw``: ``AffineTransformer._get_transformation_to_output_size`` of the reference
    (affine_transformer.py:917-956).

    ``mode`` is ``"stretch"`` (both axes scaled on their own), ``"pad"`` (one scale, the smaller ratio: the image fits
    inside) or ``"crop"`` (one scale, the larger ratio: the image fills the output).  For pad and crop ``anchor`` places
    the scaled image: ``"top_or_left"`` (no shift), ``"center"`` or ``"bottom_or_right"``; with ``k`` = 0.5 or 1 the shift
    is ``out * k - scale * in * k`` per axis.  Compose further steps (flip, rotation, crop) by matrix products on the left.
    """
    who = "output_size_transform"
    hi, wi = (float(v) for v in _hw("source_hw", source_hw, who))
    ho, wo = (float(v) for v in _hw("output_hw", output_hw, who))
    if hi <= 0 or wi <= 0:
        raise RuntimeError(f"{who}: source_hw must be positive, got {source_hw!r}")
    mode, anchor = str(mode).lower(), str(anchor).lower()
    if mode == "stretch":
        return [[wo / wi, 0.0, 0.0], [0.0, ho / hi, 0.0]]
    if mode not in ("pad", "crop"):
        raise ValueError(f"{who}: mode must be 'stretch', 'pad' or 'crop', got {mode!r}")
    s = min(ho / hi, wo / wi) if mode == "pad" else max(ho / hi, wo / wi)
    if anchor == "top_or_left":
        return [[s, 0.0, 0.0], [0.0, s, 0.0]]
    if anchor not in ("center", "bottom_or_right"):
        raise ValueError(f"{who}: anchor must be 'top_or_left', 'center' or 'bottom_or_right', got {anchor!r}")
    k = 0.5 if anchor == "center" else 1.0
    return [[s, 0.0, wo * k - s * wi * k], [0.0, s, ho * k - s * hi * k]]


def sample_photometric_params(num_groups, views_per_group, *, min_max_brightness, min_max_hue, min_max_contrast,
                              min_max_saturation, prob_brightness_aug=0.5, prob_hue_aug=0.5, prob_contrast_aug=0.5,
                              prob_saturation_aug=0.5, prob_swap_channels=0.5, generator=None) -> torch.Tensor:
    """The random decisions of ``PhotoMetricDistorter._get_augmentation_setup`` as rows for ``prepare_images``: a CPU
    float32 tensor ``[num_groups * views_per_group, 6]`` of ``(delta, alpha_pre, saturation, hue_degrees, alpha_post,
    permutation_index)``.

    One draw per group, repeated for its ``views_per_group`` consecutive rows: the reference shares one draw across all
    images of a sample.  Each augmentation is switched on with its own probability; one that is off writes the identity
    value (0, 1, 1, 0, 1, 0).  ``min_max_brightness`` is a bias in 0..255 units (the reference's convention for uint8
    images) and is divided by 255 here; hue is in degrees; contrast and saturation are factors.  The contrast factor goes
    to ``alpha_pre`` or ``alpha_post`` by a coin flip (the reference's ``contrast_mode``), never to both.  The permutation
    index is uniform over 0..5.  Eleven uniform numbers are drawn per group from ``generator`` whatever the decisions
    are, so the stream of a seeded generator does not depend on them.
    """
    who = "sample_photometric_params"
    if not is_int(num_groups) or not is_int(views_per_group) or num_groups < 0 or views_per_group < 1:
        raise RuntimeError(f"{who}: num_groups >= 0 and views_per_group >= 1 Python ints, got {num_groups!r}, {views_per_group!r}")
    ranges = {}
    for name, v in (("min_max_brightness", min_max_brightness), ("min_max_hue", min_max_hue),
                    ("min_max_contrast", min_max_contrast), ("min_max_saturation", min_max_saturation)):
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(is_number(x) and math.isfinite(x) for x in v) or v[0] > v[1]:
            raise RuntimeError(f"{who}: {name} must be (min, max) finite Python numbers with min <= max, got {v!r}")
        ranges[name] = (float(v[0]), float(v[1]))
    r = torch.rand((num_groups, 11), generator=generator, dtype=torch.float64)
    inf = torch.tensor(float("inf"))

    def within(col, name, scale=1.0):
        """uniform in the range, as float32 that the rounding does not take out of it"""
        lo, hi = (x * scale for x in ranges[name])
        v = (lo + r[:, col] * (hi - lo)).to(torch.float32)
        v = torch.where(v.double() > hi, torch.nextafter(v, -inf), v)
        return torch.where(v.double() < lo, torch.nextafter(v, inf), v)

    on_brightness, on_contrast = r[:, 0] < prob_brightness_aug, r[:, 1] < prob_contrast_aug
    on_saturation, on_hue, on_swap = r[:, 2] < prob_saturation_aug, r[:, 3] < prob_hue_aug, r[:, 4] < prob_swap_channels
    pre = r[:, 5] >= 0.5                              # contrast_mode 1: in front of the HSV stage
    one, zero = torch.ones(num_groups), torch.zeros(num_groups)
    alpha = within(7, "min_max_contrast")
    rows = torch.stack([
        torch.where(on_brightness, within(6, "min_max_brightness", 1.0 / 255.0), zero),
        torch.where(on_contrast & pre, alpha, one),
        torch.where(on_saturation, within(9, "min_max_saturation"), one),
        torch.where(on_hue, within(8, "min_max_hue"), zero),
        torch.where(on_contrast & ~pre, alpha, one),
        torch.where(on_swap, torch.clamp(torch.floor(r[:, 10] * 6.0), max=5.0).to(torch.float32), zero),
    ], dim=1)
    return rows.repeat_interleave(views_per_group, dim=0).contiguous()


def _three(name, v, who=_WHO):
    if is_number(v):
        v = (v, v, v)
    if not isinstance(v, (list, tuple)) or len(v) != 3 or not all(is_number(x) and math.isfinite(x) for x in v):
        raise RuntimeError(f"{who}: {name} must be a finite Python number or three of them, got {v!r}")
    return tuple(float(x) for x in v)


def _prepare(images, output_hw, transforms, source_hw, photometric, is_bgr, mean, std, tile_hw, pad_before_normalize, layout,
             dtype, out, coords, who=_WHO, planes=None):
    """``planes``: None, or the checked NV12 source of ``nv12._planes`` in place of ``images``"""
    if planes is not None:
        dev, (B, Hs, Ws), theirs = planes.device, planes.bhw, "planes'"
    else:
        if not isinstance(images, torch.Tensor):
            raise RuntimeError(f"{who}: images must be a tensor")
        if images.dtype != torch.uint8:
            raise TypeError(f"{who}: images must be uint8 (a decoder's output), got {images.dtype}")
        if images.dim() != 4 or images.shape[3] != 3:
            raise RuntimeError(f"{who}: images must be uint8 [B, H, W, 3], got {tuple(images.shape)}")
        dev, theirs = images.device, "images'"
        if dev.type not in ("cuda", "cpu"):
            raise RuntimeError(f"{who}: images must be CUDA or CPU tensors, got {dev}")
        B, Hs, Ws = (int(v) for v in images.shape[:3])
    if transforms is None:
        if output_hw is not None and _hw("output_hw", output_hw, who) != (Hs, Ws):
            raise RuntimeError(f"{who}: output_hw {tuple(output_hw)!r} differs from the source's {(Hs, Ws)!r}: that needs transforms")
        Ho, Wo = Hs, Ws
    else:
        Ho, Wo = (Hs, Ws) if output_hw is None else _hw("output_hw", output_hw, who)
    if not all(1 <= v <= MAX_EXTENT for v in (Hs, Ws, Ho, Wo)):
        raise RuntimeError(f"{who}: source {Hs} x {Ws} and output {Ho} x {Wo}: every extent must be in [1, {MAX_EXTENT}]")
    th, tw = _tile(tile_hw, who)
    mean3, std3 = _three("mean", mean, who), _three("std", std, who)
    if not all(s > 0 for s in std3):
        raise ValueError(f"{who}: std must be positive, got {std!r}")
    if layout not in _LAYOUTS:
        raise RuntimeError(f"{who}: layout must be 'CHW' or 'HWC', got {layout!r}")
    if dtype not in _DTYPES:
        raise TypeError(f"{who}: dtype must be torch.float32, float16 or bfloat16, got {dtype!r}")
    for name, t, dtypes, shape in (("transforms", transforms, (torch.float32,), (B, 2, 3)),
                                   ("photometric", photometric, (torch.float32,), (B, 6)),
                                   ("source_hw", source_hw, (torch.int32, torch.int64), (B, 2))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor")
        if t.is_floating_point() and torch.float32 in dtypes and t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
        if t.dtype not in dtypes or tuple(t.shape) != shape:
            raise RuntimeError(f"{who}: {name} must be {' or '.join(str(d) for d in dtypes)} {list(shape)}, "
                               f"got {t.dtype} {tuple(t.shape)}")
    Hp, Wp = padded_hw((Ho, Wo), (th, tw))
    shape = (B, 3, Hp, Wp) if layout == "CHW" else (B, Hp, Wp, 3)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise RuntimeError(f"{who}: out must be a tensor")
        if out.dtype != dtype:
            raise TypeError(f"{who}: out must be {dtype}, got {out.dtype}")
        if tuple(out.shape) != shape:
            raise RuntimeError(f"{who}: out must be {dtype} {list(shape)}, got {tuple(out.shape)}")
    for name, t in (("images", images), ("transforms", transforms), ("photometric", photometric), ("source_hw", source_hw),
                    ("out", out)):
        if t is None:
            continue
        if t.device != dev:
            raise RuntimeError(f"{who}: {name} must be on the {theirs} device {dev}, got {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous (it is not copied silently)")
    result = torch.empty(shape, dtype=dtype, device=dev) if out is None else out

    full = _nat.PrepareImagesParams() if planes is None else _nat.PrepareImagesNv12Params()
    p = full if planes is None else full.prepare
    p.batch, p.source_h, p.source_w, p.output_h, p.output_w, p.tile_h, p.tile_w = B, Hs, Ws, Ho, Wo, th, tw
    for c in range(3):
        p.mean[c], p.std[c] = mean3[c], std3[c]
    p.pad_before_normalize, p.is_bgr = int(bool(pad_before_normalize)), int(bool(is_bgr))
    p.layout, p.dtype = _LAYOUTS[layout], _DTYPES[dtype]
    p.source_hw_i64 = int(source_hw is not None and source_hw.dtype == torch.int64)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()   # noqa: E731
    rest = (ptr(source_hw), ptr(transforms), ptr(photometric), ctypes.addressof(full), ptr(result))
    if B > 0 and planes is not None:
        planes.fill(full.planes)
        _ops.run("accv_prepare_images_nv12", (ptr(planes.y), ptr(planes.uv), *rest), dev, who)
    elif B > 0:
        _ops.run("accv_prepare_images", (ptr(images), *rest), dev, who, (ptr(coords),))   # coords: the host entry only
    return result


def prepare_images(images, *, output_hw=None, transforms=None, source_hw=None, photometric=None, is_bgr=False, mean=0.0,
                   std=1.0, tile_hw=1, pad_before_normalize=True, layout="CHW", dtype=torch.float32, out=None) -> torch.Tensor:
    """Warp, photometric augmentation, normalisation and tile padding of a batch of decoded images, in one launch.

    Args:
        images: uint8 ``[B, Hs, Ws, 3]``, contiguous, on a GPU or on the CPU: a decoder's output.  Other dtypes raise
            ``TypeError``.  ``Hs, Ws`` and the output extent lie in ``[1, 16384]`` (more raises ``RuntimeError`` before
            any launch); ``B >= 0``; flat indices are 64-bit.
        output_hw: ``(Ho, Wo)`` of the warped image before padding; default and, without ``transforms``, the only
            value allowed: ``(Hs, Ws)``.
        transforms: float32 ``[B, 2, 3]`` on the images' device, read there: the FORWARD map from source to output
            coordinates ``[[a, b, tx], [c, d, ty]]`` (``inverse_map=False``), which is what the reference's
            ``AffineTransformer`` builds and also applies to points and projection matrices
            (:func:`output_size_transform` restates its resize step).  Pixel ``i`` covers ``[i, i + 1)``, its centre is at
            ``i + 0.5``, so the same matrix moves image and annotation points consistently.  ``None``: no resampling, the
            source pixel is taken as is; an identity matrix gives the same bits.
        source_hw: int32 / int64 ``[B, 2]`` rows ``(H, W)`` on the images' device, read there and clamped to
            ``[0, Hs] x [0, Ws]``: the valid region of each image inside a padded source tensor, as the ``image_hw`` of
            the neighbouring operators.  Bytes outside it are never read and count as outside the image.
        photometric: float32 ``[B, 6]`` on the images' device, one row ``(delta, alpha_pre, saturation, hue_degrees,
            alpha_post, permutation_index)`` per image (:func:`sample_photometric_params` draws them).
        is_bgr: the source's channel order, for the HSV stage.
        mean, std: a number or three, in 0..255 units and in OUTPUT channel order (after the permutation);
            ``std > 0`` or ``ValueError``.  ``ImageRange01Normalizer`` is ``mean=0, std=255``.
        tile_hw: an int or ``(tile_h, tile_w)``, each at least 1: the output extent is ``Hp = ceil(Ho / tile_h) * tile_h``
            and likewise ``Wp`` (:func:`padded_hw`).  The reference's ``tile_size_to_pad_to`` is ordered (x, y); this is
            (h, w).
        pad_before_normalize: padding pixels hold ``(0 - mean_c) / std_c`` (the StreamPETR order: padder, then
            normaliser); false: they hold 0.
        layout: ``"CHW"`` -> ``[B, 3, Hp, Wp]``, ``"HWC"`` -> ``[B, Hp, Wp, 3]``.
        dtype: float32, float16 or bfloat16; the 16-bit results are the float32 result rounded once to nearest even.
        out: an existing contiguous tensor of that shape, dtype and device to write into.

    Per output pixel ``(X, Y)`` of image ``b``, in float32:

    1. Position: ``det = a*d - b*c``; ``u = X + 0.5 - tx``, ``v = Y + 0.5 - ty``; ``sx = (d*u - b*v) / det - 0.5``,
       ``sy = (a*v - c*u) / det - 0.5``.  If an entry, ``det`` or ``1 / det`` is not finite or ``det == 0``, the whole image is
       outside.
    2. Sample: bilinear over the four neighbours of ``(floor(sx), floor(sy))``; a neighbour outside the valid region
       contributes 0.  That is ``warp_affine`` with ``fill_value=0`` and ``grid_sample`` with ``padding_mode="zeros",
       align_corners=False``.  Antialiasing is not part of it.
    3. Colour, on ``v`` = value / 255, following ``PhotoMetricDistorter._process_images``: ``clamp(v + delta)`` unless
       ``delta == 0``; ``clamp(v * alpha_pre)`` unless 1; unless ``saturation == 1 and hue_degrees == 0``: RGB -> HSV,
       ``s *= saturation`` (not clamped), ``h = (h + hue_degrees) mod 360``, HSV -> RGB by the standard piecewise-linear
       formula (``max == 0`` and ``max == min`` give ``s = 0, h = 0``; no division by zero; no clamp in this stage);
       ``clamp(v * alpha_post)`` unless 1; output channel ``k`` takes channel ``CHANNEL_PERMUTATIONS[index][k]`` (any other
       index value is 0); ``clamp(v)``.  ``clamp`` is to ``[0, 1]``.  A row of identity values equals ``photometric=None``
       bit for bit.
    4. ``out = (255 * v - mean_c) / std_c``, folded on the host to one multiply and one add per channel (computed in float64,
       rounded once to float32).

    Hue and saturation are defined in true HSV space, which is what the reference documents ("multiplicative in HSV space",
    hue in degrees), what its own tests hold the step to and what mmdet's ``PhotoMetricDistortion`` computes; DALI's internal
    colour-matrix approximation behind ``fn.hue`` / ``fn.saturation`` is not reproduced.  The reference rounds to uint8
    between its separate steps; this fused chain does not, so it differs from a step-by-step run by at most 0.5 / 255 per
    intermediate rounding before normalisation.

    Every output element is written exactly once; nothing is cleared or read beforehand.  GPU tensors run one HIP kernel on
    torch's current stream and device (a workgroup per image and 64 x 16 output tile, 4 consecutive x per lane; no
    workspace, no atomics, no host synchronisation); CPU tensors run the library's host entry over the same per-pixel
    functions, bit-equal to the kernel.  Nothing takes a gradient.
    """
    return _prepare(images, output_hw, transforms, source_hw, photometric, is_bgr, mean, std, tile_hw, pad_before_normalize,
                    layout, dtype, out, None)


def sample_positions(images, *, output_hw=None, transforms=None, source_hw=None) -> torch.Tensor:
    """Where every output pixel samples, from the library's host entry: a CPU float32 tensor ``[B, Ho, Wo, 4]`` of
    ``(x0, y0, wx, wy)`` (the top-left neighbour and the two weights; ``(-2, -2, 0, 0)`` where no neighbour can lie inside
    the valid region).  The arguments are those of :func:`prepare_images`, CPU tensors only.  Meant for tests and for
    checking a matrix convention, not for the hot path."""
    if not isinstance(images, torch.Tensor) or images.device.type != "cpu":
        raise RuntimeError("sample_positions: CPU tensors only")
    B, Hs, Ws = (int(v) for v in images.shape[:3])
    Ho, Wo = (Hs, Ws) if output_hw is None else _hw("output_hw", output_hw, "sample_positions")
    coords = torch.zeros((B, Ho, Wo, 4), dtype=torch.float32)
    _prepare(images, output_hw, transforms, source_hw, None, False, 0.0, 1.0, 1, True, "CHW", torch.float32, None, coords)
    return coords
