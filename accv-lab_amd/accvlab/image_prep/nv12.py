"""(extension) NV12 decoder surfaces as the source of the camera leg: the reference's ``convert_nv12_to_rgb``
(packages/on_demand_video_decoder, ext_impl/src/PyNvOnDemandDecoder/src/ColorConvertKernels.cu) as an operator of its own,
and :func:`prepare_images_nv12`, which is ``prepare_images`` reading the two planes directly so that the RGB batch never
exists.

A hardware video or JPEG decoder hands out NV12: a pitched Y plane followed by an interleaved, 2 x 2 subsampled UV plane.
The per-pixel arithmetic is ``csrc/nv12_arith.h``, the conversion kernel ``csrc/nv12.hip``, the fused reader the NV12
instantiation of ``csrc/image_prep.hip``.
"""
from __future__ import annotations

import ctypes

import torch

from .. import _amd_native as _nat
from .._amd_native import operands as _ops
from . import prepare as _prep

MAX_EXTENT = _nat.IP_MAX_EXTENT
_ORDERS = {"uv": 0, "vu": 1}


def nv12_planes(surfaces, hw, *, uv_row=None):
    """The two plane views ``(y, uv)`` of images of ``hw = (H, W)`` inside whole decoder surfaces.

    ``surfaces`` is a uint8 tensor ``[B, rows, pitch]`` with ``stride(-1) == 1``.  The Y plane is rows ``[0, H)``, bytes
    ``[0, W)``; the UV plane starts at row ``uv_row`` (default ``H``; a decoder that aligns the luma height passes its aligned
    height) and has ``ceil(H / 2)`` rows of ``ceil(W / 2)`` interleaved pairs.  Returns ``y`` ``[B, H, W]`` and ``uv``
    ``[B, ceil(H / 2), ceil(W / 2), 2]`` as views: nothing is copied.  Raises ``RuntimeError`` if ``pitch < 2 * ceil(W / 2)``
    or the rows do not fit.
    """
    who = "nv12_planes"
    if not isinstance(surfaces, torch.Tensor):
        raise RuntimeError(f"{who}: surfaces must be a tensor")
    if surfaces.dtype != torch.uint8:
        raise TypeError(f"{who}: surfaces must be uint8, got {surfaces.dtype}")
    if surfaces.dim() != 3 or (surfaces.numel() > 0 and surfaces.shape[2] > 1 and surfaces.stride(2) != 1):
        raise RuntimeError(f"{who}: surfaces must be uint8 [B, rows, pitch] with stride(-1) == 1, got {tuple(surfaces.shape)} "
                           f"with strides {tuple(surfaces.stride())}")
    H, W = _prep._hw("hw", hw, who)
    if H < 1 or W < 1:
        raise RuntimeError(f"{who}: hw must be positive, got {hw!r}")
    B, rows, pitch = (int(v) for v in surfaces.shape)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    first = H if uv_row is None else uv_row
    if not _ops.is_int(first) or first < H:
        raise RuntimeError(f"{who}: uv_row must be a Python int of at least H = {H}, got {uv_row!r}")
    if pitch < 2 * Wc:
        raise RuntimeError(f"{who}: a pitch of {pitch} bytes is too small for {Wc} chroma pairs ({2 * Wc} bytes) of width {W}")
    if first + Hc > rows:
        raise RuntimeError(f"{who}: {rows} rows do not hold a UV plane of {Hc} rows from row {first} on")
    y = surfaces[:, :H, :W]
    uv = surfaces[:, first:first + Hc, :2 * Wc].unflatten(2, (Wc, 2))
    return y, uv


class _Planes:
    """the checked NV12 source of one call"""

    def __init__(self, who, y, uv, full_range, as_bgr, chroma_order):
        for name, t in (("y", y), ("uv", uv)):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f"{who}: {name} must be a tensor")
            if t.dtype != torch.uint8:
                raise TypeError(f"{who}: {name} must be uint8 (a decoder's surface), got {t.dtype}")
        if y.dim() != 3:
            raise RuntimeError(f"{who}: y must be uint8 [B, H, W], got {tuple(y.shape)}")
        B, H, W = (int(v) for v in y.shape)
        if y.device.type not in ("cuda", "cpu"):
            raise RuntimeError(f"{who}: y must be a CUDA or CPU tensor, got {y.device}")
        if uv.device != y.device:
            raise RuntimeError(f"{who}: uv must be on y's device {y.device}, got {uv.device}")
        want = (B, (H + 1) // 2, (W + 1) // 2, 2)
        if tuple(uv.shape) != want:
            raise RuntimeError(f"{who}: uv must be uint8 {list(want)} for y {[B, H, W]}, got {tuple(uv.shape)}")
        if chroma_order not in _ORDERS:
            raise RuntimeError(f"{who}: chroma_order must be 'uv' (NV12) or 'vu' (NV21), got {chroma_order!r}")
        if B > 0 and W > 1 and y.stride(2) != 1:      # the strides of an empty tensor mean nothing
            raise RuntimeError(f"{who}: y must have stride(-1) == 1, got strides {tuple(y.stride())} (it is not copied silently)")
        if B > 0 and (uv.stride(3) != 1 or (want[2] > 1 and uv.stride(2) != 2)):
            raise RuntimeError(f"{who}: uv must have stride(-1) == 1 and stride(-2) == 2, got strides {tuple(uv.stride())} "
                               "(it is not copied silently)")
        self.y, self.uv, self.device, self.bhw = y, uv, y.device, (B, H, W)
        self.format = (int(bool(full_range)), int(bool(as_bgr)), _ORDERS[chroma_order])

    def fill(self, p):
        """the accv_nv12_params of these planes; uint8, so element strides are byte strides"""
        p.batch, p.height, p.width = self.bhw
        p.y_stride_batch, p.y_stride_row = self.y.stride(0), self.y.stride(1)
        p.uv_stride_batch, p.uv_stride_row = self.uv.stride(0), self.uv.stride(1)
        p.full_range, p.as_bgr, p.chroma_vu = self.format


def nv12_to_rgb(y, uv, *, full_range=False, as_bgr=False, chroma_order="uv", out=None) -> torch.Tensor:
    """NV12 planes to interleaved uint8 RGB ``[B, H, W, 3]`` in one launch: ``convert_nv12_to_rgb`` of the reference.

    Args:
        y: uint8 ``[B, H, W]``, on a GPU or on the CPU.  Other dtypes raise ``TypeError``.  ``H, W`` lie in
            ``[1, 16384]`` (more raises ``RuntimeError`` before any launch); ``B >= 0``; flat indices are 64-bit.
        uv: uint8 ``[B, ceil(H / 2), ceil(W / 2), 2]`` on the same device.  Odd ``H`` and ``W`` are legal: the last row or
            column shares the chroma sample of its partner.
        full_range: false: limited ("video") range, Y in 16..235; true: full ("JPEG") range.
        as_bgr: the triple is written as B, G, R.
        chroma_order: ``"uv"`` (NV12: U at the even byte) or ``"vu"`` (NV21); the reference's ``uidx``.
        out: an existing contiguous uint8 ``[B, H, W, 3]`` tensor on that device to write into.

    Both planes may be strided views, as decoder surfaces are pitched (:func:`nv12_planes` cuts them from whole surfaces):
    ``y.stride(-1) == 1``, ``uv.stride(-1) == 1`` and ``uv.stride(-2) == 2`` are required, row and batch strides are free;
    anything else raises ``RuntimeError`` naming the argument, and nothing is copied silently.  Nothing beyond ``W`` bytes of
    a Y row and ``2 * ceil(W / 2)`` bytes of a UV row is read.

    Per pixel ``(x, y)``, with the ``U, V`` of chroma sample ``(y // 2, x // 2)`` (taken nearest, not interpolated):

    * limited range, all int32, ``>> 20`` an arithmetic shift: ``yy = max(0, Y - 16) * 1220542``, ``uu = U - 128``,
      ``vv = V - 128``; ``R = clamp((yy + 1673527 * vv + 2**19) >> 20, 0, 255)``,
      ``G = clamp((yy - 852492 * vv - 409993 * uu + 2**19) >> 20, 0, 255)``,
      ``B = clamp((yy + 2116026 * uu + 2**19) >> 20, 0, 255)``: bit-equal to the reference.
    * full range, float32, one IEEE operation per operator in the order written: ``yy = max(0, Y) * C0``,
      ``uu = U - 127.5``, ``vv = V - 127.5``; ``r = int((yy + C1 * vv) + 0.5)``, ``g = int(((yy + C2 * vv) + C3 * uu) + 0.5)``,
      ``b = int((yy + C4 * uu) + 0.5)`` (truncating toward zero), then ``clamp((t + 2**19) >> 20, 0, 255)``; ``C0..C4`` are the
      float32 nearest 1048230.1882352941, 1470078.6196078432, -748855.7176470588, -360150.7137254902 and 1858783.6235294119.
      Documented divergence: the reference builds with fast math, so its compiler may contract these operations into fma;
      this library's definition is the uncontracted sequence, the same on the device and on the host.

    Every output byte is written exactly once.  GPU tensors run one HIP kernel on torch's current stream and device (a
    workgroup per image and 64 x 16 tile, 4 consecutive x per lane; no workspace, no atomics, no host synchronisation); CPU
    tensors run the library's host entry over the same per-pixel functions, bit-equal to the kernel.
    """
    who = "nv12_to_rgb"
    planes = _Planes(who, y, uv, full_range, as_bgr, chroma_order)
    B, H, W = planes.bhw
    dev = planes.device
    if not all(1 <= v <= MAX_EXTENT for v in (H, W)):
        raise RuntimeError(f"{who}: planes of {H} x {W}: every extent must be in [1, {MAX_EXTENT}]")
    shape = (B, H, W, 3)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise RuntimeError(f"{who}: out must be a tensor")
        if out.dtype != torch.uint8:
            raise TypeError(f"{who}: out must be {torch.uint8}, got {out.dtype}")
        if tuple(out.shape) != shape:
            raise RuntimeError(f"{who}: out must be {torch.uint8} {list(shape)}, got {tuple(out.shape)}")
        if out.device != dev:
            raise RuntimeError(f"{who}: out must be on the planes' device {dev}, got {out.device}")
        if not out.is_contiguous():
            raise RuntimeError(f"{who}: out must be contiguous (it is not copied silently)")
    result = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out
    if B > 0:
        p = _nat.Nv12Params()
        planes.fill(p)
        args = (y.data_ptr(), uv.data_ptr(), ctypes.addressof(p), result.data_ptr())
        _ops.run("accv_nv12_to_rgb", args, dev, who)
    return result


def prepare_images_nv12(y, uv, *, full_range=False, as_bgr=False, chroma_order="uv", output_hw=None, transforms=None,
                        source_hw=None, photometric=None, mean=0.0, std=1.0, tile_hw=1, pad_before_normalize=True,
                        layout="CHW", dtype=torch.float32, out=None) -> torch.Tensor:
    """:func:`prepare_images` reading NV12 planes directly, in one launch: the RGB batch never exists.

    The contract: ``prepare_images_nv12(y, uv, full_range=f, as_bgr=g, chroma_order=o, **kw)`` is bit-equal to
    ``prepare_images(nv12_to_rgb(y, uv, full_range=f, as_bgr=g, chroma_order=o), is_bgr=g, **kw)``, for GPU tensors, for CPU
    tensors and between the two.  Every source tap is converted to the uint8 triple :func:`nv12_to_rgb` would have written
    (full range: the same uncontracted float32 sequence, the documented divergence from the reference's fast-math build);
    everything after it is the arithmetic of :func:`prepare_images` unchanged.

    ``y``, ``uv``, ``full_range``, ``as_bgr`` and ``chroma_order`` are those of :func:`nv12_to_rgb` (strided plane views
    included); every other keyword is that of :func:`prepare_images` with the planes' ``(H, W)`` as the source extent.
    There is no ``is_bgr``: the channel order of the HSV stage follows ``as_bgr``.  ``source_hw`` keeps its meaning, the
    valid region inside the planes: luma outside it is never read, and the chroma sample of a valid pixel always lies in
    the plane.

    The two taps of a source row share one UV pair when ``x0`` is even and take two adjacent pairs (4 contiguous bytes) when
    it is odd; the two rows of a bilinear footprint share a chroma row when ``y0`` is even.  Same launch shape as
    :func:`prepare_images`; no workspace, no atomics, no host synchronisation.
    """
    who = "prepare_images_nv12"
    planes = _Planes(who, y, uv, full_range, as_bgr, chroma_order)
    return _prep._prepare(None, output_hw, transforms, source_hw, photometric, as_bgr, mean, std, tile_hw, pad_before_normalize,
                          layout, dtype, out, None, who=who, planes=planes)
