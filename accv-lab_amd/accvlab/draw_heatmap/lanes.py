"""Lane (polyline) rasteriser — the "lane_helpers polyline raster" of BASELINE.json config 3.

EXTENSION: the reference ships no polyline rasteriser; its lane package only samples polylines
(packages/lane_helpers/accvlab/lane_helpers/polyline/functions.py:27-111).  A lane is drawn here by composing the two
reference operators that exist: sample every lane at ``num_samples`` arc-length-uniform positions (``interpolate`` with
``relative=True``) and splat every sample as a Gaussian of a fixed radius (``draw_heatmap_batched`` with the
``small_radii`` hint: the splat kernel that walks each sample's few-pixel box).  Three launches, no host synchronisation:

    accv_polyline_sample  ->  accv_heatmap_targets_from_points_f32  ->  accv_draw_heatmap_batched_f32
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _amd_native as _nat
from ..lane_helpers.polyline import ops as _poly
from . import ops as _ops
from .ops import draw_heatmap_batched


def _fraction_rows(rows: int, num_samples: int, dev) -> torch.Tensor:
    """Arc-length fractions of the samples, one row per polyline: k / (num_samples - 1) in IEEE float32 (computed on the host so
    that the fused lane raster, which forms the same quotient inside its kernel, lands on the same samples bit for bit)."""
    if num_samples > 1:
        row = np.arange(num_samples, dtype=np.float32) / np.float32(num_samples - 1)
    else:
        row = np.zeros(1, np.float32)
    return torch.from_numpy(row).to(dev).unsqueeze(0).expand(rows, num_samples).contiguous()


def _check_polylines(polylines, num_samples: int) -> None:
    if not (isinstance(polylines, torch.Tensor) and polylines.is_cuda):
        raise RuntimeError("polylines must be a CUDA tensor")
    if not (polylines.dim() == 4 and polylines.size(3) == 2):
        raise RuntimeError("polylines must be of shape [batch, lanes, points, 2]")
    if not (polylines.dtype == torch.float32):
        raise RuntimeError(f"polylines: expected float32 but found {polylines.dtype}")
    if not (num_samples >= 1):
        raise RuntimeError("num_samples must be >= 1")


def _point_counts(num_points, b: int, l: int, p: int, dev):
    """``num_points`` int32 / int64 ``[B, L]`` -> flat counts ``[B * L]`` for the kernels (None: every point is valid)."""
    if num_points is None:
        return None
    if not (num_points.shape == (b, l) and num_points.device == dev):
        raise RuntimeError("num_points must be of shape [batch, lanes] on the polylines' device")
    _poly._check_sizes(num_points.reshape(-1), p, "num_points")
    return num_points.contiguous().view(b * l)


def _lane_sizes(num_lanes, b: int, l: int, per_lane: int, dev) -> torch.Tensor:
    """Objects per frame for the splat kernels: the first ``num_lanes[b]`` lanes of ``per_lane`` objects each (None: all ``l``
    lanes, a cached constant).  The kernels clamp a count to [0, l * per_lane]; clamping the lanes first keeps the product
    from overflowing.  int32 / int64 pass through, other dtypes become int64."""
    if num_lanes is None:
        n = l * per_lane
        return _ops._device_constant(("full", b, n, dev), lambda: torch.full((b,), n, dtype=torch.int32, device=dev))
    if not (num_lanes.shape == (b,)):
        raise RuntimeError("num_lanes must be of shape [batch]")
    if not (num_lanes.device == dev):
        raise RuntimeError("num_lanes must be on the polylines' device")
    sizes = num_lanes.contiguous() if per_lane == 1 else num_lanes.clamp(0, l) * per_lane
    return sizes if sizes.dtype in (torch.int32, torch.int64) else sizes.to(torch.int64)


def _samples(polylines: torch.Tensor, num_samples: int, counts, group_boxes_ptr: int = 0) -> torch.Tensor:
    """The sampler launch on checked polylines (``counts`` from :func:`_point_counts`) -> f32 ``[B, L * num_samples, 2]``."""
    b, l, p, _ = polylines.shape
    dev = polylines.device
    if b * l == 0:
        return torch.empty((b, l * num_samples, 2), dtype=torch.float32, device=dev)
    # arc-length fractions 0..1, one row per lane (a cached constant: no per-call kernel)
    frac = _ops._device_constant(("frac", b * l, num_samples, dev), lambda: _fraction_rows(b * l, num_samples, dev))
    samples = _poly._gpu(polylines.contiguous().view(b * l, p, 2), frac, counts, None, True, True, False, group_boxes_ptr)[0]
    return samples.view(b, l * num_samples, 2)


def sample_lane_targets(polylines: torch.Tensor, num_samples: int, radius: int, out_size_factor: float = 1.0, *,
                        num_points: Optional[torch.Tensor] = None):
    """``polylines`` f32 ``[B, L, P, 2]`` (x, y in source pixels; ``num_points`` int ``[B, L]`` = valid points per
    lane, default all) -> ``(centers i32 [B, L*num_samples, 2], radii i32 [B, L*num_samples])`` at the heat-map stride
    ``out_size_factor``: ``c = int(sample / stride)``.  Samples of empty lanes get radius -1 (never drawn)."""
    _check_polylines(polylines, num_samples)
    b, l, p, _ = polylines.shape
    dev = polylines.device
    counts = _point_counts(num_points, b, l, p, dev)
    centers = torch.empty((b, l * num_samples, 2), dtype=torch.int32, device=dev)
    radii = torch.empty((b, l * num_samples), dtype=torch.int32, device=dev)
    if b * l == 0:
        return centers, radii
    samples = _samples(polylines, num_samples, counts)
    with _nat.device_guard(dev):
        _nat.check(_nat.lib().accv_heatmap_targets_from_points_f32(
            samples.data_ptr(), b * l * num_samples, float(out_size_factor), int(radius), centers.data_ptr(),
            radii.data_ptr(), _nat.stream_ptr(dev)), "sample_lane_targets")
    return centers, radii


def draw_polylines_batched(heatmap: torch.Tensor, polylines: torch.Tensor, num_samples: int, radius: int,
                           out_size_factor: float = 1.0, diameter_to_sigma_factor: float = 6.0, k_scale: float = 1.0,
                           *, num_points: Optional[torch.Tensor] = None, num_lanes: Optional[torch.Tensor] = None,
                           clear: bool = False) -> None:
    """Draw ``polylines`` f32 ``[B, L, P, 2]`` into ``heatmap`` f32 ``[B, H, W]`` (in place, element-wise max; with
    ``clear=True`` fused zero-fill + draw) as chains of Gaussians of ``radius``.

    ``num_points`` int ``[B, L]``: valid points per lane; ``num_lanes`` int ``[B]``: only the first ``num_lanes[b]``
    lanes of a frame are drawn (both default to "all").  Choose ``num_samples`` so that the sample spacing
    (lane length / stride / (num_samples-1)) stays below ``radius`` for a gap-free line.

    Radii of a few pixels take :func:`draw_polylines_multiscale` with this one scale: on an aligned map its two-launch path
    (sampler + group boxes, then the point splat with its two-level cull: stride 4 of config 3 ≈ 19 + 6 µs against 30 + 6 + 4 µs
    for sampler -> integer targets -> ``draw_heatmap_batched``), on other maps the latter; the results are bit-identical
    (``tests/test_lane_raster_gpu.py`` compares the two formulations)."""
    if 0 <= radius <= 7:
        draw_polylines_multiscale([heatmap], polylines, num_samples, radius, [out_size_factor], diameter_to_sigma_factor,
                                  k_scale, num_points=num_points, num_lanes=num_lanes, clear=clear)
        return
    _draw_polylines_via_targets(heatmap, polylines, num_samples, radius, out_size_factor, diameter_to_sigma_factor, k_scale,
                                num_points=num_points, num_lanes=num_lanes, clear=clear)


def _draw_polylines_via_targets(heatmap: torch.Tensor, polylines: torch.Tensor, num_samples: int, radius: int,
                                out_size_factor: float = 1.0, diameter_to_sigma_factor: float = 6.0, k_scale: float = 1.0,
                                *, num_points: Optional[torch.Tensor] = None, num_lanes: Optional[torch.Tensor] = None,
                                clear: bool = False) -> None:
    """The composition of the reference operators spelled out: sampler -> integer targets -> ``draw_heatmap_batched`` (three
    launches; any radius, any map alignment).  The parity tests pin the lane raster stage by stage on this formulation."""
    centers, radii = sample_lane_targets(polylines, num_samples, radius, out_size_factor, num_points=num_points)
    b, l = polylines.shape[:2]
    sizes = _lane_sizes(num_lanes, b, l, num_samples, polylines.device)
    draw_heatmap_batched(heatmap, SimpleNamespace(tensor=centers, sample_sizes=sizes),
                         SimpleNamespace(tensor=radii, sample_sizes=sizes), diameter_to_sigma_factor, k_scale,
                         clear=clear, small_radii=radius <= 7)


def sample_lanes(polylines: torch.Tensor, num_samples: int, *, num_points: Optional[torch.Tensor] = None,
                 group_boxes_ptr: int = 0) -> torch.Tensor:
    """Arc-length-uniform samples of ``polylines`` f32 ``[B, L, P, 2]`` -> f32 ``[B, L * num_samples, 2]`` (source
    pixels; samples of empty lanes are NaN).  One launch of the polyline sampler; with ``group_boxes_ptr`` (and
    ``num_samples % 64 == 0``) the same launch also writes the bounding box of every 64 consecutive samples there."""
    _check_polylines(polylines, num_samples)
    b, l, p, _ = polylines.shape
    return _samples(polylines, num_samples, _point_counts(num_points, b, l, p, polylines.device), group_boxes_ptr)


# the fused kernel (sampling inside the tile waves) for the shapes it takes; False = always sampler + point splat (the tests
# compare the two bit for bit)
FUSED_SAMPLER = True


def _splat_points(geometry, strides, samples: torch.Tensor, sizes: torch.Tensor, radius: int, diameter_to_sigma_factor, k_scale,
                  clear: bool, work: torch.Tensor, boxes_given: bool) -> None:
    """ONE launch of the multi-scale point splat: ``geometry`` from ``ops._one_launch_maps`` for the samples' batch and device,
    ``samples`` f32 ``[B, N, 2]``, ``sizes`` from :func:`_lane_sizes`, ``work`` of accv_draw_points_workspace_bytes(B, N)
    bytes (with ``boxes_given``: holding the group boxes of every 64 samples already, written by the sampler)."""
    ptrs, hs, ws = geometry
    k = len(strides)
    b, n = samples.shape[:2]
    st = (ctypes.c_float * k)(*strides)
    flags = (_nat.HM_CLEAR if clear else 0) | (_nat.HM_COUNTS_I64 if sizes.dtype == torch.int64 else 0) | \
        (_nat.HM_GROUP_BOXES_GIVEN if boxes_given else 0) | _ops._FORCED_FLAGS
    dev = samples.device
    with _nat.device_guard(dev):
        status = _nat.lib().accv_draw_points_multiscale_f32(
            ptrs, hs, ws, st, k, b, samples.data_ptr(), sizes.data_ptr(), n, int(radius),
            float(diameter_to_sigma_factor), float(k_scale), flags, work.data_ptr(), work.numel(), _nat.stream_ptr(dev))
    _nat.check(status, "draw_polylines_multiscale")


class _SamplerJob:
    """The polyline sampler as a rider of the box-map launch (ops._launch_box_maps): where it reads the polylines and where it
    writes the samples and the group boxes (``work``, as :func:`_splat_points` reads them)."""

    def __init__(self, polylines, num_points, num_samples, work):
        b, l, p, _ = polylines.shape
        self.points = polylines.contiguous()
        self.num_polylines, self.num_points, self.num_samples, self.work = b * l, p, num_samples, work
        self.counts = _point_counts(num_points, b, l, p, polylines.device)
        self.flags = _nat.HM_POINT_COUNTS_I64 if self.counts is not None and self.counts.dtype == torch.int64 else 0
        self.samples = torch.empty((b, l * num_samples, 2), dtype=torch.float32, device=polylines.device)


def draw_targets_multiscale(heatmaps, centers, bboxes, out_size_factors, lane_heatmaps, polylines: torch.Tensor, num_samples: int,
                            radius: int, lane_out_size_factors=None, diameter_to_sigma_factor: float = 6.0, k_scale: float = 1.0, *,
                            num_points: Optional[torch.Tensor] = None, num_lanes: Optional[torch.Tensor] = None,
                            clear: bool = False) -> None:
    """(extension) Box maps and lane maps of one training step (BASELINE config 3).  Equivalent to::

        draw_heatmap_multiscale(heatmaps, centers, bboxes, out_size_factors, diameter_to_sigma_factor, k_scale, clear=clear)
        draw_polylines_multiscale(lane_heatmaps, polylines, num_samples, radius, lane_out_size_factors or out_size_factors,
                                  diameter_to_sigma_factor, k_scale, num_points=num_points, num_lanes=num_lanes, clear=clear)

    bit for bit, in TWO launches instead of three: the polyline sampler's workgroups ride in the box-map launch, which does not
    depend on them, and the point splat follows.  Needs polylines of at most 64 points and a multiple of 64 samples, and every
    map and object on the polylines' device with their batch; other inputs run the two calls above.  (Sparse lane sets, which
    ``draw_polylines_multiscale`` alone rasterises with its one-launch kernel, also take the rider here: 32.3 against 33.9 us
    per step on config 3's maps with one polyline per frame.)"""
    heatmaps, lane_heatmaps = list(heatmaps), list(lane_heatmaps)
    strides = [float(f) for f in out_size_factors]
    lane_strides = [float(f) for f in (out_size_factors if lane_out_size_factors is None else lane_out_size_factors)]
    shape = polylines.shape if isinstance(polylines, torch.Tensor) else ()
    box_geo = None
    if len(shape) == 4 and shape[3] == 2 and polylines.is_cuda and polylines.dtype == torch.float32 and \
            shape[0] * shape[1] > 0 and shape[2] <= 64 and num_samples % 64 == 0 and 64 <= num_samples <= (1 << 20) and \
            radius >= 0 and len(heatmaps) == len(strides) and len(lane_heatmaps) == len(lane_strides):
        b, dev = shape[0], polylines.device
        objects = _ops._box_objects(centers, bboxes)      # (raises what draw_heatmap_multiscale would)
        if objects[0].size(0) == b and objects[0].device == dev:
            # every map is looked at ONCE here and the arrays are handed to the launches (the python side of a step was 31 us
            # against 38 us of kernels)
            lane_geo = _ops._one_launch_maps(lane_heatmaps, b, dev)
            box_geo = _ops._one_launch_maps(heatmaps, b, dev) if lane_geo is not None else None
    if box_geo is None:
        _ops.draw_heatmap_multiscale(heatmaps, centers, bboxes, strides, diameter_to_sigma_factor, k_scale, clear=clear)
        draw_polylines_multiscale(lane_heatmaps, polylines, num_samples, radius, lane_strides, diameter_to_sigma_factor, k_scale,
                                  num_points=num_points, num_lanes=num_lanes, clear=clear)
        return
    l = shape[1]
    sizes = _lane_sizes(num_lanes, b, l, num_samples, dev)
    work = torch.empty(_nat.lib().accv_draw_points_workspace_bytes(b, l * num_samples), dtype=torch.uint8, device=dev)
    job = _SamplerJob(polylines, num_points, num_samples, work)
    _ops._launch_box_maps(box_geo, strides, objects, diameter_to_sigma_factor, k_scale, clear, job)
    _splat_points(lane_geo, lane_strides, job.samples, sizes, radius, diameter_to_sigma_factor, k_scale, clear, work, True)


def draw_polylines_multiscale(heatmaps, polylines: torch.Tensor, num_samples: int, radius: int, out_size_factors,
                              diameter_to_sigma_factor: float = 6.0, k_scale: float = 1.0, *,
                              num_points: Optional[torch.Tensor] = None, num_lanes: Optional[torch.Tensor] = None,
                              clear: bool = False) -> None:
    """Lane raster at several strides: equivalent to ``draw_polylines_batched(heatmaps[s], polylines, num_samples, radius,
    out_size_factors[s], ...)`` for every scale, in THREE launches altogether (sampler, group boxes, one splat over the
    tiles of all scales) instead of three per scale.  The splat culls in two levels — 64 consecutive samples share a
    bounding box — so a tile only walks the stretches of lane that can reach it.  Always uses the box-walking small-splat
    arithmetic (meant for radii of a few pixels)."""
    heatmaps = list(heatmaps)
    strides = [float(f) for f in out_size_factors]
    if not (len(heatmaps) == len(strides) and len(heatmaps) >= 1):
        raise RuntimeError("heatmaps and out_size_factors must have the same, non-zero length")
    _check_polylines(polylines, num_samples)
    b, l, p, _ = polylines.shape
    dev = polylines.device
    geometry = _ops._one_launch_maps(heatmaps, b, dev) if radius >= 0 else None
    if geometry is None:   # odd widths / more than four scales / a negative radius: the per-scale operator
        _ops._check_maps(heatmaps, b, dev, "polylines")
        for hm, f in zip(heatmaps, strides):
            _draw_polylines_via_targets(hm, polylines, num_samples, radius, f, diameter_to_sigma_factor, k_scale,
                                        num_points=num_points, num_lanes=num_lanes, clear=clear)
        return
    counts = _point_counts(num_points, b, l, p, dev)
    lib = _nat.lib()
    k = len(heatmaps)
    if FUSED_SAMPLER and b * l > 0 and lib.accv_draw_polylines_fused_applicable(geometry[1], geometry[2], k, b, l, p, num_samples):
        # ONE launch: the tile waves sample the polylines themselves (no sampler launch, no sample buffer)
        lanes = _lane_sizes(num_lanes, b, l, 1, dev)
        pts = polylines.contiguous()
        flags = (_nat.HM_CLEAR if clear else 0) | (_nat.HM_COUNTS_I64 if lanes.dtype == torch.int64 else 0) | \
            (_nat.HM_POINT_COUNTS_I64 if counts is not None and counts.dtype == torch.int64 else 0) | _ops._FORCED_FLAGS
        with _nat.device_guard(dev):
            status = lib.accv_draw_polylines_multiscale_f32(
                geometry[0], geometry[1], geometry[2], (ctypes.c_float * k)(*strides), k, b, pts.data_ptr(),
                l, p, counts.data_ptr() if counts is not None else None, lanes.data_ptr(), int(num_samples), int(radius),
                float(diameter_to_sigma_factor), float(k_scale), flags, _nat.stream_ptr(dev))
        _nat.check(status, "draw_polylines_multiscale")
        return
    sizes = _lane_sizes(num_lanes, b, l, num_samples, dev)
    work = torch.empty(lib.accv_draw_points_workspace_bytes(b, l * num_samples), dtype=torch.uint8, device=dev)
    # the sampler writes the group boxes itself when the groups of 64 do not straddle lanes (one launch less)
    boxes_by_sampler = num_samples % 64 == 0 and b * l > 0
    samples = _samples(polylines, num_samples, counts, work.data_ptr() if boxes_by_sampler else 0)
    _splat_points(geometry, strides, samples, sizes, radius, diameter_to_sigma_factor, k_scale, clear, work, boxes_by_sampler)
