"""(extension) The random decisions of the reference's ``AffineTransformer`` (packages/dali_pipeline_framework,
processing_steps/affine_transformer.py) as the ``[N, 2, 3]`` forward matrices that ``prepare_images(transforms=...)`` and
``accvlab.draw_heatmap.camera_augment_boxes`` take: a list of step descriptors named after the reference's steps and
:func:`sample_image_transforms`, which draws and composes them on the host.

The definition (``M`` is the running 3 x 3 matrix, ``(H, W) = source_hw``, ``c = (W/2, H/2)``): a step applies iff its
uniform draw is ``< prob``; a parameter with ``max`` is uniform in ``[min, max]``, without it exactly ``min``; each step
sets ``M <- S . M`` with ``S``

* ``Translation``: the translation by ``t``;
* ``UniformScaling`` / ``NonUniformScaling``: ``T(c) . diag(sx, sy) . T(-c)`` (a horizontal flip is
  ``NonUniformScaling(0.5, (-1, 1))``);
* ``Rotation``: about ``c`` by ``θ = -angle`` (degrees) as ``[[cos θ, -sin θ], [sin θ, cos θ]]``, so that a positive angle
  turns the picture anticlockwise on screen;
* ``Shearing``: about ``c`` as ``[[1, tan ax], [tan ay, 1]]``, angles in degrees;
* ``ShiftInsideOriginalImage``: with the images of ``(0, 0)`` and ``(W, H)`` under ``M`` and ``lo`` / ``hi`` their per-axis
  minimum and maximum, a shift drawn in ``[-lo, extent - hi]`` per enabled axis (the two ends swapped if reversed; 0 when
  the interval is empty or the axis is off);
* ``ShiftToAlignWithOriginalImageBorder``: ``ty = -lo_y`` (top), ``tx = -lo_x`` (left), ``ty = H - hi_y`` (bottom) or
  ``tx = W - hi_x`` (right);
* ``Selection``: one more uniform picks the first option whose cumulative probability it does not exceed.

The two shift steps raise ``ValueError`` if a ``Rotation`` or a ``Shearing`` can precede them, inside a ``Selection`` too.
The result is ``output_size_transform(source_hw, output_hw, mode, anchor) . M``.  One deliberate divergence: the
reference's fixed-factor ``NonUniformScaling`` forgets the prior matrix; this one composes like every other step.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .._amd_native.operands import is_int, is_number
from .prepare import _hw, output_size_transform

_BORDERS = ("top", "left", "bottom", "right")


def _prob(who, p):
    if not is_number(p) or not 0.0 <= p <= 1.0:
        raise RuntimeError(f"{who}: prob must be a number in [0, 1], got {p!r}")


def _pair(who, name, v):
    if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(is_number(x) and math.isfinite(x) for x in v):
        raise RuntimeError(f"{who}: {name} must be two finite numbers (x, y), got {v!r}")
    return float(v[0]), float(v[1])


def _scalar_range(who, lo, hi):
    if not is_number(lo) or not math.isfinite(lo) or (hi is not None and (not is_number(hi) or not math.isfinite(hi) or hi < lo)):
        raise RuntimeError(f"{who}: min must be a finite number and max, if given, a finite number not below it, got {lo!r}, {hi!r}")


def _pair_range(who, lo, hi):
    lo = _pair(who, "min_xy", lo)
    if hi is not None:
        hi = _pair(who, "max_xy", hi)
        if hi[0] < lo[0] or hi[1] < lo[1]:
            raise RuntimeError(f"{who}: max_xy must not lie below min_xy, got {lo!r}, {hi!r}")


def _between(lo, hi, u):
    return lo if hi is None else lo + u * (hi - lo)


def _about_center(lin, hw):
    """T(c) . lin . T(-c) for the 2 x 2 matrix `lin`"""
    c = np.array([hw[1] / 2.0, hw[0] / 2.0])
    S = np.eye(3)
    S[:2, :2] = lin
    S[:2, 2] = c - np.asarray(lin) @ c
    return S


def _shift(tx, ty):
    S = np.eye(3)
    S[0, 2], S[1, 2] = tx, ty
    return S


def _extent_of(M, hw):
    """per-axis minimum and maximum of the images of (0, 0) and (W, H) under M"""
    p0, p1 = (M @ np.array([0.0, 0.0, 1.0]))[:2], (M @ np.array([float(hw[1]), float(hw[0]), 1.0]))[:2]
    return np.minimum(p0, p1), np.maximum(p0, p1)


@dataclass(frozen=True)
class Translation:
    """translate by ``t``, uniform in ``[min_xy, max_xy]`` per axis (pixels)"""
    prob: float
    min_xy: Tuple[float, float]
    max_xy: Optional[Tuple[float, float]] = None
    draws = 3

    def __post_init__(self):
        _prob("Translation", self.prob), _pair_range("Translation", self.min_xy, self.max_xy)

    def matrix(self, M, hw, u):
        hi = self.max_xy or (None, None)
        return _shift(_between(float(self.min_xy[0]), hi[0], u[0]), _between(float(self.min_xy[1]), hi[1], u[1]))


@dataclass(frozen=True)
class ShiftInsideOriginalImage:
    """shift the transformed image by a random amount that keeps it inside (or, if larger, covering) the viewport"""
    prob: float
    shift_x: bool
    shift_y: bool
    draws = 3
    needs_axis_aligned = True

    def __post_init__(self):
        _prob("ShiftInsideOriginalImage", self.prob)

    def matrix(self, M, hw, u):
        lo, hi = _extent_of(M, hw)
        t = [0.0, 0.0]
        for d, (on, extent) in enumerate(((self.shift_x, hw[1]), (self.shift_y, hw[0]))):
            a, b = -lo[d], extent - hi[d]
            if a > b:
                a, b = b, a
            if on and a < b:
                t[d] = a + u[d] * (b - a)
        return _shift(*t)


@dataclass(frozen=True)
class ShiftToAlignWithOriginalImageBorder:
    """shift the transformed image so that it touches one border of the viewport"""
    prob: float
    border: str
    draws = 1
    needs_axis_aligned = True

    def __post_init__(self):
        _prob("ShiftToAlignWithOriginalImageBorder", self.prob)
        if self.border not in _BORDERS:
            raise RuntimeError(f"ShiftToAlignWithOriginalImageBorder: border must be one of {_BORDERS}, got {self.border!r}")

    def matrix(self, M, hw, u):
        lo, hi = _extent_of(M, hw)
        return {"top": _shift(0.0, -lo[1]), "left": _shift(-lo[0], 0.0), "bottom": _shift(0.0, hw[0] - hi[1]),
                "right": _shift(hw[1] - hi[0], 0.0)}[self.border]


@dataclass(frozen=True)
class Rotation:
    """rotate about the image centre by an angle in degrees, positive anticlockwise on screen"""
    prob: float
    min_rot: float
    max_rot: Optional[float] = None
    draws = 2
    breaks_axis_alignment = True

    def __post_init__(self):
        _prob("Rotation", self.prob), _scalar_range("Rotation", self.min_rot, self.max_rot)

    def matrix(self, M, hw, u):
        th = -math.radians(_between(float(self.min_rot), self.max_rot, u[0]))
        return _about_center([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]], hw)


@dataclass(frozen=True)
class UniformScaling:
    """scale both axes by one factor about the image centre"""
    prob: float
    min_scaling: float
    max_scaling: Optional[float] = None
    draws = 2

    def __post_init__(self):
        _prob("UniformScaling", self.prob), _scalar_range("UniformScaling", self.min_scaling, self.max_scaling)

    def matrix(self, M, hw, u):
        s = _between(float(self.min_scaling), self.max_scaling, u[0])
        return _about_center([[s, 0.0], [0.0, s]], hw)


@dataclass(frozen=True)
class NonUniformScaling:
    """scale each axis by its own factor about the image centre; ``(-1, 1)`` is the horizontal flip"""
    prob: float
    min_xy: Tuple[float, float]
    max_xy: Optional[Tuple[float, float]] = None
    draws = 3

    def __post_init__(self):
        _prob("NonUniformScaling", self.prob), _pair_range("NonUniformScaling", self.min_xy, self.max_xy)

    def matrix(self, M, hw, u):
        hi = self.max_xy or (None, None)
        sx, sy = _between(float(self.min_xy[0]), hi[0], u[0]), _between(float(self.min_xy[1]), hi[1], u[1])
        return _about_center([[sx, 0.0], [0.0, sy]], hw)


@dataclass(frozen=True)
class Shearing:
    """shear about the image centre, angles in degrees"""
    prob: float
    min_xy: Tuple[float, float]
    max_xy: Optional[Tuple[float, float]] = None
    draws = 3
    breaks_axis_alignment = True

    def __post_init__(self):
        _prob("Shearing", self.prob), _pair_range("Shearing", self.min_xy, self.max_xy)

    def matrix(self, M, hw, u):
        hi = self.max_xy or (None, None)
        ax, ay = _between(float(self.min_xy[0]), hi[0], u[0]), _between(float(self.min_xy[1]), hi[1], u[1])
        return _about_center([[1.0, math.tan(math.radians(ax))], [math.tan(math.radians(ay)), 1.0]], hw)


@dataclass(frozen=True)
class Selection:
    """apply one of ``options`` (a step, a sequence of steps, or ``None`` for "nothing"), chosen with ``option_probs``"""
    prob: float
    option_probs: Tuple[float, ...]
    options: tuple

    def __post_init__(self):
        _prob("Selection", self.prob)
        if (not isinstance(self.option_probs, (list, tuple)) or not isinstance(self.options, (list, tuple))
                or len(self.option_probs) != len(self.options) or not self.options):
            raise RuntimeError("Selection: option_probs and options must be sequences of one non-zero length")
        if not all(is_number(p) and p >= 0 for p in self.option_probs) or abs(sum(self.option_probs) - 1.0) > 1e-6:
            raise RuntimeError(f"Selection: option_probs must be non-negative and sum to 1, got {self.option_probs!r}")
        for o in self.sequences:
            for s in o:
                if not hasattr(s, "prob"):
                    raise RuntimeError(f"Selection: an option must be a step, a sequence of steps or None, got {s!r}")

    @property
    def sequences(self):
        return tuple(() if o is None else tuple(o) if isinstance(o, (list, tuple)) else (o,) for o in self.options)

    @property
    def draws(self):
        return 2 + sum(s.draws for o in self.sequences for s in o)


def _check_order(steps, breakers_before, who):
    """ValueError if a shift step can follow a rotation or a shearing; returns whether one can precede what follows"""
    for s in steps:
        if isinstance(s, Selection):
            after = [_check_order(o, breakers_before, who) for o in s.sequences]
            breakers_before = breakers_before or any(after)
        else:
            if getattr(s, "needs_axis_aligned", False) and breakers_before:
                raise ValueError(f"{who}: {type(s).__name__} cannot follow a step that may rotate or shear the image")
            breakers_before = breakers_before or getattr(s, "breaks_axis_alignment", False)
    return breakers_before


def _apply(steps, M, hw, u, col):
    """M after `steps`, reading the uniforms u[col:]; returns (M, the column behind the steps' draws)"""
    for s in steps:
        if isinstance(s, Selection):
            on, pick = u[col] < s.prob, u[col + 1]
            col += 2
            chosen, acc = len(s.sequences) - 1, 0.0
            for i, p in enumerate(s.option_probs):
                acc += p
                if pick <= acc:
                    chosen = i
                    break
            for i, o in enumerate(s.sequences):
                if on and i == chosen:
                    M, col = _apply(o, M, hw, u, col)
                else:
                    col += sum(x.draws for x in o)
        else:
            if u[col] < s.prob:
                M = s.matrix(M, hw, u[col + 1: col + s.draws]) @ M
            col += s.draws
    return M, col


def sample_image_transforms(num_groups, views_per_group, steps, *, source_hw, output_hw=None, mode="stretch", anchor="center",
                            generator=None) -> torch.Tensor:
    """The forward matrices of a batch of camera images as a CPU float32 tensor ``[num_groups * views_per_group, 2, 3]``:
    the tensor both ``prepare_images(transforms=...)`` and ``camera_augment_boxes`` take.

    One draw per group, repeated for its ``views_per_group`` consecutive rows: the reference builds one matrix per sample
    for all its cameras.  ``steps`` is a sequence of the step descriptors of this module, applied in order as the module
    docstring defines; ``source_hw`` is the extent ``(H, W)`` of the decoded images.  With ``output_hw`` the result is
    ``output_size_transform(source_hw, output_hw, mode, anchor) . M``, else ``M``.  Everything is computed in float64 and
    rounded once.  Each step draws a fixed number of float64 uniforms from ``generator`` (its decision, its parameters,
    and for a ``Selection`` those of every option) whatever the decisions are, so the stream of a seeded generator does
    not depend on them.

    Raises ``ValueError`` if ``ShiftInsideOriginalImage`` or ``ShiftToAlignWithOriginalImageBorder`` can follow a
    ``Rotation`` or a ``Shearing``.
    """
    who = "sample_image_transforms"
    if not is_int(num_groups) or not is_int(views_per_group) or num_groups < 0 or views_per_group < 1:
        raise RuntimeError(f"{who}: num_groups >= 0 and views_per_group >= 1 Python ints, got {num_groups!r}, {views_per_group!r}")
    if not isinstance(steps, (list, tuple)) or not all(hasattr(s, "prob") and hasattr(s, "draws") for s in steps):
        raise RuntimeError(f"{who}: steps must be a sequence of step descriptors")
    hw = _hw("source_hw", source_hw, who)
    if hw[0] <= 0 or hw[1] <= 0:
        raise RuntimeError(f"{who}: source_hw must be positive, got {source_hw!r}")
    _check_order(steps, False, who)
    final = np.eye(3)
    if output_hw is not None:
        final[:2] = np.array(output_size_transform(hw, output_hw, mode, anchor))
    total = sum(s.draws for s in steps)
    u = torch.rand((num_groups, total), generator=generator, dtype=torch.float64).numpy()
    out = np.zeros((num_groups, 2, 3), np.float32)
    for g in range(num_groups):
        M, col = _apply(steps, np.eye(3), hw, u[g], 0)
        assert col == total
        out[g] = (final @ M)[:2]
    return torch.from_numpy(out).repeat_interleave(views_per_group, dim=0).contiguous()
