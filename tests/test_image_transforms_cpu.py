"""sample_image_transforms and the step descriptors of accvlab.image_prep: the composition against hand-made float64
products, the StreamPETR recipe, the draw count, the refusals, and the shared pixel convention of prepare_images and
camera_augment_boxes."""
import math

import numpy as np
import pytest
import torch

from accvlab.image_prep import (NonUniformScaling, Rotation, Selection, Shearing, ShiftInsideOriginalImage,
                                ShiftToAlignWithOriginalImageBorder, Translation, UniformScaling, output_size_transform,
                                prepare_images, sample_image_transforms)

H, W = 900, 1600


def T(x, y):
    return np.array([[1.0, 0.0, x], [0.0, 1.0, y], [0.0, 0.0, 1.0]])


def about(lin):
    S = np.eye(3)
    S[:2, :2] = lin
    return T(W / 2, H / 2) @ S @ T(-W / 2, -H / 2)


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


def test_fixed_steps_equal_a_hand_composed_float64_product_rounded_once():
    th = -math.radians(30.0)
    tan = math.tan(math.radians(10.0))
    steps = [Translation(1.0, (3.0, -2.0)), NonUniformScaling(1.0, (-1.0, 1.0)), Rotation(1.0, 30.0), Shearing(0.0, (5.0, 5.0)),
             Shearing(1.0, (10.0, 0.0)), UniformScaling(1.0, 1.25), NonUniformScaling(1.0, (0.5, 2.0)),
             Selection(1.0, (0.0, 1.0), (Translation(1.0, (100.0, 0.0)), (Translation(1.0, (0.0, 7.0)), UniformScaling(0.0, 3.0)))),
             Selection(0.0, (1.0,), (Translation(1.0, (55.0, 55.0)),))]
    M = T(3, -2)
    for S in (about([[-1, 0], [0, 1]]), about([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]), about([[1, tan], [0, 1]]),
              about([[1.25, 0], [0, 1.25]]), about([[0.5, 0], [0, 2.0]]), T(0, 7)):
        M = S @ M
    got = sample_image_transforms(2, 1, steps, source_hw=(H, W), generator=gen())
    assert got.dtype == torch.float32 and got.shape == (2, 2, 3) and got.device.type == "cpu"
    assert np.array_equal(got[0].numpy(), M[:2].astype(np.float32)) and torch.equal(got[0], got[1])
    out = np.eye(3)
    out[:2] = output_size_transform((H, W), (256, 704), "pad", "center")
    got = sample_image_transforms(1, 1, steps, source_hw=(H, W), output_hw=(256, 704), mode="pad", generator=gen())
    assert np.array_equal(got[0].numpy(), (out @ M)[:2].astype(np.float32))


def test_a_positive_rotation_turns_the_picture_anticlockwise_on_screen():
    m = sample_image_transforms(1, 1, [Rotation(1.0, 90.0)], source_hw=(H, W))[0].double().numpy()
    right_of_centre = m @ np.array([W / 2 + 10, H / 2, 1.0])
    assert np.allclose(right_of_centre, [W / 2, H / 2 - 10], atol=1e-3)          # y grows downwards: it went up


STREAM_PETR = [NonUniformScaling(0.5, (-1.0, 1.0)), UniformScaling(1.0, 0.9, 1.1), ShiftToAlignWithOriginalImageBorder(1.0, "bottom")]


def test_stream_petr_recipe_lands_the_bottom_border_on_the_output_height():
    Ho, Wo = 256, 704
    m = sample_image_transforms(200, 6, STREAM_PETR, source_hw=(H, W), output_hw=(Ho, Wo), mode="crop", anchor="bottom_or_right",
                                generator=gen(3)).double()
    assert m.shape == (1200, 2, 3)
    groups = m.reshape(200, 6, 2, 3)
    assert bool((groups == groups[:, :1]).all())                                  # the views of a group share one matrix
    g = groups[:, 0]
    bottom = g[:, 1, 1] * H + g[:, 1, 2]
    assert float((bottom - Ho).abs().max()) <= 1e-3
    base = max(Ho / H, Wo / W)
    scale = g[:, 1, 1] / base
    assert float(scale.min()) >= 0.9 - 1e-6 and float(scale.max()) <= 1.1 + 1e-6 and float(scale.max() - scale.min()) > 0.1
    assert bool((g[:, 0, 0].abs() / base - scale).abs().max() < 1e-6) and bool((g[:, 0, 1] == 0).all())
    flipped = g[:, 0, 0] < 0
    assert 50 < int(flipped.sum()) < 150
    assert len({tuple(r.reshape(-1).tolist()) for r in g}) == 200


def test_the_number_of_draws_per_group_does_not_depend_on_the_decisions():
    def recipe(p, q):
        return [NonUniformScaling(p, (-1.0, 1.0)), UniformScaling(p, 0.9, 1.1), Translation(p, (0.0, 0.0), (4.0, 4.0)), Rotation(p, -5.0),
                Shearing(p, (1.0, 1.0)), Selection(p, (q, 1.0 - q), (ShiftInsideOriginalImage(p, True, False), None)),
                Selection(1.0 - p, (1.0 - q, q), ((Translation(1.0, (1.0, 1.0)), UniformScaling(p, 2.0)), Rotation(1.0, 3.0)))]

    states, expected = [], 3 + 2 + 3 + 2 + 3 + (2 + 3) + (2 + 3 + 2 + 2)
    for p, q in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.3)):
        steps = recipe(p, q)
        # the shift sits in front of every rotation of its own recipe only through the Selection's options: reorder
        steps = [steps[5]] + steps[:5] + steps[6:]
        g = gen(11)
        sample_image_transforms(7, 2, steps, source_hw=(H, W), generator=g)
        states.append(g.get_state())
        assert sum(s.draws for s in steps) == expected
    ref = gen(11)
    torch.rand((7, expected), generator=ref, dtype=torch.float64)
    assert all(torch.equal(s, ref.get_state()) for s in states)


def test_rotation_or_shearing_before_a_shift_step_is_refused():
    shift, align = ShiftInsideOriginalImage(1.0, True, True), ShiftToAlignWithOriginalImageBorder(1.0, "top")
    for steps in ([Rotation(0.0, 5.0), shift], [Shearing(0.5, (1.0, 1.0)), UniformScaling(1.0, 2.0), align],
                  [Selection(0.5, (0.5, 0.5), (Rotation(1.0, 5.0), None)), align],
                  [Selection(1.0, (1.0,), ((Rotation(1.0, 5.0), shift),))]):
        with pytest.raises(ValueError, match="rotate or shear"):
            sample_image_transforms(1, 1, steps, source_hw=(H, W))
    sample_image_transforms(1, 1, [shift, align, Rotation(1.0, 5.0), Selection(1.0, (1.0,), (Shearing(1.0, (1.0, 1.0)),))], source_hw=(H, W))


def test_shift_inside_keeps_a_smaller_image_inside_and_a_larger_one_covering():
    for factor in (0.5, 1.5):
        m = sample_image_transforms(50, 1, [NonUniformScaling(0.5, (-1.0, 1.0)), UniformScaling(1.0, factor), ShiftInsideOriginalImage(1.0, True, True)],
                                    source_hw=(H, W), generator=gen(5)).double()
        p0, p1 = m[:, :, 2], m[:, :, 0] * W + m[:, :, 1] * H + m[:, :, 2]
        lo, hi = torch.minimum(p0, p1), torch.maximum(p0, p1)
        extent = torch.tensor([W, H], dtype=torch.float64)
        if factor < 1:
            assert bool((lo >= -1e-3).all()) and bool((hi <= extent + 1e-3).all())
        else:
            assert bool((lo <= 1e-3).all()) and bool((hi >= extent - 1e-3).all())
        assert float(lo[:, 0].max() - lo[:, 0].min()) > 50
    only_y = sample_image_transforms(20, 1, [UniformScaling(1.0, 0.5), ShiftInsideOriginalImage(1.0, False, True)], source_hw=(H, W), generator=gen(6))
    assert bool((only_y[:, 0, 2] == W / 4).all()) and float(only_y[:, 1, 2].max() - only_y[:, 1, 2].min()) > 50


@pytest.mark.parametrize("border,expect", [("top", (None, 0.0, None, None)), ("left", (0.0, None, None, None)),
                                           ("bottom", (None, None, None, float(H))), ("right", (None, None, float(W), None))])
def test_align_with_each_border(border, expect):
    m = sample_image_transforms(1, 1, [NonUniformScaling(1.0, (-0.5, 0.75)), ShiftToAlignWithOriginalImageBorder(1.0, border)],
                                source_hw=(H, W))[0].double()
    p0, p1 = m[:, 2], m[:, 0] * W + m[:, 1] * H + m[:, 2]
    got = (float(min(p0[0], p1[0])), float(min(p0[1], p1[1])), float(max(p0[0], p1[0])), float(max(p0[1], p1[1])))
    for g, e in zip(got, expect):
        assert e is None or abs(g - e) <= 1e-3


def test_wrong_arguments_are_refused():
    with pytest.raises(RuntimeError, match="sum to 1"):
        Selection(1.0, (0.5, 0.4), (None, None))
    with pytest.raises(RuntimeError):
        Selection(1.0, (1.0,), (3,))
    with pytest.raises(RuntimeError, match="border"):
        ShiftToAlignWithOriginalImageBorder(1.0, "middle")
    with pytest.raises(RuntimeError, match="prob"):
        Rotation(1.5, 3.0)
    with pytest.raises(RuntimeError):
        UniformScaling(1.0, 1.1, 0.9)
    with pytest.raises(RuntimeError):
        Translation(1.0, (1.0,))
    with pytest.raises(RuntimeError):
        sample_image_transforms(1, 0, [], source_hw=(H, W))
    with pytest.raises(RuntimeError):
        sample_image_transforms(1, 1, [3], source_hw=(H, W))
    assert sample_image_transforms(0, 3, STREAM_PETR, source_hw=(H, W)).shape == (0, 2, 3)
    assert torch.equal(sample_image_transforms(2, 1, [], source_hw=(H, W))[1], torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_box_warped_by_camera_augment_boxes_encloses_the_bright_pixels_of_the_warped_image(seed):
    """The matrix moves the image in prepare_images and the box in camera_augment_boxes by one convention: pixel i covers
    [i, i + 1) with its centre at i + 0.5.  A bilinear sample at source position p reads the pixels floor(p - 0.5) and the
    next one, so an output pixel is bright only if its centre maps to within half a source pixel of the rectangle, and fully
    bright if it maps at least half a source pixel inside.  Half a source pixel is 0.5 * s output pixels for the matrix
    scale s (at most 0.75 * 1.1 here): that is the tolerance, well inside the one pixel of the bilinear footprint.  A
    half-pixel disagreement between the two conventions moves one side by 0.5 output pixels and breaks it."""
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import camera_augment_boxes

    hs, ws, ho, wo = 48, 64, 36, 48
    x0, y0, x1, y1 = 9, 7, 30, 25                                                 # bright pixels x0 .. x1 - 1, y0 .. y1 - 1
    img = torch.zeros((1, hs, ws, 3), dtype=torch.uint8)
    img[0, y0:y1, x0:x1] = 255
    steps = [NonUniformScaling(0.5, (-1.0, 1.0)), UniformScaling(1.0, 0.9, 1.1), Translation(1.0, (-6.0, -5.0), (6.0, 5.0))]
    t = sample_image_transforms(1, 1, steps, source_hw=(hs, ws), output_hw=(ho, wo), generator=gen(seed))
    out = prepare_images(img, output_hw=(ho, wo), transforms=t)[0, 0]
    boxes = RaggedBatch(torch.tensor([[[x0, y0, x1, y1]]], dtype=torch.float32), sample_sizes=torch.tensor([1]))
    res = camera_augment_boxes(boxes, t, image_hw=(ho, wo), check_occlusion=False, crop=False, order_corners=True)
    bx0, by0, bx1, by1 = res.bboxes.tensor[0, 0].tolist()
    ys, xs = torch.nonzero(out > 0, as_tuple=True)
    assert len(xs) > 100
    cx, cy = xs.double() + 0.5, ys.double() + 0.5
    tol = 0.5 * abs(float(t[0, 0, 0])) + 1e-3
    assert abs(float(t[0, 0, 0])) == abs(float(t[0, 1, 1])) and tol < 1.0
    assert float(cx.min()) >= bx0 - tol and float(cx.max()) <= bx1 + tol and float(cy.min()) >= by0 - tol and float(cy.max()) <= by1 + tol
    # and the other way round: every pixel whose centre lies one pixel inside the box (and the image) is fully bright
    X, Y = torch.meshgrid(torch.arange(wo) + 0.5, torch.arange(ho) + 0.5, indexing="xy")
    inside = (X >= bx0 + tol) & (X <= bx1 - tol) & (Y >= by0 + tol) & (Y <= by1 - tol)
    assert int(inside.sum()) > 50 and float(out[inside].min()) >= 255.0 - 1e-2
