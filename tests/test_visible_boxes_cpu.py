"""visible_bbox_mask / select_visible_bboxes without a GPU: the library's host entry (CPU tensors) against the reference's
hand-written vector, hand-worked geometry edges and the numpy canvas painter of visible_boxes_cases.py; the argument errors
and the ctypes binding alone.  All comparisons are torch.equal on booleans."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import visible_boxes_cases as vc  # noqa: E402

from accvlab.batching_helpers import RaggedBatch, batched_bool_indexing  # noqa: E402
from accvlab.draw_heatmap import get_centers_and_radii, select_visible_bboxes, visible_bbox_mask  # noqa: E402
from accvlab.draw_heatmap.visible_boxes import MAX_BOXES  # noqa: E402

op = visible_bbox_mask
REF = [(vc.REF_BOXES, vc.REF_DEPTHS, vc.REF_HW)]
MODES = {"occlusion": (dict(), vc.REF_OCCLUSION), "size": (dict(check_occlusion=False, minimum_size=2), vc.REF_SIZE),
         "both": (dict(minimum_size=2), [a & b for a, b in zip(vc.REF_OCCLUSION, vc.REF_SIZE)])}


def _bool(rows):
    return torch.tensor(rows, dtype=torch.bool).reshape(len(rows) if isinstance(rows[0], list) else 1, -1)


# ------------------------------------------------------------------------------------------------------ reference literal
@pytest.mark.parametrize("hw_as", ["tuple", "tensor", "int64"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_reference_vector(mode, hw_as):
    """visible_bbox_selector_test.py:62-80 and :169-184 of the reference"""
    kw, want = MODES[mode]
    assert torch.equal(vc.oracle(REF, 11, **kw), _bool(want)), "the oracle disagrees with the reference's expectation"
    assert torch.equal(vc.run(op, REF, hw_as=hw_as, **kw), _bool(want))


def test_max_boxes_is_at_least_256_and_one_more_slot_raises():
    assert MAX_BOXES >= 256
    boxes, depths, hw = vc.batch([([[1, 1, 2, 2]], [1], (8, 8))], G=MAX_BOXES + 1)
    with pytest.raises(RuntimeError, match="visible_bbox_mask.*MAX_BOXES"):
        op(boxes, depths, image_hw=hw)


# -------------------------------------------------------------------------------------------------------- partition edges
@pytest.mark.parametrize("kw", [dict(), dict(shrink_to_int=True), dict(minimum_size=3)], ids=["expand", "shrink", "with_size"])
def test_frame_sizes_at_wave_and_word_boundaries_with_hostile_padding(kw):
    frames = vc.partition_frames()
    assert [len(f[0]) for f in frames] == list(vc.PARTITION_SIZES) and MAX_BOXES == 256
    want = vc.oracle(frames, 256, **kw)
    assert torch.equal(vc.run(op, frames, **kw), want)
    real = sum(vc.PARTITION_SIZES)
    assert 0.1 * real < int(want.sum()) < 0.9 * real, "the case shows too little of one outcome"


# --------------------------------------------------------------------------------------------------------- geometry edges
@pytest.mark.parametrize("shrink", [False, True])
def test_geometry_edges_by_hand(shrink):
    names = sorted(vc.GEOMETRY)
    frames, want = vc.geometry_frames(names), vc.geometry_expected(shrink, 5, names)
    oracle = vc.oracle(frames, 5, shrink_to_int=shrink)
    got = vc.run(op, frames, shrink_to_int=shrink)
    for b, k in enumerate(names):
        assert torch.equal(oracle[b], want[b]), f"{k}: the oracle disagrees with the hand-worked expectation"
        assert torch.equal(got[b], want[b]), f"{k}: got {got[b].tolist()}, expected {want[b].tolist()}"


def test_two_frames_with_different_image_hw_rows():
    want = _bool(vc.TWO_SIZES_EXPECTED)
    assert torch.equal(vc.oracle(vc.TWO_SIZES, 2), want)
    assert torch.equal(vc.run(op, vc.TWO_SIZES), want)


def test_size_test_clips_raw_coordinates_and_fails_on_nan():
    boxes = [[-5, 1, 1.5, 9], [-5, 1, 2, 9], [18.5, 1, 30, 9], [4, 11, 9, 30], [4, vc.NAN, 9, 5], [9, 9, 4, 2], [4, 4, 5.5, 5.5]]
    frames = [(boxes, [1] * 7, vc.HW)]
    for ms, want in ((2, [0, 1, 0, 0, 0, 1, 0]), (1.5, [1, 1, 1, 0, 0, 1, 1]), (0, [1, 1, 1, 1, 0, 1, 1])):
        kw = dict(check_occlusion=False, minimum_size=ms)
        assert torch.equal(vc.oracle(frames, 7, **kw), _bool(want)), ms
        assert torch.equal(vc.run(op, frames, **kw), _bool(want)), ms


# ------------------------------------------------------------------------------------------------------------------ sweeps
@pytest.mark.parametrize("shrink", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_sweep_against_the_canvas_oracle(seed, shrink):
    frames = vc.sweep_frames(seed)
    G = max(len(f[0]) for f in frames)
    want = vc.oracle(frames, G, shrink_to_int=shrink)
    real, seen = sum(len(f[0]) for f in frames), int(want.sum())
    print(f"seed {seed} shrink {shrink}: {real} boxes, {seen / real:.1%} visible, {1 - seen / real:.1%} hidden")
    assert seen >= real / 5 and real - seen >= real / 5, "the sweep shows too little of one outcome"
    assert torch.equal(vc.run(op, frames, shrink_to_int=shrink), want)
    kw = dict(shrink_to_int=shrink, minimum_size=2.5)
    assert torch.equal(vc.run(op, frames, **kw), vc.oracle(frames, G, **kw))


# ------------------------------------------------------------------------------------------------ image-size independence
def test_full_hd_frame_with_128_boxes_against_the_canvas():
    frames = [vc.random_frame(np.random.default_rng(5), 128, (1080, 1920))]
    want = vc.oracle(frames, 128)
    assert 20 < int(want.sum()) < 108
    assert torch.equal(vc.run(op, frames, hw_as="tuple"), want)


def test_image_of_2_to_the_24_squared():
    assert torch.equal(vc.run(op, [vc.HUGE]), _bool(vc.HUGE_EXPECTED))
    b, d, hw = vc.HUGE
    assert torch.equal(vc.run(op, [(b[:5], d[:5], hw)], hw_as="tuple"), _bool(vc.HUGE_WITHOUT_LAST_EXPECTED))
    # values beyond 2^24 and below 0 are clamped: the same frame under an image_hw of 2^40, and nothing under -3
    assert torch.equal(vc.run(op, [(b, d, (1 << 40, 1 << 40))], hw_as="int64"), _bool(vc.HUGE_EXPECTED))
    assert not bool(vc.run(op, [(b, d, (-3, 50))]).any())


# ------------------------------------------------------------------------------------------------------------- the bindings
def test_ctypes_binding_alone_gives_the_same_result_and_sample_sizes_may_be_int32():
    from accvlab import _amd_native as nat

    frames = vc.sweep_frames(4, count=6)
    boxes, depths, hw = vc.batch(frames, size_dtype=torch.int32)
    B, G = boxes.tensor.shape[:2]
    want = vc.oracle(frames, G, minimum_size=2)
    assert torch.equal(op(boxes, depths, image_hw=hw, minimum_size=2).tensor, want)
    out = torch.full((B, G), 7, dtype=torch.uint8)
    p = nat.VisibleBoxesParams(2.0, 0, 0, 1, 1, 0)
    status = nat.ctypes_lib().accv_visible_boxes_host(boxes.tensor.data_ptr(), depths.tensor.data_ptr(), boxes.sample_sizes.data_ptr(),
                                                      hw.data_ptr(), 0, B, G, ctypes.addressof(p), out.data_ptr())
    assert status == 0, nat.ctypes_lib().accv_last_error()
    assert torch.equal(out, want.to(torch.uint8))


def test_c_entry_refuses_bad_arguments_before_reading_them():
    from accvlab import _amd_native as nat

    lib, d = nat.ctypes_lib(), ctypes.c_void_p(64)
    ok = nat.VisibleBoxesParams(0.0, 8, 8, 1, 0, 0)
    neither = nat.VisibleBoxesParams(0.0, 8, 8, 0, 0, 0)
    for fn, extra in ((lib.accv_visible_boxes, (None,)), (lib.accv_visible_boxes_host, ())):
        call = lambda *a: fn(*a, *extra)   # noqa: E731
        assert call(d, d, d, None, 0, 2, 4, None, d) == -1 and b"null params" in lib.accv_last_error()
        assert call(d, d, d, None, 0, -1, 4, ctypes.addressof(ok), d) == -1
        assert call(d, d, d, None, 4, 2, 4, ctypes.addressof(ok), d) == -1 and b"unknown flags" in lib.accv_last_error()
        assert call(d, d, d, None, 0, 2, 4, ctypes.addressof(neither), d) == -1 and b"at least one" in lib.accv_last_error()
        assert call(d, d, d, None, 0, 2, 257, ctypes.addressof(ok), d) == -1 and b"at most 256" in lib.accv_last_error()
        assert call(d, None, d, None, 0, 2, 4, ctypes.addressof(ok), d) == -1 and b"needs depths" in lib.accv_last_error()
        assert call(d, d, d, None, 0, 2, 4, ctypes.addressof(ok), None) == -1
        assert call(ctypes.c_void_p(66), d, d, None, 0, 2, 4, ctypes.addressof(ok), d) == -1 and b"aligned" in lib.accv_last_error()
        assert call(None, None, None, None, 0, 0, 4, ctypes.addressof(ok), None) == 0
        assert call(None, None, None, None, 0, 2, 0, ctypes.addressof(ok), None) == 0


# ------------------------------------------------------------------------------------------------- select_visible_bboxes
def test_select_equals_mask_then_bool_indexing_and_feeds_the_centre_front_end():
    frames = vc.sweep_frames(6, count=5)
    boxes, depths, hw = vc.batch(frames, hostile_padding=False)
    centers = boxes.create_with_sample_sizes_like_self((boxes.tensor[..., :2] + boxes.tensor[..., 2:]) / 2)
    ids = boxes.create_with_sample_sizes_like_self(torch.arange(boxes.tensor.shape[1]).repeat(len(frames), 1))
    kw = dict(image_hw=hw, minimum_size=2)
    mask, b2, d2, c2, i2 = select_visible_bboxes(boxes, depths, centers, ids, **kw)
    want = op(boxes, depths, **kw)
    assert torch.equal(mask.tensor, want.tensor) and 0 < int(want.tensor.sum()) < sum(len(f[0]) for f in frames)
    for got, src in ((b2, boxes), (d2, depths), (c2, centers), (i2, ids)):
        ref = batched_bool_indexing(src, want)
        assert isinstance(got, RaggedBatch) and torch.equal(got.tensor, ref.tensor) and torch.equal(got.sample_sizes, ref.sample_sizes)
    assert torch.equal(b2.sample_sizes, want.tensor.sum(1))
    for b in range(len(frames)):
        assert i2.tensor[b, :int(i2.sample_sizes[b])].tolist() == torch.nonzero(want.tensor[b]).ravel().tolist()
    c, r = get_centers_and_radii(c2, b2, 4.0)                       # as they are: same layout, same sizes
    assert c.tensor.shape == c2.tensor.shape and r.tensor.shape == d2.tensor.shape and c.sample_sizes is c2.sample_sizes
    only_size = select_visible_bboxes(boxes, None, image_hw=hw, check_occlusion=False, minimum_size=2)
    assert only_size[2] is None and torch.equal(only_size[0].tensor, op(boxes, image_hw=hw, check_occlusion=False, minimum_size=2).tensor)


# --------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_name_the_operator():
    boxes, depths, hw = vc.batch(REF)
    sizes = boxes.sample_sizes
    rb = lambda t, s=sizes: RaggedBatch(t, sample_sizes=s)   # noqa: E731
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="visible_bbox_mask: bboxes must be float32"):
            op(rb(boxes.tensor.to(dtype)), depths, image_hw=hw)
        with pytest.raises(TypeError, match="visible_bbox_mask: depths must be float32"):
            op(boxes, depths.tensor.to(dtype), image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: bboxes must be float32"):
        op(rb(boxes.tensor.to(torch.int32)), depths, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: bboxes must be float32 \\[B, G_max, 4\\]"):
        op(rb(boxes.tensor[..., :3].contiguous()), depths, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: bboxes must be float32 \\[B, G_max, 4\\]"):
        op(rb(boxes.tensor[None], sizes[None]), depths, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: bboxes must be a RaggedBatch"):
        op(boxes.tensor, depths, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: check_occlusion needs depths"):
        op(boxes, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: at least one of check_occlusion and minimum_size"):
        op(boxes, depths, image_hw=hw, check_occlusion=False)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: depths must be float32 \\[1, 11\\]"):
        op(boxes, depths.tensor.repeat(2, 1), image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: an image_hw tensor must be int32 or int64 \\[1, 2\\]"):
        op(boxes, depths, image_hw=hw.repeat(2, 1))
    with pytest.raises(RuntimeError, match="visible_bbox_mask: an image_hw tensor must be int32 or int64 \\[1, 2\\]"):
        op(boxes, depths, image_hw=hw.to(torch.float32))
    with pytest.raises(RuntimeError, match="visible_bbox_mask: image_hw must be \\(H, W\\) Python ints"):
        op(boxes, depths, image_hw=(100.0, 200))
    with pytest.raises(RuntimeError, match="visible_bbox_mask: bboxes must be contiguous"):
        op(rb(boxes.tensor.repeat(1, 1, 2)[..., ::2]), depths, image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: minimum_size must be a Python number"):
        op(boxes, depths, image_hw=hw, minimum_size="2")


def test_empty_batches_and_empty_frames():
    for B, G in ((0, 5), (3, 0)):
        boxes = RaggedBatch(torch.zeros((B, G, 4)), sample_sizes=torch.zeros((B,), dtype=torch.int64))
        got = op(boxes, torch.zeros((B, G)), image_hw=(8, 8))
        assert got.tensor.shape == (B, G) and got.tensor.dtype == torch.bool
    assert not bool(vc.run(op, [([], [], (8, 8)), ([], [], (8, 8))], G=7).any())
