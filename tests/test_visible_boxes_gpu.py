"""visible_bbox_mask / select_visible_bboxes on the GPU: the kernel against the reference's hand-written vector, the
hand-worked geometry edges, the numpy canvas painter of visible_boxes_cases.py and the host entry, at the wave and bit-word
boundaries of its work partition, with guard bands, a non-default stream, a storage offset, no host synchronisation, and end
to end into the heat-map draw.  All comparisons are torch.equal on booleans."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import visible_boxes_cases as vc  # noqa: E402

from accvlab.batching_helpers import RaggedBatch, batched_bool_indexing  # noqa: E402
from accvlab.draw_heatmap import (draw_heatmap_batched, get_centers_and_radii, select_visible_bboxes,  # noqa: E402
                                  visible_bbox_mask)
from accvlab.draw_heatmap.visible_boxes import MAX_BOXES  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = visible_bbox_mask
REF = [(vc.REF_BOXES, vc.REF_DEPTHS, vc.REF_HW)]
MODES = {"occlusion": (dict(), vc.REF_OCCLUSION), "size": (dict(check_occlusion=False, minimum_size=2), vc.REF_SIZE),
         "both": (dict(minimum_size=2), [a & b for a, b in zip(vc.REF_OCCLUSION, vc.REF_SIZE)])}


def _bool(rows):
    return torch.tensor(rows, dtype=torch.bool).reshape(len(rows) if isinstance(rows[0], list) else 1, -1)


@pytest.mark.parametrize("hw_as", ["tuple", "tensor", "int64"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_reference_vector(mode, hw_as):
    """visible_bbox_selector_test.py:62-80 and :169-184 of the reference"""
    kw, want = MODES[mode]
    assert torch.equal(vc.run(op, REF, DEV, hw_as=hw_as, **kw), _bool(want))


def test_one_more_slot_than_max_boxes_raises_before_any_launch():
    boxes, depths, hw = vc.batch([([[1, 1, 2, 2]], [1], (8, 8))], G=MAX_BOXES + 1, device=DEV)
    with pytest.raises(RuntimeError, match="visible_bbox_mask.*MAX_BOXES"):
        op(boxes, depths, image_hw=hw)


@pytest.mark.parametrize("kw", [dict(), dict(shrink_to_int=True), dict(minimum_size=3)], ids=["expand", "shrink", "with_size"])
def test_frame_sizes_at_wave_and_word_boundaries_with_hostile_padding(kw):
    frames = vc.partition_frames()
    assert [len(f[0]) for f in frames] == list(vc.PARTITION_SIZES) and MAX_BOXES == 256
    assert torch.equal(vc.run(op, frames, DEV, **kw), vc.oracle(frames, 256, **kw))


@pytest.mark.parametrize("shrink", [False, True])
def test_geometry_edges_by_hand(shrink):
    names = sorted(vc.GEOMETRY)
    got = vc.run(op, vc.geometry_frames(names), DEV, shrink_to_int=shrink)
    want = vc.geometry_expected(shrink, 5, names)
    for b, k in enumerate(names):
        assert torch.equal(got[b], want[b]), f"{k}: got {got[b].tolist()}, expected {want[b].tolist()}"


def test_two_frames_with_different_image_hw_rows():
    assert torch.equal(vc.run(op, vc.TWO_SIZES, DEV), _bool(vc.TWO_SIZES_EXPECTED))


@pytest.mark.parametrize("shrink", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_sweep_against_the_canvas_oracle(seed, shrink):
    frames = vc.sweep_frames(seed)
    G = max(len(f[0]) for f in frames)
    want = vc.oracle(frames, G, shrink_to_int=shrink)
    real, seen = sum(len(f[0]) for f in frames), int(want.sum())
    assert seen >= real / 5 and real - seen >= real / 5, "the sweep shows too little of one outcome"
    assert torch.equal(vc.run(op, frames, DEV, shrink_to_int=shrink), want)
    kw = dict(shrink_to_int=shrink, minimum_size=2.5)
    assert torch.equal(vc.run(op, frames, DEV, **kw), vc.oracle(frames, G, **kw))


def test_full_hd_frame_with_128_boxes_against_the_canvas():
    frames = [vc.random_frame(np.random.default_rng(5), 128, (1080, 1920))]
    assert torch.equal(vc.run(op, frames, DEV, hw_as="tuple"), vc.oracle(frames, 128))


def test_image_of_2_to_the_24_squared():
    assert torch.equal(vc.run(op, [vc.HUGE], DEV), _bool(vc.HUGE_EXPECTED))
    b, d, hw = vc.HUGE
    assert torch.equal(vc.run(op, [(b[:5], d[:5], hw)], DEV, hw_as="tuple"), _bool(vc.HUGE_WITHOUT_LAST_EXPECTED))
    assert torch.equal(vc.run(op, [(b, d, (1 << 40, 1 << 40))], DEV, hw_as="int64"), _bool(vc.HUGE_EXPECTED))
    assert not bool(vc.run(op, [(b, d, (-3, 50))], DEV).any())


def test_a_frame_of_256_boxes_without_two_equal_edges():
    """the largest cell grid the kernel can meet: 512 distinct edges per axis"""
    rng = np.random.default_rng(9)
    xs, ys = rng.permutation(600)[:512], rng.permutation(600)[:512]
    boxes = np.stack([xs[:256], ys[:256], xs[256:], ys[256:]], 1).astype(np.float32)
    frames = [(boxes, rng.permutation(256).astype(np.float32), (600, 600))]
    want = vc.oracle(frames, 256)
    assert 25 < int(want.sum()) < 231
    assert torch.equal(vc.run(op, frames, DEV), want)


# ------------------------------------------------------------------------------------------------------------ paths agree
def test_host_and_device_agree_on_every_case():
    for name, frames, kws in vc.all_case_sets():
        for kw in kws:
            assert torch.equal(vc.run(op, frames, DEV, **kw), vc.run(op, frames, "cpu", **kw)), (name, kw)


def test_ctypes_binding_alone_between_guard_bands():
    from accvlab import _amd_native as nat

    frames = vc.partition_frames(seed=8)[3:8] + vc.sweep_frames(4, count=3)
    boxes, depths, hw = vc.batch(frames, G=131, device=DEV, size_dtype=torch.int32)
    B, G, pad = len(frames), 131, 512
    buf = torch.full((pad + B * G + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
    p = nat.VisibleBoxesParams(2.0, 0, 0, 1, 1, 0)
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    status = nat.ctypes_lib().accv_visible_boxes(boxes.tensor.data_ptr(), depths.tensor.data_ptr(), boxes.sample_sizes.data_ptr(),
                                                 hw.data_ptr(), 0, B, G, ctypes.addressof(p), buf[pad:].data_ptr(), stream)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + B * G:] == 0xA5).all()), "wrote outside its buffer"
    # every byte inside was written: the sentinel is gone, padding slots included
    assert torch.equal(buf[pad: pad + B * G].view(B, G).cpu(), vc.oracle(frames, G, minimum_size=2).to(torch.uint8))


def test_non_default_stream_storage_offset_and_no_host_synchronisation():
    frames = vc.sweep_frames(11, count=8)
    boxes, depths, hw = vc.batch(frames, device=DEV)
    B, G = boxes.tensor.shape[:2]
    want = vc.oracle(frames, G)
    # a view one float (boxes, depths) and one int (image_hw) into its storage: 4-byte aligned only
    shifted = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)   # noqa: E731
    b2 = RaggedBatch(shifted(boxes.tensor), sample_sizes=boxes.sample_sizes)
    d2, hw2 = shifted(depths.tensor), shifted(hw)
    assert b2.tensor.storage_offset() == 1 and d2.storage_offset() == 1 and hw2.storage_offset() == 1
    op(boxes, depths, image_hw=hw)                                  # warm-up: library load, allocator
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            on_stream = op(boxes, depths, image_hw=hw)
        offset = op(b2, d2, image_hw=hw2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(on_stream.tensor.cpu(), want) and torch.equal(offset.tensor.cpu(), want)
    again = op(boxes, depths, image_hw=hw)
    assert torch.equal(again.tensor, on_stream.tensor)


# ------------------------------------------------------------------------------------------------- select_visible_bboxes
def test_select_equals_mask_then_bool_indexing_and_feeds_the_heat_map_draw():
    frames = vc.sweep_frames(6, count=5)
    boxes, depths, hw = vc.batch(frames, hostile_padding=False, device=DEV)
    centers = boxes.create_with_sample_sizes_like_self((boxes.tensor[..., :2] + boxes.tensor[..., 2:]) / 2)
    kw = dict(image_hw=hw, minimum_size=2)
    mask, b2, d2, c2 = select_visible_bboxes(boxes, depths, centers, **kw)
    want = op(boxes, depths, **kw)
    assert torch.equal(mask.tensor, want.tensor)
    assert torch.equal(mask.tensor.cpu(), vc.oracle(frames, boxes.tensor.shape[1], minimum_size=2))
    for got, src in ((b2, boxes), (d2, depths), (c2, centers)):
        ref = batched_bool_indexing(src, want)
        assert got.tensor.is_cuda and torch.equal(got.tensor, ref.tensor) and torch.equal(got.sample_sizes, ref.sample_sizes)
    c, r = get_centers_and_radii(c2, b2, 1.0)                       # as they are: same layout, same sizes
    assert c.sample_sizes is c2.sample_sizes
    hm = torch.full((len(frames), 64, 96), float("nan"), device=DEV)
    draw_heatmap_batched(hm, c, r, clear=True)
    assert bool(torch.isfinite(hm).all()) and float(hm.max()) == 1.0


def test_wrong_devices_and_dtypes_are_refused():
    boxes, depths, hw = vc.batch(REF, device=DEV)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: image_hw must be on the boxes' device"):
        op(boxes, depths, image_hw=hw.cpu())
    with pytest.raises(RuntimeError, match="visible_bbox_mask: depths must be on the boxes' device"):
        op(boxes, depths.tensor.cpu(), image_hw=hw)
    with pytest.raises(RuntimeError, match="visible_bbox_mask: sample_sizes must be on the boxes' device"):
        op(RaggedBatch(boxes.tensor, sample_sizes=boxes.sample_sizes.cpu()), depths, image_hw=hw)
    with pytest.raises(TypeError, match="visible_bbox_mask: bboxes must be float32"):
        op(RaggedBatch(boxes.tensor.half(), sample_sizes=boxes.sample_sizes), depths, image_hw=hw)
