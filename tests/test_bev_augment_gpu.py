"""bev_augment_boxes on the GPU: the kernel against the two numpy oracles of bev_augment_cases.py and against the host
entry, at the edges of its work partition (wave, chunk of 256 slots, more than one pass over the matrices), with guard
bands, on a side stream, on views with a storage offset, and without a host synchronisation."""
import numpy as np
import pytest
import torch

import bev_augment_cases as cases
from bev_augment_cases import built, check_case, run

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_kernel_equals_the_float32_oracle_the_host_entry_and_lies_within_the_bar_of_the_float64_one(name):
    case, a, got = check_case(name, DEV)
    cases.assert_same(got, run(case, "cpu"), f"{name}: device against host entry:")


def test_reference_data_every_part_off_returns_the_inputs():
    case, a = built("reference")
    got = run(case, DEV)
    off = 3                                    # the frame with the identity row
    assert torch.equal(got["boxes"][off], torch.from_numpy(case.boxes[off]))
    for g, m in zip(got["pts"] + got["frs"], case.pts + case.frs):
        assert torch.equal(g[off], torch.from_numpy(m[off]))


@pytest.mark.parametrize("sizes_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("labels_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("valid_dtype", [torch.bool, torch.uint8])
def test_valid_label_and_count_dtypes(valid_dtype, labels_dtype, sizes_dtype):
    case, a = built("dtypes")
    typed = cases.Case(case.boxes, case.sizes, case.rows, labels=case.labels, valid=case.valid, point_range=case.point_range,
                       sizes_dtype=sizes_dtype)
    got = run(typed, DEV, labels_dtype=labels_dtype, valid_dtype=valid_dtype)
    assert got["labels"].dtype == labels_dtype
    cases.assert_same(got, a)


def test_counts_are_clamped_to_the_slots():
    case, _ = built("dtypes")
    wild = cases.Case(case.boxes, [1000, -5, 41], case.rows, labels=case.labels, valid=case.valid, point_range=case.point_range)
    cases.assert_same(run(wild, DEV), cases.oracle_a(wild))


@pytest.mark.parametrize("name", ["matrices-full", "sizes-D9-alternate", "sweep-2-output"])
def test_storage_offset_of_one_element_on_boxes_params_and_a_matrix_tensor(name):
    """the views are 4-byte aligned only: the matrix rows must not move as 16-byte vectors"""
    check_case(name, DEV, offset=True)


def test_side_stream():
    case, a = built("sweep-1-input")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = run(case, DEV)
    cases.assert_same(got, a)


def test_no_host_synchronisation_and_two_runs_are_bitwise_identical():
    from accvlab.draw_heatmap import bev_augment_boxes

    case, a = built("sweep-2-output")
    boxes, rows, kw = cases.to_torch(case, DEV)
    first = bev_augment_boxes(boxes, rows, **kw)                 # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bev_augment_boxes(boxes, rows, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    got = cases.flatten(out, case)
    cases.assert_same(got, a)
    cases.assert_same(got, cases.flatten(first, case))


@pytest.mark.parametrize("trampoline", [False, True])
def test_every_output_lies_between_guard_bands_through_the_c_entry_alone(trampoline):
    cases.check_guard_bands("matrices-full", DEV, labels=False, trampoline=trampoline)
    cases.check_guard_bands("sizes-D9-alternate", DEV, labels=True, trampoline=trampoline)


def test_center_point_targets_on_the_output_equals_center_point_targets_on_the_oracle():
    cases.check_end_to_end("sweep-1-input", DEV)


def test_wrong_devices_are_refused_before_any_launch():
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import bev_augment_boxes as op

    case, _ = built("dtypes")
    boxes, rows, kw = cases.to_torch(case, DEV)
    mats = torch.zeros((case.boxes.shape[0], 1, 4, 4))
    for call in (lambda: op(boxes, rows.cpu()), lambda: op(boxes, rows, labels=kw["labels"].tensor.cpu()),
                 lambda: op(boxes, rows, valid=kw["valid"].cpu()), lambda: op(boxes, rows, point_transforms=[mats]),
                 lambda: op(boxes, rows, frame_transforms=[mats]),
                 lambda: op(RaggedBatch(boxes.tensor, sample_sizes=boxes.sample_sizes.cpu()), rows)):
        with pytest.raises(RuntimeError, match="device"):
            call()


def test_parameter_helpers_on_the_device():
    from accvlab.draw_heatmap import bev_augmentation_params, sample_bev_augmentation

    angles = torch.tensor([0.0, 1.0, -2.0], device=DEV)
    rows = bev_augmentation_params(angles, 1.1, (1.0, 2.0, 3.0))
    assert rows.device.type == "cuda" and torch.equal(rows.cpu(), bev_augmentation_params(angles.cpu(), 1.1, (1.0, 2.0, 3.0)))
    g = torch.Generator(device=DEV).manual_seed(3)
    drawn = sample_bev_augmentation(64, (-0.4, 0.4), (0.9, 1.1), (1.0, 1.0, 0.5), generator=g)
    assert drawn.device.type == "cuda" and drawn.shape == (64, 7)
    again = sample_bev_augmentation(64, (-0.4, 0.4), (0.9, 1.1), (1.0, 1.0, 0.5), generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(drawn, again)
    assert float(drawn[:, 0].abs().max()) <= np.float32(0.4) and float(drawn[:, 3].min()) >= np.float32(0.9)
