"""camera_augment_boxes on the GPU: the kernel against the two numpy oracles of camera_boxes_cases.py and against the host
entry, at the edges of its work partition (wave, 256 slots, more than one pass over the matrix elements), with guard bands,
on a side stream, on views with a storage offset, and without a host synchronisation."""
import numpy as np
import pytest
import torch

import camera_boxes_cases as cases
import test_camera_boxes_cpu as cpu
from camera_boxes_cases import built, check_case, run

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_kernel_equals_the_float32_oracle_the_host_entry_and_lies_within_the_bar_of_the_float64_one(name):
    case, a, got = check_case(name, DEV)
    cases.assert_same(got, run(case, "cpu"), f"{name}: device against host entry:")


def test_identity_cross_check_with_the_existing_operators():
    cpu.check_identity_cross_check(DEV)


@pytest.mark.parametrize("sizes_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("categories_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("valid_dtype,hw_dtype", [(torch.bool, torch.int32), (torch.uint8, torch.int64)])
def test_count_category_valid_and_image_hw_dtypes(valid_dtype, hw_dtype, categories_dtype, sizes_dtype):
    case, a = built("dtypes")
    typed = cases.Case(case.boxes, case.sizes, case.transforms, hw=case.hw, centers=case.centers, depths=case.depths,
                       categories=case.categories, valid=case.valid, mats=case.mats, sizes_dtype=sizes_dtype, **case.kw)
    got = run(typed, DEV, categories_dtype=categories_dtype, valid_dtype=valid_dtype, hw_dtype=hw_dtype)
    assert got["categories"].dtype == categories_dtype
    cases.assert_same(got, a)


@pytest.mark.parametrize("name", ["dtypes", "partition-G65", "matrices-shapes", "matrices-big"])
def test_storage_offset_of_one_element_and_optional_fields_as_ragged_batches(name):
    """the views are 4-byte aligned only: nothing may move as a 16-byte vector"""
    case, a = built(name)
    cases.assert_same(run(case, DEV, ragged_fields=True, offset=True), a, name)


def test_side_stream():
    case, a = built("sweep-1")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = run(case, DEV)
    cases.assert_same(got, a)


def test_no_host_synchronisation_and_two_runs_are_bitwise_identical():
    from accvlab.draw_heatmap import camera_augment_boxes

    case, a = built("sweep-1")
    boxes, t, kw = cases.to_torch(case, DEV)
    first = camera_augment_boxes(boxes, t, **kw)                 # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = camera_augment_boxes(boxes, t, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    got = cases.flatten(out, case)
    cases.assert_same(got, a)
    cases.assert_same(got, cases.flatten(first, case))


@pytest.mark.parametrize("trampoline", [False, True])
def test_every_output_lies_between_guard_bands_through_the_c_entry_alone(trampoline):
    for name in ("partition-G65", "partition-G256", "matrices-big", "dtypes"):
        cases.check_guard_bands(name, DEV, trampoline=trampoline)


def test_the_c_entry_checks_its_arguments_before_any_launch():
    cpu.check_c_entry_refusals(DEV)


def test_wrong_dtypes_shapes_and_layouts_are_refused_before_any_launch():
    cpu.check_refusals(DEV)


def test_wrong_devices_are_refused_before_any_launch():
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import camera_augment_boxes as op

    case, _ = built("dtypes")
    boxes, t, kw = cases.to_torch(case, DEV)
    mats = torch.zeros((case.boxes.shape[0], 4, 4))
    for key in ("centers", "depths", "categories", "valid", "image_hw"):
        with pytest.raises(RuntimeError, match="device"):
            op(boxes, t, **{**kw, key: kw[key].cpu()})
    for call in (lambda: op(boxes, t.cpu(), **kw), lambda: op(boxes, t, **{**kw, "projection_matrices": [mats]}),
                 lambda: op(RaggedBatch(boxes.tensor, sample_sizes=boxes.sample_sizes.cpu()), t, **kw)):
        with pytest.raises(RuntimeError, match="device"):
            call()
