"""lidar_depth_targets on CPU tensors: the library's serial host entry (accv_depth_targets_cpu) against the float32
definition and the float64 evaluation of depth_targets_cases.py — ragged point counts, every camera / channel / row count,
both size dtypes, hostile filler, extents and strides that do not divide, every band split, the automatic two-band split,
hand-placed points at every edge of the definition, bins, image_transforms against camera_augment_boxes' matrices, guard
bands through the C entry alone, reproducibility, errors, empty inputs and the largest batch (65535 frames)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_targets_cases as cases  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402

DEV = "cpu"


def test_band_limit_is_exported_and_fits_the_default_lds():
    from accvlab.draw_heatmap import depth_targets

    assert nat.DT_BAND_CELLS == depth_targets.DT_BAND_CELLS == 8192
    assert nat.DT_BAND_CELLS * 4 < 64 * 1024 and nat.DT_BAND_CELLS % 64 == 0
    assert nat.HOST_ENTRY_NAMES["accv_depth_targets"] == "accv_depth_targets_cpu"


@pytest.mark.parametrize("B,C,D,R,size_dtype,image_hw,downsample", cases.CONFIGS)
def test_against_the_float32_definition_and_float64(B, C, D, R, size_dtype, image_hw, downsample):
    cases.check_config(DEV, B, C, D, R, size_dtype, image_hw, downsample)


def test_points_off_a_16_byte_boundary():
    cases.check_misaligned_points(DEV)


def test_every_band_split_of_a_tiny_map_gives_the_same_bits():
    cases.check_band_splits(DEV)


def test_maps_around_the_band_limit_and_points_at_the_band_edges():
    cases.check_multi_band(DEV, nat.DT_BAND_CELLS)


def test_hand_placed_points_at_every_edge_of_the_definition():
    cases.check_hand_placed(DEV)


def test_image_transforms_equal_the_matrices_of_camera_augment_boxes():
    cases.check_image_transforms(DEV)


def test_two_calls_give_identical_bits_and_no_input_is_modified():
    cases.check_reproducible_and_inputs_untouched(DEV)


def test_no_frames_no_points_and_clamped_sizes():
    cases.check_empty(DEV)


def test_guard_bands_and_complete_write_through_the_c_entry_alone():
    cases.check_guard_bands(DEV, nat.DT_BAND_CELLS)


def test_most_frames_a_call_takes():
    cases.check_most_frames(DEV)


def test_every_documented_error():
    cases.check_errors(DEV, nat.DT_BAND_CELLS, other_dev="meta")
