"""voxelize_points on CPU tensors: the library's sequential host entry (accv_voxelize_cpu) against the numpy float32
restatement of the loop in voxelize_cases.py, bit for bit on all five outputs — random configurations, the sizes of the
device's work partition, truncation by max_points and max_voxels (mmcv's `continue` rule), table sizes, hand-placed points at
every edge of the definition, augmentation rows, concatenate_voxels, guard bands through the C entry alone, errors and empty
inputs; and the cases that enter the launch regimes of the device (many chunks, large index lists, max_voxels and
max_points at their crossings, wide rows, a grid of 2^30 cells, 65535 frames), which pin the host entry at the same inputs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import voxelize_cases as cases  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402

DEV = "cpu"


def test_limits_are_exported_and_the_host_entry_is_named():
    from accvlab import point_cloud

    assert (point_cloud.MIN_D, point_cloud.MAX_D, point_cloud.MAX_POINTS, point_cloud.MAX_VOXELS) == (3, 16, 128, 2 ** 20)
    assert nat.HOST_ENTRY_NAMES["accv_voxelize"] == "accv_voxelize_cpu"
    assert set(point_cloud.__all__) >= {"voxelize_points", "Voxels", "concatenate_voxels"}


def test_workspace_size_rule():
    """keys, first indices and numbers of the table (the power of two that is at least 2 P, or the one given), the slot of
    every point, the index lists and a count per chunk of 4096 points, each rounded up to 16 bytes; 0 for sizes the call refuses"""
    size = nat.lib().accv_voxelize_workspace_bytes
    up = lambda n: -(-n // 16) * 16                                                      # noqa: E731
    assert size(3, 1000, 50, 7, 0) == up(3 * 2048 * 8) + up(3 * 2048 * 4) + up(3 * 1000 * 4) + up(3 * 50 * 7 * 4) + up(3 * 1 * 4)
    assert size(3, 4097, 50, 7, 0) - size(3, 4096, 50, 7, 8192 * 2) == up(3 * 4097 * 4) - up(3 * 4096 * 4) + up(3 * 2 * 4) - up(3 * 1 * 4)
    assert size(3, 1024, 50, 7, 0) == size(3, 1000, 50, 7, 0) + up(3 * 1024 * 4) - up(3 * 1000 * 4)
    assert size(3, 1025, 50, 7, 0) == size(3, 1025, 50, 7, 4096) > size(3, 1025, 50, 7, 2048) > 0
    assert size(1, 0, 1, 1, 0) == 16 + 16 + 0 + 16 + 16
    for bad in ((3, 1024, 50, 7, 1024), (3, 1000, 50, 7, 1500), (3, 1000, 0, 7, 0), (3, 1000, 50, 129, 0), (3, 1000, 2 ** 20 + 1, 7, 0),
                (-1, 1000, 50, 7, 0), (65536, 10, 50, 7, 0), (1, 2 ** 31 - 1, 50, 7, 0), (1, 10, 50, 7, 2 ** 32)):
        assert size(*bad) == 0, bad


@pytest.mark.parametrize("B,D,size_dtype,grid,T,V,below", cases.CONFIGS)
def test_random_configurations_against_the_definition(B, D, size_dtype, grid, T, V, below):
    cases.check_config(DEV, B, D, size_dtype, grid, T, V, below)


def test_sizes_around_the_device_work_partition():
    cases.check_partition(DEV, 256, 4096)


def test_truncation_by_max_points_and_max_voxels_follows_the_continue_rule():
    cases.check_truncation(DEV)


def test_table_sizes_two_calls_and_untouched_inputs():
    cases.check_table_pressure(DEV)


def test_hand_placed_points_at_every_edge_of_the_definition():
    cases.check_hand_placed(DEV)


def test_augmentation_rows_equal_augmented_points():
    cases.check_augmentation(DEV)


def test_concatenate_voxels_against_slice_and_cat():
    cases.check_concatenate(DEV)


def test_points_off_a_16_byte_boundary():
    cases.misaligned_points(DEV)


def test_no_frames_no_points_and_sizes_of_zero():
    cases.check_empty(DEV)


def test_guard_bands_and_complete_write_through_the_c_entry_alone():
    cases.check_guard_bands(DEV)


def test_every_documented_error():
    cases.check_errors(DEV, other_dev="meta")


# the regimes of the device's work partition, with its constants as literals: 1024 lanes x 4 points a chunk, 65536 list
# words a filling workgroup, at most 64 of those a frame
def test_prefix_over_130_chunks():
    cases.check_many_chunks(DEV, 130, 1024, 4)


def test_prefix_over_1025_chunks():
    cases.check_many_chunks(DEV, 1025, 1024, 4)


def test_lists_of_more_than_one_filling_workgroup():
    cases.check_list_fill(DEV, 65536, 64)


def test_max_voxels_crossed_inside_a_lane_between_waves_and_between_chunks():
    cases.check_budget_crossings(DEV, 4, 4096)


@pytest.mark.parametrize("T", [1, 2, 128])
def test_voxels_of_max_points_minus_one_to_plus_one_points(T):
    cases.check_point_budget(DEV, T)


@pytest.mark.parametrize("D", [6, 8, 12, 15, 16])
def test_row_widths_with_and_without_rows_and_off_a_16_byte_boundary(D):
    cases.check_row_widths(DEV, D)


def test_grid_of_two_to_the_thirty_cells():
    cases.check_large_keys(DEV)


def test_most_frames_a_call_takes():
    cases.check_most_frames(DEV)
