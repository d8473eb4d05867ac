"""scatter_to_bev on CPU tensors: the library's host entries (accv_bev_scatter_cpu, accv_bev_scatter_bwd_cpu) against the
sequential numpy loop of bev_scatter_cases.py, bit for bit on canvas, index and grad_features in float32, float16 and
bfloat16 — the shapes around the device's tile and channel chunk, row counts around its workgroup, occupancy patterns,
duplicates, rows outside the map, the padded form fed by voxelize_points, misaligned views, guard bands through the C entries
alone, empty inputs, errors, and mmdet3d's composition in torch with its autograd backward."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bev_scatter_cases as cases  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402

DEV = "cpu"
THREADS, TILE, CHUNK = 256, 64, 64      # the device's work partition, as literals


def test_surface_and_host_entry_names():
    from accvlab import point_cloud

    assert point_cloud.MAX_CHANNELS == nat.BS_MAX_C == 1024
    assert nat.HOST_ENTRY_NAMES["accv_bev_scatter"] == "accv_bev_scatter_cpu"
    assert nat.HOST_ENTRY_NAMES["accv_bev_scatter_bwd"] == "accv_bev_scatter_bwd_cpu"


@pytest.mark.parametrize("nx", [1, 3, 4, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=str)
def test_map_and_channel_shapes_against_the_definition(dtype, nx):
    cases.check_shapes(DEV, dtype, nx, CHUNK)


def test_row_counts_around_a_workgroup():
    cases.check_row_counts(DEV, THREADS)


def test_empty_frames_full_and_empty_tiles_and_corner_cells():
    cases.check_occupancy(DEV, TILE)


def test_duplicates_the_highest_row_wins():
    cases.check_duplicates(DEV, THREADS)


def test_rows_outside_are_unplaced_and_z_is_ignored():
    cases.check_outside(DEV)


def test_padded_form_on_the_coors_of_voxelize_points():
    cases.check_padded_form(DEV)


def test_views_off_a_16_byte_boundary():
    cases.check_misaligned(DEV)


def test_guard_bands_and_complete_write_through_the_c_entries_alone():
    cases.check_guard_bands(DEV)


def test_against_the_torch_composition_of_mmdet3d_and_its_autograd():
    cases.check_against_torch(DEV)


def test_no_frames_no_rows_no_cells():
    cases.check_empty(DEV)


def test_every_documented_error():
    cases.check_errors(DEV, other_dev="meta")


def test_c_entries_refuse_bad_arguments():
    lib = nat.ctypes_lib()
    d = 64
    ok = (d, d, 4, 0, 2, 4, 3, 5, 4, 4, d, d)
    bad = {"negative": (d, d, -1, 0, 2, 4, 3, 5, 4, 4, d, d), "channels": (d, d, 4, 0, 2, 1025, 3, 5, 4, 4, d, d),
           "elem_size": (d, d, 4, 0, 2, 4, 3, 5, 4, 8, d, d), "coor_width": (d, d, 4, 0, 2, 4, 3, 5, 2, 4, d, d),
           "rows == B * V": (d, d, 4, 3, 2, 4, 3, 5, 3, 4, d, d), "2^31": (d, d, 4, 0, 2, 4, 2 ** 15, 2 ** 15, 4, 4, d, d),
           "null pointer": (d, d, 4, 0, 2, 4, 3, 5, 4, 4, None, d), "aligned": (d, d, 4, 0, 2, 4, 3, 5, 4, 4, d, d + 2)}
    for text, args in bad.items():
        assert lib.accv_bev_scatter_cpu(*args) == -1 and text.encode() in lib.accv_last_error(), (text, lib.accv_last_error())
    assert lib.accv_bev_scatter_cpu(*ok[:4], 0, *ok[5:10], None, None) == 0        # no frames
    assert lib.accv_bev_scatter_bwd_cpu(None, None, None, 0, 0, 2, 4, 3, 5, 4, 4, None) == 0     # no rows
    assert lib.accv_bev_scatter_bwd_cpu(None, None, None, 4, 0, 2, 4, 3, 5, 4, 4, None) == -1
