"""pillar_features and voxel_mean on CPU tensors: the library's host entries (accv_pillar_features_cpu, accv_voxel_mean_cpu)
against the numpy float32 restatement of the definition in pillar_features_cases.py, bit for bit — every point count, T, D,
flag subset and num_features at the voxel counts around the device's workgroup, both input forms and a Voxels tuple, hostile
padding, NaN payloads, the real output of voxelize_points, a misaligned view, guard bands through the C entries alone, errors
and empty inputs; and torch's composition of mmdet3d's forward, which may differ in the cluster channels only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pillar_features_cases as cases  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402

DEV = "cpu"
MAX_GROUP, LDS_FLOATS = 64, 8192      # the device's work partition, as literals


def test_surface_and_host_entry_names():
    from accvlab import point_cloud

    assert set(point_cloud.__all__) >= {"pillar_features", "voxel_mean", "scatter_to_bev", "MAX_CHANNELS"}
    assert nat.HOST_ENTRY_NAMES["accv_pillar_features"] == "accv_pillar_features_cpu"
    assert nat.HOST_ENTRY_NAMES["accv_voxel_mean"] == "accv_voxel_mean_cpu"
    assert (nat.PF_CLUSTER, nat.PF_CENTER, nat.PF_DISTANCE) == (1, 2, 4)


@pytest.mark.parametrize("T", [1, 2, 20, 128])
def test_every_width_count_and_flag_subset_against_the_definition(T):
    cases.check_shapes(DEV, T, MAX_GROUP, LDS_FLOATS)


def test_both_forms_and_a_voxels_tuple():
    cases.check_forms(DEV)


def test_on_the_output_of_voxelize_points():
    cases.check_after_voxelize(DEV)


def test_voxels_off_a_16_byte_boundary():
    cases.check_misaligned(DEV)


def test_guard_bands_and_complete_write_through_the_c_entries_alone():
    cases.check_guard_bands(DEV, MAX_GROUP, LDS_FLOATS)


def test_workgroup_ranges_off_a_16_byte_boundary_under_aligned_tensors():
    cases.check_dispatch(DEV, MAX_GROUP, LDS_FLOATS)


def test_against_the_torch_composition_of_mmdet3d():
    cases.check_against_torch(DEV)


def test_every_documented_error():
    cases.check_errors(DEV, other_dev="meta")


def test_no_voxels():
    cases.check_empty(DEV)


def test_c_entries_refuse_bad_arguments():
    lib = nat.ctypes_lib()
    p = nat.PillarFeaturesParams()
    p.voxel_size[:], p.range_min[:], p.coor_width = (0.5, 0.5, 4.0), (-4.0, -4.0, -2.0), 4
    import ctypes

    adr = ctypes.addressof(p)
    assert lib.accv_pillar_features_cpu(None, 1, 4, 4, None) == -1 and b"null params" in lib.accv_last_error()
    assert lib.accv_pillar_features_cpu(adr, 0, 4, 4, None) == 0
    assert lib.accv_pillar_features_cpu(adr, 1, 4, 4, None) == -1 and b"null pointer" in lib.accv_last_error()
    assert lib.accv_pillar_features_cpu(adr, 1, 129, 4, None) == -1 and b"T" in lib.accv_last_error()
    assert lib.accv_pillar_features_cpu(adr, 1, 4, 17, None) == -1 and b"D" in lib.accv_last_error()
    p.coor_width = 5
    assert lib.accv_pillar_features_cpu(adr, 0, 4, 4, None) == -1 and b"coor_width" in lib.accv_last_error()
    assert lib.accv_voxel_mean_cpu(None, None, 0, 4, 4, 4, None) == 0
    assert lib.accv_voxel_mean_cpu(None, None, 0, 4, 4, 5, None) == -1 and b"num_features" in lib.accv_last_error()
    assert lib.accv_voxel_mean_cpu(None, None, 2, 4, 4, 4, None) == -1 and b"null pointer" in lib.accv_last_error()
