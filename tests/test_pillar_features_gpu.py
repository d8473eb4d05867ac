"""pillar_features and voxel_mean on the GPU: the kernel against the numpy float32 restatement of the definition in
pillar_features_cases.py and against the host entry on the same inputs, bit for bit — the cases of
test_pillar_features_cpu.py on the device, with the voxel counts around the kernel's voxels-per-workgroup G derived from
the constants read from the source (G is smallest, 4, at T = 128, D = 16), a voxels view off a 16-byte boundary (4-byte
loads), outputs off a 16-byte boundary through the C entries (4-byte stores), a non-default stream and a hipGraph capture
and replay."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pillar_features_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "pillar_features.hip")).read()
THREADS, MAX_GROUP, LDS_FLOATS = (int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1))
                                  for name in ("kThreads", "kMaxGroup", "kLdsFloats"))
assert (THREADS, MAX_GROUP, LDS_FLOATS) == (256, 64, 8192)
assert "const long long fit = kLdsFloats / (T * D);" in _SRC and "fit > kMaxGroup ? kMaxGroup : fit" in _SRC     # group_of
assert cases.group_of(128, 16, MAX_GROUP, LDS_FLOATS) == 4 and cases.group_of(20, 4, MAX_GROUP, LDS_FLOATS) == 64
assert cases.group_of(128, 3, MAX_GROUP, LDS_FLOATS) == 21


@pytest.mark.parametrize("T", [1, 2, 20, 128])
def test_every_width_count_and_flag_subset_against_the_definition(T):
    cases.check_shapes(DEV, T, MAX_GROUP, LDS_FLOATS)


def test_gpu_against_cpu_tensors():
    for T, D in ((20, 4), (128, 16), (5, 7)):
        G = cases.group_of(T, D, MAX_GROUP, LDS_FLOATS)
        vox, num, coors = cases.make_voxels(40 + D, 2 * G + 1, T, D)
        on_dev, on_host = cases.to_dev(DEV, vox, num, coors), cases.to_dev("cpu", vox, num, coors)
        kw = dict(with_distance=True, **cases.GRID)
        cases.assert_bits(cases.pillar_features(*on_dev, **kw), cases.pillar_features(*on_host, **kw), f"T {T}, D {D}")
        clean = cases.mean_input(vox, num)
        cases.assert_bits(cases.voxel_mean(cases.to_dev(DEV, clean)[0], on_dev[1]), cases.voxel_mean(torch.from_numpy(clean), on_host[1]),
                          f"mean, T {T}, D {D}")


def test_both_forms_and_a_voxels_tuple():
    cases.check_forms(DEV)


def test_on_the_output_of_voxelize_points():
    cases.check_after_voxelize(DEV)


def test_voxels_off_a_16_byte_boundary():
    cases.check_misaligned(DEV)


def test_guard_bands_and_complete_write_through_the_c_entries_alone():
    cases.check_guard_bands(DEV, MAX_GROUP, LDS_FLOATS)


def test_workgroup_ranges_off_a_16_byte_boundary_under_aligned_tensors():
    """the three mixed instantiations of the decoration and the 4-byte voxel mean, entered by divisibility alone"""
    assert "const bool vec_in = (addr(a.voxels) & 15u) == 0 && ((long long)a.G * a.T * a.D) % 4 == 0;" in _SRC
    assert "const bool vec_out = (addr(a.out) & 15u) == 0 && ((long long)a.G * a.T * a.F) % 4 == 0;" in _SRC
    cases.check_dispatch(DEV, MAX_GROUP, LDS_FLOATS)


def test_against_the_torch_composition_of_mmdet3d():
    cases.check_against_torch(DEV)


def test_every_documented_error_is_raised_before_a_launch():
    cases.check_errors(DEV, other_dev="cpu")


def test_no_voxels():
    cases.check_empty(DEV)


def _stream_case():
    vox, num, coors = cases.make_voxels(61, 300, 20, 4)
    return vox, num, coors, dict(with_distance=True, **cases.GRID)


def test_runs_on_the_current_stream():
    """the launch goes to torch's current stream: on a side stream, after a copy that stream alone waits for"""
    vox, num, coors, kw = _stream_case()
    want = cases.definition(vox, num, coors, **kw)
    _, tn, tc = cases.to_dev(DEV, vox, num, coors)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tv = torch.zeros(vox.shape, device=DEV)
        tv.copy_(torch.from_numpy(vox).to(DEV))
        got = cases.pillar_features(tv, tn, tc, **kw)
    side.synchronize()
    cases.assert_bits(got, want, "side stream")


def test_graph_capture_and_replay_give_the_bits_of_the_eager_call():
    vox, num, coors, kw = _stream_case()
    tv, tn, tc = cases.to_dev(DEV, vox, num, coors)
    eager, eager_mean = cases.pillar_features(tv, tn, tc, **kw), cases.voxel_mean(tv, tn, num_features=3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, captured_mean = cases.pillar_features(tv, tn, tc, **kw), cases.voxel_mean(tv, tn, num_features=3)
    other, other_num, _ = cases.make_voxels(62, 300, 20, 4)
    tv.copy_(torch.from_numpy(other))
    tn.copy_(torch.from_numpy(other_num))
    graph.replay()
    torch.cuda.synchronize()
    cases.assert_bits(captured, cases.definition(other, other_num, coors, **kw), "replay on new voxels")
    cases.assert_bits(captured_mean, cases.mean_definition(other, other_num, 3), "replay on new voxels, mean")
    tv.copy_(torch.from_numpy(vox))
    tn.copy_(torch.from_numpy(num))
    graph.replay()
    torch.cuda.synchronize()
    cases.assert_bits(captured, eager, "replay")
    cases.assert_bits(captured_mean, eager_mean, "replay, mean")
