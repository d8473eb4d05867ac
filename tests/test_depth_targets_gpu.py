"""lidar_depth_targets on the GPU: the kernel against the float32 definition and the float64 evaluation of
depth_targets_cases.py and against the host entry on the same inputs — the cases of test_depth_targets_cpu.py on the device,
the edges of the kernel's point loop (a workgroup's T lanes, one step of T * U points), GPU against CPU tensors bit for bit,
guard bands through the C entry alone for 16-byte and 4-byte stores, reproducibility, a non-default stream, errors before
any launch, empty inputs and B = 65535 frames, the limit of the grid's z extent."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_targets_cases as cases  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "depth_targets.hip")).read()
T, U = (int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1)) for name in ("kThreads", "kUnroll"))
assert (T, U) == (1024, 4)


@pytest.mark.parametrize("B,C,D,R,size_dtype,image_hw,downsample", cases.CONFIGS)
def test_against_the_float32_definition_and_float64(B, C, D, R, size_dtype, image_hw, downsample):
    cases.check_config(DEV, B, C, D, R, size_dtype, image_hw, downsample)


@pytest.mark.parametrize("D", [3, 4])
def test_point_loop_edges_and_gpu_against_cpu_tensors(D):
    """P at T -+ 1 (covered by the ragged sizes too) and at one and two steps of T * U points -+ 1, for the 16-byte and the
    4-byte loads; the same call on CPU tensors gives the same bits"""
    kw = dict(image_hw=(30, 44), downsample=2, depth_range=cases.DEPTH_RANGE, depth_bins=cases.BINS)
    for sizes in ((T * U - 1, T * U, T * U + 1), (2 * T * U + 1, T - 1, T)):
        case = cases.random_case(sizes[0], sizes, 2, D, 3, (30, 44))
        got, host = cases.run(case, DEV, **kw), cases.run(case, "cpu", **kw)
        cases.check_equal(got, cases.definition(case["points"], case["sizes"], case["projection"], **kw), f"{sizes}")
        assert torch.equal(got.depth.cpu(), host.depth) and torch.equal(got.bins.cpu(), host.bins)
        assert int((got.depth != 0).sum()) > 100


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
    """B = 65535 is gridDim.z of the launch; the same batch on CPU tensors gives the same bits"""
    cases.check_most_frames(DEV, other_dev="cpu")


def test_every_documented_error_is_raised_before_a_launch():
    cases.check_errors(DEV, nat.DT_BAND_CELLS, other_dev="cpu")


def test_runs_on_the_current_stream():
    """the launch goes to torch's current stream: on a side stream, after work that stream alone waits for"""
    case = cases.random_case(61, (1025, 257), 6, 4, 3, (32, 48))
    kw = dict(image_hw=(32, 48), downsample=4, depth_range=cases.DEPTH_RANGE, depth_bins=cases.BINS)
    want = cases.definition(case["points"], case["sizes"], case["projection"], **kw)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pts = cases.ragged(case["points"], case["sizes"], DEV)
        pts.tensor.mul_(1.0)       # enqueued on the side stream; the operator must follow it there
        got = cases.lidar_depth_targets(pts, torch.from_numpy(case["projection"]).to(DEV), **kw)
    side.synchronize()
    cases.check_equal(got, want, "side stream")
