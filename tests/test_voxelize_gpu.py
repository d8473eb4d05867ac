"""voxelize_points on the GPU: the five kernels against the numpy float32 restatement of the sequential loop in
voxelize_cases.py and against the host entry on the same inputs, bit for bit on all five outputs — the cases of
test_voxelize_cpu.py on the device, the edges of the kernels' work partition (a lane per point in workgroups of kThreads; the
counting and numbering workgroups' chunk of kScanThreads * kUnroll points), the hash table at its smallest legal size, guard
bands around every output and the workspace through the C entry alone, a non-default stream, a hipGraph capture and replay,
errors before any launch and empty inputs.

The launch regimes, each entered by one test with shapes derived from the constants read from the source: the numbering
workgroup's sum over more than 2 * 64 and more than kScanThreads chunks (partial sums in three waves; a lane's second
trip); index lists of more than kScanThreads * 64 words a frame (two and three filling workgroups, the 4-byte tail), also
through the C entry into a workspace of zero bytes; max_voxels crossed inside a lane's kUnroll points, between lanes, waves
and chunks; voxels of max_points - 1, max_points and max_points + 1 points up to max_points = 128; rows of 6, 8, 12, 15 and
16 channels; a grid of 2^30 cells; 65535 frames."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import voxelize_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "voxelize.hip")).read()
THREADS, SCAN_THREADS, UNROLL = (int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1))
                                 for name in ("kThreads", "kScanThreads", "kUnroll"))
assert (THREADS, SCAN_THREADS, UNROLL) == (256, 1024, 4)
FILL_BLOCKS = int(re.search(r"constexpr int kFillBlocks = (\d+);", _SRC).group(1))
LIST_WORDS = SCAN_THREADS * 64       # the index words one list-filling workgroup takes: check_args' fill_blocks
assert FILL_BLOCKS == 64 and "(long long)kScanThreads * 64" in _SRC


@pytest.mark.parametrize("B,D,size_dtype,grid,T,V,below", cases.CONFIGS)
def test_random_configurations_against_the_definition(B, D, size_dtype, grid, T, V, below):
    cases.check_config(DEV, B, D, size_dtype, grid, T, V, below)


def test_work_partition_edges_and_table_size_rule():
    cases.check_partition(DEV, THREADS, SCAN_THREADS * UNROLL)


def test_gpu_against_cpu_tensors():
    """the same call on CPU tensors gives the same bits, with and without rows, for 16-byte and 4-byte rows"""
    sizes = (SCAN_THREADS * UNROLL + 1, 0, THREADS + 1)
    for D in (4, 7):
        pts = cases.random_points(70 + D, sizes, D)
        for aug in (None, cases.rows(D, 3)):
            kw = dict(max_points=5, max_voxels=200, augmentation=aug, **cases.VOXELS3D)
            cases.check_equal(cases.run(pts, sizes, DEV, **kw), cases.run(pts, sizes, "cpu", **kw), f"D {D}")


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


def test_guard_bands_workspace_and_complete_write_through_the_c_entry_alone():
    cases.check_guard_bands(DEV)


def test_every_documented_error_is_raised_before_a_launch():
    cases.check_errors(DEV, other_dev="cpu")


# ------------------------------------------------------------------------------------ the regimes of the work partition
def test_prefix_over_130_chunks_carries_through_three_waves():
    """the last numbering workgroup has 2 * 64 + 2 chunks in front of it: lanes of waves 0, 1 and 2 hold a count each"""
    cases.check_many_chunks(DEV, 2 * cases.WAVE + 2, SCAN_THREADS, UNROLL)


def test_prefix_over_1025_chunks_takes_a_second_trip():
    """kScanThreads + 1 chunks in front of the last numbering workgroup: lane 0 reads two counts; 4.2 M points"""
    cases.check_many_chunks(DEV, SCAN_THREADS + 1, SCAN_THREADS, UNROLL)


def test_lists_of_more_than_one_filling_workgroup():
    cases.check_list_fill(DEV, LIST_WORDS, FILL_BLOCKS)


def test_lists_of_more_than_one_filling_workgroup_in_a_zeroed_workspace_through_the_c_entry():
    cases.check_list_fill_workspace(DEV, LIST_WORDS, FILL_BLOCKS)


def test_max_voxels_crossed_inside_a_lane_between_waves_and_between_chunks():
    cases.check_budget_crossings(DEV, UNROLL, SCAN_THREADS * UNROLL)


@pytest.mark.parametrize("T", [1, 2, 128])
def test_voxels_of_max_points_minus_one_to_plus_one_points(T):
    cases.check_point_budget(DEV, T)


@pytest.mark.parametrize("D", [6, 8, 12, 15, 16])
def test_row_widths_with_and_without_rows_and_off_a_16_byte_boundary(D):
    cases.check_row_widths(DEV, D)


def test_grid_of_two_to_the_thirty_cells():
    cases.check_large_keys(DEV)


def test_most_frames_a_call_takes():
    """B = 65535 is gridDim.y of all five launches"""
    cases.check_most_frames(DEV)


def _stream_case():
    sizes = (1500, 257)
    pts = cases.random_points(81, sizes, 4)
    kw = dict(max_points=3, max_voxels=150, **cases.VOXELS3D)
    return pts, sizes, cases.rows(8, 2), kw


def test_runs_on_the_current_stream():
    """the memset and the launches go to torch's current stream: on a side stream, after work that stream alone waits for"""
    pts, sizes, rows, kw = _stream_case()
    want = cases.definition(pts, sizes, augmentation=rows, **kw)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rb = cases.ragged(cases.np.zeros_like(pts), sizes, DEV)
        rb.tensor.copy_(torch.from_numpy(pts).to(DEV))       # enqueued on the side stream (a copy keeps the NaN payloads); the
        #                                                      operator must follow it there
        got = cases.voxelize_points(rb, augmentation=torch.from_numpy(rows).to(DEV), return_point_voxel=True, **kw)
    side.synchronize()
    cases.check_equal(got, want, "side stream")


def test_graph_capture_and_replay_give_the_bits_of_the_eager_call():
    """one linear chain: the memset node and the five kernel nodes; the replay runs on new points in the captured tensor"""
    pts, sizes, rows, kw = _stream_case()
    rb, aug = cases.ragged(pts, sizes, DEV), torch.from_numpy(rows).to(DEV)
    eager = cases.voxelize_points(rb, augmentation=aug, return_point_voxel=True, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = cases.voxelize_points(rb, augmentation=aug, return_point_voxel=True, **kw)
    other = cases.random_points(82, sizes, 4)
    rb.tensor.copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize()
    cases.check_equal(captured, cases.definition(other, sizes, augmentation=rows, **kw), "replay on new points")
    rb.tensor.copy_(torch.from_numpy(pts))
    graph.replay()
    torch.cuda.synchronize()
    cases.check_equal(captured, eager, "replay")
