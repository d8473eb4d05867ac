"""scatter_to_bev on the GPU: the mark, write and backward kernels against the sequential numpy loop of bev_scatter_cases.py
and against the host entries on the same inputs, bit for bit on canvas, index and grad_features in float32, float16 and
bfloat16 — the cases of test_bev_scatter_cpu.py on the device, with the edge shapes derived from the constants read from the
source (lanes of a workgroup, cells of a tile, channels of a chunk), a non-default stream and a hipGraph capture and replay
of forward + backward."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bev_scatter_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "bev_scatter.hip")).read()
THREADS, TILE, CHUNK = (int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1)) for name in ("kThreads", "kTileW", "kChunk"))
assert (THREADS, TILE, CHUNK) == (256, 64, 64)


@pytest.mark.parametrize("nx", [1, 3, 4, TILE - 1, TILE, TILE + 1, 2 * TILE + 2])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=str)
def test_map_and_channel_shapes_against_the_definition(dtype, nx):
    cases.check_shapes(DEV, dtype, nx, CHUNK)


def test_gpu_against_cpu_tensors():
    B, ny, nx, C = 3, 5, 2 * TILE + 2, CHUNK + 8
    coors = cases.random_coors(31, 2 * THREADS + 1, B, ny, nx)
    for dtype in cases.DTYPES:
        feats = cases.random_values(900, (coors.shape[0], C), dtype, "cpu")
        go = cases.random_values(901, (B, C, ny, nx), dtype, "cpu")
        host = cases.run_case("cpu", dtype, coors, B, ny, nx, C, 0, "host", features=feats, grad=go)
        dev = cases.run_case(DEV, dtype, coors, B, ny, nx, C, 0, "device", features=feats.to(DEV), grad=go.to(DEV))
        for a, b, name in zip(dev, host, ("canvas", "index", "grad_features")):
            cases.assert_bits(a, b, f"device against host, {name}, {dtype}")


def test_row_counts_around_a_workgroup():
    cases.check_row_counts(DEV, THREADS)


def test_empty_frames_full_and_empty_tiles_and_corner_cells():
    cases.check_occupancy(DEV, TILE)


def test_duplicates_the_highest_row_wins_across_workgroups():
    cases.check_duplicates(DEV, THREADS)


def test_rows_outside_are_unplaced_and_z_is_ignored():
    cases.check_outside(DEV)


def test_padded_form_on_the_coors_of_voxelize_points():
    cases.check_padded_form(DEV)


def test_views_off_a_16_byte_boundary_take_the_element_path():
    cases.check_misaligned(DEV)


def test_guard_bands_and_complete_write_through_the_c_entries_alone():
    cases.check_guard_bands(DEV)


def test_against_the_torch_composition_of_mmdet3d_and_its_autograd():
    cases.check_against_torch(DEV)


def test_no_frames_no_rows_no_cells():
    cases.check_empty(DEV)


def test_every_documented_error_is_raised_before_a_launch():
    cases.check_errors(DEV, other_dev="cpu")


def _stream_case(dtype):
    B, ny, nx, C = 2, 6, TILE + 8, 16
    coors = cases.random_coors(41, 300, B, ny, nx)
    return coors, B, ny, nx, C, cases.random_values(910, (300, C), dtype, DEV), cases.random_values(911, (B, C, ny, nx), dtype, DEV)


def test_runs_on_the_current_stream():
    """the memset and the launches of forward and backward go to torch's current stream: on a side stream, after a copy
    that stream alone waits for"""
    coors, B, ny, nx, C, feats, go = _stream_case(torch.float32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        late = torch.zeros_like(feats)
        late.copy_(feats)
        cases.run_case(DEV, torch.float32, coors, B, ny, nx, C, 0, "side stream", features=late, grad=go)
    side.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_graph_capture_and_replay_of_forward_and_backward(dtype):
    """one linear chain: the memset node, mark, write and the backward launch; the replay runs on new features, new coors
    and a new upstream gradient in the captured tensors"""
    coors, B, ny, nx, C, feats, go = _stream_case(dtype)
    tc = torch.from_numpy(coors).to(DEV)
    feats.requires_grad_(True)

    def step():
        canvas, index = cases.scatter_to_bev(feats, tc, grid_hw=(ny, nx), batch_size=B, return_index=True)
        grad, = torch.autograd.grad(canvas, feats, go)
        return canvas, index, grad

    # torch's documented recipe for capturing a backward, which the other captures of an autograd pass in this suite follow:
    # the warm-up iterations run on a side stream that waits for the current one, and the current stream waits for it
    # before the capture begins
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    other = cases.random_coors(42, 300, B, ny, nx)
    with torch.no_grad():
        tc.copy_(torch.from_numpy(other))
        feats.copy_(cases.random_values(912, (300, C), dtype, DEV))
        go.copy_(cases.random_values(913, (B, C, ny, nx), dtype, DEV))
    graph.replay()
    torch.cuda.synchronize()
    want_canvas, want_index = cases.definition(cases.bits_of(feats).numpy(), other, B, ny, nx)
    cases.assert_bits(captured[0], want_canvas, "replay on new inputs: canvas")
    cases.assert_bits(captured[1], want_index, "replay on new inputs: index")
    cases.assert_bits(captured[2], cases.backward_definition(cases.bits_of(go).numpy(), other, want_index, B, ny, nx),
                      "replay on new inputs: grad_features")
    assert not torch.equal(captured[1], eager[1])
