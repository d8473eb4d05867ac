"""center_point_targets on the GPU: the kernel against the per-object float32 definition of center_targets_cases.py and
against the host entry, at the edges of its work partition (wave, chunk of kThreads slots, the max_objs cut), with guard
bands, reproducibility, graph capture, no host synchronisation, and end to end into the heat-map draw and the centre-point
regression loss."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_targets_cases import (NUSC, NUSC_TASKS, RADIUS_CFG, UNIT, check, check_device_against_host, check_pinned, definition,  # noqa: E402
                                  edge_case, make_case, radius_boundary_case, ragged, run)

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import (CenterPointTargets, center_point_targets, center_regression_loss,  # noqa: E402
                                  draw_heatmap_batched)

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = center_point_targets


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "center_targets.hip")).read()
WAVE = int(_constant(_SRC, "kWave"))
THREADS = int(_constant(_SRC, "kThreads"))          # slots per chunk
assert (WAVE, THREADS) == (64, 256)
ALL_TEN = (tuple(range(10)),)


def to_host(rb):
    return ragged(rb.tensor.cpu(), rb.sample_sizes.cpu())


def both(boxes, labels, tasks, cfg, what="", **kw):
    """device against the definition, and against the host path on the same inputs"""
    got, want = run(op, boxes, labels, tasks, cfg, **kw)
    assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for r in got for x in r)
    check(got, want, what + " device")
    host = op(to_host(boxes), to_host(labels), tasks, **cfg, **kw)
    check_device_against_host(got, host, want[0]["approx_channels"], what + " device against host")
    return got, want


def _sizes(B, N, k):
    """ragged sizes that include 0 and N"""
    return ([N, 0, min(N, N // 2 + 1)] if k == 0 else [0, N, N // 3])[:B]


# --------------------------------------------------------------------------------------------- the kernel's work partition
@pytest.mark.parametrize("B", [0, 1, 3])
@pytest.mark.parametrize("N", [0, 1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1])
def test_slot_counts_across_waves_and_chunks(N, B):
    for k in (0, 1):
        sizes = _sizes(B, N, k)
        boxes, labels = make_case(B, N, sizes, seed=N + B, device=DEV)
        got, want = both(boxes, labels, NUSC_TASKS, NUSC, f"B={B} N={N} sizes={sizes}")
        for r in got:
            assert r.centers.tensor.shape == (B, min(500, N), 2) and r.targets.tensor.shape == (B, min(500, N), 10)   # max_objs = 500
    if B == 3 and N >= WAVE:
        assert sum(int(w["sizes"].sum()) for w in want) > N // 4, "the case keeps too few objects to show anything"


@pytest.mark.parametrize("max_objs", [0, 10, WAVE, THREADS, THREADS + 1, 2 * THREADS + 1, 1000])
def test_max_objs_cut_inside_a_wave_at_a_wave_boundary_at_a_chunk_boundary_and_beyond(max_objs):
    """frame 0: every slot is a candidate of the one task, so the cut falls on slot max_objs; frame 1: mixed labels, the
    cut falls on a candidate rank somewhere inside a chunk; frame 2: fewer candidates than any cut but 0 and 10"""
    N = 2 * THREADS + 1
    boxes, labels = make_case(3, N, [N, N, 40], seed=11, device=DEV)
    labels.tensor[0] = 3
    got, want = both(boxes, labels, ALL_TEN, NUSC, f"max_objs={max_objs}", max_objs=max_objs)
    src = want[0]["source"]
    assert src.shape[1] == min(max_objs, N) and (max_objs == 0 or src[0].max() < max_objs)


@pytest.mark.parametrize("D", [7, 9])
@pytest.mark.parametrize("norm_bbox", [True, False])
@pytest.mark.parametrize("label_dtype,size_dtype", [(torch.int32, torch.int64), (torch.int64, torch.int32)])
def test_box_widths_size_encodings_and_index_dtypes(label_dtype, size_dtype, norm_bbox, D):
    boxes, labels = make_case(3, 70, [70, 0, 41], D=D, seed=D, label_dtype=label_dtype, size_dtype=size_dtype, device=DEV)
    both(boxes, labels, NUSC_TASKS, NUSC, norm_bbox=norm_bbox)
    got = op(boxes, labels.tensor, NUSC_TASKS, **NUSC, norm_bbox=norm_bbox)          # labels as a plain tensor
    check(got, definition(boxes.tensor, labels.tensor, boxes.sample_sizes, NUSC_TASKS, **NUSC, norm_bbox=norm_bbox))


def test_one_task_eight_tasks_absent_classes_labels_minus_one_and_63_and_an_all_dropped_frame():
    boxes, labels = make_case(3, THREADS + 9, [THREADS + 9, THREADS + 9, 17], seed=3, classes=12, device=DEV)
    boxes.tensor[1, :, 4] = -1.0                                   # frame 1: no box has a positive length
    labels.tensor[labels.tensor == 5] = 4                          # class 5 never occurs
    assert bool((labels.tensor == -1).any()) and bool((labels.tensor == 63).any())
    eight = ((0,), (1,), (2, 3), (4,), (5,), (6, 7, 8), (63,), (9, 10, 11))
    for tasks in (((3, 1, 63),), eight):
        got, want = both(boxes, labels, tasks, NUSC, f"T={len(tasks)}")
        assert all(w["sizes"][1] == 0 for w in want)
    assert want[4]["sizes"].sum() == 0 and want[6]["sizes"].sum() > 0


@pytest.mark.parametrize("D", [7, 9])
def test_edges_of_the_validity_rule_and_special_values(D):
    boxes, labels, kept = edge_case(D, device=DEV)
    got, want = both(boxes, labels, ((0,),), UNIT, "edges")
    r = got[0]
    assert r.source.tensor[0, :len(kept)].tolist() == kept
    W, _ = UNIT["grid_size"]
    assert r.centers.tensor[0, :4, 0].tolist() == [0, 0, W - 1, W - 1]     # x = -0.5, 0, W - 1, W - 0.5
    inf_dx = kept.index(22)
    assert r.radii.tensor[0, inf_dx].item() == 2 and r.targets.tensor[0, inf_dx, 3].item() == float("inf")
    if D == 9:                                                              # a special velocity reaches its own row only
        bad = ~torch.isfinite(r.targets.tensor[0, :len(kept)])
        rows = [kept.index(s) for s in (23, 24, 25)]
        assert bool(bad[rows, 8].all()) and int(bad[rows].sum()) == 3


def test_radii_on_an_integer_boundary():
    """boxes whose smallest root is an integer or a few float32 steps from one: a device square root that is not correctly
    rounded shows here (test_center_targets_cpu.py shows that a root off by one ulp changes dozens of these radii)"""
    boxes, labels = radius_boundary_case(DEV)
    got, want = both(boxes, labels, ((0,),), RADIUS_CFG, "radius boundary")
    assert want[0]["sizes"].tolist() == [boxes.tensor.shape[1]]
    assert got[0].radii.tensor[0, 4:351:9].tolist() == list(range(2, 41))


def test_pinned_vector():
    check_pinned(op, DEV)


def test_empty_extents_launch_nothing():
    for B, N, max_objs in ((0, 5, 500), (2, 0, 500), (2, 5, 0)):
        boxes, labels = make_case(B, N, [N] * B, seed=4, device=DEV)
        for r in op(boxes, labels, NUSC_TASKS, **NUSC, max_objs=max_objs):
            assert r.centers.tensor.shape == (B, min(max_objs, N), 2) and r.centers.tensor.is_cuda
            assert r.centers.sample_sizes.shape == (B,) and not bool(r.centers.sample_sizes.any())


def test_wrong_devices_are_refused():
    boxes, labels = make_case(2, 6, [6, 3], seed=6, device=DEV)
    with pytest.raises(RuntimeError, match="center_point_targets: labels must be on the boxes' device"):
        op(boxes, labels.tensor.cpu(), NUSC_TASKS, **NUSC)
    with pytest.raises(RuntimeError, match="center_point_targets: sample_sizes must be on the boxes' device"):
        op(RaggedBatch(boxes.tensor, sample_sizes=boxes.sample_sizes.cpu()), labels, NUSC_TASKS, **NUSC)


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,N,max_objs,D", [(3, 9, 500, 9), (2, THREADS + 3, 100, 7), (1, 5, 5, 9)])
def test_guard_bands_and_complete_write_of_all_six_outputs_and_the_sizes(B, N, max_objs, D):
    from accvlab import _amd_native as nat

    T, M, pad = len(NUSC_TASKS), min(max_objs, N), 512
    boxes, labels = make_case(B, N, [N, 0, N // 2][:B], D=D, seed=N, label_dtype=torch.int32, device=DEV)

    def banded(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
        return buf, buf[pad: pad + nbytes].view(dtype).view(shape)

    shapes = dict(centers=((T, B, M, 2), torch.int32), radii=((T, B, M), torch.int32), labels=((T, B, M), torch.int32),
                  targets=((T, B, M, D + 1), torch.float32), indices=((T, B, M), torch.int64), source=((T, B, M), torch.int32),
                  sizes=((T, B), torch.int64))
    bands = {k: banded(*v) for k, v in shapes.items()}
    p = nat.CenterPointTargetsParams()
    p.pc_range[0], p.pc_range[1], p.voxel_size[0], p.voxel_size[1] = NUSC["pc_range"][0], NUSC["pc_range"][1], 0.2, 0.2
    p.out_size_factor, p.gaussian_overlap, p.min_radius, p.max_objs, p.norm_bbox, p.num_tasks = 8.0, 0.1, 2, max_objs, 1, T
    for c in range(64):
        p.class_task[c] = nat.CT_NO_TASK
    for t, ids in enumerate(NUSC_TASKS):
        for pos, c in enumerate(ids):
            p.class_task[c], p.class_pos[c] = t, pos
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    status = nat.ctypes_lib().accv_center_point_targets(
        boxes.tensor.data_ptr(), labels.tensor.data_ptr(), boxes.sample_sizes.data_ptr(), nat.CT_COUNTS_I64, B, N, D, 64, 64, M,
        ctypes.addressof(p), *(bands[k][1].data_ptr() for k in ("centers", "radii", "labels", "targets", "indices", "source", "sizes")),
        stream)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    torch.cuda.synchronize()
    for name, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{name}: wrote outside its buffer"
    # every slot inside was written: the pre-filled sentinel is gone wherever the definition has a value, padding included
    got = [CenterPointTargets(*(RaggedBatch(bands[k][1][t].clone(), sample_sizes=sizes)
                                for k in ("centers", "radii", "labels", "targets", "indices", "source")))
           for t, sizes in enumerate(bands["sizes"][1].clone().unbind(0))]
    check(got, definition(boxes.tensor, labels.tensor, boxes.sample_sizes, NUSC_TASKS, **NUSC, max_objs=max_objs), "banded")


# -------------------------------------------------------------------------- reproducibility, no synchronisation, graphs
def _flat(result):
    return [x.tensor for r in result for x in r] + [r.centers.sample_sizes for r in result]


def test_two_runs_are_bitwise_identical():
    N = 2 * THREADS + 1
    boxes, labels = make_case(3, N, [N, 0, 300], seed=8, device=DEV)
    first = _flat(op(boxes, labels, NUSC_TASKS, **NUSC, max_objs=300))
    for _ in range(2):
        again = _flat(op(boxes, labels, NUSC_TASKS, **NUSC, max_objs=300))
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_no_host_synchronisation():
    boxes, labels = make_case(3, 70, [70, 0, 41], seed=9, device=DEV)
    op(boxes, labels, NUSC_TASKS, **NUSC)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = op(boxes, labels, NUSC_TASKS, **NUSC)
        empty = op(boxes, labels, NUSC_TASKS, **NUSC, max_objs=0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    check(got, definition(boxes.tensor, labels.tensor, boxes.sample_sizes, NUSC_TASKS, **NUSC))
    assert len(empty) == 6


def test_graph_capture_and_replay_equal_eager():
    N = THREADS + 9
    a = make_case(3, N, [N, 0, 41], seed=12, device=DEV)
    b = make_case(3, N, [7, N, N], seed=13, device=DEV)
    boxes, labels = ragged(a[0].tensor.clone(), a[0].sample_sizes.clone()), ragged(a[1].tensor.clone(), a[1].sample_sizes.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            op(boxes, labels, NUSC_TASKS, **NUSC)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(boxes, labels, NUSC_TASKS, **NUSC)
    for case in (b, a):
        boxes.tensor.copy_(case[0].tensor)
        labels.tensor.copy_(case[1].tensor)
        boxes.sample_sizes.copy_(case[0].sample_sizes)
        graph.replay()
        torch.cuda.synchronize()
        eager = op(case[0], case[1], NUSC_TASKS, **NUSC)
        for x, y in zip(_flat(out), _flat(eager)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        check(out, definition(case[0].tensor, case[1].tensor, case[0].sample_sizes, NUSC_TASKS, **NUSC), "replay")


# --------------------------------------------------------------------------------------------------------------- end to end
def test_outputs_feed_the_heatmap_draw_and_the_regression_loss_like_the_per_object_loop():
    """2 frames, 2 tasks, a 32 x 24 grid: the maps and the loss of the per-object loop (the definition's centres, radii,
    labels and targets; the maps drawn by the project's CPU oracle, the loss summed in float64)"""
    from oracle import h1 as oracle

    tasks, (W, H), B, N = ((0, 1, 2), (3, 4)), UNIT["grid_size"], 2, 24
    boxes, labels = make_case(B, N, [N, 15], seed=21, cfg=UNIT, classes=5, device=DEV)
    got, want = run(op, boxes, labels, tasks, UNIT, gaussian_overlap=0.5)      # overlap 0.5: radii from 2 to 6 cells
    assert len({int(v) for w in want for v in w["radii"].ravel()}) > 3
    check(got, want, "end to end")
    g = torch.Generator().manual_seed(5)
    for r, w, ids in zip(got, want, tasks):
        assert int(w["sizes"].sum()) >= 4
        hm = torch.full((B, len(ids), H, W), float("nan"), device=DEV)
        draw_heatmap_batched(hm, r.centers, r.radii, labels=r.labels, clear=True)
        ref = np.zeros((B, len(ids), H, W), np.float32)
        oracle.draw_heatmap_batched(ref, w["centers"], w["radii"], w["sizes"], labels=w["labels"], clear=True)
        err = float(np.abs(hm.cpu().numpy() - ref).max())
        assert err <= 1e-5, f"maps differ by {err}"
        for b in range(B):                                          # a peak of 1 at every centre, in its class plane
            for n in range(int(w["sizes"][b])):
                x, y = w["centers"][b, n]
                assert hm[b, w["labels"][b, n], y, x].item() == 1.0
        maps = torch.randn(B, 10, H, W, generator=g).to(DEV)
        loss = center_regression_loss(maps, r.centers, r.targets)
        m64, total, count = maps.cpu().double().numpy(), 0.0, 0
        target = w["exact"].astype(np.float64) + w["approx"]        # disjoint channels
        for b in range(B):
            for n in range(int(w["sizes"][b])):
                x, y = w["centers"][b, n]
                total += np.abs(m64[b, :, y, x] - target[b, n]).sum()
                count += 1
        ref_loss = total / max(count, 1)
        assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
