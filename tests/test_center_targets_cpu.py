"""center_point_targets without a GPU: the library's host entry (CPU tensors) against the per-object float32 definition of
center_targets_cases.py, the edge list of the validity rule, the pinned hand-computed vector, every RuntimeError of the
argument checks and the ACCV_EINVAL paths of both C-ABI entries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_targets_cases import (NUSC, NUSC_TASKS, RADIUS_CFG, UNIT, check, check_pinned, definition, edge_case, make_case,  # noqa: E402
                                  radii_with_root_off_by_one_ulp, radius_boundary_case, ragged, run)

from accvlab.draw_heatmap import CenterPointTargets, center_point_targets  # noqa: E402

op = center_point_targets


@pytest.mark.parametrize("norm_bbox", [True, False])
@pytest.mark.parametrize("D", [7, 9])
def test_host_path_equals_the_definition(D, norm_bbox):
    boxes, labels = make_case(3, 70, [70, 0, 41], D=D, seed=D)
    got, want = run(op, boxes, labels, NUSC_TASKS, NUSC, norm_bbox=norm_bbox)
    assert len(got) == 6 and all(isinstance(r, CenterPointTargets) for r in got)
    assert sum(int(w["sizes"].sum()) for w in want) > 30, "the case keeps too few objects to show anything"
    check(got, want, f"D={D} norm_bbox={norm_bbox}")


@pytest.mark.parametrize("label_dtype,size_dtype", [(torch.int32, torch.int32), (torch.int64, torch.int32), (torch.int32, torch.int64)])
def test_label_and_size_dtypes_and_labels_as_a_plain_tensor(label_dtype, size_dtype):
    boxes, labels = make_case(2, 33, [33, 20], seed=1, label_dtype=label_dtype, size_dtype=size_dtype)
    got, want = run(op, boxes, labels, NUSC_TASKS, NUSC)
    check(got, want)
    check(op(boxes, labels.tensor, NUSC_TASKS, **NUSC), want, "plain labels")


@pytest.mark.parametrize("max_objs", [0, 1, 5, 6, 500])
def test_max_objs_cuts_the_candidates_before_the_validity_test(max_objs):
    """frame 0 holds 12 objects of class 0, every other one out of range: 6 candidates survive an uncut run"""
    boxes, labels = make_case(2, 12, [12, 7], seed=2)
    labels.tensor[0] = 0
    boxes.tensor[0, :, :2] = 1.0
    boxes.tensor[0, 0::2, 0] = 1000.0
    boxes.tensor[0, :, 3] = 1.0
    got, want = run(op, boxes, labels, ((0,), (1, 2, 3)), NUSC, max_objs=max_objs)
    assert want[0]["sizes"][0] == min(max_objs, 12) // 2
    assert got[0].centers.tensor.shape == (2, min(max_objs, 12), 2)
    check(got, want, f"max_objs={max_objs}")


def test_single_task_eight_tasks_absent_classes_and_a_frame_where_everything_is_dropped():
    boxes, labels = make_case(3, 40, [40, 40, 17], seed=3, classes=12)
    boxes.tensor[1, :, 4] = -1.0                                   # frame 1: no box has a positive length
    labels.tensor[labels.tensor == 5] = 4                          # class 5 never occurs
    eight = ((0,), (1,), (2, 3), (4,), (5,), (6, 7, 8), (63,), (9, 10, 11))
    for tasks in (((3, 1, 63),), eight):
        got, want = run(op, boxes, labels, tasks, NUSC)
        assert all(w["sizes"][1] == 0 for w in want)
        check(got, want, f"T={len(tasks)}")
    assert want[4]["sizes"].sum() == 0 and want[6]["sizes"].sum() > 0   # the absent class; label 63 is a class like any other


@pytest.mark.parametrize("D", [7, 9])
def test_edges_of_the_validity_rule_and_special_values(D):
    boxes, labels, kept = edge_case(D)
    got, want = run(op, boxes, labels, ((0,),), UNIT)
    assert want[0]["source"][0, :len(kept)].tolist() == kept, "the definition disagrees with the hand-worked edge list"
    check(got, want, "edges")
    r = got[0]
    assert r.source.tensor[0, :len(kept)].tolist() == kept
    W, H = UNIT["grid_size"]
    xs = r.centers.tensor[0, :4, 0].tolist()
    assert xs == [0, 0, W - 1, W - 1], xs                          # x = -0.5, 0, W - 1, W - 0.5
    assert r.targets.tensor[0, 0, 0].item() == -0.5 and r.targets.tensor[0, 3, 0].item() == 0.5
    inf_dx = kept.index(22)
    assert r.radii.tensor[0, inf_dx].item() == 2 and r.targets.tensor[0, inf_dx, 3].item() == float("inf")
    if D == 9:                                                      # a special velocity reaches its own row, channel 8, only
        t = r.targets.tensor[0, :len(kept)]
        bad = ~torch.isfinite(t)
        rows = [kept.index(s) for s in (23, 24, 25)]
        assert bad[rows, 8].all() and bad[rows].sum() == 3


def test_radii_on_an_integer_boundary_and_the_cases_would_notice_a_root_off_by_an_ulp():
    boxes, labels = radius_boundary_case()
    got, want = run(op, boxes, labels, ((0,),), RADIUS_CFG)
    n = boxes.tensor.shape[1]
    assert want[0]["sizes"].tolist() == [n]
    check(got, want, "radius boundary")
    radii = want[0]["radii"][0].tolist()
    assert radii[4:351:9] == list(range(2, 41)), "w = 2 k, l = 3 k must give radius k exactly"
    for direction in (1, -1):
        wrong = radii_with_root_off_by_one_ulp(boxes, direction)
        flips = sum(a != b for a, b in zip(radii, wrong))
        assert flips >= 20, f"a root off by {direction} ulp changes only {flips} radii: the case does not sit on the boundary"


def test_pinned_vector():
    check_pinned(op, "cpu")


def test_empty_extents_touch_nothing():
    for B, N, max_objs in ((0, 5, 500), (2, 0, 500), (2, 5, 0)):
        boxes, labels = make_case(B, N, [N] * B, seed=4)
        got = op(boxes, labels, NUSC_TASKS, **NUSC, max_objs=max_objs)
        M = min(max_objs, N)
        for r in got:
            assert r.centers.tensor.shape == (B, M, 2) and r.targets.tensor.shape == (B, M, 10) and r.source.tensor.shape == (B, M)
            assert r.centers.sample_sizes.shape == (B,) and not r.centers.sample_sizes.any()


def test_tasks_are_views_of_single_allocations():
    boxes, labels = make_case(2, 9, [9, 4], seed=5)
    got = op(boxes, labels, NUSC_TASKS, **NUSC)
    for name in CenterPointTargets._fields:
        first = getattr(got[0], name).tensor
        for t, r in enumerate(got):
            x = getattr(r, name).tensor
            assert x.is_contiguous() and x.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
            assert x.data_ptr() == first.data_ptr() + t * first.numel() * first.element_size()


# ------------------------------------------------------------------------------------------------------- argument checks
def _raises(match, boxes, labels, tasks=NUSC_TASKS, **kw):
    cfg = dict(NUSC)
    cfg.update(kw)
    with pytest.raises(RuntimeError, match="center_point_targets: .*" + match):
        op(boxes, labels, tasks, **cfg)


def test_argument_checks_raise_runtime_errors_with_the_operators_name():
    boxes, labels = make_case(2, 6, [6, 3], seed=6)
    bt, lt, sz = boxes.tensor, labels.tensor, boxes.sample_sizes
    _raises("boxes must be a RaggedBatch", bt, labels)
    _raises("boxes must be float32", ragged(bt.double(), sz), labels)
    _raises("boxes must be float32", ragged(bt[..., :8].contiguous(), sz), labels)
    _raises("boxes must be float32", ragged(bt[:, :, 0].contiguous(), sz), labels)
    _raises("boxes must be contiguous", ragged(bt.transpose(0, 1).contiguous().transpose(0, 1), sz), labels)
    _raises("labels must be int32 or int64", boxes, lt.float())
    _raises("labels must be int32 or int64", boxes, lt[:, :5].contiguous())
    _raises("labels must be contiguous", boxes, lt.t().contiguous().t())
    _raises("labels must be a tensor", boxes, [[0] * 6] * 2)
    _raises("sample_sizes must be int32 or int64", ragged(bt, sz.float()), labels)
    _raises("sample_sizes must be int32 or int64", ragged(bt, sz, torch.int16), labels)
    _raises("labels must be on the boxes' device", boxes, lt.to("meta"))
    _raises("boxes must be CUDA or CPU tensors", ragged(bt.to("meta"), sz.to("meta")), lt.to("meta"))
    _raises("tasks must be a sequence of 1..8", boxes, labels, tasks=())
    _raises("tasks must be a sequence of 1..8", boxes, labels, tasks=tuple((i,) for i in range(9)))
    _raises("tasks must be a sequence of 1..8", boxes, labels, tasks=3)
    _raises(r"tasks\[1\] must be a sequence", boxes, labels, tasks=((0,), 1))
    _raises("class ids must be integers in", boxes, labels, tasks=((0, 64),))
    _raises("class ids must be integers in", boxes, labels, tasks=((-1,),))
    _raises("class ids must be integers in", boxes, labels, tasks=((1.0,),))
    _raises("class 2 is in more than one task", boxes, labels, tasks=((1, 2), (2,)))
    _raises("class 2 is in more than one task", boxes, labels, tasks=((2, 2),))
    _raises("pc_range must be a sequence", boxes, labels, pc_range=[0.0])
    _raises("voxel_size must be a sequence", boxes, labels, voxel_size=0.2)
    _raises("voxel_size and out_size_factor must be positive", boxes, labels, voxel_size=[0.2, 0.0, 8.0])
    _raises("voxel_size and out_size_factor must be positive", boxes, labels, out_size_factor=-8)
    _raises("voxel_size and out_size_factor must be positive", boxes, labels, voxel_size=[float("inf"), 0.2])
    _raises("out_size_factor must be a Python number", boxes, labels, out_size_factor=torch.tensor(8))
    _raises("pc_range and gaussian_overlap must be finite", boxes, labels, gaussian_overlap=float("nan"))
    _raises("grid_size must be", boxes, labels, grid_size=(0, 64))
    _raises("grid_size must be", boxes, labels, grid_size=(65536, 32768))
    _raises(r"grid_size\[0\] must be a Python integer", boxes, labels, grid_size=(64.0, 64))
    _raises("max_objs must be in", boxes, labels, max_objs=-1)
    _raises("max_objs must be a Python integer", boxes, labels, max_objs=5.0)
    _raises("min_radius must be a Python integer", boxes, labels, min_radius=True)


# ------------------------------------------------------------------------------------------------------------- the C-ABI
def _abi_case():
    from accvlab import _amd_native as nat

    B, N, D, M, T = 2, 5, 9, 5, 2
    boxes, labels = make_case(B, N, [5, 3], seed=7, label_dtype=torch.int32)
    p = nat.CenterPointTargetsParams()
    p.pc_range[0], p.pc_range[1], p.voxel_size[0], p.voxel_size[1] = -51.2, -51.2, 0.2, 0.2
    p.out_size_factor, p.gaussian_overlap, p.min_radius, p.max_objs, p.norm_bbox, p.num_tasks = 8.0, 0.1, 2, 500, 1, T
    for c in range(64):
        p.class_task[c], p.class_pos[c] = (c % 2, c // 2) if c < 10 else (nat.CT_NO_TASK, 0)
    outs = dict(centers=torch.zeros(T, B, M, 2, dtype=torch.int32), radii=torch.zeros(T, B, M, dtype=torch.int32),
                labels=torch.zeros(T, B, M, dtype=torch.int32), targets=torch.zeros(T, B, M, D + 1),
                indices=torch.zeros(T, B, M, dtype=torch.int64), source=torch.zeros(T, B, M, dtype=torch.int32),
                sizes=torch.zeros(T, B, dtype=torch.int64))
    return nat, boxes, labels, p, outs, dict(B=B, N=N, D=D, W=64, H=64, M=M)


def _abi_call(entry, nat, boxes, labels, p, outs, dims, flags=None, null=(), **over):
    d = dict(dims)
    d.update(over)
    ptr = lambda name, t: None if name in null else t.data_ptr()   # noqa: E731
    args = [ptr("boxes", boxes.tensor), ptr("labels", labels.tensor), ptr("counts", boxes.sample_sizes),
            nat.CT_COUNTS_I64 if flags is None else flags, d["B"], d["N"], d["D"], d["W"], d["H"], d["M"],
            None if "params" in null else ctypes.addressof(p)]
    args += [ptr("labels_out" if k == "labels" else k, outs[k])
             for k in ("centers", "radii", "labels", "targets", "indices", "source", "sizes")]
    lib = nat.ctypes_lib()
    if entry == "device":
        return lib.accv_center_point_targets(*args, None), lib.accv_last_error()
    return lib.accv_center_point_targets_host(*args), lib.accv_last_error()


@pytest.mark.parametrize("entry", ["device", "host"])
def test_cabi_argument_errors_return_einval_before_anything_is_launched(entry):
    nat, boxes, labels, p, outs, dims = _abi_case()
    call = lambda **kw: _abi_call(entry, nat, boxes, labels, p, outs, dims, **kw)   # noqa: E731
    for kw, text in ((dict(null=("params",)), b"null params"), (dict(B=-1), b"negative size"), (dict(N=-1), b"negative size"),
                     (dict(M=-1), b"negative size"), (dict(W=-1), b"negative size"), (dict(D=8), b"D = 7 or 9"),
                     (dict(D=4), b"D = 7 or 9"), (dict(flags=4), b"unknown flags"), (dict(W=0), b"grid of"),
                     (dict(W=65536, H=32768), b"grid of"), (dict(N=2 ** 31), b"limited to 2^31 - 1"),
                     (dict(M=4), b"below min(max_objs, N)"), (dict(null=("counts",)), b"null counts"),
                     (dict(null=("sizes",)), b"null counts"), (dict(null=("boxes",)), b"null boxes"),
                     (dict(null=("labels",)), b"null boxes"), (dict(null=("targets",)), b"null output"),
                     (dict(null=("centers",)), b"null output"), (dict(null=("source",)), b"null output")):
        status, err = call(**kw)
        assert status == -1 and text in err, (kw, status, err)
    for tasks in (0, 9, -1):
        p.num_tasks = tasks
        status, err = call()
        assert status == -1 and b"tasks supported" in err
    p.num_tasks = 2
    p.class_task[11] = 2
    status, err = call()
    assert status == -1 and b"class 11 is in task 2 of 2" in err
    p.class_task[11] = nat.CT_NO_TASK
    for field, value in (("voxel_size", 0.0), ("voxel_size", float("nan")), ("out_size_factor", -1.0)):
        keep = p.voxel_size[1] if field == "voxel_size" else p.out_size_factor
        if field == "voxel_size":
            p.voxel_size[1] = value
        else:
            p.out_size_factor = value
        status, err = call()
        assert status == -1 and b"must be positive" in err
        if field == "voxel_size":
            p.voxel_size[1] = keep
        else:
            p.out_size_factor = keep
    p.max_objs = -1
    assert call()[0] == -1
    p.max_objs = 500
    # misaligned outputs: the row stores are 8 bytes wide
    odd = torch.zeros(outs["targets"].numel() + 1)[1:].view_as(outs["targets"])
    status, err = _abi_call(entry, nat, boxes, labels, p, dict(outs, targets=odd), dims)
    assert status == -1 and b"8-byte aligned" in err
    # empty problems succeed with null pointers and write nothing
    for kw in (dict(B=0), dict(N=0, M=0), dict(M=0, N=0, B=0)):
        status, _ = call(null=("boxes", "labels", "counts", "centers", "radii", "labels_out", "targets", "indices", "source", "sizes"), **kw)
        assert status == 0, kw
    assert all(not t.any() for t in outs.values()), "a refused or empty call wrote to its outputs"


def test_cabi_host_entry_equals_the_definition():
    nat, boxes, labels, p, outs, dims = _abi_case()
    status, err = _abi_call("host", nat, boxes, labels, p, outs, dims)
    assert status == 0, err
    tasks = ((0, 2, 4, 6, 8), (1, 3, 5, 7, 9))
    from accvlab.batching_helpers import RaggedBatch

    got = [CenterPointTargets(*(RaggedBatch(outs[k][t], sample_sizes=sizes)
                                for k in ("centers", "radii", "labels", "targets", "indices", "source")))
           for t, sizes in enumerate(outs["sizes"].unbind(0))]
    check(got, definition(boxes.tensor, labels.tensor, boxes.sample_sizes, tasks, **NUSC), "C-ABI host")
    assert np.array_equal(outs["sizes"].numpy(), np.stack([w["sizes"] for w in definition(
        boxes.tensor, labels.tensor, boxes.sample_sizes, tasks, **NUSC)]))
