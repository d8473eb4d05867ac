"""bev_augment_boxes without a GPU: the library's host entry (accv_bev_augment_host) against the two numpy oracles of
bev_augment_cases.py, the refusals, the C entries' argument checks and the two parameter helpers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import bev_augment_cases as cases
from bev_augment_cases import F32, built, check_case, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_entry_equals_the_float32_oracle_and_lies_within_the_bar_of_the_float64_one(name):
    check_case(name, DEV)


def test_rounding_counts_of_the_header_are_the_bars_of_these_tests():
    text = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "bev_augment_arith.h")).read()
    found = {k: int(v) for k, v in re.findall(r"constexpr int k(Box|Point|Frame)Roundings = (\d+);", text)}
    assert found == {"Box": cases.N_BOX, "Point": cases.N_POINT, "Frame": cases.N_FRAME}


def test_reference_data_every_part_off_returns_the_inputs():
    case, a = built("reference")
    got = run(case, DEV)
    off = 3                                    # the frame with the identity row
    assert torch.equal(got["boxes"][off], torch.from_numpy(case.boxes[off]))
    assert torch.equal(got["pts"][0][off], torch.from_numpy(case.pts[0][off]))
    assert torch.equal(got["pts"][1][off], torch.from_numpy(case.pts[1][off]))
    assert torch.equal(got["frs"][0][off], torch.from_numpy(case.frs[0][off]))
    assert got["sizes"].tolist() == [7, 7, 7, 7] and bool(got["keep"].all())
    # the first frame by hand: (1, 2, 3) turned by π/2 is (-2, 1, 3), times 1.5, plus (0.5, 1, 1.5); sizes times 1.5
    np.testing.assert_allclose(got["boxes"][0, 4, :6].numpy(), [-2.5, 2.5, 6.0, 3.0, 2.25, 1.5], atol=1e-5)
    np.testing.assert_allclose(got["boxes"][0, 4, 7:].numpy(), [-0.3, 0.15], atol=1e-6)
    assert float(got["boxes"][0, :, 6].abs().max()) <= math.pi + 1e-6


def test_range_borders_are_inclusive_one_ulp_outside_is_dropped_and_nan_fails():
    for name in ("borders-input", "borders-output"):
        got = run(built(name)[0], DEV)
        want = [True] * 6 + [False] * 6 + [False] * 3 + [True, False, False] + [False] * 3
        assert got["keep"].tolist() == [want, want], name
    got = run(built("borders-inf")[0], DEV)
    want = [True] * 12 + [False] * 3 + [True, True, True] + [False] * 3         # only NaN fails infinite borders
    assert got["keep"].tolist() == [want, want]
    got = run(built("borders-double")[0], DEV)                       # float32(±51.2) lies outside ±51.2
    want = [False] * 4 + [True] * 2 + [False] * 9 + [True, False, False] + [False] * 3
    assert got["keep"].tolist() == [want, want]


def test_range_check_on_input_against_output():
    got = run(built("order-input")[0], DEV)
    assert got["keep"].tolist() == [[True, False, True, False, False]] and got["source"].tolist() == [[0, 2, -1, -1, -1]]
    assert got["boxes"][0, 0, 0].item() == 55.0                      # kept by its raw centre, stored augmented
    got = run(built("order-output")[0], DEV)
    assert got["keep"].tolist() == [[False, True, True, False, False]] and got["source"].tolist() == [[1, 2, -1, -1, -1]]
    assert got["labels"].tolist() == [[1, 2, 0, 0, 0]]


@pytest.mark.parametrize("sizes_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("labels_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("valid_dtype", [torch.bool, torch.uint8])
def test_valid_label_and_count_dtypes(valid_dtype, labels_dtype, sizes_dtype):
    case, a = built("dtypes")
    typed = cases.Case(case.boxes, case.sizes, case.rows, labels=case.labels, valid=case.valid, point_range=case.point_range,
                       sizes_dtype=sizes_dtype)
    got = run(typed, DEV, labels_dtype=labels_dtype, valid_dtype=valid_dtype)
    assert got["labels"].dtype == labels_dtype
    cases.assert_same(got, a)


def test_counts_are_clamped_to_the_slots():
    case, _ = built("dtypes")
    wild = cases.Case(case.boxes, [1000, -5, 41], case.rows, labels=case.labels, valid=case.valid, point_range=case.point_range)
    flat = run(wild, DEV)
    cases.assert_same(flat, cases.oracle_a(wild))
    assert flat["sizes"][1].item() == 0


@pytest.mark.parametrize("seed,on", [(1, "input"), (2, "output")])
def test_seeded_sweep_keeps_and_drops_a_fifth_each_at_least(seed, on):
    name = f"sweep-{seed}-{on}"
    case, a = built(name)
    kept, dropped = cases.sweep_shares(case, a)                       # on the oracle alone
    assert kept >= 0.2 and dropped >= 0.2, (kept, dropped)


def test_center_point_targets_on_the_output_equals_center_point_targets_on_the_oracle():
    cases.check_end_to_end("sweep-1-input", DEV)


def test_every_output_lies_between_guard_bands_through_the_ctypes_binding():
    cases.check_guard_bands("matrices-full", DEV, labels=False)
    cases.check_guard_bands("sizes-D9-alternate", DEV, labels=True)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_call():
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import bev_augment_boxes as op

    case, _ = built("dtypes")
    boxes, rows, kw = cases.to_torch(case, DEV)
    B, N, D = case.boxes.shape
    rb = lambda t, s=None: RaggedBatch(t, sample_sizes=boxes.sample_sizes if s is None else s)   # noqa: E731
    mats = torch.zeros((B, 2, 4, 4))
    bad = [
        (lambda: op(boxes.tensor, rows), "RaggedBatch"),
        (lambda: op(rb(boxes.tensor.double()), rows), "float32"),
        (lambda: op(rb(boxes.tensor[..., :8].contiguous()), rows), "7 or 9"),
        (lambda: op(rb(boxes.tensor[:, :, None]), rows), "float32"),
        (lambda: op(rb(boxes.tensor.transpose(0, 1).contiguous().transpose(0, 1), boxes.sample_sizes), rows), "contiguous"),
        (lambda: op(boxes, rows.double()), "params"),
        (lambda: op(boxes, rows[:, :6].contiguous()), "params"),
        (lambda: op(boxes, torch.zeros((B, 14))[:, ::2]), "contiguous"),
        (lambda: op(rb(boxes.tensor, boxes.sample_sizes.float()), rows), "sample_sizes"),
        (lambda: op(boxes, rows, labels=torch.zeros((B, N), dtype=torch.int16)), "labels"),
        (lambda: op(boxes, rows, labels=torch.zeros((B, N + 1), dtype=torch.int64)), "labels"),
        (lambda: op(boxes, rows, valid=torch.zeros((B, N), dtype=torch.int32)), "valid"),
        (lambda: op(boxes, rows, valid=torch.zeros((N, B), dtype=torch.bool)), "valid"),
        (lambda: op(boxes, rows, range_check_on="both"), "range_check_on"),
        (lambda: op(boxes, rows, point_range=(-1, 1)), "point_range"),
        (lambda: op(boxes, rows, point_range=((0, 0, float("nan")), (1, 1, 1))), "point_range"),
        (lambda: op(boxes, rows, point_range=((0, 0), (1, 1))), "point_range"),
        (lambda: op(boxes, rows, point_transforms=[mats] * 5), "at most 4"),
        (lambda: op(boxes, rows, frame_transforms=[mats] * 3), "at most 2"),
        (lambda: op(boxes, rows, frame_transforms=[mats[:, :, :3].contiguous()]), "frame_transforms"),
        (lambda: op(boxes, rows, point_transforms=[mats[:, :, :2].contiguous()]), "point_transforms"),
        (lambda: op(boxes, rows, point_transforms=[mats.double()]), "point_transforms"),
        (lambda: op(boxes, rows, point_transforms=[mats[:2]]), "point_transforms"),
        (lambda: op(boxes, rows, point_transforms=[torch.zeros((B, 2, 4, 8))[..., ::2]]), "contiguous"),
        (lambda: op(boxes, rows.to("meta")), "device"),
        (lambda: op(boxes, rows, point_transforms=[mats.to("meta")]), "device"),
    ]
    for call, word in bad:
        with pytest.raises(RuntimeError, match=word):
            call()


def test_c_entries_refuse_unknown_flags_null_pointers_and_bad_counts():
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    B, N, D = 2, 3, 9
    f = lambda *s: np.zeros(s, F32)   # noqa: E731
    boxes, rows, out_boxes = f(B, N, D), f(B, 7), f(B, N, D)
    counts, source, keep, sizes = np.zeros(B, np.int32), np.zeros((B, N), np.int32), np.zeros((B, N), np.uint8), np.zeros(B, np.int64)
    mats, mats_out = f(B, 1, 4, 4), f(B, 1, 4, 4)
    p = nat.BevAugmentParams()
    ptr = lambda a: a.ctypes.data   # noqa: E731

    def both(flags=0, params=p, D=D, host_only=False, **null):
        a = dict(boxes=ptr(boxes), rows=ptr(rows), labels=None, valid=None, counts=ptr(counts), out_boxes=ptr(out_boxes),
                 out_labels=None, source=ptr(source), keep=ptr(keep), sizes=ptr(sizes))
        a.update(null)
        args = (a["boxes"], a["rows"], a["labels"], a["valid"], a["counts"], flags, B, N, D,
                ctypes.addressof(params) if params is not None else None, a["out_boxes"], a["out_labels"], a["source"], a["keep"],
                a["sizes"])
        # these are host arrays: the device entry only ever sees arguments that it refuses before a launch
        return (1 if host_only else lib.accv_bev_augment(*args, None)), lib.accv_bev_augment_host(*args)

    assert both(host_only=True)[1] == 0                             # the arguments are good: the host entry runs
    for status in (both(flags=8), both(flags=1 << 31), both(params=None), both(D=8), both(rows=None), both(counts=None),
                   both(sizes=None), both(boxes=None), both(out_boxes=None), both(source=None), both(keep=None),
                   both(labels=ptr(source)), both(flags=nat.BA_LABELS_I64), both(boxes=ptr(boxes) + 2)):
        assert status[0] != 0 and status[1] != 0, status
        assert lib.accv_last_error()
    for field, value in (("num_point_transforms", 5), ("num_frame_transforms", 3), ("num_point_transforms", -1)):
        q = nat.BevAugmentParams()
        setattr(q, field, value)
        assert all(s != 0 for s in both(params=q)), field
    q = nat.BevAugmentParams()
    q.num_point_transforms, q.point_count[0], q.point_rows[0] = 1, 1, 4           # a matrix tensor without pointers
    assert all(s != 0 for s in both(params=q))
    q.point_in[0], q.point_out[0], q.point_rows[0] = ptr(mats), ptr(mats_out), 2
    assert all(s != 0 for s in both(params=q))
    q.point_rows[0] = 4
    assert both(params=q, host_only=True)[1] == 0


# ------------------------------------------------------------------------------------------------------------- helpers
def test_bev_augmentation_params_rounds_cosine_and_sine_from_the_float32_angle():
    from accvlab.draw_heatmap import bev_augmentation_params as rows_of

    angles = [0.0, math.pi / 2, -math.pi, 1e-3, 2.5, 100.0]
    want = cases.make_rows([(a, 1.0 + 0.01 * i, (i, -i, 0.5 * i)) for i, a in enumerate(angles)])
    got = rows_of(torch.tensor(angles), torch.tensor([1.0 + 0.01 * i for i in range(6)], dtype=torch.float64),
                  torch.tensor([[i, -i, 0.5 * i] for i in range(6)], dtype=torch.float32))
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, torch.from_numpy(want))
    one = rows_of(math.pi / 2, 1.5, (0.5, 1.0, 1.5), batch_size=3)
    assert torch.equal(one, torch.from_numpy(cases.make_rows([(math.pi / 2, 1.5, (0.5, 1.0, 1.5))] * 3)))
    assert torch.equal(rows_of(0.0), torch.tensor([[0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]]))
    for bad in (lambda: rows_of("x"), lambda: rows_of(0.0, translation=(1, 2)), lambda: rows_of(torch.zeros(3), torch.zeros(2))):
        with pytest.raises(RuntimeError):
            bad()


def test_sample_bev_augmentation_ranges_disabled_parts_fixed_values_and_reproducibility():
    from accvlab.draw_heatmap import sample_bev_augmentation as sample

    B = 500
    g = torch.Generator().manual_seed(7)
    rows = sample(B, (-0.3925, 0.3925), (0.95, 1.05), (0.5, 0.25, 0.0), generator=g)
    assert rows.shape == (B, 7) and rows.dtype == torch.float32
    lo, hi = F32(-0.3925), F32(0.3925)
    assert float(rows[:, 0].min()) >= lo and float(rows[:, 0].max()) <= hi and rows[:, 0].unique().numel() > B // 2
    assert float(rows[:, 3].min()) >= F32(0.95) and float(rows[:, 3].max()) <= F32(1.05)
    assert float(rows[:, 4].abs().max()) <= 0.5 and float(rows[:, 5].abs().max()) <= 0.25 and not rows[:, 6].any()
    assert float(rows[:, 4].min()) < 0 < float(rows[:, 4].max())
    a64 = rows[:, 0].double()
    assert torch.equal(rows[:, 1], a64.cos().float()) and torch.equal(rows[:, 2], a64.sin().float())
    again = sample(B, (-0.3925, 0.3925), (0.95, 1.05), (0.5, 0.25, 0.0), generator=torch.Generator().manual_seed(7))
    assert torch.equal(rows, again)
    assert not torch.equal(rows, sample(B, (-0.3925, 0.3925), (0.95, 1.05), (0.5, 0.25, 0.0), generator=g))   # the next draws
    off = sample(4, None, None, None)
    assert torch.equal(off, torch.tensor([[0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]]).expand(4, 7))
    only_scale = sample(4, None, (0.9, 1.1), None, generator=torch.Generator().manual_seed(1))
    assert torch.equal(only_scale[:, [0, 1, 2, 4, 5, 6]], off[:, [0, 1, 2, 4, 5, 6]]) and only_scale[:, 3].unique().numel() == 4
    fixed = sample(3, (0.25, 0.25), (1.1, 1.1), (0.0, 2.0, 0.0), generator=torch.Generator().manual_seed(1))
    assert torch.equal(fixed[:, 0], torch.full((3,), 0.25)) and torch.equal(fixed[:, 3], torch.full((3,), 1.1))
    assert sample(0, (0.0, 1.0)).shape == (0, 7)
    for bad in (lambda: sample(-1), lambda: sample(2, (1.0, 0.0)), lambda: sample(2, None, None, (1.0, 2.0))):
        with pytest.raises(RuntimeError):
            bad()
