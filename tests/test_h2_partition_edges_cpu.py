"""The restatement behind test_h2_partition_edges_gpu.py, checked without a GPU: the constants read from the
kernels' source are the ones the case list was derived from, `pick_vec` / `row_launch` and the other restated host decisions
give hand-computed answers, every case sits in the regime it names (with synthetic pointers of the alignment the GPU test
carves), the accumulate cases meet the exactness condition, the oracle produces a result for every case and entry point that
differs from the untouched destination exactly where a dropped trip would leave it, and the package's CPU implementations
(pad fill, mask compaction, combine_data) agree with the oracle on the same cases."""
import numpy as np
import pytest
import torch

import h2_partition_cases as hc
from oracle import h2 as oracle

ALL_ROW_CASES = [(t, n) for t in hc.ROW_TABLES for n in hc.row_case_ids(t)]
_ids = lambda v: "-".join(v) if isinstance(v, tuple) else str(v)  # noqa: E731


def test_constants_are_the_ones_the_cases_were_derived_from():
    assert hc.CONSTANTS == hc.DERIVED_FROM
    for t in hc.ROW_TABLES:
        assert [c.name for c in hc.row_cases(t)] == hc.row_case_ids(t)


def test_pick_vec_by_hand():
    assert hc.pick_vec(48, (0x1000, 0x2000)) == 16
    assert hc.pick_vec(48, (0x1008, 0x2000)) == 8 and hc.pick_vec(48, (0x1000, 0x2004)) == 4
    assert hc.pick_vec(48, (0x1002, 0x2008)) == 2 and hc.pick_vec(48, (0x1000, 0x2001)) == 1
    assert hc.pick_vec(6, (0x1000,)) == 2 and hc.pick_vec(5, (0x1000,)) == 1 and hc.pick_vec(4100 * 4, (0, 0)) == 16
    assert hc.pick_vec(24, ()) == 8 and hc.pick_vec(12, ()) == 4


def test_row_launch_by_hand():
    r = hc.row_launch(2, 5, 1)                  # scalar rows: 256 slots of one sample per workgroup
    assert (r.lg, r.slots, r.gx, r.gy, r.sample_trips, r.vector_trips) == (0, 256, 1, 2, 1, 1)
    r = hc.row_launch(3, 65, 3)                 # 3 vectors: 4 lanes (one idle), 64 slots per group, 65 slots are two groups
    assert (r.lg, r.slots, r.gx, r.idle_lanes, r.last_group_slots) == (2, 64, 2, 1, 1)
    r = hc.row_launch(70000, 3, 1)              # the existing extremes case: 70 000 samples are two trips for 4465 rows of y
    assert (r.gy, r.sample_trips) == (65535, 2)
    r = hc.row_launch(131071, 3, 1)
    assert (r.gy, r.sample_trips) == (65535, 3) and 131071 - 2 * 65535 == 1     # the third trip is blockIdx.y == 0 alone
    r = hc.row_launch(2, 4, 1025)               # 16 400-byte rows at 16 bytes: 256 lanes, five trips
    assert (r.lg, r.slots, r.gx, r.vector_trips) == (8, 1, 4, 5)
    assert [hc.row_launch(1, 1, v).lg for v in (1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129, 256, 257)] == [0, 1, 2, 2, 3, 3, 4, 6, 7, 7, 8, 8, 8]
    assert hc.row_launch(0, 0, 1).gx == 1 and hc.row_launch(0, 0, 1).gy == 1
    assert not hc.row_launch(1, (1 << 31) * 256, 1).ok and hc.row_launch(1, ((1 << 31) - 1) * 256, 1).ok


def test_pad_fill_launch_by_hand():
    p = hc.pad_fill_launch(70000, 3, 1)         # the existing cases never stride: the span is 3 vectors ...
    assert (p.gx, p.stride_trips) == (1, 1)
    p = hc.pad_fill_launch(2, 5, 1025)          # ... or gx = 21 covers it
    assert (p.gx, p.stride_trips) == (21, 1)
    p = hc.pad_fill_launch(65536, 3, 87)
    assert (p.gx, p.gy, p.sample_trips, p.stride_trips) == (1, 65535, 2, 2)
    p = hc.pad_fill_launch(4096, 700, 3, np.array([5, 700]))
    assert (p.gx, p.stride_trips) == (4, 3) and hc.pad_fill_launch(4096, 700, 3, np.array([100, 700])).stride_trips == 2
    p = hc.pad_fill_launch(1, 4097, 1025)
    assert (p.gx, p.stride_trips) == (16384, 2)


def test_mask_regime_by_hand():
    S = 4096
    assert hc.mask_workspace_bytes(1024, 2 * S) == 1024 * 2 * 4 and hc.mask_workspace_bytes(1025, 2 * S) == 0
    assert hc.mask_workspace_bytes(8, 2 * S - 1) == 0 and hc.mask_workspace_bytes(1, 65 * S + 1) == 66 * 4
    assert hc.mask_regime(1024, 2 * S, 16, 8192)[0] == "one pass" and hc.mask_regime(1024, 2 * S)[0] == "one pass"
    assert hc.mask_regime(1025, 2 * S, 16, 1 << 20)[0] == "block<16>"
    assert hc.mask_regime(2, 4 * S + 1, 16, 40) == ("two pass", 5, False) and hc.mask_regime(2, 4 * S, 16, 40) == ("one pass", 4, True)
    assert hc.mask_regime(2, 5 * S, 0, 0)[0] == "block<16>" and hc.mask_regime(2, 5 * S, 16, 39)[0] == "block<16>"
    assert hc.mask_regime(2, 5 * S, 18, 40)[0] == "block<16>" and hc.mask_regime(2, 5 * S, 16, 40, mask_ptr=1) == ("two pass", 5, False)
    assert [hc.mask_regime(4, w)[0] for w in (512, 513, 4096, 4097, 8191)] == ["one wave", "block<4>", "block<4>", "block<16>", "block<16>"]


def test_coalesce_launch_by_hand():
    l = hc.coalesce_launch(4097, [16] * 4097, [0] * 4097, [0] * 4097)
    assert (l.grid, l.item_trips) == (4096, 2)
    l = hc.coalesce_launch(3, [4095, 4096, 4112], [0, 16, 32], [0, 0, 0])
    assert l.items == [(True, 1, 15), (True, 1, 0), (True, 2, 0)] and l.item_trips == 1
    assert hc.coalesce_launch(1, [4112], [1], [0]).items == [(False, 0, 4112)]
    assert [hc.matched_trips(p, w) for p, w in ((85, 3), (64, 4), (257, 1), (171, 3))] == [1, 1, 2, 3]


@pytest.mark.parametrize("table,name", ALL_ROW_CASES, ids=lambda v: v)
def test_every_row_case_is_in_the_regime_it_names(table, name):
    c = hc.row_case(table, name)
    so, do = getattr(c, "offsets_bytes", (0, 0))
    row_bytes = c.row * np.dtype(c.dtype).itemsize
    for entry in c.entries:
        if entry in hc.ACC_ENTRIES:
            hc.check_row_regime(c, entry)
            continue
        ptrs = (0x2000 + do,) if entry == "insert_const" else (0x1000 + so, 0x2000 + do)
        if c.k > 0 or entry in ("pack", "unpack"):
            hc.check_row_regime(c, entry, hc.pick_vec(row_bytes, ptrs))
    assert c.regime and c.counts.max() == c.k and (c.counts == 0).any() or c.batch <= 3
    if c.extra:
        junk = c.idx[:, c.k:]
        assert junk.shape[1] == 3 and ((junk >= c.width) | (junk < -c.width)).all()


@pytest.mark.parametrize("table,name", ALL_ROW_CASES, ids=lambda v: v)
def test_accumulate_cases_are_exact_in_any_order(table, name):
    c = hc.row_case(table, name)
    assert hc.assert_exact_sums(c)
    if not set(hc.ACC_ENTRIES) & set(c.entries):
        return
    for entry in hc.ACC_ENTRIES:
        want = hc.acc_want(c, entry, False)
        assert np.abs(want).max(initial=0) <= hc.ACC_MAX_ABS * hc.ACC_MAX_DUP and np.array_equal(want * 4, np.round(want * 4))
        # float64 sums of such values are exact, so they survive the narrowest type unchanged
        assert np.array_equal(torch.from_numpy(want).to(torch.bfloat16).double().numpy(), want)
        assert np.array_equal(hc.acc_want(c, entry, True), np.asarray(hc.acc_want(c, entry, True), dtype=np.int32))


def _touched_samples(c, want, before):
    return np.nonzero((want.reshape(c.batch, -1) != before.reshape(c.batch, -1)).any(1))[0]


@pytest.mark.parametrize("table,name", ALL_ROW_CASES, ids=lambda v: v)
def test_oracle_result_shows_every_marked_sample(table, name):
    """the samples on either side of every trip of the sample loop (and the first and the last) are full: for each entry the
    expected result differs there from what the destination held, so a dropped trip cannot pass"""
    c = hc.row_case(table, name)
    if c.k == 0:
        return
    marks = [s for s in c.marks if all(s != p for p, _ in c.planted["a"] + c.planted["b"])]
    for entry in c.entries:
        if entry in hc.ACC_ENTRIES:
            want = hc.acc_want(c, entry, False)
            before = np.full_like(want, hc.ACC_FILL) if entry == "accumulate" else c.acc_into_f
        else:
            want = hc.copy_want(c, entry)
            if entry in ("pack", "unpack"):
                assert c.sizes[c.marks].min() == c.width and want.shape == (c.src.shape if entry == "pack" else hc.flat_rows(c).shape)
                continue
            before = {"gather_fill": np.full_like(want, 0x3C), "gather_rows": c.out0, "scatter_rows": c.into, "map_pairs": c.into,
                      "insert_const": c.into}[entry]
        touched = _touched_samples(c, want, before)
        assert set(marks) <= set(touched.tolist()), (name, entry)


def test_gather_oracle_against_take_along_axis_on_the_largest_case():
    c = hc.row_case("sample_loop", f"batch_{2 * hc.GRID_Y + 1}")
    idx = np.where(c.idx < 0, c.idx + c.width, c.idx)
    take = np.take_along_axis(c.src, idx[:, :, None], 1)
    valid = np.arange(c.k)[None, :] < c.counts[:, None]
    assert np.array_equal(hc.copy_want(c, "gather_fill"), np.where(valid[:, :, None], take, hc.FILL[c.dtype]))
    assert hc.row_launch(c.batch, c.k, 1).sample_trips == 3 and c.counts[[0, hc.GRID_Y, 2 * hc.GRID_Y]].tolist() == [c.k] * 3


@pytest.mark.parametrize("name", hc.PAD_FILL_CASES)
def test_pad_fill_cases_and_the_cpu_implementation(name):
    from accvlab.batching_helpers import batched_indexing_access_cpu as cpu

    c = hc.pad_fill_case(name)
    hc.check_pad_fill_regime(c, 0x1000)
    if c.batch > 4:
        assert {0, c.width, -3, c.width + 5} <= set(c.counts.tolist())
    assert int(np.clip(c.counts, 0, c.width).min()) == 0
    data = torch.from_numpy(c.data.copy())
    cpu.set_ragged_batch_padded_to_filler_value_in_place(data, torch.from_numpy(c.counts), c.value)
    want = oracle.pad_fill(c.data, c.counts, c.value)
    assert np.array_equal(data.numpy().view(np.uint8), want.view(np.uint8))
    valid = np.arange(c.width)[None, :] < c.counts[:, None]
    assert np.array_equal(want[valid], c.data[valid]) and (want[~valid] == c.value).all() and c.data[~valid].any() and not c.data[~valid].all()


@pytest.mark.parametrize("name", hc.MASK_CASES)
def test_mask_cases_and_the_cpu_implementation(name):
    from accvlab.batching_helpers import bool_indexing

    c = hc.mask_case(name)
    B, W = c.mask.shape
    need = hc.mask_workspace_bytes(B, W)
    ws = {"ws": (16, need), "full": (16, need), "none": (0, 0), "short": (16, need - 1), "misaligned": (18, need)}[c.call]
    assert hc.mask_regime(B, W, ws[0], ws[1], 0x1000 + c.mask_offset) == c.regime
    want_idx, want_sizes = hc.mask_want(name)
    valid = torch.from_numpy(c.valid) if c.valid is not None else None
    idx, sizes, longest = bool_indexing._compact_indices(torch.from_numpy(c.mask), valid)
    assert longest == want_idx.shape[1] and np.array_equal(sizes.numpy(), want_sizes)
    assert np.array_equal(idx.numpy()[:, :longest], want_idx) and not idx.numpy()[:, longest:].any()
    if name == "segs_65_scan_second_trip":      # hits in the last two segments of the first scan trip and in the second trip's one
        hits = np.nonzero(c.mask[0])[0] // hc.KSEG
        assert {hc.SEG_SCAN_STEP - 2, hc.SEG_SCAN_STEP - 1, hc.SEG_SCAN_STEP} <= set(hits.tolist()) and hits.max() == hc.SEG_SCAN_STEP


@pytest.mark.parametrize("table,name", [("vector_loop", "row_vecs_257"), ("lg_groups", "rv3_k65"), ("pick_vec", "src_off_1")])
def test_pack_cases_and_combine_data(table, name):
    from accvlab.batching_helpers import combine_data

    c = hc.row_case(table, name)
    flat = torch.from_numpy(hc.flat_rows(c))
    parts = [flat[o:o + n] for o, n in zip(c.offsets.tolist(), c.sizes.tolist())]
    rb = combine_data(parts)
    assert int(c.sizes.max()) == c.width
    assert np.array_equal(rb.tensor.numpy(), hc.copy_want(c, "pack")) and np.array_equal(rb.sample_sizes.numpy(), c.sizes)
    want, sizes = oracle.combine([p.numpy() for p in parts])
    assert np.array_equal(want, hc.copy_want(c, "pack")) and np.array_equal(sizes, c.sizes)


@pytest.mark.parametrize("arrangement", list(hc.COALESCE_ARRANGEMENTS))
def test_coalesce_cases(arrangement):
    c = hc.coalesce_edges(arrangement)
    launch = hc.coalesce_launch(c.n, c.nbytes, 0x1000 + c.src_off, 0x100000 + c.dst_off)
    assert launch.items == c.expect
    want, covered = hc.coalesce_want(c)
    assert covered.sum() == c.nbytes.sum()                   # no two items overlap
    for n_items, trips in ((4096, 1), (4097, 2), (8193, 3)):
        m = hc.coalesce_many(n_items)
        assert m.item_trips == trips and hc.coalesce_want(m)[1].all() and m.nbytes[-1] == 40
