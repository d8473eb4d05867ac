"""The ragged byte movers, `coalesce_kernel` and the matched pair loss at the edges of their own work partition (DESIGN.md
§9s), on the cases of h2_partition_cases.py.  Every test first asserts that its case sits in the regime it names — the host
decision restated in h2_partition_cases.py, evaluated on the tensors' actual `data_ptr()` — and then compares with
`oracle/h2.py` or a byte-wise numpy assembly BIT FOR BIT (raw bytes; the accumulate cases are built so that every order of
the atomics gives the same sums).  Only the matched-pair-loss rows carry a tolerance: the ones of
test_matched_pair_loss_gpu.py, whose helpers they import.

A row case runs through the package's Python entry where that takes the case (default index stride, torch-allocated
results, a dtype it accepts) and through the C ABI on byte buffers carved out of a sentinel buffer otherwise (a pointer off
alignment, idx_stride > w_idx, the error counter, bool rows, the unpack direction); the margins of every carved output must
come back untouched."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import h2_partition_cases as hc
from oracle import h2 as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAD, SENT = 256, 0xA5
ACC_CODE = {"float32": 0, "float64": 1, "int32": 2, "int64": 3, "float16": 4, "bfloat16": 5}


def _nat():
    from accvlab import _amd_native as nat

    return nat


def _ext():
    from accvlab.batching_helpers import batched_indexing_access_cuda as ext

    return ext


def _raw(t):
    """the bytes of a CPU tensor"""
    return t.contiguous().reshape(-1).view(torch.uint8)


def _bytes(t):
    return _raw(t.cpu()).numpy()


class Carved:
    """a copy of CPU tensor `t` inside a sentinel-filled device buffer, `off` bytes off the buffer's 256-byte alignment"""

    def __init__(self, t, off=0):
        raw = _raw(t)
        self.n, self.start = raw.numel(), PAD + off
        self.buf = torch.full((self.n + 2 * PAD + 16,), SENT, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.buf[self.start:self.start + self.n] = raw.to(DEV)
        self.ptr = self.buf.data_ptr() + self.start

    def bytes(self):
        return self.buf[self.start:self.start + self.n].cpu().numpy()

    def clean(self):
        return bool((self.buf[:self.start] == SENT).all()) and bool((self.buf[self.start + self.n:] == SENT).all())


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(getattr(torch, dtype))


def _check(status, what):
    _nat().check(status, what)


# ------------------------------------------------------------------------------------------- row kernels
@functools.lru_cache(maxsize=None)
def _copy_want(table, name, entry):
    return _bytes(_t(hc.copy_want(hc.row_case(table, name), entry)))


@functools.lru_cache(maxsize=None)
def _acc_want(table, name, entry, integer):
    return hc.acc_want(hc.row_case(table, name), entry, integer)


def _python_route(c, entry):
    if c.extra or hasattr(c, "offsets_bytes") or c.planted["a"] or entry == "unpack":
        return False
    return c.dtype != "bool" or entry in ("gather_rows", "scatter_rows", "pack")


def _run_copy_python(c, entry):
    """-> (result bytes, base pointers the vector width was picked from)"""
    ext = _ext()
    k = c.k
    idx, idx_b, counts = _t(c.idx).to(DEV), _t(c.idx_b).to(DEV), _t(c.counts).to(DEV)
    if entry == "gather_fill":
        src = _t(c.src).to(DEV)
        res = ext.forward(src, idx, counts, hc.FILL[c.dtype])
        return _bytes(res), (src.data_ptr(), res.data_ptr())
    if entry == "gather_rows":
        src, out = _t(c.src).to(DEV), _t(c.out0).to(DEV)
        ext.gather_rows(src, idx, counts, k, out)
        return _bytes(out), (src.data_ptr(), out.data_ptr())
    if entry == "scatter_rows":
        src, dst = _t(c.ins).to(DEV), _t(c.into).to(DEV)
        ext.scatter_rows(src, idx, counts, k, dst)
        return _bytes(dst), (src.data_ptr(), dst.data_ptr())
    if entry == "map_pairs":
        src = _t(c.src).to(DEV)
        res = ext.map_values_by_index_pairs(src, idx, idx_b, counts, _t(c.into).to(DEV))
        return _bytes(res), (src.data_ptr(), res.data_ptr())
    if entry == "insert_const":
        res = ext.backward_insert_const(hc.FILL[c.dtype], idx, counts, _t(c.into).to(DEV))
        return _bytes(res), (res.data_ptr(),)
    assert entry == "pack"
    flat = _t(hc.flat_rows(c)).to(DEV)
    res = ext.pack_rows(flat, _t(c.offsets).to(DEV), _t(c.sizes).to(DEV), c.width)
    return _bytes(res), (flat.data_ptr(), res.data_ptr())


def _run_copy_cabi(c, entry, err=None):
    """-> (result bytes, base pointers, margins clean)"""
    nat, lib = _nat(), _nat().lib()
    s = nat.stream_ptr(DEV)
    so, do = getattr(c, "offsets_bytes", (0, 0))
    B, W, k, stride = c.batch, c.width, c.k, c.k + c.extra
    esz = np.dtype(c.dtype).itemsize
    rb = c.row * esz
    i64 = int(c.idx_dtype == np.int64)
    idx, idx_b, counts = Carved(_t(c.idx)), Carved(_t(c.idx_b)), Carved(_t(c.counts))
    bits = _ext().element_bits(hc.FILL[c.dtype], getattr(torch, c.dtype))
    ep = err.data_ptr() if err is not None else None
    garbage = lambda a: _t(np.full(a.nbytes, 0x3C, dtype=np.uint8))  # noqa: E731   (what an uninitialised result holds)
    if entry == "gather_fill":
        src, dst = Carved(_t(c.src), so), Carved(garbage(c.out0), do)
        _check(lib.accv_ragged_gather_fill(src.ptr, dst.ptr, idx.ptr, counts.ptr, B, W, k, stride, rb, bits, esz, i64, 1, ep, s), entry)
    elif entry == "gather_rows":
        src, dst = Carved(_t(c.src), so), Carved(_t(c.out0), do)
        _check(lib.accv_ragged_gather(src.ptr, dst.ptr, idx.ptr, counts.ptr, B, W, k, stride, rb, i64, 1, ep, s), entry)
    elif entry == "scatter_rows":
        src, dst = Carved(_t(c.ins), so), Carved(_t(c.into), do)
        _check(lib.accv_ragged_scatter(src.ptr, dst.ptr, idx.ptr, counts.ptr, B, k, stride, W, rb, i64, 1, ep, s), entry)
    elif entry == "map_pairs":
        src, dst = Carved(_t(c.src), so), Carved(_t(c.into), do)
        _check(lib.accv_ragged_map_pairs(src.ptr, dst.ptr, idx.ptr, idx_b.ptr, counts.ptr, B, W, k, stride, W, rb, i64, 1, ep, s), entry)
    elif entry == "insert_const":
        src, dst = None, Carved(_t(c.into), do)
        _check(lib.accv_ragged_insert_const(dst.ptr, idx.ptr, counts.ptr, B, k, stride, W, rb, bits, esz, i64, 1, ep, s), entry)
    else:
        offs, sizes = Carved(_t(c.offsets)), Carved(_t(c.sizes))
        flat_np = hc.flat_rows(c)
        if entry == "pack":
            src, dst = Carved(_t(flat_np), so), Carved(garbage(c.src), do)
            _check(lib.accv_ragged_pack(src.ptr, dst.ptr, offs.ptr, sizes.ptr, B, W, rb, 0, s), entry)
        else:
            src, dst = Carved(_t(c.src), so), Carved(garbage(flat_np), do)
            _check(lib.accv_ragged_pack(dst.ptr, src.ptr, offs.ptr, sizes.ptr, B, W, rb, 1, s), entry)
    torch.cuda.synchronize()
    return dst.bytes(), tuple(p.ptr for p in (src, dst) if p is not None), dst.clean()


def _run_acc(c, entry, dtype, python, err=None):
    """-> (result bytes, margins clean or None); `elem_off`: the destination starts that many elements into its buffer"""
    integer = dtype.startswith("int")
    src_v, ins_v, into_v = (c.acc_src_i, c.acc_ins_i, c.acc_into_i) if integer else (c.acc_src_f, c.acc_ins_f, c.acc_into_f)
    B, W, k, stride = c.batch, c.width, c.k, c.k + c.extra
    if python:
        ext = _ext()
        idx, idx_b, idx_dup, counts = (_t(a).to(DEV) for a in (c.idx, c.idx_b, c.idx_dup, c.counts))
        if entry == "accumulate":
            res = ext.backward_new_tensor(_t(ins_v, dtype).to(DEV), idx_dup, counts, W, hc.ACC_FILL, True)
        else:
            res = ext.map_values_by_index_pairs(_t(src_v, dtype).to(DEV), idx, idx_b, counts, _t(into_v, dtype).to(DEV), True)
        return _bytes(res), None
    nat, lib = _nat(), _nat().lib()
    s = nat.stream_ptr(DEV)
    esz = torch.empty((), dtype=getattr(torch, dtype)).element_size()
    i64 = int(c.idx_dtype == np.int64)
    idx, idx_b, idx_dup, counts = (Carved(_t(a)) for a in (c.idx, c.idx_b, c.idx_dup, c.counts))
    ep = err.data_ptr() if err is not None else None
    elem_off = getattr(c, "elem_off", 0)
    if entry == "accumulate":
        src = Carved(_t(ins_v, dtype))
        dst = Carved(torch.full((B, W, c.acc_row), hc.ACC_FILL, dtype=getattr(torch, dtype)), elem_off * esz)
        a_idx, b_idx, w_src = None, idx_dup.ptr, k
    else:
        src = Carved(_t(src_v, dtype))
        dst = Carved(_t(into_v, dtype), elem_off * esz)
        a_idx, b_idx, w_src = idx.ptr, idx_b.ptr, W
    _check(lib.accv_ragged_insert_const(dst.ptr, b_idx, counts.ptr, B, k, stride, W, c.acc_row * esz, 0, esz, i64, 1, None, s), entry)
    _check(lib.accv_ragged_accumulate(src.ptr, dst.ptr, a_idx, b_idx, counts.ptr, B, w_src, k, stride, W, c.acc_row, ACC_CODE[dtype],
                                      i64, 1, ep, s), entry)
    torch.cuda.synchronize()
    return dst.bytes(), dst.clean()


def _row_test(table, name, entry):
    c = hc.row_case(table, name)
    assert entry in c.entries
    planted = hc.planted_errors(c, entry)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if c.planted["a"] else None
    if entry in hc.ACC_ENTRIES:
        hc.assert_exact_sums(c)
        hc.check_row_regime(c, entry)
        for dtype in hc.ACC_DTYPES:
            if err is not None:
                err.zero_()
            got, clean = _run_acc(c, entry, dtype, _python_route(c, entry), err)
            want = _bytes(_t(_acc_want(table, name, entry, dtype.startswith("int")), dtype))
            assert np.array_equal(got, want), f"{c.name} ({c.regime}) {entry} {dtype}"
            assert clean in (None, True), f"{c.name} {entry} {dtype}: wrote outside the destination"
            if err is not None:
                assert int(err.item()) == planted, f"{c.name} {entry} {dtype}: counted {int(err.item())} of {planted} planted"
        return
    if _python_route(c, entry):
        got, ptrs = _run_copy_python(c, entry)
        clean = True
    else:
        got, ptrs, clean = _run_copy_cabi(c, entry, err)
    row_bytes = c.row * np.dtype(c.dtype).itemsize
    if c.k > 0 or entry in ("pack", "unpack"):
        hc.check_row_regime(c, entry, hc.pick_vec(row_bytes, ptrs))
    assert np.array_equal(got, _copy_want(table, name, entry)), f"{c.name} ({c.regime}) {entry}"
    assert clean, f"{c.name} {entry}: wrote outside the destination"
    if err is not None:
        assert int(err.item()) == planted, f"{c.name} {entry}: counted {int(err.item())} of {planted} planted"


def _row_params(table, entries=hc.COPY_ENTRIES + hc.ACC_ENTRIES):
    return [pytest.param(table, n, e, id=f"{n}-{e}") for n in hc.row_case_ids(table) for e in entries]


@pytest.mark.parametrize("table,name,entry", _row_params("sample_loop"))
def test_sample_loop(table, name, entry):
    """`i += gridDim.y`: 65 535 samples are one trip, 65 536 put sample 65 535 alone into a second, 131 071 give
    blockIdx.y == 0 a third"""
    _row_test(table, name, entry)


@pytest.mark.parametrize("table,name,entry", _row_params("vector_loop"))
def test_vector_loop(table, name, entry):
    """`v += lanes`: 255 / 256 / 257 / 513 vectors (elements) per row around the 256 lanes of a row"""
    _row_test(table, name, entry)


@pytest.mark.parametrize("table,name,entry", _row_params("lg_groups"))
def test_lanes_per_row_and_slot_groups(table, name, entry):
    """every lg, with idle lanes inside a row (row_vecs off a power of two) and a full, a short and a one-slot last group"""
    _row_test(table, name, entry)


@pytest.mark.parametrize("table,name,entry", _row_params("pick_vec", hc.COPY_ENTRIES))
def test_pick_vec_by_pointer(table, name, entry):
    """48-byte rows demoted to 8 / 4 / 2 / 1-byte vectors by the source pointer alone, then by the destination pointer alone"""
    _row_test(table, name, entry)


@pytest.mark.parametrize("table,name,entry", _row_params("idx_stride", hc.INDEXED_COPY_ENTRIES + hc.ACC_ENTRIES))
def test_idx_stride_wider_than_w_idx(table, name, entry):
    """three more index columns than slots, filled with out-of-range values no kernel may read as an index"""
    _row_test(table, name, entry)


@pytest.mark.parametrize("table,name,entry", _row_params("oor", hc.INDEXED_COPY_ENTRIES + hc.ACC_ENTRIES))
def test_out_of_range_indices_in_a_second_trip(table, name, entry):
    """an index too large and one still negative after wrapping are skipped and counted once each, beside negative indices
    that wrap into range"""
    _row_test(table, name, entry)


# ------------------------------------------------------------------------------------------- accumulate, 16 bit
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("elem_off", [0, 1], ids=["even_start", "odd_start"])
@pytest.mark.parametrize("entry", hc.ACC_ENTRIES)
def test_accumulate_16bit_word_halves(entry, elem_off, dtype):
    """`atomic_add_16` works on the containing 32-bit word: rows of 257 elements (odd: consecutive rows start on alternating
    halves), duplicates on both halves of one word, and a destination that starts on an odd 16-bit element so that its first
    and last word reach into the neighbours' bytes, which must come back unchanged"""
    c = hc.row_case("vector_loop", "row_vecs_257")
    assert c.acc_row == 257 and hc.assert_exact_sums(c)
    rl = hc.check_row_regime(c, entry)
    assert rl.vector_trips == 2
    c16 = SimpleNamespace(**{**vars(c), "elem_off": elem_off})
    got, clean = _run_acc(c16, entry, dtype, python=False)
    want = _bytes(_t(_acc_want("vector_loop", "row_vecs_257", entry, False), dtype))
    valid = np.arange(c.k)[None, :] < c.counts[:, None]
    t = np.where(c.idx_dup < 0, c.idx_dup + c.width, c.idx_dup) if entry == "accumulate" else np.where(c.idx_b < 0, c.idx_b + c.width, c.idx_b)
    hit = np.bincount((np.arange(c.batch)[:, None] * c.width + t)[valid], minlength=c.batch * c.width)
    assert entry != "accumulate" or hit.max() >= 2          # a contended row: both halves of each of its words
    assert np.array_equal(got.view(np.int16), want.view(np.int16)), f"{entry} {dtype} element offset {elem_off}"
    assert clean, f"{entry} {dtype} element offset {elem_off}: the neighbours' bytes changed"


# ------------------------------------------------------------------------------------------- pad fill
@functools.lru_cache(maxsize=None)
def _pad_fill_want(name):
    c = hc.pad_fill_case(name)
    return _bytes(_t(oracle.pad_fill(c.data, c.counts, c.value)))


@pytest.mark.parametrize("name", hc.PAD_FILL_CASES)
def test_pad_fill_stride_loop(name):
    """`v += step`: the workgroups of a sample capped by the sample count (gx 1 and 4) and by the 16 384 cap, second and third
    trip; counts of 0, the width, and outside [0, width] on both sides where the batch has room for them"""
    c = hc.pad_fill_case(name)
    data = _t(c.data).to(DEV)
    hc.check_pad_fill_regime(c, data.data_ptr())
    _ext().set_ragged_batch_padded_to_filler_value_in_place(data, _t(c.counts).to(DEV), c.value)
    assert np.array_equal(_bytes(data), _pad_fill_want(name)), f"{name}"


@pytest.mark.parametrize("counts_i64", [1, 0])
def test_pad_fill_clamps_the_count(counts_i64):
    """`min(max(count, 0), width)` through the C ABI, int32 and int64 counts; the margins stay clean"""
    width, row = 6, 3
    counts = np.array([0, width, -3, width + 5], dtype=np.int64 if counts_i64 else np.int32)
    data = np.random.default_rng(5).integers(1, 1000, (4, width, row)).astype(np.float32)
    d, n = Carved(_t(data)), Carved(_t(counts))
    bits = _ext().element_bits(-10.0, torch.float32)
    _check(_nat().lib().accv_ragged_pad_fill(d.ptr, n.ptr, 4, width, row * 4, bits, 4, counts_i64, _nat().stream_ptr(DEV)), "pad fill")
    torch.cuda.synchronize()
    want = oracle.pad_fill(data, counts, np.float32(-10.0))
    assert np.array_equal(want[1], data[1]) and np.all(want[2] == -10) and np.array_equal(want[3], data[3])
    assert np.array_equal(d.bytes(), _bytes(_t(want))) and d.clean()


# ------------------------------------------------------------------------------------------- mask -> indices
@pytest.mark.parametrize("name", hc.MASK_CASES)
def test_mask_to_indices_regimes(name):
    """every branch of the regime decision of accv_ragged_mask_to_indices_ws, the published workspace size against the
    restated one, the result (indices, zero tail, sizes) against the oracle"""
    nat, lib = _nat(), _nat().lib()
    c = hc.mask_case(name)
    B, W = c.mask.shape
    need = lib.accv_ragged_mask_to_indices_workspace_bytes(B, W)
    assert need == hc.mask_workspace_bytes(B, W)
    mask = Carved(_t(c.mask), c.mask_offset)
    valid = _t(c.valid).to(DEV) if c.valid is not None else None
    idx = torch.full((B, W), -1, dtype=torch.int64, device=DEV)
    sizes = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    vp = valid.data_ptr() if valid is not None else None
    s = nat.stream_ptr(DEV)
    ws = torch.empty(need + 32, dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = {"ws": (ws.data_ptr(), need), "full": (ws.data_ptr(), need), "none": (0, 0), "short": (ws.data_ptr(), need - 1),
                        "misaligned": (ws.data_ptr() + 2, need)}[c.call]
    if need == 0:
        ws_ptr, ws_bytes = 0, 0
    assert hc.mask_regime(B, W, ws_ptr, ws_bytes, mask.ptr) == c.regime, f"{name}: not in its regime"
    if c.call == "none":
        _check(lib.accv_ragged_mask_to_indices(mask.ptr, vp, 1, B, W, idx.data_ptr(), sizes.data_ptr(), s), name)
    else:
        _check(lib.accv_ragged_mask_to_indices_ws(mask.ptr, vp, 1, B, W, idx.data_ptr(), sizes.data_ptr(), ws_ptr or None, ws_bytes, s), name)
    want_idx, want_sizes = hc.mask_want(name)
    longest = want_idx.shape[1]
    got = idx.cpu().numpy()
    assert np.array_equal(sizes.cpu().numpy(), want_sizes), f"{name}: sizes"
    assert np.array_equal(got[:, :longest], want_idx), f"{name}: indices"
    assert not got[:, longest:].any(), f"{name}: zero tail"


# ------------------------------------------------------------------------------------------- accv_mtc_coalesce
def _coalesce(c, check_expect=None):
    """gather into a carved `packed`, then scatter from it into a fresh carved buffer"""
    nat, lib = _nat(), _nat().lib()
    s = nat.stream_ptr(DEV)
    src = Carved(_t(c.data))
    packed = Carved(torch.full((c.total,), 0x11, dtype=torch.uint8))
    items = torch.from_numpy(np.stack([src.ptr + c.src_off, c.dst_off, c.nbytes], 1).astype(np.int64)).to(DEV)
    launch = hc.coalesce_launch(c.n, c.nbytes, src.ptr + c.src_off, packed.ptr + c.dst_off)
    if check_expect is not None:
        assert launch.items == check_expect, launch.items
    _check(lib.accv_mtc_coalesce(items.data_ptr(), c.n, packed.ptr, 0, s), "coalesce")
    torch.cuda.synchronize()
    want, covered = hc.coalesce_want(c)
    assert np.array_equal(packed.bytes(), np.where(covered, want, 0x11)), "gathered bytes"
    assert packed.clean() and src.clean()
    back = Carved(torch.full((len(c.data),), 0x22, dtype=torch.uint8))
    items2 = torch.from_numpy(np.stack([back.ptr + c.src_off, c.dst_off, c.nbytes], 1).astype(np.int64)).to(DEV)
    _check(lib.accv_mtc_coalesce(items2.data_ptr(), c.n, packed.ptr, 1, s), "coalesce, scatter")
    torch.cuda.synchronize()
    in_item = np.zeros(len(c.data), dtype=bool)
    for o, n in zip(c.src_off, c.nbytes):
        in_item[o:o + n] = True
    assert np.array_equal(back.bytes(), np.where(in_item, c.data, 0x22)), "scattered bytes"
    assert back.clean() and packed.clean()
    assert np.array_equal(packed.bytes(), np.where(covered, want, 0x11)), "scatter changed the packed buffer"
    return launch


@pytest.mark.parametrize("n_items,trips", [(hc.COALESCE_GRID_CAP, 1), (hc.COALESCE_GRID_CAP + 1, 2), (2 * hc.COALESCE_GRID_CAP + 1, 3)])
def test_coalesce_item_loop(n_items, trips):
    """`it += gridDim.x`: 4096 items are one trip, 4097 give block 0 a second, 8193 a third; both directions"""
    c = hc.coalesce_many(n_items)
    launch = _coalesce(c)
    assert (launch.grid, launch.item_trips) == (hc.COALESCE_GRID_CAP, trips)


@pytest.mark.parametrize("arrangement", list(hc.COALESCE_ARRANGEMENTS))
def test_coalesce_vector_loop_and_tails(arrangement):
    """items of 0 .. 4112 bytes: n16 of 255 / 256 / 257 (the vector loop's second trip), byte tails of 1 and 15, and the byte
    path alone when the source or the destination is off 16 bytes; both directions"""
    c = hc.coalesce_edges(arrangement)
    launch = _coalesce(c, c.expect)
    if arrangement == "aligned":
        assert sorted({t for _, t, _ in launch.items}) == [0, 1, 2] and {15, 1} <= {b for _, _, b in launch.items}


# ------------------------------------------------------------------------------------------- matched pair loss
_MATCHED_SHAPES = {255: (85, 3), 256: (64, 4), 257: (257, 1), 513: (171, 3)}     # pairs x inner (or classes)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("total", hc.MATCHED_TOTALS)
@pytest.mark.parametrize("kind", hc.MATCHED_KINDS)
def test_matched_pair_loss_thread_loop(kind, total, dtype):
    """`t += 256` of matched_reduce_kernel and its backward: pairs x inner of 255 / 256 / 257 / 513 in sample 0 (fewer in the
    others), every kind, float32 and float16.  Forward against oracle.h2.gather + the loss in float64 numpy, gradients against
    float64 autograd over the same formulation, at the tolerances of test_matched_pair_loss_gpu.py"""
    import accvlab.batching_helpers as bh
    import test_matched_pair_loss_gpu as mp

    beta, eps = 0.5, 1e-6
    pairs, inner = (total, 1) if kind == "iou_xyxy" else _MATCHED_SHAPES[total]
    work = 1 if kind == "iou_xyxy" else inner
    assert pairs * work == total and hc.matched_trips(pairs, work) == -(-total // hc.MATCHED_THREADS)
    B, na, nb = 3, pairs + 3, pairs + 7
    if kind == "iou_xyxy":
        a, b, w, ia, ib, counts = mp._box_case(total, B, na, nb, pairs)
    else:
        a, b, w, ia, ib, counts, _ = mp._case(total, b=B, na=na, nb=nb, k=pairs, inner=(inner,))
    assert int(counts[0]) == pairs
    g = np.random.default_rng(total)
    labels = g.integers(0, inner, size=(B, na)) if kind == "onehot_l1" else None
    if kind == "onehot_l1":
        b = g.uniform(0.05, 0.95, size=b.shape).astype(np.float32)   # no score equal to its target: |.| has no kink there
    ta, tb, tw = (torch.from_numpy(x).to(DEV).to(dtype) for x in (a, b, w))
    a64, b64, w64 = (t.double().cpu().numpy() for t in (ta, tb, tw))       # the values the kernel sees
    K = ia.shape[1]
    valid = np.arange(K)[None, :] < counts[:, None]
    gb, gw = oracle.gather(b64, ib, counts, 0.0), oracle.gather(w64, ia, counts, 0.0)
    if kind == "onehot_l1":
        glab = oracle.gather(labels, ia, counts, 0)
        per = np.abs((np.arange(inner)[None, None, :] == glab[..., None]).astype(np.float64) - gb).sum(-1)
    elif kind == "iou_xyxy":
        per = mp._iou_loss_np(oracle.gather(a64, ia, counts, 0.0), gb, eps)
    else:
        per = mp._loss_np(oracle.gather(a64, ia, counts, 0.0) - gb, kind, beta).sum(-1)
    want = np.where(valid, per * gw, 0.0).sum(1)
    ra = bh.RaggedBatch(torch.from_numpy(ia).to(DEV), sample_sizes=torch.from_numpy(counts).to(DEV))
    rbb = bh.RaggedBatch(torch.from_numpy(ib).to(DEV), sample_sizes=torch.from_numpy(counts).to(DEV))
    ta.requires_grad_(kind != "onehot_l1"), tb.requires_grad_(True), tw.requires_grad_(True)
    first = torch.from_numpy(labels).to(DEV) if kind == "onehot_l1" else ta
    out = bh.matched_pair_loss_sum(first, tb, ra, rbb, tw, kind=kind, beta=beta, eps=eps)
    fwd_tol = 1e-5 if dtype == torch.float32 and kind in ("l1", "l2", "smooth_l1") else 2e-5
    assert float(np.abs(out.detach().cpu().numpy() - want).max()) <= fwd_tol * max(1.0, float(np.abs(want).max()))
    up = torch.linspace(0.5, 1.5, B, device=DEV, dtype=out.dtype)
    (out * up).sum().backward()
    # float64 autograd over the same formulation
    ca, cb, cw = (torch.from_numpy(x).to(DEV).requires_grad_(True) for x in (a64, b64, w64))
    wrap = lambda i, n: torch.from_numpy(np.where(valid, np.where(i < 0, i + n, i), 0)).to(DEV)  # noqa: E731
    idx_a, idx_b = wrap(ia, na), wrap(ib, nb)
    take = lambda t, i: torch.gather(t, 1, i.reshape(i.shape + (1,) * (t.dim() - 2)).expand(i.shape + t.shape[2:]))  # noqa: E731
    g2 = take(cb, idx_b)
    if kind == "onehot_l1":
        onehot = (torch.arange(inner, device=DEV)[None, None, :] == take(torch.from_numpy(labels).to(DEV), idx_a)[..., None]).double()
        l = (onehot - g2).abs().sum(-1)
    elif kind == "iou_xyxy":
        l = mp._iou_loss_torch(take(ca, idx_a), g2, eps)
    else:
        g1 = take(ca, idx_a)
        d = g1 - g2
        l = (d.abs() if kind == "l1" else d * d if kind == "l2"
             else torch.nn.functional.smooth_l1_loss(g1, g2, beta=beta, reduction="none")).sum(-1)
    ref = (l * take(cw, idx_a) * torch.from_numpy(valid).to(DEV)).sum(1)
    assert float((out.detach().double() - ref.detach()).abs().max()) <= fwd_tol * max(1.0, float(ref.detach().abs().max()))
    (ref * up.double()).sum().backward()
    tol = mp._TOL[dtype]
    grads = [(tb.grad, cb.grad), (tw.grad, cw.grad)] + ([(ta.grad, ca.grad)] if kind != "onehot_l1" else [])
    for got, exp in grads:
        assert got.dtype == dtype
        assert float((got.double() - exp).abs().max()) <= tol * max(1.0, float(exp.abs().max())), f"{kind} {total} {dtype}"


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_are_error_returns():
    """limits that no test can cross in seconds are checked as refusals: idx_stride < w_idx, a negative extent, a vector
    width below the filler's element size; the row kernels' `gx > 2^31 - 1` needs 2^31 index slots and is reached by no test"""
    lib = _nat().lib()
    t = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    assert lib.accv_ragged_gather(p, p, p, p, 1, 2, 2, 1, 4, 1, 1, None, None) != 0                 # stride below the slots
    assert lib.accv_ragged_pad_fill(p, p, -1, 2, 4, 0, 4, 1, None) != 0
    assert lib.accv_ragged_gather_fill(p + 2, p + 16, p + 32, p + 48, 1, 1, 1, 1, 4, 0, 4, 1, 1, None, None) != 0   # 2-byte aligned float32
    assert lib.accv_ragged_accumulate(p, p, None, p, p, 1, 1, 1, 1, 1, 1, 6, 1, 1, None, None) != 0  # dtype code
    assert lib.accv_mtc_coalesce(p, -1, p, 0, None) != 0
    assert hc.row_launch(1, (hc.GRID_X_MAX + 1) * hc.THREADS, 1).ok is False and hc.row_launch(1, hc.GRID_X_MAX * hc.THREADS, 1).ok
