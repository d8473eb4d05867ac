"""Inputs at the edges of the work partition of the ragged byte movers (`csrc/ragged_ops.hip`), of `coalesce_kernel`
(`csrc/tensor_copier.hip`) and of the matched pair loss (`csrc/matched_loss.hip`), shared by
test_h2_partition_edges_cpu.py (the restatement, the regimes, the exactness condition, the package's CPU paths) and
test_h2_partition_edges_gpu.py (the kernels).  DESIGN.md §9s has the tables.

Every constant a shape is derived from is read from the source text, so that a changed constant moves the cases or fails
here.  The host decisions are restated in plain Python (`pick_vec`, `row_launch`, `pad_fill_launch`, `mask_regime`,
`coalesce_launch`); every case names the regime it is for in `expect`, and the tests compare that with the restatement
evaluated on the case's actual tensors.  Inputs are seeded, not hand-written: byte movers are compared bit for bit, and
random bytes make every row different from every other and from what the destination held before."""
import os
import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "accv-lab_amd", "csrc")


def _read(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _one(pattern, text, group=1):
    """the single value every match of `pattern` agrees on"""
    found = {m if isinstance(m, str) else m[group - 1] for m in re.findall(pattern, text)}
    assert len(found) == 1, (pattern, found)
    return int(found.pop(), 0)


_RAG = _read("ragged_ops.hip")
_COP = _read("tensor_copier.hip")
_ML = _read("matched_loss.hip")

THREADS = _one(r"__launch_bounds__\((\d+)\)", _RAG)                       # every row kernel, pad fill, the segment kernels
assert _one(r"rows_per_block = (\d+) >> lg", _RAG) == THREADS and _one(r"\(long long\)blockIdx\.x \* \((\d+) >> g\.lg\)", _RAG) == THREADS
LG_MAX = _one(r"while \(lg < (\d+) && \(1ll << lg\) < row_vecs\)", _RAG)
assert 1 << LG_MAX == THREADS
GRID_Y = _one(r"batch < (\d+) \? \(batch > 0 \? batch : 1\) : \d+", _RAG)     # y extent of the row kernels' grid
assert _one(r"batch < \d+ \? \(batch > 0 \? batch : 1\) : (\d+)", _RAG) == GRID_Y
assert _one(r"gy = batch < (\d+) \? batch : \d+;", _RAG) == GRID_Y and _one(r"gy = batch < \d+ \? batch : (\d+);", _RAG) == GRID_Y
GRID_X_MAX = _one(r"r\.ok = gx <= (0x[0-9a-f]+)ll;", _RAG)
PAD_FILL_CAP = _one(r"long long gx = (\d+) / gy;", _RAG)                  # workgroups of one pad-fill launch
assert _one(r"span_blocks = \(width \* row_vecs \+ (\d+)\) / \d+;", _RAG) == THREADS - 1
KSEG = _one(r"constexpr int kSeg = (\d+);", _RAG)
ONE_PASS_SEGS = _one(r"constexpr int kOnePassSegs = (\d+);", _RAG)
SEG_BATCH_MAX = _one(r"width < 2 \* kSeg \|\| batch > (\d+)\) return 0;", _RAG)
SEG_GRID_MAX = _one(r"segs > (\d+) \|\| batch > \d+\) return 0;", _RAG)
MASK_BLOCK_WIDTH = _one(r"if \(width > (\d+) && batch <= 0x7fffffff\)", _RAG)   # above: a workgroup per row
MASK_BLOCK16_WIDTH = _one(r"if \(width > (\d+)\)\s+hipLaunchKernelGGL\(\(mask_to_indices_block_kernel<16>\)", _RAG)
SEG_SCAN_STEP = _one(r"for \(int s0 = 0; s0 < segs; s0 \+= (\d+)\)", _RAG)   # segment counts one wave sums per trip
_m = re.search(r"std::min<long long>\(n_items, (\d+) \* (\d+)\)", _COP)
COALESCE_GRID_CAP = int(_m.group(1)) * int(_m.group(2))
COALESCE_THREADS = _one(r"__launch_bounds__\((\d+)\) void coalesce_kernel", _COP)
MATCHED_THREADS = _one(r"for \(long long t = threadIdx\.x; t < total; t \+= (\d+)\)", _ML)
# the values the case lists below were derived from: a change here must be followed by a look at every case
CONSTANTS = dict(THREADS=THREADS, LG_MAX=LG_MAX, GRID_Y=GRID_Y, GRID_X_MAX=GRID_X_MAX, PAD_FILL_CAP=PAD_FILL_CAP, KSEG=KSEG,
                 ONE_PASS_SEGS=ONE_PASS_SEGS, SEG_BATCH_MAX=SEG_BATCH_MAX, SEG_GRID_MAX=SEG_GRID_MAX,
                 MASK_BLOCK_WIDTH=MASK_BLOCK_WIDTH, MASK_BLOCK16_WIDTH=MASK_BLOCK16_WIDTH, SEG_SCAN_STEP=SEG_SCAN_STEP,
                 COALESCE_GRID_CAP=COALESCE_GRID_CAP, COALESCE_THREADS=COALESCE_THREADS, MATCHED_THREADS=MATCHED_THREADS)
DERIVED_FROM = dict(THREADS=256, LG_MAX=8, GRID_Y=65535, GRID_X_MAX=0x7fffffff, PAD_FILL_CAP=16384, KSEG=4096, ONE_PASS_SEGS=4,
                    SEG_BATCH_MAX=1024, SEG_GRID_MAX=65535, MASK_BLOCK_WIDTH=512, MASK_BLOCK16_WIDTH=4096, SEG_SCAN_STEP=64,
                    COALESCE_GRID_CAP=4096, COALESCE_THREADS=256, MATCHED_THREADS=256)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- the host decisions, restated
def pick_vec(row_bytes, pointers):
    """vector bytes of a copy: the widest of 16 / 8 / 4 / 2 / 1 that divides the row size and every base pointer"""
    bits = int(row_bytes)
    for p in pointers:
        bits |= int(p)
    for vb in (16, 8, 4, 2):
        if bits % vb == 0:
            return vb
    return 1


def row_launch(batch, width, row_vecs):
    """row_launch: lg (2^lg lanes per row), slots of one sample per workgroup, grid (gx, gy), trips of the sample loop of
    blockIdx.y == 0 and trips of a lane's vector loop"""
    lg = 0
    while lg < LG_MAX and (1 << lg) < row_vecs:
        lg += 1
    slots = THREADS >> lg
    gx = _cdiv(width, slots)
    gy = min(max(batch, 1), GRID_Y)
    return SimpleNamespace(lg=lg, lanes=1 << lg, slots=slots, gx=max(gx, 1), gy=gy, ok=gx <= GRID_X_MAX,
                           sample_trips=_cdiv(batch, gy), vector_trips=_cdiv(row_vecs, 1 << lg),
                           idle_lanes=(1 << lg) - min(row_vecs, 1 << lg), last_group_slots=width - (max(gx, 1) - 1) * slots)


def pad_fill_launch(batch, width, row_vecs, counts=None):
    """accv_ragged_pad_fill: grid (gx, gy) and the trips of the stride loop `v += step` of the sample with the longest
    padding (count clamped to [0, width])"""
    gy = min(batch, GRID_Y)
    span_blocks = _cdiv(width * row_vecs, THREADS)
    gx = min(span_blocks, max(1, PAD_FILL_CAP // gy))
    c = 0 if counts is None else int(np.clip(np.asarray(counts), 0, width).min())
    return SimpleNamespace(gx=gx, gy=gy, sample_trips=_cdiv(batch, gy), stride_trips=_cdiv((width - c) * row_vecs, gx * THREADS))


def mask_workspace_bytes(batch, width):
    """accv_ragged_mask_to_indices_workspace_bytes"""
    if batch <= 0 or width < 2 * KSEG or batch > SEG_BATCH_MAX:
        return 0
    segs = _cdiv(width, KSEG)
    if segs > SEG_GRID_MAX or batch > SEG_GRID_MAX:
        return 0
    return batch * segs * 4


def mask_regime(batch, width, workspace_ptr=0, workspace_bytes=0, mask_ptr=0):
    """(kernel family, segments, 16-byte loads) of accv_ragged_mask_to_indices_ws"""
    need = mask_workspace_bytes(batch, width)
    segs = _cdiv(width, KSEG)
    vec = mask_ptr % 16 == 0 and width % 16 == 0
    if need > 0 and segs <= ONE_PASS_SEGS:
        return "one pass", segs, vec
    if need > 0 and workspace_ptr and workspace_bytes >= need and workspace_ptr % 4 == 0:
        return "two pass", segs, vec
    if width > MASK_BLOCK_WIDTH:
        return ("block<16>" if width > MASK_BLOCK16_WIDTH else "block<4>"), 0, False
    return "one wave", 0, False


def coalesce_launch(n_items, nbytes, src_ptrs, dst_ptrs):
    """accv_mtc_coalesce: grid, trips of the item loop of block 0, and per item (vectorised, vector-loop trips, tail bytes)"""
    grid = min(n_items, COALESCE_GRID_CAP)
    items = []
    for n, s, d in zip(nbytes, src_ptrs, dst_ptrs):
        vec = (int(s) | int(d)) % 16 == 0
        n16 = int(n) >> 4 if vec else 0
        items.append((vec, _cdiv(n16, COALESCE_THREADS), int(n) - 16 * n16))
    return SimpleNamespace(grid=grid, item_trips=_cdiv(n_items, grid) if grid else 0, items=items)


def matched_trips(pairs, work):
    return _cdiv(pairs * work, MATCHED_THREADS)


# ------------------------------------------------------------------------------------------- row-kernel cases
COPY_ENTRIES = ("gather_fill", "gather_rows", "scatter_rows", "map_pairs", "insert_const", "pack", "unpack")
ACC_ENTRIES = ("accumulate", "map_pairs_acc")
INDEXED_COPY_ENTRIES = COPY_ENTRIES[:5]
ACC_DTYPES = ("float32", "float64", "int32", "int64", "float16", "bfloat16")
ACC_MAX_ABS, ACC_STEP, ACC_MAX_DUP = 2.0, 0.25, 16      # the exactness condition, see assert_exact_sums
FILL = {"int32": -7, "uint8": 0x5A, "bool": True}
ACC_FILL = -3


def _random(g, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return g.integers(0, 2, shape).astype(np.bool_)
    info = np.iinfo(dtype)
    return g.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


def _quarters(g, shape):
    """multiples of 1/4 in [-2, 2]: float64 (for the float types) and small integers (for the integer types)"""
    q = g.integers(-8, 9, shape)
    return q / 4.0, g.integers(-2, 3, shape).astype(np.int64)


def rows_case(name, regime, batch, width, k, row, dtype="int32", *, seed, expect, extra=0, idx_dtype=np.int64, sparse=False,
              oor=False, acc_row=None, entries=None):
    """One input set for every entry point.  `width` slots on the indexed side, `k` index slots per sample, `row` elements of
    `dtype` per copied row, `acc_row` elements per accumulated row.  idx / idx_b hold distinct in-range indices per sample (a
    quarter of them written negative, wrapping once); idx_dup holds duplicates (accumulate).  `extra` columns behind the k
    slots hold out-of-range junk (idx_stride > w_idx).  `sparse`: most samples are empty, the ones on either side of every
    trip of the sample loop are full.  `oor`: the last valid slot of three samples is out of range (idx and idx_dup of two
    of them, idx_b of the third); the oracle sees those samples one slot shorter."""
    assert k <= width or k == 0
    g = np.random.default_rng(seed)
    B, W = batch, width
    perm = np.argsort(g.random((B, W)), axis=1)
    perm_b = np.argsort(g.random((B, W)), axis=1)
    idx, idx_b = perm[:, :k].astype(np.int64), perm_b[:, :k].astype(np.int64)
    idx = np.where(g.random((B, k)) < 0.25, idx - W, idx)
    idx_b = np.where(g.random((B, k)) < 0.25, idx_b - W, idx_b)
    m = min(W, max(2, _cdiv(k, 4)))
    idx_dup = g.integers(0, m, (B, k)).astype(np.int64)
    idx_dup = np.where(g.random((B, k)) < 0.25, idx_dup - W, idx_dup)
    counts = g.integers(0, k + 1, B).astype(np.int64)
    sizes = g.integers(0, W + 1, B).astype(np.int64)
    marks = sorted({s for t in range(_cdiv(B, GRID_Y) + 1) for s in (t * GRID_Y - 1, t * GRID_Y, t * GRID_Y + 1) if 0 <= s < B} | {0, B - 1})
    if sparse:
        keep = np.arange(B) % 97 == 0
        counts, sizes = np.where(keep, counts, 0), np.where(keep, sizes, 0)
    counts[marks], sizes[marks] = k, W
    if B > 3 and 2 not in marks:
        counts[2], sizes[2] = 0, 0
    planted = {"a": [], "b": []}
    if oor:
        assert B >= 3 and k >= 2
        sa, sb, sc = B - 1, 0, (97 if B > 97 else B // 2)
        for s in (sa, sb, sc):
            counts[s] = k
        idx[sa, k - 1], idx_dup[sa, k - 1] = W + 5, W          # too large
        idx[sb, k - 1], idx_dup[sb, k - 1] = -W - 1, -W - 9    # still negative after the wrap
        idx_b[sc, k - 1] = 2 * W
        idx[sa, 0], idx_dup[sb, 0] = perm[sa, 0] - W, -1       # negative indices that wrap into range, beside them
        planted = {"a": [(sa, k - 1), (sb, k - 1)], "b": [(sc, k - 1)]}
    junk = np.full((B, extra), W + 1000, dtype=np.int64)
    junk[:, ::2] = -W - 1000
    wide = lambda a: np.concatenate([a, junk], 1).astype(idx_dtype)  # noqa: E731
    c = SimpleNamespace(name=name, regime=regime, batch=B, width=W, k=k, row=row, dtype=dtype, extra=extra, expect=expect,
                        idx=wide(idx), idx_b=wide(idx_b), idx_dup=wide(idx_dup), counts=counts, sizes=sizes,
                        offsets=np.cumsum(sizes) - sizes, planted=planted, marks=marks, idx_dtype=np.dtype(idx_dtype),
                        acc_row=row if acc_row is None else acc_row,
                        entries=entries or (COPY_ENTRIES + ACC_ENTRIES), seed=seed)
    c.src = _random(g, (B, W, row), dtype)            # gathered from / the padded side of pack
    c.ins = _random(g, (B, k, row), dtype)            # scattered
    c.into = _random(g, (B, W, row), dtype)           # what the scattered-into tensor held
    c.out0 = _random(g, (B, k, row), dtype)           # what gather_rows' output held
    c.acc_src_f, c.acc_src_i = _quarters(g, (B, W, c.acc_row))
    c.acc_ins_f, c.acc_ins_i = _quarters(g, (B, k, c.acc_row))
    c.acc_into_f, c.acc_into_i = _quarters(g, (B, W, c.acc_row))
    return c


def oracle_counts(c, pairs):
    """the counts the oracle sees: a sample whose last valid slot holds a planted out-of-range index is one slot shorter"""
    counts = c.counts.copy()
    for s, j in c.planted["a"] + (c.planted["b"] if pairs else []):
        assert j == counts[s] - 1
        counts[s] -= 1
    return counts


def planted_errors(c, entry):
    return len(c.planted["a"]) + (len(c.planted["b"]) if entry in ("map_pairs", "map_pairs_acc") else 0)


def assert_exact_sums(c):
    """The exactness condition of the accumulate cases: values are multiples of 1/4 with |v| <= 2 and no target receives more
    than 16 of them, so every partial sum, in any order, is a multiple of 1/4 of magnitude <= 32 — exact in bfloat16 (8
    significant bits at a step of 1/4 reach 64), the narrowest type."""
    for a in (c.acc_src_f, c.acc_ins_f, c.acc_into_f):
        assert np.abs(a).max(initial=0) <= ACC_MAX_ABS and np.array_equal(a / ACC_STEP, np.round(a / ACC_STEP))
    for a in (c.acc_src_i, c.acc_ins_i, c.acc_into_i):
        assert np.abs(a).max(initial=0) <= ACC_MAX_ABS
    valid = np.arange(c.k)[None, :] < c.counts[:, None]
    for targets in (c.idx_dup[:, :c.k], c.idx_b[:, :c.k]):
        t = np.where(targets < 0, targets + c.width, targets)
        ok = valid & (t >= 0) & (t < c.width)
        flat = (np.arange(c.batch)[:, None] * c.width + t)[ok]
        assert np.bincount(flat, minlength=1).max(initial=0) <= ACC_MAX_DUP
    return True


def _sample_loop():
    out = []
    for batch, trips, what in ((GRID_Y, 1, "one trip"), (GRID_Y + 1, 2, "second trip, sample 65535 only"),
                               (2 * GRID_Y + 1, 3, "third trip, blockIdx.y == 0 only")):
        out.append(rows_case(f"batch_{batch}", f"sample loop {what}", batch, 3, 2, 1, seed=batch, sparse=True,
                             expect=dict(vb=4, row_vecs=1, lg=0, sample_trips=trips, vector_trips=1)))
    return out


def _vector_loop():
    out = []
    for elems, acc in ((1020, 255), (1024, 256), (1028, 257), (2052, 513)):
        rv = elems // 4
        out.append(rows_case(f"row_vecs_{rv}", f"vector loop {_cdiv(rv, THREADS)} trips, row_vecs {rv} at vb 16, accumulate rows of {acc}",
                             2, 5, 4, elems, seed=elems, acc_row=acc,
                             expect=dict(vb=16, row_vecs=rv, lg=8, sample_trips=1, vector_trips=_cdiv(rv, THREADS),
                                         acc_vector_trips=_cdiv(acc, THREADS))))
    out.append(rows_case("row_vecs_257_vb1", "vector loop second trip at vb 1", 2, 5, 4, 257, "bool", seed=77, acc_row=257,
                         expect=dict(vb=1, row_vecs=257, lg=8, sample_trips=1, vector_trips=2, acc_vector_trips=2)))
    return out


LG_ROW_VECS = (1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129)


def _lg_groups():
    out = []
    for rv in LG_ROW_VECS:
        lg = row_launch(1, 1, rv).lg
        slots = THREADS >> lg
        for k in (slots - 1, slots, slots + 1):
            rl = row_launch(3, k, rv)
            out.append(rows_case(f"rv{rv}_k{k}", f"lg {lg}, {rl.idle_lanes} idle lanes, {rl.gx} slot groups, last holds {rl.last_group_slots}",
                                 3, k + 2, k, 4 * rv, seed=1000 * rv + k, acc_row=rv,
                                 expect=dict(vb=16, row_vecs=rv, lg=lg, sample_trips=1, vector_trips=1, gx=rl.gx,
                                             last_group_slots=rl.last_group_slots, idle_lanes=rl.idle_lanes)))
    return out


PICK_VEC_OFFSETS = (8, 4, 2, 1)


def _pick_vec():
    """48-byte rows; (source offset, destination offset) in bytes off 16-byte alignment"""
    out = []
    for side in ("src", "dst"):
        for off in PICK_VEC_OFFSETS:
            offs = (off, 0) if side == "src" else (0, off)
            c = rows_case(f"{side}_off_{off}", f"vb = {off} by {'source' if side == 'src' else 'destination'} pointer", 3, 7, 5, 48, "uint8",
                          seed=50 + off + (10 if side == "dst" else 0), entries=COPY_ENTRIES,
                          expect=dict(vb=off, row_vecs=48 // off, sample_trips=1))
            c.offsets_bytes = offs
            out.append(c)
    return out


def _idx_stride():
    return [rows_case(f"stride_{np.dtype(t).name}", f"idx_stride = w_idx + 3, {np.dtype(t).name} indices", 3, 9, 6, 4, seed=300 + i, extra=3,
                      idx_dtype=t, entries=INDEXED_COPY_ENTRIES + ACC_ENTRIES, acc_row=3,
                      expect=dict(vb=16, row_vecs=1, lg=0, sample_trips=1, vector_trips=1)) for i, t in enumerate((np.int32, np.int64))]


def _oor():
    ent = INDEXED_COPY_ENTRIES + ACC_ENTRIES
    return [rows_case("oor_sample_second_trip", "out-of-range index in the sample loop's second trip", GRID_Y + 1, 3, 2, 1, seed=401,
                      sparse=True, oor=True, entries=ent, expect=dict(vb=4, row_vecs=1, lg=0, sample_trips=2, vector_trips=1)),
            rows_case("oor_vector_second_trip", "out-of-range index of a row whose lanes take a second vector trip", 3, 5, 4, 1028,
                      seed=402, oor=True, entries=ent, acc_row=257,
                      expect=dict(vb=16, row_vecs=257, lg=8, sample_trips=1, vector_trips=2, acc_vector_trips=2))]


@lru_cache(maxsize=None)
def row_cases(table):
    return {"sample_loop": _sample_loop, "vector_loop": _vector_loop, "lg_groups": _lg_groups, "pick_vec": _pick_vec,
            "idx_stride": _idx_stride, "oor": _oor}[table]()


ROW_TABLES = ("sample_loop", "vector_loop", "lg_groups", "pick_vec", "idx_stride", "oor")


def row_case_ids(table):
    """names without building the inputs (collection stays cheap)"""
    if table == "sample_loop":
        return [f"batch_{b}" for b in (GRID_Y, GRID_Y + 1, 2 * GRID_Y + 1)]
    if table == "vector_loop":
        return ["row_vecs_255", "row_vecs_256", "row_vecs_257", "row_vecs_513", "row_vecs_257_vb1"]
    if table == "lg_groups":
        return [f"rv{rv}_k{(THREADS >> row_launch(1, 1, rv).lg) + d}" for rv in LG_ROW_VECS for d in (-1, 0, 1)]
    if table == "pick_vec":
        return [f"{s}_off_{o}" for s in ("src", "dst") for o in PICK_VEC_OFFSETS]
    if table == "idx_stride":
        return ["stride_int32", "stride_int64"]
    return ["oor_sample_second_trip", "oor_vector_second_trip"]


def row_case(table, name):
    return next(c for c in row_cases(table) if c.name == name)


def check_row_regime(c, entry, vb=None):
    """the restatement evaluated on the case (and, for a copy, on the vector width found from its actual pointers) against
    what the case claims; returns the launch"""
    e = c.expect
    if entry in ACC_ENTRIES:
        rl = row_launch(c.batch, c.k, c.acc_row)
        assert rl.vector_trips == e.get("acc_vector_trips", 1) and rl.sample_trips == e["sample_trips"], (c.name, entry, vars(rl))
        return rl
    row_bytes = c.row * np.dtype(c.dtype).itemsize
    if vb is None:
        vb = pick_vec(row_bytes, ())
    if entry == "insert_const" and hasattr(c, "offsets_bytes") and c.offsets_bytes[1] == 0:
        assert vb == 16                                   # only the destination pointer counts, and it is aligned
    else:
        assert vb == e["vb"], (c.name, entry, vb)
    width = c.width if entry in ("pack", "unpack") else c.k
    rl = row_launch(c.batch, width, row_bytes // vb)
    assert rl.ok and rl.sample_trips == e["sample_trips"], (c.name, entry, vars(rl))
    if vb == e["vb"]:
        assert row_bytes // vb == e["row_vecs"]
        for key in ("lg", "vector_trips"):
            assert key not in e or getattr(rl, key) == e[key], (c.name, entry, key, vars(rl))
        if entry not in ("pack", "unpack"):
            for key in ("gx", "last_group_slots", "idle_lanes"):
                assert key not in e or getattr(rl, key) == e[key], (c.name, entry, key, vars(rl))
    return rl


# ------------------------------------------------------------------------------------------- the oracle of a row entry
def _valid(c, n):
    return np.arange(c.k)[None, :] < n[:, None]


def copy_want(c, entry):
    """expected result of a copy entry, in the case's dtype"""
    from oracle import h2 as oracle

    k = c.k
    n = oracle_counts(c, entry == "map_pairs")
    if entry == "gather_fill":
        return oracle.gather(c.src, c.idx[:, :k], n, FILL[c.dtype])
    if entry == "gather_rows":     # rows the kernel skips keep what the output held
        got = oracle.gather(c.src, c.idx[:, :k], n, 0)
        return np.where(_valid(c, n)[:, :, None], got, c.out0)
    if entry == "scatter_rows":
        return oracle.scatter_insert(c.ins, c.idx[:, :k], n, c.into)
    if entry == "map_pairs":
        return oracle.map_pairs(c.src, c.idx[:, :k], c.idx_b[:, :k], n, c.into)
    if entry == "insert_const":
        return oracle.insert_const(FILL[c.dtype], c.idx[:, :k], n, c.into)
    mask = np.arange(c.width)[None, :] < c.sizes[:, None]
    if entry == "pack":            # flat rows in order -> padded, zeros behind
        want = np.zeros_like(c.src)
        want[mask] = c.src[mask]
        return want
    assert entry == "unpack"
    return c.src[mask]


def flat_rows(c):
    return c.src[np.arange(c.width)[None, :] < c.sizes[:, None]]


def acc_want(c, entry, integer):
    """expected result of an accumulate entry, summed in float64 (int64) by the oracle"""
    from oracle import h2 as oracle

    k = c.k
    n = oracle_counts(c, entry == "map_pairs_acc")
    src, ins, into = (c.acc_src_i, c.acc_ins_i, c.acc_into_i) if integer else (c.acc_src_f, c.acc_ins_f, c.acc_into_f)
    if entry == "accumulate":
        return oracle.scatter_new(ins, c.idx_dup[:, :k], n, c.width, ACC_FILL, True)
    want = oracle.map_pairs(src, c.idx[:, :k], c.idx_b[:, :k], n, into, accumulate=True)
    for s, j in c.planted["a"]:     # "set first, then add" is a clear pass over the TARGET indices followed by the adds: a pair
        o = int(c.idx_b[s, j])      # whose source index is out of range has its (valid) target cleared and nothing added
        want[s, o + c.width if o < 0 else o] = 0
    return want


# ------------------------------------------------------------------------------------------- pad fill
def pad_fill_case(name):
    """(case) data [batch, width, row] of `dtype`, counts, the expected launch"""
    spec = {
        # name: (batch, width, row elems, dtype, vb, gx, stride trips)
        "gx_1_capped_by_gy": (GRID_Y + 1, 3, 87, "bool", 1, 1, 2),
        "gx_4_second_trip": (4096, 400, 3, "float16", 2, 4, 2),
        "gx_4_third_trip": (4096, 700, 3, "float16", 2, 4, 3),
        "gx_at_the_cap": (1, 4097, 1025, "bool", 1, PAD_FILL_CAP, 2),
    }[name]
    batch, width, row, dtype, vb, gx, trips = spec
    g = np.random.default_rng(len(name) + batch)
    if dtype == "bool":
        data = g.integers(0, 2, (batch, width, row)).astype(np.bool_)
        value = True if name == "gx_at_the_cap" else False
    else:
        data = g.integers(-2000, 2000, (batch, width, row)).astype(np.float16)
        value = -10.0
    counts = g.integers(0, width + 1, batch).astype(np.int64)
    counts[0] = 0                                            # the longest padding: the stride loop's last trip
    if batch > 4:
        counts[[1, 2, 3, batch - 1]] = [width, -3, width + 5, 0]   # nothing to fill; the clamp on both sides
        counts[min(batch - 2, GRID_Y)] = 0                   # the sample loop's second trip (batch > GRID_Y) fills a whole sample
    return SimpleNamespace(name=name, data=data, counts=counts, value=value, batch=batch, width=width, row=row, dtype=dtype,
                           expect=dict(vb=vb, gx=gx, stride_trips=trips))


PAD_FILL_CASES = ("gx_1_capped_by_gy", "gx_4_second_trip", "gx_4_third_trip", "gx_at_the_cap")
PAD_FILL_CLAMP_COUNTS = (0, "width", -3, "width+5")


def check_pad_fill_regime(c, ptr=0):
    row_bytes = c.row * np.dtype(c.dtype).itemsize
    vb = pick_vec(row_bytes, (ptr,))
    pl = pad_fill_launch(c.batch, c.width, row_bytes // vb, c.counts)
    assert (vb, pl.gx, pl.stride_trips) == (c.expect["vb"], c.expect["gx"], c.expect["stride_trips"]), (c.name, vb, vars(pl))
    assert c.data.nbytes < 20 * 1000 * 1000
    return pl


# ------------------------------------------------------------------------------------------- mask -> indices
def _mask(g, batch, width, density):
    return g.random((batch, width)) < density


@lru_cache(maxsize=None)
def mask_case(name):
    """mask [B, W] bool, valid (or None), the regime (with a full workspace, an aligned mask), how the call is made"""
    g = np.random.default_rng(sum(map(ord, "fallback" if name.startswith("fallback_") else name)))   # the fallbacks share one mask
    S = KSEG
    valid, call, off = None, "ws", 0
    if name in ("batch_1025_block16", "batch_1024_one_pass"):
        # the same rows: the first 1024 of the 1025; density low (the oracle is a python loop), rows 0 / 1 dense and empty
        mask = _mask(np.random.default_rng(8192), SEG_BATCH_MAX + 1, 2 * S, 0.03)
        mask[0], mask[1] = True, False
        mask[2, :S], mask[3, S:] = False, False             # all hits in the second / in the first segment
        mask[SEG_BATCH_MAX] = _mask(g, 1, 2 * S, 0.5)[0]
        regime = ("block<16>", 0, False)
        if name == "batch_1024_one_pass":
            mask, regime = mask[:SEG_BATCH_MAX], ("one pass", 2, True)
    elif name == "segs_5_two_pass_bytes":
        mask = _mask(g, 2, ONE_PASS_SEGS * S + 1, 0.3)
        mask[:, -1] = [True, False]                          # the single column of the fifth segment
        regime = ("two pass", ONE_PASS_SEGS + 1, False)
    elif name == "segs_65_scan_second_trip":
        width = SEG_SCAN_STEP * S + 1
        mask = _mask(g, 1, width, 0.02)
        mask[0, (SEG_SCAN_STEP - 1) * S + 7] = mask[0, SEG_SCAN_STEP * S - 1] = mask[0, width - 1] = True   # segments 63, 63, 64
        mask[0, (SEG_SCAN_STEP - 2) * S + 100] = True
        regime = ("two pass", SEG_SCAN_STEP + 1, False)
    elif name.startswith("fallback_"):
        mask = _mask(g, 2, 5 * S, 0.4)
        call = name[len("fallback_"):]                       # none / short / misaligned / full
        regime = ("two pass", 5, True) if call == "full" else ("block<16>", 0, False)
    elif name in ("valid_inside_group_one_pass", "valid_inside_group_two_pass"):
        segs = ONE_PASS_SEGS if name.endswith("one_pass") else ONE_PASS_SEGS + 1
        mask = _mask(g, 3, segs * S, 0.5)
        valid = np.array([S * 1 + 5, S * (segs - 1) + 5, 5], dtype=np.int64)
        mask[:, 5:16] = True                                 # hits behind the limit inside its 16-byte group ...
        mask[0, S + 5:S + 16] = True                         # ... must not count
        mask[1, S * (segs - 1) + 5:S * (segs - 1) + 16] = True
        regime = ("one pass" if segs == ONE_PASS_SEGS else "two pass", segs, True)
    elif name in ("valid_0_m1_over_one_pass", "valid_0_m1_over_two_pass", "valid_0_m1_over_block16", "valid_0_m1_over_block4",
                  "valid_0_m1_over_one_wave"):
        kind = name[len("valid_0_m1_over_"):]
        batch, width = {"one_pass": (4, 2 * S), "two_pass": (4, 5 * S), "block16": (SEG_BATCH_MAX + 1, 2 * S), "block4": (4, 1000),
                        "one_wave": (4, 100)}[kind]
        if kind == "block16":                                # only the first four rows matter; the rest is empty
            mask = np.zeros((batch, width), dtype=bool)
            mask[:4] = _mask(g, 4, width, 0.5)
        else:
            mask = _mask(g, batch, width, 0.5)
        valid = np.full(batch, width, dtype=np.int64)
        valid[:4] = [0, -1, width + 9, width // 2 + 3]
        regime = {"one_pass": ("one pass", 2, True), "two_pass": ("two pass", 5, True), "block16": ("block<16>", 0, False),
                  "block4": ("block<4>", 0, False), "one_wave": ("one wave", 0, False)}[kind]
    elif name in ("base_off_16_one_pass", "base_off_16_two_pass"):
        segs = 2 if name.endswith("one_pass") else 5
        mask = _mask(g, 2, segs * S, 0.3)
        off = 1
        regime = ("one pass" if segs == 2 else "two pass", segs, False)
    else:
        raise KeyError(name)
    return SimpleNamespace(name=name, mask=mask, valid=valid, regime=regime, call=call, mask_offset=off)


MASK_CASES = ("batch_1025_block16", "batch_1024_one_pass", "segs_5_two_pass_bytes", "segs_65_scan_second_trip", "fallback_full",
              "fallback_none", "fallback_short", "fallback_misaligned", "valid_inside_group_one_pass", "valid_inside_group_two_pass",
              "valid_0_m1_over_one_pass", "valid_0_m1_over_two_pass", "valid_0_m1_over_block16", "valid_0_m1_over_block4",
              "valid_0_m1_over_one_wave", "base_off_16_one_pass", "base_off_16_two_pass")


@lru_cache(maxsize=None)
def mask_want(name):
    """(indices [B, longest], sizes) of the oracle; the two 8192-wide cases share one run of it"""
    from oracle import h2 as oracle

    if name == "batch_1024_one_pass":
        idx, sizes = mask_want("batch_1025_block16")
        idx, sizes = idx[:SEG_BATCH_MAX], sizes[:SEG_BATCH_MAX]
        return idx[:, :int(sizes.max())], sizes
    if name.startswith("fallback_") and name != "fallback_full":
        return mask_want("fallback_full")
    c = mask_case(name)
    if name == "valid_0_m1_over_block16":                    # the rows behind the fourth are empty
        idx, sizes = oracle.indices_from_mask(c.mask[:4], c.valid[:4])
        pad = len(c.mask) - 4
        return np.concatenate([idx, np.zeros((pad, idx.shape[1]), dtype=np.int64)]), np.concatenate([sizes, np.zeros(pad, dtype=np.int64)])
    return oracle.indices_from_mask(c.mask, c.valid)


def check_mask_regime(c, mask_ptr=0, ws_ptr=16, ws_bytes=None):
    batch, width = c.mask.shape
    need = mask_workspace_bytes(batch, width)
    got = mask_regime(batch, width, ws_ptr, need if ws_bytes is None else ws_bytes, mask_ptr)
    assert got == c.regime, (c.name, got, c.regime)
    return need


# ------------------------------------------------------------------------------------------- coalesce
COALESCE_EDGE_SIZES = (0, 1, 15, 16, 17, 4095, 4096, 4111, 4112)
COALESCE_ARRANGEMENTS = {"aligned": (0, 0)} | {f"src_off_{o}": (o, 0) for o in (1, 4, 8)} | {f"dst_off_{o}": (0, o) for o in (1, 4, 8)}


def coalesce_many(n_items):
    """items of 1..40 bytes, packed back to back in a shuffled order; the last item of every trip of block 0 (items
    grid - 1 ... and the very last) is 40 bytes"""
    g = np.random.default_rng(n_items)
    nbytes = g.integers(1, 41, n_items).astype(np.int64)
    grid = min(n_items, COALESCE_GRID_CAP)
    for it in {n_items - 1, grid - 1, min(grid, n_items - 1), min(2 * grid, n_items - 1)}:
        nbytes[it] = 40
    order = g.permutation(n_items)
    dst = np.zeros(n_items, dtype=np.int64)
    dst[order] = np.cumsum(nbytes[order]) - nbytes[order]
    src = np.cumsum(nbytes) - nbytes                         # offsets inside one source buffer
    data = g.integers(0, 256, int(nbytes.sum()), dtype=np.uint8)
    return SimpleNamespace(n=n_items, nbytes=nbytes, src_off=src, dst_off=dst, data=data, total=int(nbytes.sum()),
                           item_trips=_cdiv(n_items, grid))


def coalesce_edges(arrangement):
    """the edge sizes; every source starts `src_off` bytes, every destination `dst_off` bytes off a 16-byte boundary"""
    so, do = COALESCE_ARRANGEMENTS[arrangement]
    g = np.random.default_rng(so * 16 + do)
    nbytes = np.array(COALESCE_EDGE_SIZES, dtype=np.int64)
    pitch = 4112 + 32
    src = np.arange(len(nbytes)) * pitch + so
    dst = np.arange(len(nbytes))[::-1] * pitch + do
    data = g.integers(0, 256, pitch * len(nbytes) + 16, dtype=np.uint8)
    expect = [(so == 0 and do == 0, _cdiv(int(n) >> 4, COALESCE_THREADS) if so == 0 and do == 0 else 0,
               int(n) % 16 if so == 0 and do == 0 else int(n)) for n in nbytes]
    return SimpleNamespace(n=len(nbytes), nbytes=nbytes, src_off=src, dst_off=dst, data=data, total=pitch * len(nbytes) + 16,
                           expect=expect)


def coalesce_want(c):
    """the byte-wise assembly: (packed bytes, mask of the bytes an item covers)"""
    packed = np.zeros(c.total, dtype=np.uint8)
    covered = np.zeros(c.total, dtype=bool)
    for s, d, n in zip(c.src_off, c.dst_off, c.nbytes):
        packed[d:d + n] = c.data[s:s + n]
        covered[d:d + n] = True
    return packed, covered


# ------------------------------------------------------------------------------------------- matched pair loss
MATCHED_TOTALS = (255, 256, 257, 513)
MATCHED_KINDS = ("l1", "l2", "smooth_l1", "iou_xyxy", "onehot_l1")
