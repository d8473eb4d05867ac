"""Shapes at the edges of the launch regimes of csrc/polyline.hip (the sampler of SURVEY §8 f1 and its backward, DESIGN.md
§9c), shared by test_polyline_edges_cpu.py (the plan, and the host path on the small cases) and test_polyline_edges_gpu.py.
DESIGN.md §9k has the table of decisions and loops next to the case that crosses each one.

plan() restates the launch plan in Python:

  * the forward launcher accv_polyline_sample_boxes: ``wide`` / ``threads``, ``min_chunk``, the kSpreadGroups rule, ``chunks``,
    ``per_chunk``, ``p.q_chunk`` and the final ``chunks`` (the block between "queries per workgroup: everything, unless ..."
    and ``const dim3 grid``), and accv_polyline_scratch_bytes (``need <= kLdsBudgetBytes``);
  * grad_plan(): the same chunking without the forward's ``!p.use_scratch`` condition, ``region_bytes``, ``use_ws``,
    ``ws_acc``, ``ws_slab``.

A case proves its regime from outside where an entry point shows it:

    accv_polyline_scratch_bytes(batch, P, dtype)               == 0 (LDS) or P * acc * batch (scratch)
    accv_polyline_grad_workspace_bytes(batch, P, Q, D, dtype)  == ws_acc + ws_slab of the restatement

The second fixes ``use_ws`` (``ws_acc`` is zero or not) and, through the slab term ``align256(chunks * batch * P * D * acc)``,
the backward's ``chunks``.  The forward's chunk count has no entry point: where the scratch path is off it is the
backward's (the same arithmetic on the same arguments), on the scratch path it is 1; each row states the arithmetic.
"""
from types import SimpleNamespace

import torch

from test_polyline_grad_gpu import _lattice  # noqa: F401  (the integer lattice of the gradient tests, unchanged)

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
CODE = {F32: 0, F64: 1, F16: 2, BF16: 3}       # the dtype codes of the polyline entry points
HALF = (F16, BF16)
name = lambda d: str(d).split(".")[-1]  # noqa: E731

# constants of csrc/polyline.hip
K_THREADS, K_WIDE_THREADS = 256, 1024
K_LDS_BUDGET = 48 * 1024          # kLdsBudgetBytes: the forward's arc-length array
K_WIDE_POINTS = 2048              # kWidePoints
K_SPREAD_GROUPS = 512             # kSpreadGroups
K_GRAD_LDS_BUDGET = 64 * 1024     # kGradLdsBudgetBytes: dynamic + static LDS of a backward workgroup
K_MAX_GROUPS = 4096               # the launch stays at about this many workgroups
K_CHUNK_BATCH_LIMIT = 2048        # ``batch < 2048``
K_SUM_GRID = 4096 * 256           # elements one trip of polyline_grad_sum_kernel covers
INT_MAX = 2 ** 31 - 1


def acc_size(dtype):
    return 8 if dtype == F64 else 4


def align256(v):
    return (v + 255) // 256 * 256


def _ceil(a, b):
    return -(-a // b)


def plan(batch, P, Q, D, dtype):
    """the launch plan of the sampler (fwd_*) and of its backward for one shape"""
    acc = acc_size(dtype)
    threads = K_WIDE_THREADS if P >= K_WIDE_POINTS else K_THREADS
    min_chunk = max(threads, _ceil(P // 4, threads) * threads)
    spread = batch * _ceil(Q, threads) <= K_SPREAD_GROUPS
    if spread:
        min_chunk = threads

    def chunking(allowed):
        chunks = 1
        if allowed and Q >= 2 * min_chunk and batch < K_CHUNK_BATCH_LIMIT:
            chunks = max(1, min(_ceil(Q, min_chunk), K_MAX_GROUPS // batch))
        per_chunk = _ceil(Q, chunks)
        q_chunk = max(threads, min(_ceil(per_chunk, threads) * threads, INT_MAX - threads))
        return max(1, _ceil(Q, q_chunk)), q_chunk

    use_scratch = P * acc > K_LDS_BUDGET
    chunks, q_chunk = chunking(True)
    fwd_chunks, fwd_q_chunk = chunking(not use_scratch)
    region = max(1, P) * (D + 2) * acc
    use_ws = region + threads * 8 > K_GRAD_LDS_BUDGET
    return SimpleNamespace(
        threads=threads, min_chunk=min_chunk, spread=spread, chunks=chunks, q_chunk=q_chunk,
        use_scratch=use_scratch, scratch_bytes=P * acc * batch if use_scratch else 0, fwd_chunks=fwd_chunks,
        fwd_q_chunk=fwd_q_chunk, use_ws=use_ws, ws_acc=align256(region) * batch * chunks if use_ws else 0,
        ws_slab=align256(chunks * batch * P * D * acc) if chunks > 1 else 0, sum_count=batch * P * D)


def _lib():
    from accvlab import _amd_native as nat

    return nat.lib()


def entry_points(batch, P, Q, D, dtype):
    """(scratch bytes, backward workspace bytes) as the library answers"""
    lib = _lib()
    return (int(lib.accv_polyline_scratch_bytes(batch, P, CODE[dtype])),
            int(lib.accv_polyline_grad_workspace_bytes(batch, P, Q, D, CODE[dtype])))


def assert_plan_matches_library(batch, P, Q, D, dtype):
    pl = plan(batch, P, Q, D, dtype)
    sb, wb = entry_points(batch, P, Q, D, dtype)
    assert sb == pl.scratch_bytes, (batch, P, Q, D, dtype, sb, pl.scratch_bytes)
    assert wb == pl.ws_acc + pl.ws_slab, (batch, P, Q, D, dtype, wb, pl.ws_acc, pl.ws_slab)
    return pl


def _r(threads, chunks, q_chunk, ws, scratch=False, fwd_chunks=None, spread=None):
    """the regime a row names: workgroup size, backward chunks and queries per chunk, workspace accumulators, forward scratch
    path, forward chunks (default: the backward's; 1 on the scratch path), spread rule (None: not what the row is about)"""
    return dict(threads=threads, chunks=chunks, q_chunk=q_chunk, use_ws=ws, use_scratch=scratch,
                fwd_chunks=(1 if scratch else chunks) if fwd_chunks is None else fwd_chunks, spread=spread)


def case(batch, P, Q, D, relative, regimes, ps=None, qs=None, max_step=3, sliced=False, host=False):
    """regimes: {dtype: _r(...)} — the storage types of the row and the regime each is in.  ps / qs: point and query counts
    per polyline (None: all).  sliced: the gradient is also compared with the sum over single-chunk launches.  host: small
    enough for the host path in the CPU file."""
    assert ps is None or len(ps) == batch
    assert qs is None or len(qs) == batch
    return SimpleNamespace(batch=batch, P=P, Q=Q, D=D, relative=relative, regimes=regimes, dtypes=list(regimes), ps=ps, qs=qs,
                           max_step=max_step, sliced=sliced, host=host)


BOTH = (False, True)
# name -> row.  T = threads, mc = min_chunk; "spread" = batch * ceil(Q / T) <= 512 makes mc = T.
CASES = {
    # ---- workgroup size: kWidePoints 2047 / 2048, both spread into three chunks
    # 2047: T = 256, mc = max(256, ceil(511 / 256) * 256) = 512, spread (3 * 3 = 9) -> 256; chunks = min(ceil(600 / 256), 4096 / 3)
    # = 3, per_chunk = 200 -> q_chunk = 256.  f32 region 2047 * 4 * 4 + 256 * 8 = 34800 <= 65536: LDS; f64 region 65504 + 2048:
    # a 256-thread workgroup with workspace accumulators, chunked, in f64.  Query counts at the chunk border 512.
    "wg256_p2047": case(3, 2047, 600, 2, BOTH, {F32: _r(256, 3, 256, False), F64: _r(256, 3, 256, True)},
                        ps=[2047, 682, 0], qs=[600, 513, 511], sliced=True, host=True),
    # 2048: T = 1024, mc = 1024; chunks = min(ceil(2100 / 1024), 1365) = 3, per_chunk = 700 -> q_chunk = 1024.
    # region 2048 * 16 + 8192 = 40960: LDS
    "wg1024_p2048": case(3, 2048, 2100, 2, BOTH, {F32: _r(1024, 3, 1024, False)}, ps=[2048, 2047, 1], qs=[2100, 2049, 1024],
                         sliced=True, host=True),
    # ---- arc_prefix trips, 256 threads: n_seg = 255 / 256 / 257 (per = 1, 1, 2: with 257 the threads from 129 on own no
    # segment), 1024 / 1025 (one and two trips of s0 += 4 * 256; per = 4 and 5: the threads from 205 on own none), and 0 / 1 / 2
    # points.  Q = 300 < 2 * 256: one chunk of q_chunk 512 (a second trip of the query loop).  Every type in LDS.
    "prefix_trips_256": case(8, 1026, 300, 2, BOTH, {d: _r(256, 1, 512, False) for d in (F32, F64, F16, BF16)},
                             ps=[0, 1, 2, 256, 257, 258, 1025, 1026], qs=[300, 300, 300, 299, 300, 257, 300, 300], host=True),
    # ---- arc_prefix trips, 1024 threads: n_seg = 4097 (two trips of s0 += 4 * 1024, per = 5), 4096 (one, per = 4), 1024 (per 1)
    # region 4098 * 16 + 8192 = 73760 (f32, f16, bf16), 4098 * 32 + 8192 (f64): EVERY storage type is on the workspace path
    "prefix_trips_1024": case(6, 4098, 300, 2, BOTH, {d: _r(1024, 1, 1024, True) for d in (F32, F64, BF16)},
                              ps=[4098, 4097, 1025, 2, 1, 0], qs=[300, 300, 299, 300, 300, 300], host=True),
    # ---- backward LDS / workspace: region + T * 8 <= 65536.  f32 at 1024 threads: 3584 * 16 + 8192 = 65536 / 3585: 65552
    "grad_lds_f32_p3584": case(2, 3584, 300, 2, BOTH, {F32: _r(1024, 1, 1024, False)}, ps=[3584, 3583], qs=[300, 17], host=True),
    "grad_ws_f32_p3585": case(2, 3585, 300, 2, BOTH, {F32: _r(1024, 1, 1024, True)}, ps=[3585, 3584], qs=[300, 17], host=True),
    # f64 at 256 threads: 1984 * 32 + 2048 = 65536 / 1985: 65568; at 1024 threads 2048 * 32 + 8192
    "grad_lds_f64_p1984": case(2, 1984, 300, 2, BOTH, {F64: _r(256, 1, 512, False)}, ps=[1984, 700], qs=[300, 17], host=True),
    "grad_ws_f64_p1985": case(2, 1985, 300, 2, BOTH, {F64: _r(256, 1, 512, True)}, ps=[1985, 700], qs=[300, 17], host=True),
    "grad_ws_f64_p2048": case(2, 2048, 300, 2, BOTH, {F64: _r(1024, 1, 1024, True)}, ps=[2048, 700], qs=[300, 17], host=True),
    # 256 threads and a run-time D: 2047 * 7 * 4 + 2048 = 59364 (LDS) / 2047 * 8 * 4 + 2048 = 67552 (workspace)
    "grad_lds_d5_p2047": case(2, 2047, 100, 5, BOTH, {F32: _r(256, 1, 256, False)}, ps=[2047, 1000], qs=[100, 99], host=True),
    "grad_ws_d6_p2047": case(2, 2047, 100, 6, BOTH, {F32: _r(256, 1, 256, True)}, ps=[2047, 1000], qs=[100, 99], host=True),
    # ---- forward scratch threshold P * acc <= 49152.  T = 1024, spread (1 * 2) -> mc = 1024; chunks = min(2, 4096) = 2,
    # q_chunk = 1024: the backward takes the workspace (P * 16 > 65536), two chunks and the slab on both sides; the forward
    # takes LDS and two chunks at 12288, scratch and ONE chunk of 2048 queries (two trips of its query loop) at 12289.
    # max_step = 1: the total stays below 2^24 / 1088, so that fraction * total is exact in f32
    "fwd_lds_p12288": case(1, 12288, 2048, 2, BOTH, {F32: _r(1024, 2, 1024, True)}, max_step=1, host=True),
    "fwd_scratch_p12289": case(1, 12289, 2048, 2, BOTH, {d: _r(1024, 2, 1024, True, scratch=True) for d in (F32, F16, BF16)},
                               max_step=1, host=True),
    # f64: 6144 * 8 = 49152 / 6145.  Q = 300: one chunk
    "fwd_lds_f64_p6144": case(2, 6144, 300, 2, BOTH, {F64: _r(1024, 1, 1024, True)}, ps=[6144, 2000], qs=[300, 299],
                              max_step=1, host=True),
    "fwd_scratch_f64_p6145": case(2, 6145, 300, 2, BOTH, {F64: _r(1024, 1, 1024, True, scratch=True)}, ps=[6145, 2000],
                                  qs=[300, 299], max_step=1, host=True),
    # the scratch path with ragged counts, in f32 and in the two half types (their f32 arc lengths take scratch as well)
    "fwd_scratch_ragged": case(4, 12300, 300, 2, BOTH, {d: _r(1024, 1, 1024, True, scratch=True) for d in (F32, F16, BF16)},
                               ps=[12300, 4100, 1, 0], qs=[300, 299, 300, 0], max_step=1, host=True),
    # ---- ``batch < 2048``: T = 256, mc = 256, not spread (2047 * 2 groups); Q = 512 >= 2 * mc.  2047: chunks = min(2,
    # 4096 / 2047 = 2) = 2, q_chunk = 256; the slab sum covers 2047 * 260 * 2 = 1 064 440 > 4096 * 256 elements: the summing
    # kernel's grid stride takes its second trip (the rows of the last 16 polylines).  2048: one chunk
    "batch_2047": case(2047, 260, 512, 2, (True,), {F32: _r(256, 2, 256, False)}, sliced=True),
    "batch_2048": case(2048, 260, 512, 2, (True,), {F32: _r(256, 1, 512, False)}),
    # ---- kSpreadGroups: 512 / 513 workgroups.  At P = 40 and at Q = 600 the rule is crossed but cannot show: mc = 256 either
    # way at P = 40 (257 chunks at 65537), and 512 / 513 polylines x ceil(600 / 256) = 3 groups are past the rule on both sides
    # (mc = 512 > Q / 2: one chunk).  The rows stay for what they are: 256 / 257 chunks of one polyline pair, and 512 / 513
    # single-chunk polylines of 1100 points
    "spread_p40_q65536": case(2, 40, 65536, 2, (True,), {F32: _r(256, 256, 256, False, spread=True)}),
    "spread_p40_q65537": case(2, 40, 65537, 2, (True,), {F32: _r(256, 257, 256, False, spread=False)}),
    "groups_b512_q600": case(512, 1100, 600, 2, (True,), {F32: _r(256, 1, 768, False, spread=False)}),
    "groups_b513_q600": case(513, 1100, 600, 2, (True,), {F32: _r(256, 1, 768, False, spread=False)}),
    # where the rule shows, P / 4 > T: at P = 1100 mc = ceil(275 / 256) * 256 = 512 unless spread.
    # 2 * ceil(65536 / 256) = 512 groups: spread, 256 chunks of 256; 2 * 257 = 514: chunks = min(ceil(65537 / 512), 2048) = 129,
    # per_chunk = 509 -> q_chunk = 512: every thread takes two queries
    "spread_on_q65536": case(2, 1100, 65536, 2, (True,), {F32: _r(256, 256, 256, False, spread=True)}, qs=[65536, 65535]),
    "spread_off_q65537": case(2, 1100, 65537, 2, (True,), {F32: _r(256, 129, 512, False, spread=False)}, qs=[65537, 65025]),
    # 256 * 2 = 512 groups: spread, two chunks of 256; 257 * 2 = 514: mc = 512 > Q / 2, one chunk
    "spread_on_b256": case(256, 1100, 512, 2, (True,), {F32: _r(256, 2, 256, False, spread=True)}),
    "spread_off_b257": case(257, 1100, 512, 2, (True,), {F32: _r(256, 1, 512, False, spread=False)}),
    # 19 * 27 = 513 groups exactly: chunks = min(ceil(6912 / 512), 215) = 14, per_chunk = 494 -> q_chunk = 512
    "spread_off_513_groups": case(19, 1100, 6912, 2, (True,), {F32: _r(256, 14, 512, False, spread=False)}),
    # ---- chunks capped by 4096 / batch: T = 256, mc = 256; chunks = min(ceil(40000 / 256) = 157, 4096 / 64 = 64) = 64,
    # per_chunk = 625 -> q_chunk = 768 (three queries per thread), chunks = ceil(40000 / 768) = 53
    "chunks_capped": case(64, 30, 40000, 2, (True,), {F32: _r(256, 53, 768, False)}),
    # ---- query counts at the chunk borders: T = 256, spread (5 * 6), chunks = min(6, 819) = 6, q_chunk = 256.  Counts 767 /
    # 768 / 769: chunk 3 of the first two has no live query, chunk 2 of the first lacks one, chunk 2 of the second is full,
    # chunk 3 of the third has exactly one; 0: no live query anywhere; an empty polyline with every query
    "chunk_borders": case(5, 600, 1300, 2, BOTH, {F32: _r(256, 6, 256, False), F64: _r(256, 6, 256, False)},
                          ps=[600, 600, 200, 600, 0], qs=[767, 768, 769, 0, 1300], sliced=True, host=True),
    # ---- type x regime
    # f16 / bf16 chunked: T = 256, spread (3 * 20), chunks = min(20, 1365), per_chunk = 250 -> q_chunk = 256
    "half_chunked": case(3, 600, 5000, 2, BOTH, {d: _r(256, 20, 256, False) for d in HALF}, ps=[600, 200, 0],
                         qs=[5000, 2507, 4999]),
    # f16 / bf16 on the workspace with 1024 threads: 4000 * 16 + 8192 = 72192
    "half_ws_1024": case(2, 4000, 700, 2, BOTH, {d: _r(1024, 1, 1024, True) for d in HALF}, ps=[4000, 1333], qs=[700, 357]),
    # a run-time D, chunked: T = 256, spread (3 * 8), chunks = 8, per_chunk = 250 -> q_chunk = 256
    "runtime_d_chunked": case(3, 300, 2000, 4, BOTH, {F32: _r(256, 8, 256, False)}, ps=[300, 100, 0], qs=[2000, 1007, 1999],
                              sliced=True, host=True),
}
RUNS = [(which, dtype) for which, row in CASES.items() for dtype in row.dtypes]
RUN_IDS = [f"{w}-{name(d)}" for w, d in RUNS]


def assert_regime(which, dtype):
    """the row is in the regime it names: the restated plan gives it, and the entry points give the restated plan"""
    row = CASES[which]
    pl = assert_plan_matches_library(row.batch, row.P, row.Q, row.D, dtype)
    for key, want in row.regimes[dtype].items():
        if want is not None:
            assert getattr(pl, key) == want, (which, dtype, key, getattr(pl, key), want)
    sb, wb = entry_points(row.batch, row.P, row.Q, row.D, dtype)
    assert (sb > 0) == row.regimes[dtype]["use_scratch"] and (wb > 0) == (pl.use_ws or pl.chunks > 1)
    return pl


def relatives(which, dtype):
    """the ``relative`` settings of a row for one storage type.  A float16 fraction carries 11 bits: its product with a total
    length above 2^13 is not exact in f32, the kernel (f32) and the reference (f64) may then stand on different sides of a
    vertex, where the gradient jumps — such pairs run absolute queries only.  (bfloat16 fractions carry 8 bits, f32 ones
    k / 1024 eleven with totals kept below 2^24 / 1088.)"""
    row = CASES[which]
    if dtype == F16 and row.P * row.max_step > 8192:
        return tuple(r for r in row.relative if not r)
    return row.relative


def inputs(which, relative):
    """float64 lattice points [batch, P, D], queries [batch, Q], point and query counts (int64 tensors or None)"""
    row = CASES[which]
    seed = sum(map(ord, which)) + int(relative)
    p, fr = _lattice(row.batch, row.P, row.Q, row.D, relative, seed=seed, max_step=row.max_step)
    ps = None if row.ps is None else torch.tensor(row.ps)
    qs = None if row.qs is None else torch.tensor(row.qs)
    if row.ps is not None and qs is None:
        qs = torch.full((row.batch,), row.Q)
    if row.qs is not None and ps is None:
        ps = torch.full((row.batch,), row.P)
    return p, fr, ps, qs


def sweep_shapes():
    """(batch, P, Q, D, dtype) around every threshold of the plan, +- 1 (and a little further) on each side"""
    out = set()
    near = lambda v: (v - 2, v - 1, v, v + 1, v + 2)  # noqa: E731
    for dtype in (F32, F64, F16, BF16):
        for P in near(2048) + near(3584) + near(1984) + near(12288) + near(6144) + near(1024) + (1, 2, 40, 1100):
            for Q in (0, 1, 300, 511, 512, 513, 2047, 2048, 2049, 2100):
                for batch in (1, 2, 3):
                    out.add((batch, P, Q, 2, dtype))
        for D in (1, 2, 3, 4, 5, 6, 7):                                    # the LDS budget in D
            for P in near(2047) + near(1170) + near(1638):
                out.add((2, P, 100, D, dtype))
        for batch in near(2048) + near(512) + near(256) + near(170) + near(4096) + (64, 19):   # batch rules
            for Q in (511, 512, 513, 600, 6912, 40000):
                for P in (30, 260, 1100):
                    out.add((batch, P, Q, 2, dtype))
        for Q in near(65536) + near(512) + near(1024) + near(2048) + near(131072):             # query rules
            for P in (40, 1100, 2048, 5000):
                for batch in (1, 2):
                    out.add((batch, P, Q, 2, dtype))
        # q_chunk capped at INT_MAX - T: no launch of 2^31 queries is run, but the capped value makes two chunks of one
        # (batch 2048: not chunked otherwise), and the slab term of the workspace shows them
        for Q in (INT_MAX, INT_MAX - 255, INT_MAX - 256, INT_MAX - 1024, INT_MAX - 1025, 2 ** 30):
            for batch, P in ((2048, 30), (2048, 2048), (1, 30), (4096, 40)):
                out.add((batch, P, Q, 2, dtype))
    return sorted(out, key=lambda s: (CODE[s[4]],) + s[:4])


# ---------------------------------------------------------------------------------------------- runs and comparison rules
def _poly():
    from accvlab.lane_helpers import polyline

    return polyline


def _ragged(t, sizes):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(t, sample_sizes=sizes)


def acc_eps(dtype, device):
    """epsilon of the type the arc lengths are kept in: double on the host path and for f64 storage, else float"""
    cpu = torch.device(device).type == "cpu"
    return torch.finfo(F64 if cpu or dtype == F64 else F32).eps


def forward(pd, fd, ps, qs, relative, counts=torch.int64):
    """samples [B, Q, D] and lengths [B] through the public operators (fixed-size ones without counts)"""
    poly = _poly()
    with torch.no_grad():
        if ps is None:
            return poly.interpolate(pd, fd, relative=relative), poly.lengths(pd)
        prb = _ragged(pd, ps.to(pd.device, counts))
        out = poly.interpolate_var_size_batch(prb, _ragged(fd, qs.to(pd.device, counts)), relative=relative).tensor
        return out, poly.lengths_var_size_batch(prb)


def live_mask(qs, batch, Q, device):
    if qs is None:
        return torch.ones((batch, Q), dtype=torch.bool, device=device)
    return torch.arange(Q, device=device).unsqueeze(0) < qs.to(device).unsqueeze(1)


def check_forward(out, lens, ref, ref_lens, qs, dtype, what):
    """the forward bounds: f64 1e-9 absolute; f32 on the lattice 1e-6 max|ref| (arc lengths and d - C_i are exact there, a
    sample is a w0 + c w1 with one rounding each in the two divisions, the two products and the sum: about 2.5 eps of the
    coordinate scale, the bound leaves a factor three); f16 / bf16 one rounding of the f32 result on top: eps(dtype) |ref|.
    Lengths are exact on the lattice in f32 and f64, one rounding in the half types.  NaN exactly where the reference has it."""
    b, q, _ = ref.shape
    live = live_mask(qs, b, q, ref.device).unsqueeze(-1).expand_as(ref)
    got, want = out.double()[live], ref[live]
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN samples differ"
    got, want = got[~torch.isnan(want)], want[~torch.isnan(want)]
    if want.numel():
        scale = float(want.abs().max())
        err = (got - want).abs()
        bound = {F64: torch.full_like(err, 1e-9), F32: torch.full_like(err, 1e-6 * scale)}.get(dtype)
        if bound is None:
            bound = torch.finfo(dtype).eps * want.abs() + 1e-6 * scale
        print(f"{what} samples: max error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3e}, "
              f"max |ref| {scale:.3e}")
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} samples outside, max error {float(err.max()):.3e}"
    assert torch.equal(torch.isnan(lens), torch.isnan(ref_lens)), f"{what}: NaN lengths differ"
    gl, wl = torch.nan_to_num(lens.double()), torch.nan_to_num(ref_lens)
    if dtype in HALF:
        assert bool(((gl - wl).abs() <= torch.finfo(dtype).eps * wl.abs()).all()), f"{what}: lengths"
    else:
        assert torch.equal(gl, wl), f"{what}: lengths differ by {float((gl - wl).abs().max()):.3e}"


def api_grads(pd, fd, ps, qs, relative, g, gl):
    """gradients (points, distances) of <interpolate, g> + <lengths, gl> through autograd (gl None: the samples alone)"""
    poly = _poly()
    pr, dr = pd.detach().clone().requires_grad_(), fd.detach().clone().requires_grad_()
    b, q = fd.shape
    ps = torch.full((b,), pd.shape[1]) if ps is None else ps
    qs = torch.full((b,), q) if qs is None else qs
    prb = _ragged(pr, ps.to(pd.device))
    outs = [poly.interpolate_var_size_batch(prb, _ragged(dr, qs.to(pd.device)), relative=relative).tensor]
    ws = [g]
    if gl is not None:
        outs.append(poly.lengths_var_size_batch(prb))
        ws.append(gl)
    torch.autograd.backward(outs, ws)
    return pr.grad, dr.grad


def sliced_grads(pd, fd, ps, qs, relative, g, gl, width):
    """the same gradients from launches of at most `width` queries per polyline (one chunk each: Q <= threads is below
    2 * min_chunk), the point gradients summed in float64"""
    b, q = fd.shape
    qs = torch.full((b,), q) if qs is None else qs
    gp, gd = None, []
    for lo in range(0, q, width):
        hi = min(q, lo + width)
        part = api_grads(pd, fd[:, lo:hi].contiguous(), ps, (qs - lo).clamp(0, hi - lo), relative, g[:, lo:hi].contiguous(),
                         gl if lo == 0 else None)
        gp = part[0].double() if gp is None else gp + part[0].double()
        gd.append(part[1])
    return gp, torch.cat(gd, 1)


def bitwise_zero(t):
    """+0 in every element (a -0 or a denormal is not)"""
    return t.numel() == 0 or not bool(t.contiguous().view(torch.uint8).any())
