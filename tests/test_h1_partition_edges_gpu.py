"""The heat-map rasteriser at the edges of its own work partition: every dispatch regime of `dispatch_splat`
and every shape-dependent loop of the splat kernels, the flat API's binning kernels and the front-end kernels, on the
deterministic cases of h1_partition_cases.py.  A case asserts the regime it names from outside — the instantiation and the
grid `accv_draw_heatmap_last_dispatch` reports against the restated dispatch, the hits per tile and cull round from the numpy
cull — and compares with the CPU oracle (float64 inside) at 1e-5 absolute.  Bit equality is asked only where the suite already
holds it: 128 x 32 against 128 x 16 tiles, write-through / adaptive against plain stores, the flat call's single launch
against the binned one, the multi-scale launches against the per-scale operators."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import h1_partition_cases as hc
from oracle import h1 as oracle

pytestmark = pytest.mark.gpu
ATOL = 1e-5
DEV = "cuda:0"
_name = lambda v: v.name  # noqa: E731


def rb(t, sizes):
    return SimpleNamespace(tensor=t, sample_sizes=sizes)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _err(got, ref):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max())


def _nat():
    from accvlab import _amd_native as nat

    return nat


@functools.lru_cache(maxsize=None)
def _built(name, TW, TH, odd):
    """(case, oracle of the fused-clear draw, old map, oracle of the in-place draw): computed once, never modified"""
    cs = (hc.STRUCTURAL.get(name) or (lambda *_: hc.SMALL[name]()))(TW, TH, odd)
    base = hc.base_map((len(cs.counts), cs.H, cs.W), cs.k)
    return cs, hc.oracle_batched(cs, clear=True), base, hc.oracle_batched(cs, clear=False, base=base)


def _draw(cs, v, base):
    """the case through the batched API with the hints of variant `v`; the instantiation and the grid are the restated ones"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    B = len(cs.counts)
    c, r, n = _t(cs.centers, np.int32), _t(cs.radii, np.int32), _t(cs.counts, np.int64)
    hm = torch.full((B, cs.H, cs.W), 123.0, device=DEV) if v.clear else torch.from_numpy(base).to(DEV)   # clear ignores what was there
    draw_heatmap_batched(hm, rb(c, n), rb(r, n), 6.0, cs.k, clear=v.clear, **v.kwargs)
    assert _nat().last_dispatch() == hc.expected_dispatch(v, B, cs.H, cs.W), _nat().last_dispatch()
    return hm


def _check_variant(name, v):
    cs, ref_clear, base, ref_inplace = _built(name, v.TW, v.TH, v.odd)
    for plane, tile, *want in cs.named:
        if isinstance(want[0], tuple):                                  # hits of the tile per cull round
            assert hc.tile_rounds(cs, plane, tile, v.TW, v.TH) == want[0], (plane, tile)
    got = _draw(cs, v, base)
    err = _err(got, ref_clear if v.clear else ref_inplace)
    assert err <= ATOL, err
    ref_v = hc.family_reference(v)
    if ref_v is not None:
        assert torch.equal(got, _draw(cs, ref_v, base)), f"{v.name} differs from {ref_v.name}"
    return cs, got


@pytest.mark.parametrize("v", hc.VARIANTS, ids=_name)
@pytest.mark.parametrize("name", list(hc.STRUCTURAL))
def test_structural_case_in_every_instantiation(name, v):
    """round_splits: hits of one tile in cull round 1 only, 2 only, 3 only, 1 and 3 with none in 2, 64 in a round, odd and even
    counts, planes of 0 / 1 / 64 / 65 / 130 candidates (k > 0 and k < 0); box_edges: box edges inside a lane's four columns
    and on the half-wave row, a box that is the whole tile; off_map: radius 0, centres off the map, an empty box; cover: the
    adaptive store policy's sum on both sides of its threshold and on it.  In place the old map holds distinct values above
    and below what is drawn, so a repeated or a missing first-touch load shows."""
    cs, got = _check_variant(name, v)
    if name == "cover" and v.sm == hc.STORE_ADAPTIVE:
        assert cs.cover[0] < cs.dense_area == cs.cover[1] < cs.cover[2]


@pytest.mark.parametrize("v", hc.SMALL_VARIANTS, ids=_name)
@pytest.mark.parametrize("name", list(hc.SMALL))
def test_small_splat_walks(name, v):
    """small_rows: more hits than one pass of the row walk at every rows_hint 1..7 (even heights clipped by the top and by the
    bottom edge); small_walk: the 16-lane walk at 8 rows and above, a box 128 x 16, an empty box, three trips of four hits,
    dirty and untouched segments in one tile; small_fetch: the second trip of the candidate loop (300 objects)"""
    cs, _ = _check_variant(name, v)
    for plane, tile, *want in cs.named:
        if len(want) == 1 and not isinstance(want[0], tuple):          # small_rows: (rows_hint)
            nh, rows = hc.round_rows(cs, plane, tile, v.TW, v.TH)
            assert rows == want[0] and (nh > 64 // rows or rows == 1)
        elif len(want) == 2:                                            # small_walk: (hits, rows_hint)
            assert hc.round_rows(cs, plane, tile, v.TW, v.TH) == tuple(want)


@pytest.mark.parametrize("clear", [True, False])
def test_base_off_16_bytes_takes_the_scalar_tiles(clear):
    """`vec4` needs a width that is a multiple of 4 AND a 16-byte aligned base: a map of width 264 that starts 4 bytes into its
    buffer runs PX = 1 (the structural cases reach PX = 1 through the width)"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    cs, ref_clear, base, ref_inplace = _built("round_splits", 128, 16, False)
    B = len(cs.counts)
    buf = torch.full((B * cs.H * cs.W + 8,), 9.0, device=DEV)
    hm = buf[1:1 + B * cs.H * cs.W].view(B, cs.H, cs.W)
    assert hm.data_ptr() % 16 == 4 and cs.W % 4 == 0
    if not clear:
        hm.copy_(torch.from_numpy(base))
    n = _t(cs.counts, np.int64)
    draw_heatmap_batched(hm, rb(_t(cs.centers, np.int32), n), rb(_t(cs.radii, np.int32), n), 6.0, cs.k, clear=clear)
    v = next(u for u in hc.VARIANTS if u.PX == 1 and u.clear == clear)
    assert _nat().last_dispatch() == hc.expected_dispatch(v, B, cs.H, cs.W)
    assert _err(hm, ref_clear if clear else ref_inplace) <= ATOL
    assert float(buf[0]) == 9.0 and bool((buf[1 + B * cs.H * cs.W:] == 9.0).all())


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("v", [u for u in hc.VARIANTS if u.name in ("px4_r8_clear_sm0", "px4_r8_inplace_sm5", "px1_clear", "small_inplace_sm0")],
                         ids=_name)
def test_counts_below_zero_and_above_the_padded_length(v, dtype):
    """`plane_objects` clamps a sample's count to [0, n_max]: -3 draws nothing, n_max + 7 draws every slot, as int32 and int64"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    cs = hc.box_edges(v.TW, v.TH, v.odd)
    n_max = cs.radii.shape[1]
    cs.radii[cs.radii == 50] = 1                                    # (the padded slots of the case: now drawn by plane 1)
    cs.counts = np.array([-3, n_max + 7, 2], dtype=np.int64)
    base = hc.base_map((3, cs.H, cs.W))
    ref = hc.oracle_batched(cs, clear=v.clear, base=base)
    assert float(np.abs(ref[0] - (0.0 if v.clear else base[0])).max()) == 0.0 and bool((ref[1] != (0.0 if v.clear else base[1])).any())
    hm = torch.full((3, cs.H, cs.W), 123.0, device=DEV) if v.clear else torch.from_numpy(base).to(DEV)
    n = _t(cs.counts, dtype)
    draw_heatmap_batched(hm, rb(_t(cs.centers, np.int32), n), rb(_t(cs.radii, np.int32), n), 6.0, cs.k, clear=v.clear, **v.kwargs)
    assert _nat().last_dispatch() == hc.expected_dispatch(v, 3, cs.H, cs.W)
    assert _err(hm, ref) <= ATOL


# ------------------------------------------------------------------------------------------- linear grids
_HINTS = {"tile": {}, "small": dict(small_radii=True)}


@pytest.mark.parametrize("hint", list(_HINTS))
@pytest.mark.parametrize("clear", [True, False])
def test_flat_call_with_more_planes_than_a_grid_dimension(clear, hint):
    """70 000 planes of 8 x 16: a one-dimensional grid of 70 000 tiles (`locate_tile`'s linear branch from the flat entry
    point), behind the three-kernel binning with 69 planes per thread of the scan"""
    from accvlab.draw_heatmap import draw_heatmap

    cs = hc.many_planes_flat()
    ref = np.zeros((cs.P, cs.H, cs.W), dtype=np.float32) if clear else hc.base_map((cs.P, cs.H, cs.W))
    oracle.draw_heatmap_flat(ref, cs.centers, cs.radii, cs.idx, 6.0, 0.9)
    hm = torch.full((cs.P, cs.H, cs.W), 3.0, device=DEV) if clear else torch.from_numpy(hc.base_map((cs.P, cs.H, cs.W))).to(DEV)
    draw_heatmap(hm, _t(cs.centers, np.int32), _t(cs.radii, np.int32), _t(cs.idx, np.int32), 6.0, 0.9, clear=clear, **_HINTS[hint])
    assert hc.is_linear(_nat().last_dispatch()) == (True, cs.P), _nat().last_dispatch()
    assert ("splat_small_kernel" in _nat().last_dispatch()) == (hint == "small")
    assert _err(hm, ref) <= ATOL


def test_scalar_tiles_on_a_linear_grid_with_two_tile_columns():
    """70 000 planes of 1 x 33 (width off 4: PX = 1, 32-pixel tiles): tile = plane * 2 + column, so both quotients of the
    linear branch's divisions matter"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    P, H, W, n_max = hc.GRID_Z + 4465, 1, 33, 3
    p, i = np.meshgrid(np.arange(P), np.arange(n_max), indexing="ij")
    c = np.stack([(p * 7 + i * 13) % (W + 2) - 1, np.zeros_like(p)], -1)
    r = (p + i) % 3
    counts = p[:, 0] % (n_max + 1)
    ref = np.zeros((P, H, W), dtype=np.float32)
    oracle.draw_heatmap_batched(ref, c, r, counts, clear=True)
    hm = torch.full((P, H, W), 2.0, device=DEV)
    draw_heatmap_batched(hm, rb(_t(c, np.int32), _t(counts, np.int64)), rb(_t(r, np.int32), _t(counts, np.int64)), clear=True)
    assert _nat().last_dispatch() == f"splat_kernel<PX=1,R=8,CLEAR=1,SM=0> grid({2 * P},1,1) block(64)"
    assert _err(hm, ref) <= ATOL
    assert ref[hc.GRID_Z:, 0, 32].max() > 0 and ref[hc.GRID_Z:, 0, :32].max() > 0      # both tile columns, past the grid limit


@pytest.mark.parametrize("hint", list(_HINTS))
@pytest.mark.parametrize("clear", [True, False])
def test_classwise_call_with_more_planes_than_a_grid_dimension(clear, hint):
    """7 x 10 000 class planes of 4 x 8: the linear tile's plane splits into (sample, class) by `plane / n_classes`; labels -1
    and C are drawn nowhere; a count above the padded length is clamped"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    cw = hc.many_planes_classwise()
    shape = (cw.B, cw.C, cw.H, cw.W)
    ref = np.zeros(shape, dtype=np.float32) if clear else hc.base_map(shape)
    oracle.draw_heatmap_batched(ref, cw.centers, cw.radii, cw.counts, labels=cw.labels, k=0.9, clear=clear)
    hm = torch.full(shape, 3.0, device=DEV) if clear else torch.from_numpy(hc.base_map(shape)).to(DEV)
    n = _t(cw.counts, np.int64)
    draw_heatmap_batched(hm, rb(_t(cw.centers, np.int32), n), rb(_t(cw.radii, np.int32), n), 6.0, 0.9, rb(_t(cw.labels, np.int32), n),
                         clear=clear, **_HINTS[hint])
    assert hc.is_linear(_nat().last_dispatch()) == (True, cw.B * cw.C), _nat().last_dispatch()
    assert _err(hm, ref) <= ATOL


@pytest.mark.parametrize("tile_rows", [hc.GRID_Y - 1, hc.GRID_Y, hc.GRID_Y + 1], ids=["65535_rows", "65536_rows", "65537_rows"])
def test_more_tile_rows_than_a_grid_dimension(tile_rows):
    """H = 16 n + 1, W = 4 (16 MB): n + 1 tile rows of the 128 x 16 kernels on either side of the 3-D grid's limit; objects in
    the first, a middle and the last tile row.  The tile kernel in place and fused clear, the small-splat kernel, the scalar
    tiles (base off 16 bytes); two samples, where the linear tile's plane is a quotient by 65 537"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    linear = tile_rows + 1 > hc.GRID_Y
    for B in ((1, 2) if tile_rows == hc.GRID_Y + 1 else (1,)):
        cs = hc.many_tile_rows(tile_rows, B=B)
        c, r, n = _t(cs.centers, np.int32), _t(cs.radii, np.int32), _t(cs.counts, np.int64)
        ref = np.zeros((B, cs.H, cs.W), dtype=np.float32)
        oracle.draw_heatmap_batched(ref, cs.centers, cs.radii, cs.counts, k=0.9, clear=True)
        runs = [("clear", dict(clear=True)), ("small", dict(clear=True, small_radii=True))] if B == 1 else [("clear", dict(clear=True))]
        for what, kw in runs:
            hm = torch.full((B, cs.H, cs.W), 5.0, device=DEV)
            draw_heatmap_batched(hm, rb(c, n), rb(r, n), 6.0, 0.9, tile_rows=8, **kw)
            d = _nat().last_dispatch()
            assert hc.is_linear(d) == ((True, B * (tile_rows + 1)) if linear else (False, 1)), d
            assert ("splat_small_kernel" in d) == (what == "small")
            assert _err(hm, ref) <= ATOL, what
        if B == 1:
            base = torch.full((1, cs.H, cs.W), -0.5, device=DEV)
            base[0, ::7] = 0.6                                        # above most of what is drawn
            want = base.cpu().numpy().copy()
            oracle.draw_heatmap_batched(want, cs.centers, cs.radii, cs.counts, k=0.9)
            hm = base.clone()
            draw_heatmap_batched(hm, rb(c, n), rb(r, n), 6.0, 0.9, tile_rows=8)
            assert "CLEAR=0,SM=5" in _nat().last_dispatch() and hc.is_linear(_nat().last_dispatch())[0] == linear
            assert _err(hm, want) <= ATOL
            buf = torch.full((cs.H * cs.W + 8,), 7.0, device=DEV)
            off = buf[1:1 + cs.H * cs.W].view(1, cs.H, cs.W)
            draw_heatmap_batched(off, rb(c, n), rb(r, n), 6.0, 0.9, clear=True)
            assert "PX=1" in _nat().last_dispatch() and hc.is_linear(_nat().last_dispatch())[0] == linear
            assert _err(off, ref) <= ATOL


def test_taller_tiles_bring_the_tile_rows_back_under_the_limit():
    """the same map with 128 x 32 tiles has 32 769 tile rows: a 3-D grid again, the same map bit for bit"""
    from accvlab.draw_heatmap import draw_heatmap_batched

    cs = hc.many_tile_rows(hc.GRID_Y + 1)
    c, r, n = _t(cs.centers, np.int32), _t(cs.radii, np.int32), _t(cs.counts, np.int64)
    a, b = torch.empty((1, cs.H, cs.W), device=DEV), torch.empty((1, cs.H, cs.W), device=DEV)
    draw_heatmap_batched(a, rb(c, n), rb(r, n), clear=True, tile_rows=16)
    assert _nat().last_dispatch() == "splat_kernel<PX=4,R=16,CLEAR=1,SM=0> grid(1,32769,1) block(64)"
    draw_heatmap_batched(b, rb(c, n), rb(r, n), clear=True, tile_rows=8)
    assert hc.is_linear(_nat().last_dispatch()) == (True, hc.GRID_Y + 2)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- flat API: binning, thresholds
@pytest.mark.parametrize("name", list(hc.BINNING))
def test_flat_binning_boundaries(name):
    """1 025 / 8 192 / 8 193 planes, 65 536 / 65 537 objects, 262 145 objects: both binning paths on either side of the host
    rule, the second trip of every loop over planes and objects.  The last object alone draws one pixel; plane indices -1 and
    P are ignored"""
    from accvlab.draw_heatmap import draw_heatmap

    P, N, path = hc.BINNING[name]
    assert hc.bin_path(P, N) == path and not hc.flat_direct(P, 8, 16, N)
    cs = hc.flat_binning(P, N)
    for clear in (True, False):
        ref = np.zeros((P, cs.H, cs.W), dtype=np.float32) if clear else hc.base_map((P, cs.H, cs.W))
        oracle.draw_heatmap_flat(ref, cs.centers, cs.radii, cs.idx, 6.0, 0.9)
        hm = torch.full((P, cs.H, cs.W), 4.0, device=DEV) if clear else torch.from_numpy(hc.base_map((P, cs.H, cs.W))).to(DEV)
        draw_heatmap(hm, _t(cs.centers, np.int32), _t(cs.radii, np.int32), _t(cs.idx, np.int32), 6.0, 0.9, clear=clear)
        assert _nat().last_dispatch().startswith(f"splat_kernel<PX=4,R=8,CLEAR={int(clear)},")
        assert _err(hm, ref) <= ATOL, clear
        if clear:
            assert float(hm[cs.last]) == np.float32(0.9)


class _Spy:
    """the library binding with the names of the entry points that were called"""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        if name.startswith("accv_draw_heatmap") and name.endswith("_f32"):
            self.called.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("which", list(hc.FLAT_DIRECT_EDGES))
def test_flat_direct_thresholds_either_side(which, monkeypatch):
    """2 048 / 2 049 objects, 65 535 / 65 536 planes, tiles x rounds 200 000 / 250 000: the flat call as ONE class-wise launch
    on the near side, binning + flat entry point on the far side; the same map from either (bit for bit with the binned path
    forced on the near side's input), the oracle's to 1e-5"""
    from accvlab.draw_heatmap import draw_heatmap, ops

    nat = _nat()
    for side, (P, H, W, N) in zip(("direct", "binned"), hc.FLAT_DIRECT_EDGES[which]):
        c, r, idx = hc.flat_objects(P, H, W, N)
        ref = np.zeros((P, H, W), dtype=np.float32)
        oracle.draw_heatmap_flat(ref, c, r, idx, 6.0, 0.9)
        args = (_t(c, np.int32), _t(r, np.int32), _t(idx, np.int32), 6.0, 0.9)
        spy = _Spy(nat.lib())
        with monkeypatch.context() as m:
            m.setattr(ops._nat, "lib", lambda spy=spy: spy)
            hm = torch.full((P, H, W), 4.0, device=DEV)
            draw_heatmap(hm, *args, clear=True)
        assert spy.called == ["accv_draw_heatmap_batched_f32" if side == "direct" else "accv_draw_heatmap_flat_f32"], (side, spy.called)
        d = nat.last_dispatch()
        assert hc.is_linear(d) == ((True, P) if P > hc.GRID_Z else (False, 1)), d
        assert _err(hm, ref) <= ATOL, side
        if side == "direct":
            with monkeypatch.context() as m:
                m.setattr(ops, "_FLAT_DIRECT_MAX_OBJECTS", 0)
                binned = torch.full((P, H, W), 4.0, device=DEV)
                draw_heatmap(binned, *args, clear=True)
            assert torch.equal(hm, binned)


# ------------------------------------------------------------------------------------------- multi-scale prologue
def _float_objects(B, sw, sh):
    from accvlab.batching_helpers import combine_data

    cs, bs = [], []
    for b in range(B):
        n = 6 - 2 * b
        i = torch.arange(n, dtype=torch.float32)
        c = torch.stack([(37.0 + 83.0 * i + 11.0 * b) % sw, (9.0 + 13.0 * i + 5.0 * b) % sh], 1)
        half = torch.stack([3.0 + 2.0 * i, 2.0 + i, 4.0 + i, 2.5 + 1.5 * i], 1)
        cs.append(c)
        bs.append(torch.cat([c - half[:, :2], c + half[:, 2:]], 1))
    crb = combine_data(cs, device=torch.device(DEV))
    return crb, combine_data(bs, device=torch.device(DEV), other_with_same_sample_sizes=crb)


@pytest.mark.parametrize("clear", [True, False])
@pytest.mark.parametrize("scales", [(0,), (0, 2), (0, 1, 2), (3, 1, 2, 0), (3, 0, 2, 4)], ids=lambda s: "scales_" + "".join(map(str, s)))
def test_multiscale_prologue(scales, clear):
    """one to four scales in one launch; a scale of zero extent between two others (skipped: three scales remain); scales of ONE
    tile (full and partial) next to one of nine; the default order (fewest tiles first) and the caller's.  Equal to the per-scale
    operators bit for bit, to the oracle on their integer targets to 1e-5; the grid is the sum of the scales' tiles"""
    from accvlab.draw_heatmap import draw_heatmap_batched, draw_heatmap_multiscale, get_centers_and_radii, ops

    nat = _nat()
    B, sw, sh = 2, 528.0, 70.0
    # (stride, H, W): one full tile; zero rows; 3 x 3 tiles; one partial tile; one tile row of three
    table = [(8.0, 16, 128), (4.0, 0, 8), (2.0, 35, 264), (16.0, 5, 36), (2.0, 9, 264)]
    crb, brb = _float_objects(B, sw, sh)
    strides = [table[s][0] for s in scales]
    tiles = sum(B * -(-table[s][2] // 128) * -(-table[s][1] // (2 * hc.BOX_TILE_R)) for s in scales)
    base = [torch.from_numpy(hc.base_map((B, table[s][1], table[s][2]))).to(DEV) for s in scales]
    results = []
    for flag in (0, nat.HM_CALLER_SCALE_ORDER):
        maps = [t.clone() for t in base]
        ops._FORCED_FLAGS = flag
        try:
            draw_heatmap_multiscale(maps, crb, brb, strides, 6.0, 0.8, clear=clear)
        finally:
            ops._FORCED_FLAGS = 0
        assert nat.last_dispatch() == f"splat_multi_kernel<PX=4,R=8,CLEAR={int(clear)},SM=0> grid({tiles},1,1) block(64)", nat.last_dispatch()
        results.append(maps)
    for i, s in enumerate(scales):
        assert torch.equal(results[0][i], results[1][i])
        if table[s][1] == 0:
            continue
        ci, ri = get_centers_and_radii(crb, brb, strides[i])
        ref = base[i].clone()
        draw_heatmap_batched(ref, ci, ri, 6.0, 0.8, clear=clear)
        assert torch.equal(results[0][i], ref), f"scale {s}"
        want = base[i].cpu().numpy().copy()
        oracle.draw_heatmap_batched(want, ci.tensor.cpu().numpy(), ri.tensor.cpu().numpy(), crb.sample_sizes.cpu().numpy(), k=0.8, clear=clear)
        assert _err(results[0][i], want) <= ATOL
        assert float(want.max()) > 0.75 or not clear              # an object's centre lies on every map


# ------------------------------------------------------------------------------------------- lane raster: group-box rounds
@pytest.mark.parametrize("stride,waves", [(4.0, 4), (1.0, 1)])
@pytest.mark.parametrize("clear", [True, False])
def test_point_splat_with_more_than_64_sample_groups(stride, waves, clear):
    """5 lanes x 1 024 samples per frame = 80 groups of 64: the two-level cull's loop over rounds of 64 group boxes takes a
    second trip, which holds the last lane.  Four waves per tile (a coarse map) and one (a fine map), against the three-launch
    formulation through integer targets bit for bit and the oracle on those targets"""
    from accvlab.draw_heatmap import draw_polylines_multiscale, sample_lane_targets
    from accvlab.draw_heatmap.lanes import _draw_polylines_via_targets as via_targets

    nat = _nat()
    B, L, P, Q, radius = 2, 5, 12, 1024, 2
    sw, sh = (2048.0, 512.0) if waves == 1 else (1024.0, 256.0)
    j = torch.arange(P, dtype=torch.float32)
    pts = torch.zeros(B, L, P, 2)
    for b in range(B):
        for lane in range(L):
            pts[b, lane, :, 0] = 20.0 + (sw - 40.0) * j / (P - 1)
            pts[b, lane, :, 1] = 30.0 + (sh - 60.0) * lane / (L - 1) + 9.0 * (j % 2) + 3.0 * b
    pts = pts.to(DEV)
    assert L * Q // 64 > hc.KCAND and (L - 1) * Q // 64 >= hc.KCAND          # the last lane's groups are all in the second round
    H, W = int(sh / stride), int(sw / stride)
    base = torch.from_numpy(hc.base_map((B, H, W)) * 0.5).to(DEV)
    got = base.clone()
    draw_polylines_multiscale([got], pts, Q, radius, [stride], 6.0, 0.9, clear=clear)
    d = nat.last_dispatch()
    assert d.startswith("splat_points_multi_kernel") and f"block({64 * waves})" in d, d
    ref = base.clone()
    via_targets(ref, pts, Q, radius, stride, 6.0, 0.9, clear=clear)
    assert torch.equal(got, ref)
    centers, radii = sample_lane_targets(pts, Q, radius, stride)
    want = base.cpu().numpy().copy()
    oracle.draw_heatmap_batched(want, centers.cpu().numpy(), radii.cpu().numpy(), np.full(B, L * Q), k=0.9, clear=clear)
    assert _err(got, want) <= ATOL
    last_lane_row = int((30.0 + (sh - 60.0)) / stride)
    assert float(want[0, last_lane_row].max()) > (0.85 if clear else 0.0) and float(got[0, last_lane_row].max()) >= 0.89


# ------------------------------------------------------------------------------------------- front-end kernels
def test_target_kernels_grid_stride_second_trip():
    """targets_from_boxes_kernel / targets_from_points_kernel run at most 4 096 workgroups of 256: 1 048 576 + 3 objects put
    three in the second trip of the grid-stride loop.  Boxes against the CPU path of the operator (bit for bit, as the suite
    holds it), points against float32 numpy (IEEE division) with NaN points -> radius -1"""
    from accvlab.draw_heatmap import get_centers_and_radii

    nat = _nat()
    n = hc.TARGETS_GRID_CAP * hc.TARGETS_THREADS + 3
    i = torch.arange(n, dtype=torch.float32)
    c = torch.stack([(i * 0.37) % 1900.0, (i * 0.73) % 1000.0], 1)
    half = torch.stack([5.0 + 3.0 * (i % 7.0), 6.0 + 4.0 * (i % 5.0), 5.5 + 6.0 * (i % 3.0), 4.5 + 2.0 * (i % 11.0)], 1)
    boxes = torch.cat([c - half[:, :2], c + half[:, 2:]], 1)
    gc, gr = get_centers_and_radii(c.to(DEV), boxes.to(DEV), 4.0)
    wc, wr = get_centers_and_radii(c, boxes, 4.0)
    assert torch.equal(gc.cpu(), wc) and torch.equal(gr.cpu(), wr)
    assert int(wr.min()) >= 2 and int(wr.max()) >= 4 and len(set(wr[-3:].tolist()) | set(wc[-3:].flatten().tolist())) > 2

    pts = c.clone()
    pts[5] = float("nan")
    pts[n - 2, 1] = float("nan")
    out_c = torch.full((n, 2), -9, dtype=torch.int32, device=DEV)
    out_r = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    nat.check(nat.lib().accv_heatmap_targets_from_points_f32(pts.to(DEV).data_ptr(), n, 3.0, 2, out_c.data_ptr(), out_r.data_ptr(),
                                                            nat.stream_ptr(torch.device(DEV))), "targets_from_points")
    p = pts.numpy()
    bad = np.isnan(p).any(1)
    with np.errstate(invalid="ignore"):
        want_c = np.where(bad[:, None], 0, (p / np.float32(3.0)).astype(np.int32))
    assert np.array_equal(out_c.cpu().numpy(), want_c)
    assert np.array_equal(out_r.cpu().numpy(), np.where(bad, -1, 2))
