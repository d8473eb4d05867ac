"""The cases of h1_partition_cases.py without a GPU: every case is in the regime it names, by the numpy
restatement of the cull; the CPU oracle draws something for it and draws something else once the hits the case is named
for are taken out (a case that cannot fail tests nothing); the host rules (`_flat_direct`, the binning rule, the launch
geometry) sit where the cases assume them; and the two division-free index computations of `walk_hits` equal integer
division over their whole range."""
import numpy as np
import pytest

import h1_partition_cases as hc
from oracle import h1 as oracle


def _geom_id(g):
    return f"{g[0]}x{g[1]}{'_odd' if g[2] else ''}"


# ------------------------------------------------------------------------------------------- structural cases
@pytest.mark.parametrize("geom", hc.GEOMETRIES, ids=_geom_id)
@pytest.mark.parametrize("name", list(hc.STRUCTURAL))
def test_structural_cases_are_in_their_regime_and_the_oracle_sees_their_hits(name, geom):
    TW, TH, odd = geom
    cs = hc.STRUCTURAL[name](TW, TH, odd)
    assert (cs.W % 4 != 0) == odd and -(-cs.W // TW) == 3 and -(-cs.H // TH) == 3      # 3 x 3 tiles, the last ones partial
    assert cs.W % TW != 0 and cs.H % TH != 0
    for plane, tile, want in cs.named:
        assert hc.tile_rounds(cs, plane, tile, TW, TH) == want, (plane, tile)
    base = hc.base_map((len(cs.counts), cs.H, cs.W), cs.k)
    # (k < 0: the cleared zero wins everywhere, so the draw shows in place only)
    draw = (lambda radii=None: hc.oracle_batched(cs, clear=True, radii=radii)) if cs.k > 0 else \
        (lambda radii=None: hc.oracle_batched(cs, clear=False, base=base, radii=radii))
    full = draw()
    assert np.isfinite(full).all() and float(np.abs(full).max()) > 0.0
    gone = draw(hc.without(cs, cs.target))
    for b in range(len(cs.counts)):
        if cs.target[b, :int(cs.counts[b])].any() and b != getattr(cs, "drawn_by_none", -1):
            assert not np.array_equal(full[b], gone[b]), b
    inplace = hc.oracle_batched(cs, clear=False, base=base)
    # in place: some pixels keep the old map (above what is drawn), some are raised: a repeated or a missing first-touch
    # load changes the result
    assert bool((inplace == base).any()) and bool((inplace != base).any())
    touched = inplace != base
    assert bool((base[touched] != 0).all()), "a raised pixel whose old value a zero-initialised accumulator would lose"


@pytest.mark.parametrize("geom", hc.GEOMETRIES, ids=_geom_id)
def test_round_splits_name_every_split(geom):
    TW, TH, odd = geom
    cs = hc.round_splits(TW, TH, odd)
    seen = {want for _, _, want in cs.named}
    # first touched in round 1, 2 and 3; a round without hits between two with hits; 64 hits in a round; no hit at all
    assert {(3, 0, 0), (0, 4, 0), (0, 0, 1), (0, 0, 2), (5, 0, 2), (64, 0, 0), (64, 64, 2), (0, 64, 1), (0, 0, 0)} <= seen
    assert {int(c) for c in cs.counts} >= {0, 1, hc.KCAND, hc.KCAND + 1, 2 * hc.KCAND + 2}           # 0, 1, 64, 65, 130 candidates
    assert any(sum(w) % 2 for w in seen) and any(sum(w) % 2 == 0 and sum(w) for w in seen)
    # the row table's loop `t += 64`: nh * TH on both sides of 64
    per_round_hits = {h for w in seen for h in w if h}
    assert any(h * TH <= 64 for h in per_round_hits) and any(h * TH > 64 for h in per_round_hits)
    # the other slots sit in tile (0, 1) and nowhere else: the target tile has a round WITHOUT hits while the launch has none
    for plane, tile, want in cs.named:
        n = int(cs.counts[plane])
        filler = hc.tile_rounds(cs, plane, hc.FILLER_TILE, TW, TH)
        assert sum(filler) + sum(want) >= n - sum(want) or n == 0
    # a round's hits show in the oracle: without them a sparse plane differs (crowded planes repeat centres), and a plane
    # without hits in that round never does
    full = hc.oracle_batched(cs, clear=True)
    for q in range(3):
        mask = cs.target.copy()
        mask[:, :q * hc.KCAND] = False
        mask[:, (q + 1) * hc.KCAND:] = False
        gone = hc.oracle_batched(cs, clear=True, radii=hc.without(cs, mask))
        for plane, _, want in cs.named:
            differs = not np.array_equal(full[plane], gone[plane])
            assert differs == (want[q] > 0) or (sum(want) > 10 and want[q] > 0), (plane, q)


@pytest.mark.parametrize("geom", hc.GEOMETRIES, ids=_geom_id)
def test_box_edges_off_map_and_cover_regimes(geom):
    TW, TH, odd = geom
    cs = hc.box_edges(TW, TH, odd)
    plane, slot, tile_xy = cs.whole
    tile = hc.tile_bounds(*tile_xy, TW, TH, cs.H, cs.W)
    box = hc.clipped_boxes(cs.centers[plane], cs.radii[plane], tile, cs.H, cs.W)[slot]
    assert tuple(box) == (0, TW, 0, TH)                 # xhi == 32 PX, yhi == 2 R: the largest value of either byte
    edges = hc.clipped_boxes(cs.centers[0], cs.radii[0], (0, 0, cs.W, cs.H), cs.H, cs.W)
    assert {1, 2, 3} <= set((edges[:, 0] % 4).tolist()) and {1, 2, 3} <= set((edges[:, 1] % 4).tolist())
    R = TH // 2
    assert R in edges[:, 3].tolist() and R in edges[:, 2].tolist()      # last row R - 1, first row R

    cs = hc.off_map(TW, TH, odd)
    plane, slot = cs.empty_box
    for ty in range(3):
        for tx in range(3):
            tile = hc.tile_bounds(tx, ty, TW, TH, cs.H, cs.W)
            assert hc.cull(cs.centers[plane], cs.radii[plane], int(cs.counts[plane]), tile)[slot]     # passes the cull everywhere
            assert not hc.clipped_boxes(cs.centers[plane], cs.radii[plane], tile, cs.H, cs.W)[slot].any()   # ... with an empty box
    # plane 1 holds only objects that stop short of the map (or have a negative radius / an empty box): nothing is drawn
    assert float(np.abs(hc.oracle_batched(cs, clear=True)[1]).max()) == 0.0
    whole_map = (0, 0, cs.W, cs.H)
    short = hc.clipped_boxes(cs.centers[1], cs.radii[1], whole_map, cs.H, cs.W)[:int(cs.counts[1])]
    assert not short[np.asarray(cs.radii[1][:int(cs.counts[1])]) >= 0].any()

    cs = hc.cover(TW, TH, odd)
    if not odd:      # the adaptive store policy exists for PX == 4 only
        assert cs.cover[0] < cs.dense_area and cs.cover[1] == cs.dense_area and cs.cover[2] == cs.dense_area + 1
        assert cs.cover[3] < cs.dense_area < cs.cover[4] and cs.dense_area == float(np.float32(0.75) * np.float32(cs.H) * np.float32(cs.W))
        assert max(cs.cover) < 1 << 24          # integers a float adds exactly, in any order


# ------------------------------------------------------------------------------------------- the small-splat kernel
def test_small_rows_has_more_hits_than_one_pass_at_every_height():
    cs = hc.small_rows()
    assert sorted({rows for _, _, rows in cs.named}) == list(range(1, 8))
    assert [w for _, w in hc.rows_hint_planes() if w != "inside"].count("top") == 3
    full = hc.oracle_batched(cs, clear=True)
    for plane, tile, rows in cs.named:
        nh, tallest = hc.round_rows(cs, plane, tile, hc.SMALL_TW, hc.SMALL_TH)
        per_pass = 64 // rows
        assert (nh, tallest) == (hc.KCAND, rows)
        assert nh > per_pass or rows == 1          # rows == 1: a pass takes the 64 hits a round can have
        # no other tile of the plane sees a taller box, and the hits of the later passes show in the oracle
        for ty in range(3):
            for tx in range(3):
                if (tx, ty) != tile:
                    assert hc.round_rows(cs, plane, (tx, ty), hc.SMALL_TW, hc.SMALL_TH)[0] == 0
        if rows > 1:
            later = np.zeros(cs.radii.shape, dtype=bool)
            later[plane, per_pass:] = True          # every slot is a hit: hit h is slot h
            gone = hc.oracle_batched(cs, clear=True, radii=hc.without(cs, later))
            assert not np.array_equal(full[plane], gone[plane])


def test_small_walk_and_fetch_regimes():
    cs = hc.small_walk()
    for plane, tile, nh, rows in cs.named:
        assert hc.round_rows(cs, plane, tile, hc.SMALL_TW, hc.SMALL_TH) == (nh, rows)
    assert cs.named[0][2] > 2 * 4                    # more than two trips of `h0 += 4`
    plane, slot, tile_xy = cs.whole
    tile = hc.tile_bounds(*tile_xy, hc.SMALL_TW, hc.SMALL_TH, cs.H, cs.W)
    assert tuple(hc.clipped_boxes(cs.centers[plane], cs.radii[plane], tile, cs.H, cs.W)[slot]) == (0, 128, 0, 16)
    right = hc.tile_bounds(2, 1, hc.SMALL_TW, hc.SMALL_TH, cs.H, cs.W)
    assert tuple(hc.clipped_boxes(cs.centers[plane], cs.radii[plane], right, cs.H, cs.W)[slot]) == (0, 8, 0, 16)
    empty = int(cs.counts[0]) - 1
    top = hc.tile_bounds(1, 0, hc.SMALL_TW, hc.SMALL_TH, cs.H, cs.W)
    assert hc.cull(cs.centers[0], cs.radii[0], int(cs.counts[0]), top)[empty]
    assert not hc.clipped_boxes(cs.centers[0], cs.radii[0], top, cs.H, cs.W)[empty].any()
    full = hc.oracle_batched(cs, clear=True)
    for plane in range(3):       # every hit shows: without hits 4.. (the later trips of `h0 += 4`) the plane differs
        later = np.zeros(cs.radii.shape, dtype=bool)
        later[plane, 4:int(cs.counts[plane])] = True
        assert not np.array_equal(full[plane], hc.oracle_batched(cs, clear=True, radii=hc.without(cs, later))[plane])
    # in place a tile has dirty and untouched 4-pixel segments
    base = hc.base_map(full.shape)
    inplace = hc.oracle_batched(cs, clear=False, base=base)
    seg = (inplace != base)[2, :hc.SMALL_TH, hc.SMALL_TW:2 * hc.SMALL_TW].reshape(hc.SMALL_TH, -1, 4).any(-1)
    assert bool(seg.any()) and not bool(seg.all())

    cs = hc.small_fetch()
    for plane, tile, want in cs.named:
        assert hc.tile_rounds(cs, plane, tile, hc.SMALL_TW, hc.SMALL_TH) == want
    assert int(cs.counts[0]) > hc.SMALL_FETCH * hc.KCAND
    full = hc.oracle_batched(cs, clear=True)
    assert not np.array_equal(full, hc.oracle_batched(cs, clear=True, radii=hc.without(cs, cs.target)))


# ------------------------------------------------------------------------------------------- launch geometry and host rules
def test_expected_dispatch_restates_the_launch_geometry():
    v = {u.name: u for u in hc.VARIANTS}
    assert hc.expected_dispatch(v["px4_r8_clear_sm0"], 2, 35, 264) == "splat_kernel<PX=4,R=8,CLEAR=1,SM=0> grid(3,3,2) block(64)"
    assert hc.expected_dispatch(v["px4_r16_inplace_sm5"], 2, 67, 264) == "splat_kernel<PX=4,R=16,CLEAR=0,SM=5> grid(3,3,2) block(64)"
    assert hc.expected_dispatch(v["px1_inplace"], 3, 35, 69) == "splat_kernel<PX=1,R=8,CLEAR=0,SM=0> grid(3,3,3) block(64)"
    assert hc.expected_dispatch(v["small_clear_sm4"], 3, 41, 264) == "splat_small_kernel<PX=4,R=8,CLEAR=1,SM=4> grid(3,3,3) block(64)"
    # both sides of either limit of the 3-D grid
    assert hc.expected_grid("splat_kernel", 4, 8, hc.GRID_Z, 4, 8)[0] == (1, 1, hc.GRID_Z)
    assert hc.expected_grid("splat_kernel", 4, 8, hc.GRID_Z + 1, 4, 8)[0] == (hc.GRID_Z + 1, 1, 1)
    assert hc.expected_grid("splat_kernel", 4, 8, 1, 16 * hc.GRID_Y, 4)[0] == (1, hc.GRID_Y, 1)
    assert hc.expected_grid("splat_kernel", 4, 8, 1, 16 * hc.GRID_Y + 1, 4)[0] == (hc.GRID_Y + 1, 1, 1)
    assert hc.expected_grid("splat_kernel", 4, 16, 1, 16 * (hc.GRID_Y + 1) + 1, 4)[0] == (1, 32769, 1)     # taller tiles: 3-D again
    assert hc.expected_grid("splat_kernel", 1, 8, 70000, 1, 33)[0] == (140000, 1, 1)
    assert hc.is_linear("splat_kernel<PX=4,R=8,CLEAR=1,SM=0> grid(70000,1,1) block(64)") == (True, 70000)
    assert hc.is_linear("splat_kernel<PX=4,R=8,CLEAR=1,SM=0> grid(1,1,7) block(64)")[0] is False


def test_linear_grid_cases_and_their_oracle():
    cs = hc.many_planes_flat()
    assert cs.P > hc.GRID_Z and hc.bin_path(cs.P, len(cs.idx)) == "three_kernels" and -(-cs.P // hc.BIN_WG) > 1
    assert not hc.flat_direct(cs.P, cs.H, cs.W, len(cs.idx))
    assert int(cs.idx.min()) < 0 and int(cs.idx.max()) >= cs.P
    ref = np.zeros((cs.P, cs.H, cs.W), dtype=np.float32)
    oracle.draw_heatmap_flat(ref, cs.centers, cs.radii, cs.idx)
    drawn = ref.reshape(cs.P, -1).max(1) > 0
    assert drawn[hc.GRID_Z:].any() and drawn[:hc.GRID_Z].any() and not drawn.all()
    assert all(drawn[m] for m in (0, hc.GRID_Z, cs.P - 1))

    cw = hc.many_planes_classwise()
    assert cw.B * cw.C > hc.GRID_Z and {-1, cw.C} <= set(cw.labels.ravel().tolist())
    assert int(cw.counts.max()) > cw.labels.shape[1]
    ref = np.zeros((cw.B, cw.C, cw.H, cw.W), dtype=np.float32)
    oracle.draw_heatmap_batched(ref, cw.centers, cw.radii, cw.counts, labels=cw.labels)
    per_sample = ref.reshape(cw.B, -1).max(1)
    assert per_sample[0] > 0 and per_sample[cw.B - 1] > 0 and per_sample[2] == 0          # sample 2 has no objects
    assert ref[cw.B - 1, cw.C - 1].max() > 0 and ref[0, 0].max() > 0

    for rows in (hc.GRID_Y, hc.GRID_Y + 1, hc.GRID_Y + 2):
        tall = hc.many_tile_rows(rows)
        assert -(-tall.H // 16) == rows + 1
        ref = np.zeros((1, tall.H, tall.W), dtype=np.float32)
        oracle.draw_heatmap_batched(ref, tall.centers, tall.radii, tall.counts)
        for ty in tall.rows:
            assert ref[0, 16 * ty:16 * ty + 16].max() > 0, ty


@pytest.mark.parametrize("name", list(hc.BINNING))
def test_binning_cases_sit_where_the_host_rule_puts_them(name):
    P, N, path = hc.BINNING[name]
    assert hc.bin_path(P, N) == path
    cs = hc.flat_binning(P, N)
    assert not hc.flat_direct(P, cs.H, cs.W, N)
    assert int(cs.idx.min()) == -1 and int(cs.idx.max()) == P
    ref = np.zeros((P, cs.H, cs.W), dtype=np.float32)
    oracle.draw_heatmap_flat(ref, cs.centers, cs.radii, cs.idx)
    assert ref[cs.last] == 1.0
    ref2 = np.zeros_like(ref)
    oracle.draw_heatmap_flat(ref2, cs.centers[:-1], cs.radii[:-1], cs.idx[:-1])
    assert ref2[cs.last] == 0.0                                   # the object of the last loop trip alone draws that pixel
    assert 0 < int((ref > 0).sum()) < ref.size // 2               # sparse: a dropped or misplaced object shows
    assert ref[P - 1].max() > 0 and ref[min(hc.BIN_WG, P - 1)].max() > 0


def test_binning_boundaries_are_the_constants_of_the_source():
    assert hc.BINNING["planes_1025"][0] == hc.BIN_WG + 1 and -(-hc.BINNING["planes_1025"][0] // hc.BIN_WG) == 2
    assert hc.bin_path(hc.BIN_SMALL_PLANES, hc.BIN_SMALL_OBJECTS) == "bin_small"
    assert hc.bin_path(hc.BIN_SMALL_PLANES + 1, 1) == hc.bin_path(1, hc.BIN_SMALL_OBJECTS + 1) == "three_kernels"
    n = hc.BINNING["objects_262145"][1]
    assert min(-(-n // hc.BIN_THREADS), hc.BIN_GRID_CAP) * hc.BIN_THREADS == n - 1      # exactly one object in the second trip


def test_flat_direct_thresholds():
    from accvlab.draw_heatmap import ops

    assert (ops._FLAT_DIRECT_MAX_OBJECTS, ops._FLAT_DIRECT_MAX_ROUNDS) == (hc.FLAT_DIRECT_MAX_OBJECTS, hc.FLAT_DIRECT_MAX_ROUNDS)
    for which, (direct, binned) in hc.FLAT_DIRECT_EDGES.items():
        assert ops._flat_direct(*direct) is True and hc.flat_direct(*direct), which
        assert ops._flat_direct(*binned) is False and not hc.flat_direct(*binned), which
    p, h, w, n = hc.FLAT_DIRECT_EDGES["rounds"][0]
    assert p * -(-n // hc.KCAND) == hc.FLAT_DIRECT_MAX_ROUNDS                # the last product the single launch takes
    # the restatement agrees with the rule over a grid around every threshold
    for planes in (0, 1, 2, hc.GRID_Z - 1, hc.GRID_Z, hc.GRID_Z + 1):
        for n in (0, 1, 63, 64, 65, 2047, 2048, 2049):
            for h, w in ((0, 8), (1, 1), (16, 128), (17, 129), (270, 480)):
                assert ops._flat_direct(planes, h, w, n) == hc.flat_direct(planes, h, w, n), (planes, h, w, n)


# ------------------------------------------------------------------------------------------- walk_hits' index computations
def test_division_free_row_index_of_the_16_lane_walk_is_exact():
    """`py = (int)(((float)q + 0.5f) * inv_w)` with `inv_w = 1.0f / (float)w` for q / w, w in 1..128 and q in [0, 16 w): every
    box a 128 x 16 tile can hold.  Evaluated in float32 as the device does; the library is compiled with correctly rounded
    float division (no fast-math switch in csrc/Makefile), so numpy's float32 1 / w is the device's inv_w"""
    assert "-ffast-math" not in open(hc.os.path.join(hc._CSRC, "Makefile")).read()
    assert "(int)(((float)q + 0.5f) * inv_w)" in hc._SMALL and "1.0f / (float)max(w, 1)" in hc._SMALL
    bad = 0
    for w in range(1, hc.SMALL_TW + 1):
        q = np.arange(hc.SMALL_TH * w, dtype=np.int64)
        inv_w = np.float32(1.0) / np.float32(w)
        py = ((q.astype(np.float32) + np.float32(0.5)) * inv_w).astype(np.int32)
        bad += int((py != q // w).sum())
    assert bad == 0


def test_division_free_hit_index_of_the_row_walk_is_exact():
    """`hl = (int)((float)lane * (1.0f / (float)rows) + 1e-3f)` for lane / rows, lane in 0..63 and rows in 1..7, in float32;
    and with the product and the sum contracted into one fused multiply-add (one rounding), which the compiler may do: the
    exact value is more than 1e-4 away from the next integer either way"""
    from fractions import Fraction

    assert "(int)((float)lane * (1.0f / (float)rows_hint) + 1e-3f)" in hc._SMALL
    lane = np.arange(64, dtype=np.int64)
    for rows in range(1, 8):
        inv = np.float32(1.0) / np.float32(rows)
        hl = (lane.astype(np.float32) * inv + np.float32(1e-3)).astype(np.int32)
        assert np.array_equal(hl, lane // rows), rows
        for ln in range(64):
            exact = Fraction(ln) * Fraction(float(inv)) + Fraction(float(np.float32(1e-3)))
            assert ln // rows + Fraction(1, 10000) < exact < ln // rows + 1 - Fraction(1, 10000), (ln, rows)
