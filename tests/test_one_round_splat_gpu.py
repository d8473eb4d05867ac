"""The fused-clear splat wave with 128 x 32 pixel tiles (`tile_rows=16`: what a one-round launch runs) against the 128 x 16
tiles bit for bit and against the CPU oracle to 1e-5, at the places where the wave's accumulate chain changes shape: a tile whose
running hit count passes 8 / 11 / 14 (the steps of the hit-count classes tried for the wave's issue priority) within
one cull round and across rounds, one / two / three cull rounds, pairs of hits and the odd one left over, column factors evaluated by one half-wave and handed to the other (box edges inside a
lane's four columns, boxes that end on the half-wave boundary), partial tiles in both directions."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import h1 as oracle

pytestmark = pytest.mark.gpu
ATOL = 1e-5
DEV = "cuda:0"


def rb(t, sizes):
    return SimpleNamespace(tensor=t, sample_sizes=sizes)


def _check(centers, radii, counts, H, W, k=1.0, factor=6.0):
    """centers [B, N, 2], radii [B, N], counts [B] (numpy): rows16 == rows8 bit for bit, both within ATOL of the oracle"""
    from accvlab import _amd_native as nat
    from accvlab.draw_heatmap import draw_heatmap_batched

    B = len(counts)
    c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.int32)).to(DEV)
    r = torch.from_numpy(np.ascontiguousarray(radii, dtype=np.int32)).to(DEV)
    n = torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(DEV)
    tall = torch.full((B, H, W), 123.0, device=DEV)      # clear=True must ignore what was there
    flat = torch.full((B, H, W), -7.0, device=DEV)
    draw_heatmap_batched(tall, rb(c, n), rb(r, n), factor, k, clear=True, tile_rows=16)
    assert nat.last_dispatch().startswith("splat_kernel<PX=4,R=16,CLEAR=1,SM=0>"), nat.last_dispatch()
    draw_heatmap_batched(flat, rb(c, n), rb(r, n), factor, k, clear=True, tile_rows=8)
    assert nat.last_dispatch().startswith("splat_kernel<PX=4,R=8,CLEAR=1,SM=0>"), nat.last_dispatch()
    assert torch.equal(tall, flat)
    ref = np.full((B, H, W), 55.0, dtype=np.float32)
    oracle.draw_heatmap_batched(ref, np.asarray(centers, dtype=np.int32), np.asarray(radii, dtype=np.int32),
                                np.asarray(counts, dtype=np.int64), factor=factor, k=k, clear=True)
    err = float(np.abs(tall.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max())
    assert err <= ATOL, err
    return tall


def _in_one_tile(rng, B, N, H, W, tile_x, tile_y, rmax):
    """N objects per plane, every centre inside the 128 x 32 tile (tile_x, tile_y), clipped to the map"""
    x0, y0 = tile_x * 128, tile_y * 32
    cx = rng.integers(x0, min(x0 + 128, W), (B, N))
    cy = rng.integers(y0, min(y0 + 32, H), (B, N))
    return np.stack([cx, cy], -1), rng.integers(0, rmax + 1, (B, N))


@pytest.mark.parametrize("W", [128, 132, 260])
@pytest.mark.parametrize("H", [31, 32, 33, 48])
def test_small_maps_all_objects_in_one_tile(H, W):
    """B = 2; per-plane counts 0, 1, 64, 65, 130 (no / one / two / three cull rounds), every object centred in ONE tile — that
    tile holds every hit of its plane (tens of hits, spanning rounds, even and odd hit counts) while
    its neighbours get the few that reach them; partial tiles in both directions and the W % 4 == 0 edge off the 128 grid"""
    rng = np.random.default_rng(1000 * H + W)
    for counts, tile in (((0, 130), (0, 0)), ((1, 65), ((W - 1) // 128, (H - 1) // 32)), ((64, 130), (min(1, (W - 1) // 128), 0)),
                         ((65, 1), (0, (H - 1) // 32))):
        c, r = _in_one_tile(rng, 2, 130, H, W, tile[0], tile[1], rmax=40)
        _check(c, r, counts, H, W)


@pytest.mark.parametrize("k", [1.0, -0.75, 2.5])
def test_hits_of_one_tile_pass_8_11_14_round_by_round(k):
    """tile (1, 0) of a 48 x 260 map collects a chosen number of hits in each of the three cull rounds of a 130-object plane,
    so that its running hit count passes 8 / 11 / 14 in different rounds (or not at all); the other objects of
    every round sit in tile (0, 1) with radii that do not reach tile (1, 0)"""
    H, W, N = 48, 260, 130
    rng = np.random.default_rng(7)
    per_round = ((5, 4, 2), (7, 1, 2), (3, 9, 2), (10, 1, 0), (13, 1, 1), (9, 5, 0), (2, 2, 1), (14, 0, 2))   # running: 5 9 11 | 7 8 10 | 3 12 14 | ...
    B = len(per_round)
    c = np.zeros((B, N, 2), dtype=np.int64)
    r = np.zeros((B, N), dtype=np.int64)
    for b, (h1, h2, h3) in enumerate(per_round):
        c[b, :, 0], c[b, :, 1], r[b] = rng.integers(0, 100, N), rng.integers(40, 48, N), rng.integers(0, 6, N)   # tile (0, 1) only
        chosen = list(rng.choice(64, h1, replace=False)) + list(64 + rng.choice(64, h2, replace=False)) + list(128 + rng.choice(2, h3, replace=False))
        for j in chosen:
            c[b, j] = (rng.integers(140, 250), rng.integers(4, 28))
            r[b, j] = rng.integers(1, 30)
    _check(c, r, [N] * B, H, W, k=k)


def test_box_edges_inside_a_lane_and_on_the_half_wave_boundary():
    """clipped boxes whose left / right edges fall at x % 4 = 1, 2, 3 (inside the four columns one lane holds, so the mask of a
    column factor differs between neighbouring columns of one lane) and boxes whose last row is 15 or whose first row is 16 of
    a 32-row tile (the two half-waves of the tall tile; the tile boundary of the flat one), alone and as pairs"""
    H, W = 48, 260
    objs = []
    for left in (1, 2, 3):
        for right in (1, 2, 3):
            # box columns [x - r, x + r + 1): choose r, then x with (x - r) % 4 == left and (x + r + 1) % 4 == right
            for r in range(2, 12):
                for x in range(r, W - r):
                    if (x - r) % 4 == left and (x + r + 1) % 4 == right:
                        break
                else:
                    continue
                objs.append((x + 128 * (left % 2), 15 - r, r))      # last row 15
                objs.append((x + 128 * (right % 2), 16 + r, r))     # first row 16
                break
    objs += [(130, 15, 0), (131, 16, 0), (129, 10, 5), (255, 21, 5), (258, 40, 3), (127, 31, 7)]
    assert any((x - r) % 4 == 1 for x, _, r in objs) and any((x + r + 1) % 4 == 3 for x, _, r in objs)
    n = len(objs)
    c = np.zeros((3, n, 2), dtype=np.int64)
    r = np.zeros((3, n), dtype=np.int64)
    for b in range(3):
        order = np.random.default_rng(b).permutation(n)      # other pairings of the hits
        c[b] = np.array([(o[0], o[1]) for o in objs])[order]
        r[b] = np.array([o[2] for o in objs])[order]
    _check(c, r, [n, n - 1, 1], H, W)


@pytest.mark.parametrize("k", [1.0, -1.0])
def test_radius_zero_and_centres_off_the_map(k):
    """radius 0 (one pixel), centres left / right / above / below the map whose boxes reach in, and ones that do not; k < 0
    (every product is negative: the cleared zero wins inside the boxes too)"""
    H, W = 33, 132
    rng = np.random.default_rng(3)
    N = 70
    c = np.stack([rng.integers(-40, W + 40, (2, N)), rng.integers(-40, H + 40, (2, N))], -1)
    r = rng.integers(0, 45, (2, N))
    r[:, ::3] = 0
    c[0, :4] = [(0, 0), (W - 1, H - 1), (W, H), (-1, -1)]
    r[0, :4] = [0, 0, 1, 1]
    c[1, :4] = [(-30, 16), (W + 29, 15), (64, -20), (65, H + 19)]
    r[1, :4] = [30, 30, 20, 20]
    _check(c, r, [N, 65], H, W, k=k)


def test_a_launch_the_one_round_rule_selects():
    """8 x 1080 x 1920 with 128 objects of radius >= 200 per frame: the dispatch takes the 128 x 32 tiles by itself (4080 tiles,
    all resident at once), every tile has tens of hits in two cull rounds, and the map equals the 128 x 16 draw bit for bit"""
    from accvlab import _amd_native as nat
    from accvlab.draw_heatmap import draw_heatmap_batched

    frames, h, w, n_obj = 8, 1080, 1920, 128
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert frames * 15 * 68 > 24 * cus and frames * 15 * 34 <= 16 * cus, "the test's shape assumes 256 compute units"
    g = torch.Generator().manual_seed(5)
    c = torch.stack([torch.randint(0, w, (frames, n_obj), generator=g), torch.randint(0, h, (frames, n_obj), generator=g)], -1).int().to(DEV)
    r = torch.randint(200, 420, (frames, n_obj), generator=g).int().to(DEV)
    n = torch.full((frames,), n_obj, dtype=torch.int64, device=DEV)
    got = torch.full((frames, h, w), 9.0, device=DEV)
    draw_heatmap_batched(got, rb(c, n), rb(r, n), clear=True)
    assert "R=16" in nat.last_dispatch(), nat.last_dispatch()
    ref = torch.full((frames, h, w), -3.0, device=DEV)
    draw_heatmap_batched(ref, rb(c, n), rb(r, n), clear=True, tile_rows=8)
    assert "R=8" in nat.last_dispatch()
    assert torch.equal(got, ref)
    assert 0.0 <= float(got.min()) and 0.99 < float(got.max()) <= 1.0      # every centre on the map: its pixel holds k = 1
