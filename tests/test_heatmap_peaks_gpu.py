"""Heat-map peak extraction (accvlab.draw_heatmap.heatmap_peaks) against its definition, computed here on the CPU in
float64: max_pool2d local-maximum suppression, then torch.sort(..., descending=True, stable=True) cut at k.  Every output
is compared with torch.equal: the op copies values and indices, so no tolerance applies."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# odd sizes; one chunk (4096 elements) exactly and one row above it; rows below and above a chunk; W past the widest
# chunk (2048 columns, column tiles with halo); the k = group size map
SHAPES = [(2, 37, 53), (2, 3, 37, 53), (1, 1, 64, 64), (1, 1, 65, 64), (1, 2, 128, 33), (2, 1, 7, 2500), (1, 1, 16, 20)]


def reference(heat, k, kernel=3, per_class=False):
    """the definition on the CPU in float64: (scores, indices, classes, ys, xs)"""
    x = heat.detach().cpu().double()
    x4 = x if x.dim() == 4 else x.unsqueeze(1)
    B, C, H, W = x4.shape
    hmax = F.max_pool2d(x4, kernel, stride=1, padding=(kernel - 1) // 2)
    s = x4 * (hmax == x4)
    flat = s.reshape(B * C, H * W) if per_class else s.reshape(B, C * H * W)
    sc, order = torch.sort(flat, dim=1, descending=True, stable=True)
    sc, order = sc[:, :k], order[:, :k]
    if per_class:
        cls = torch.arange(C).repeat(B).unsqueeze(1).expand(-1, k)
        inds = order
    else:
        cls, inds = order // (H * W), order % (H * W)
    out = (sc.to(heat.dtype), inds, cls.contiguous(), inds // W, inds % W)
    if per_class:
        out = tuple(t.reshape(B, C, k) for t in out)
    return out


def run(heat, k, **kw):
    from accvlab.draw_heatmap import heatmap_peaks

    return heatmap_peaks(heat, k, **kw)


def assert_matches(heat, k, **kw):
    got = run(heat, k, **kw)
    want = reference(heat, k, **kw)
    for name, g, w in zip(("scores", "indices", "classes", "ys", "xs"), got, want):
        assert g.dtype == w.dtype, (name, g.dtype, w.dtype)
        assert g.shape == w.shape, (name, tuple(g.shape), tuple(w.shape))
        g = g.cpu()
        if not torch.equal(g, w):
            bad = (g != w).nonzero()[:5].tolist()
            pytest.fail(f"{name} differs ({kw}, k={k}) at {bad}: got {[g[tuple(i)].item() for i in bad]}, "
                        f"want {[w[tuple(i)].item() for i in bad]}")
    return got


def seeded(shape, dtype, seed, fn="randn"):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = getattr(torch, fn)(shape, device=DEV, generator=g)
    return x.to(dtype)


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_parity_grid(dtype, shape, per_class):
    heat = seeded(shape, dtype, seed=sum(shape))
    C = shape[1] if len(shape) == 4 else 1
    group = shape[-1] * shape[-2] * (1 if per_class else C)
    for kernel in (1, 3, 5, 7):
        for k in sorted({1, 7, 100, 1024, group}):
            if k <= min(group, 1024):
                assert_matches(heat, k, kernel=kernel, per_class=per_class)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("per_class", [False, True])
def test_quantised_maps_break_ties_by_index(dtype, per_class):
    """a few levels only: long runs of equal scores, ordered by flat index"""
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    heat = (torch.randint(0, 4, (3, 2, 45, 70), device=DEV, generator=g).float() * 0.25).to(dtype)
    for kernel in (1, 3, 7):
        for k in (5, 300, 1024):
            assert_matches(heat, k, kernel=kernel, per_class=per_class)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_all_zero_map_returns_the_first_indices(dtype):
    heat = torch.zeros(2, 3, 40, 50, dtype=dtype, device=DEV)
    for per_class in (False, True):
        got = assert_matches(heat, 1024, per_class=per_class)
        expect = torch.arange(1024, device=DEV)
        flat = got.indices.reshape(-1, 1024)
        if per_class:
            assert torch.equal(flat, expect.expand_as(flat))   # every plane: 0 .. k-1
        else:
            assert torch.equal(got.classes * 40 * 50 + got.indices, expect.expand(2, -1))
        assert bool((got.scores == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_negative_maps_rank_peaks_below_suppressed_zeros(dtype):
    """suppressed negatives score -0.0, which ties with +0.0 and ranks above every negative peak"""
    heat = -(seeded((2, 2, 30, 34), torch.float32, seed=3, fn="rand") + 0.1)
    heat = heat.to(dtype)
    for per_class in (False, True):
        for k in (10, 1020):
            got = assert_matches(heat, k, per_class=per_class)
            assert bool((got.scores[..., :10] == 0).all())
    # the whole group: the zeros in index order, then the peaks from the largest down
    got = assert_matches(heat, 30 * 34, per_class=True)
    nz = got.scores[0, 0] < 0
    assert bool(nz.any()) and bool((nz[1:] >= nz[:-1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_plateaus_larger_than_the_window_survive_whole(dtype):
    heat = torch.zeros(1, 60, 70, dtype=dtype, device=DEV)
    heat[0, 10:22, 5:17] = 2.5     # 144 equal maxima, wider than any window
    heat[0, 40:43, 50:60] = 3.0
    heat[0, 30, 30] = -1.0
    for kernel in (3, 7):
        got = assert_matches(heat, 200, kernel=kernel)
        assert bool((got.scores[0, :30] == 3.0).all()) and bool((got.scores[0, 30:174] == 2.5).all())
        assert torch.equal(got.ys[0, :30], torch.arange(40, 43, device=DEV).repeat_interleave(10))


@pytest.mark.parametrize("per_class", [False, True])
def test_drawn_objects_are_the_top_peaks(per_class):
    """well separated objects drawn by draw_heatmap_batched(..., clear=True) into class planes: the top peaks are
    exactly the drawn centres, score 1.0, with their classes (equal scores in flat-index order)"""
    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import draw_heatmap_batched

    B, C, H, W = 3, 4, 96, 136
    g = torch.Generator()
    g.manual_seed(11)
    centres, radii, labels, want = [], [], [], []
    for b in range(B):
        n = 6 + b
        cells = torch.randperm(4 * 5, generator=g)[:n]          # a 4 x 5 grid of cells 24 x 27 apart
        ys, xs = 12 + 24 * (cells // 5), 13 + 27 * (cells % 5)
        cls = torch.randint(0, C, (n,), generator=g)
        centres.append(torch.stack([xs, ys], 1).to(torch.int32))
        radii.append(torch.randint(1, 6, (n,), generator=g).to(torch.int32))
        labels.append(cls.to(torch.int32))
        want.append(sorted((int(c), int(y), int(x)) for c, y, x in zip(cls, ys, xs)))
    c_rb = combine_data(centres, device=DEV)
    r_rb = combine_data(radii, device=DEV, other_with_same_sample_sizes=c_rb)
    l_rb = combine_data(labels, device=DEV, other_with_same_sample_sizes=c_rb)
    heat = torch.empty((B, C, H, W), device=DEV)
    draw_heatmap_batched(heat, c_rb, r_rb, 6.0, 1.0, l_rb, clear=True)
    got = assert_matches(heat, 20, per_class=per_class)
    for b in range(B):
        if per_class:
            found = []
            for c in range(C):
                top = got.scores[b, c] == 1.0
                found += [(c, int(y), int(x)) for y, x in zip(got.ys[b, c][top], got.xs[b, c][top])]
                assert int(top.sum()) == sum(1 for t in want[b] if t[0] == c)
                assert bool(top[:int(top.sum())].all())
            assert sorted(found) == want[b]
        else:
            n = len(want[b])
            assert bool((got.scores[b, :n] == 1.0).all()) and bool((got.scores[b, n:] < 1.0).all())
            found = [(int(c), int(y), int(x)) for c, y, x in zip(got.classes[b, :n], got.ys[b, :n], got.xs[b, :n])]
            assert found == want[b]     # class-major flat order = sorted (class, y, x)


def test_no_host_synchronisation():
    heat = seeded((2, 3, 50, 60), torch.float32, seed=5)
    run(heat, 10)   # load the library outside the checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = run(heat, 100)
        b = run(heat, 100, per_class=True, kernel=5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert a.scores.shape == (2, 100) and b.scores.shape == (2, 3, 100)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_runs_are_bitwise_reproducible_and_leave_the_input(dtype):
    heat = (seeded((4, 5, 90, 130), torch.float32, seed=9, fn="rand") * 8).round().to(dtype)   # many ties
    before = heat.clone()
    for per_class in (False, True):
        a = run(heat, 500, per_class=per_class)
        b = run(heat, 500, per_class=per_class)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert torch.equal(heat, before)


def test_input_errors():
    from accvlab.draw_heatmap import heatmap_peaks

    heat = torch.rand(2, 3, 16, 20, device=DEV)
    bad = [
        (heat.cpu(), 5, {}),
        (heat.transpose(2, 3), 5, {}),
        (heat.double(), 5, {}),
        (heat.to(torch.int32), 5, {}),
        (heat[0, 0], 5, {}),
        (heat.unsqueeze(0), 5, {}),
        (heat, 5, {"kernel": 2}),
        (heat, 5, {"kernel": 0}),
        (heat, 5, {"kernel": 9}),
        (heat, 5, {"kernel": -1}),
        (heat, 0, {}),
        (heat, -3, {}),
        (heat, 1025, {}),
        (heat, 321, {"per_class": True}),      # group = 16 * 20
        (heat[:, :1].contiguous(), 321, {}),
        (torch.rand(1, 10, 10, device=DEV), 101, {}),
    ]
    for h, k, kw in bad:
        with pytest.raises(RuntimeError):
            heatmap_peaks(h, k, **kw)
    assert heatmap_peaks(heat, 960).scores.shape == (2, 960)     # the whole frame is allowed
    empty = heatmap_peaks(torch.rand(0, 3, 8, 8, device=DEV), 4)
    assert empty.scores.shape == (0, 4)


def test_full_size():
    """the project's headline map, 64 x 1080 x 1920 float32, k = 100"""
    heat = seeded((64, 1080, 1920), torch.float32, seed=42, fn="rand")
    assert_matches(heat, 100)
    del heat


def test_offsets_beyond_2_pow_31():
    """a bf16 map of more than 2^31 elements (W wider than a chunk: column tiles) with peaks planted past 2^31"""
    from accvlab.draw_heatmap import heatmap_peaks

    B, H, W = 2, 32768, 32800
    assert B * H * W > 2 ** 31
    heat = torch.zeros((B, H, W), dtype=torch.bfloat16, device=DEV)
    plants = [(1, 32710, 5, 3.0), (1, 32767, 32799, 2.0), (1, 32740, 20000, 1.5), (0, 100, 200, 4.0),
              (0, 32767, 32799, 0.5)]
    for b, y, x, v in plants:
        heat[b, y, x] = v
        assert b == 0 or b * H * W + y * W + x > 2 ** 31
    got = heatmap_peaks(heat, 8)
    torch.cuda.synchronize()
    for b in range(B):
        mine = sorted((p for p in plants if p[0] == b), key=lambda p: -p[3])
        n = len(mine)
        assert got.scores[b, :n].float().tolist() == [p[3] for p in mine]
        assert got.ys[b, :n].tolist() == [p[1] for p in mine] and got.xs[b, :n].tolist() == [p[2] for p in mine]
        assert got.indices[b, :n].tolist() == [p[1] * W + p[2] for p in mine]
        assert got.indices[b, n:].tolist() == list(range(8 - n))   # then the zeros in index order
        assert bool((got.scores[b, n:] == 0).all()) and bool((got.classes[b] == 0).all())
    del heat
