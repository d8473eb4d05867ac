"""NaN, ±inf, -0.0, subnormals and out-of-range fillers through the GPU ops, each against the float64 definition its own
test file uses (a copy of the helper where the file has one).  Comparisons are NaN-aware: the NaN masks must be equal,
finite entries meet the bar of the op's existing tests, indices and copied bytes are exactly equal."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_special_values_cpu import COMMON, INT_VIEW, PER_TYPE, WIDTH, reference_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLOATS = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
HALF_FLOATS = [torch.float32, torch.float16, torch.bfloat16]


def _name(d):
    return str(d).split(".")[-1]


def bits_of(t):
    """the stored bit patterns of a float tensor, as non-negative int64 (CPU)"""
    v = t.detach().cpu().contiguous().view(INT_VIEW[t.dtype]).long()
    return v & ((1 << WIDTH[t.dtype]) - 1) if WIDTH[t.dtype] < 64 else v


def from_bits(bits, dtype):
    """a CPU tensor of dtype holding exactly the given bit patterns"""
    w = WIDTH[dtype]
    signed = [b - (1 << w) if b >> (w - 1) else b for b in bits]
    return torch.tensor(signed, dtype=INT_VIEW[dtype]).view(dtype)


def assert_nan_aware(got, want, rtol=0.0, atol=0.0, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        bad = (gn != wn).nonzero()[:5].tolist()
        pytest.fail(f"{what}: NaN masks differ at {bad}: got {[got[tuple(i)].item() for i in bad]}, "
                    f"want {[want[tuple(i)].item() for i in bad]}")
    g, w = got[~wn], want[~wn]
    inf = torch.isinf(w)
    assert torch.equal(g[inf], w[inf]), f"{what}: infinities differ"
    err, tol = (g[~inf] - w[~inf]).abs(), atol + rtol * w[~inf].abs()
    if not bool((err <= tol).all()):
        pytest.fail(f"{what}: max excess {float((err - tol).max()):.3e}")


# ---------------------------------------------------------------------------------------------------- fillers
def _values(dtype):
    return COMMON + PER_TYPE[dtype]


def _ragged_case(dtype):
    from accvlab.batching_helpers import RaggedBatch

    data = (torch.arange(3 * 6 * 2, dtype=torch.float64).reshape(3, 6, 2) - 30).to(dtype).to(DEV)
    idx = torch.tensor([[5, 0, 3, 0], [1, 2, 0, 0], [4, 4, 4, 4]], device=DEV)
    sizes = torch.tensor([3, 0, 1], device=DEV)
    return data, RaggedBatch(idx, sample_sizes=sizes)


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_gather_fill_writes_static_cast_bits(dtype):
    import accvlab.batching_helpers as bh

    data, idx = _ragged_case(dtype)
    pad = torch.arange(4, device=DEV)[None, :] >= idx.sample_sizes[:, None]
    want_rows = data[torch.arange(3, device=DEV)[:, None], idx.tensor.clamp(max=5)]
    for v in _values(dtype):
        out = bh.batched_indexing_access(data, idx, filler_value=v).tensor
        assert out.dtype == dtype and out.shape == (3, 4, 2)
        got = bits_of(out)
        assert bool((got[pad.cpu()] == reference_bits(v, dtype)).all()), (v, got[pad.cpu()].unique().tolist())
        assert torch.equal(got[~pad.cpu()], bits_of(want_rows)[~pad.cpu()]), v


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_inverse_indexing_fill_writes_static_cast_bits(dtype):
    import accvlab.batching_helpers as bh

    data, idx = _ragged_case(dtype)
    T = 7
    hit = torch.zeros(3, T, dtype=torch.bool)
    for i, (row, n) in enumerate(zip(idx.tensor.tolist(), idx.sample_sizes.tolist())):
        for j in range(n):
            hit[i, row[j]] = True
    for v in _values(dtype):
        out = bh.batched_inverse_indexing_access(data[:, :4].contiguous(), idx, T, filler_value=v)
        got = bits_of(out)
        assert out.shape == (3, T, 2)
        assert bool((got[~hit] == reference_bits(v, dtype)).all()), (v, got[~hit].unique().tolist())
        assert torch.equal(got[0, 5], bits_of(data[0, 0])) and torch.equal(got[2, 4], bits_of(data[2, 0]))


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32, torch.int64], ids=_name)
def test_pad_fill_gpu_equals_cpu_and_static_cast(dtype):
    from accvlab.batching_helpers import RaggedBatch

    base = (torch.arange(2 * 5 * 3, dtype=torch.float64).reshape(2, 5, 3) - 7).to(dtype)
    sizes = torch.tensor([2, 5])
    pad = torch.arange(5)[None, :] >= sizes[:, None]
    values = _values(dtype) if dtype in FLOATS else [0, -0.0, 7, -3, 1.7, -1.7, 2 ** 20]
    for v in values:
        gpu = RaggedBatch(base.to(DEV), sample_sizes=sizes.to(DEV)).with_padded_set_to(v).tensor.cpu()
        cpu = RaggedBatch(base.clone(), sample_sizes=sizes).with_padded_set_to(v).tensor
        if dtype in FLOATS:
            assert torch.equal(bits_of(gpu), bits_of(cpu)), v
            assert bool((bits_of(gpu)[pad] == reference_bits(v, dtype)).all()), v
            assert torch.equal(bits_of(gpu)[~pad], bits_of(base)[~pad])
        else:
            assert torch.equal(gpu, cpu) and bool((gpu[pad] == int(v)).all()), v
        inplace = RaggedBatch(base.to(DEV), sample_sizes=sizes.to(DEV))
        inplace.set_padded_to(v)
        assert torch.equal(inplace.tensor.cpu().view(torch.uint8), gpu.view(torch.uint8)), v


def _payload_rows(dtype):
    """a [1, 6, 2] batch of special bit patterns: NaN payloads of both signs, ±inf, ±0, the smallest subnormal"""
    w = WIDTH[dtype]
    e = {16: (0x7C00, 0x7C01, 0x7E00) if dtype == torch.float16 else (0x7F80, 0x7F81, 0x7FC1),
         32: (0x7F800000, 0x7F800001, 0x7FC00123), 64: (0x7FF0000000000000, 0x7FF0000000000001, 0x7FF8000000000123)}[w]
    sign = 1 << (w - 1)
    inf, snan, qnan = e
    pats = [qnan, qnan | sign, snan, snan | sign, inf, inf | sign, 0, sign, 1, 1 | sign, qnan ^ 0x20, (qnan ^ 0x20) | sign]
    return from_bits(pats, dtype).reshape(1, 6, 2)


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_nan_payloads_are_copied_bit_for_bit(dtype):
    import accvlab.batching_helpers as bh

    rows = _payload_rows(dtype)
    data = rows.to(DEV)
    perm = [5, 3, 0, 4, 1, 2]
    idx = bh.RaggedBatch(torch.tensor([perm], device=DEV), sample_sizes=torch.tensor([6], device=DEV))
    want = bits_of(rows[:, perm])
    # gather
    assert torch.equal(bits_of(bh.batched_indexing_access(data, idx).tensor), want)
    # scatter into a fresh tensor (inverse indexing): out[perm[j]] = data[j]
    inv = bh.batched_inverse_indexing_access(data, idx, 6)
    assert torch.equal(bits_of(inv)[0, perm], bits_of(rows)[0])
    # write into a copy of an existing tensor
    into = torch.full((1, 8, 2), 3.0, dtype=dtype, device=DEV)
    out = bh.batched_indexing_write(data, idx, into)
    got = bits_of(out)
    assert torch.equal(got[0, perm], bits_of(rows)[0])
    assert torch.equal(got[0, 6:], bits_of(into.cpu())[0, 6:])
    # pair mapping: target[tgt[j]] = source[src[j]]
    src = bh.RaggedBatch(torch.tensor([[1, 4, 0, 2]], device=DEV), sample_sizes=torch.tensor([4], device=DEV))
    tgt = bh.RaggedBatch(torch.tensor([[7, 0, 3, 5]], device=DEV), sample_sizes=torch.tensor([4], device=DEV))
    mapped = bits_of(bh.batched_index_mapping(data, src, tgt, into))
    assert torch.equal(mapped[0, [7, 0, 3, 5]], bits_of(rows)[0, [1, 4, 0, 2]])
    assert torch.equal(mapped[0, [1, 2, 4, 6]], bits_of(into.cpu())[0, [1, 2, 4, 6]])


_ACC_DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64]


@pytest.mark.parametrize("dtype", _ACC_DTYPES, ids=_name)
def test_accumulate_of_duplicates_with_nan_and_inf(dtype):
    from accvlab.batching_helpers.batched_indexing_access_cuda import backward_new_tensor

    nan, inf = math.nan, math.inf
    floats = dtype in FLOATS
    # per target: contributions, and the order-independent outcome
    groups = [([1.0, 2.0, 0.5], 3.5), ([0.25, -0.25, 0.125], 0.125)]
    if floats:
        groups += [([nan, 1.0], nan), ([inf, 1.0, 2.0], inf), ([-inf, 0.25], -inf), ([inf, -inf], nan),
                   ([nan, inf, -inf, 3.0], nan), ([-inf, -inf, 1.0], -inf), ([2.0, nan], nan), ([0.5], 0.5)]
    else:
        groups = [([1, 2, 5], 8), ([-7, 3], -4), ([100, -100, 1], 1), ([9], 9), ([-1, -1, -1, -1], -4)]
    T = len(groups) + 3                                    # three targets nobody writes: they keep the filler 0
    g = torch.Generator().manual_seed(7)
    for trial in range(3):
        slots = [(t, c) for t, (cs, _) in enumerate(groups) for c in cs]
        order = torch.randperm(len(slots), generator=g).tolist()
        slots = [slots[o] for o in order]
        K = len(slots)
        vals = torch.tensor([c for _, c in slots], dtype=torch.float64)
        # two columns: the f16 / bf16 CAS path on both halves of a 32-bit word whatever the target's parity
        to_insert = vals.reshape(1, K, 1).expand(1, K, 2).contiguous().to(dtype).to(DEV)
        idx = torch.tensor([[t for t, _ in slots]], device=DEV)
        out = backward_new_tensor(to_insert, idx, torch.tensor([K], device=DEV), T, 0.0, True).cpu()
        want = torch.tensor([r for _, r in groups] + [0.0] * 3, dtype=torch.float64).reshape(1, T, 1).expand(1, T, 2)
        if floats:
            assert_nan_aware(out, want, what=f"trial {trial}")
        else:
            assert torch.equal(out, want.to(dtype)), trial


# ---------------------------------------------------------------------------------------------------- heatmap_peaks
def peaks_reference(heat, k, kernel=3, per_class=False):
    """the definition on the CPU in float64 (copy of test_heatmap_peaks_gpu.reference)"""
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


def assert_peaks_match(heat, k, **kw):
    from accvlab.draw_heatmap import heatmap_peaks

    got = heatmap_peaks(heat, k, **kw)
    want = peaks_reference(heat, k, **kw)
    assert got.scores.dtype == heat.dtype
    assert_nan_aware(got.scores.float(), want[0].float(), what=f"scores {kw} k={k}")
    for name, g, w in zip(("indices", "classes", "ys", "xs"), got[1:], want[1:]):
        g = g.cpu()
        if not torch.equal(g, w):
            bad = (g != w).nonzero()[:5].tolist()
            pytest.fail(f"{name} differ ({kw}, k={k}) at {bad}: got {[g[tuple(i)].item() for i in bad]}, "
                        f"want {[w[tuple(i)].item() for i in bad]}")


def _special_map(shape, dtype, seed, n_nan=3):
    """seeded noise with NaN (both signs), ±inf, -0.0 and (f32) subnormals in the middle, on the map's corners and edges,
    on the row-chunk border (64 rows of <= 64 columns) and on the column-tile seam at 2047 / 2048"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    H, W = shape[-2], shape[-1]
    flat = x.view(-1, H, W)
    picks = [(H // 2, W // 2), (0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, 0), (0, W // 2)]
    if H > 64:
        picks += [(63, 5), (64, 5), (63, W - 2)]
    if W > 2048:
        picks += [(1, 2047), (2, 2048), (H - 1, 2047), (0, 2049)]
    specials = [math.nan, math.inf, -math.inf, -0.0, math.inf, -math.inf]
    if dtype == torch.float32:
        specials += [2.0 ** -149, -(2.0 ** -140), 2.0 ** -130]
    for p in range(flat.shape[0]):
        for n, (r, c) in enumerate(picks):
            flat[p, r, c] = specials[(n + p) % len(specials)]
        r = torch.randint(0, H, (n_nan,), generator=g)
        c = torch.randint(0, W, (n_nan,), generator=g)
        flat[p, r, c] = math.nan
        flat[p, (r + 1) % H, c] = math.inf          # a suppressed +inf next to a NaN scores NaN
    out = x.to(dtype)
    neg_nan = from_bits([{torch.float32: 0xFFC00000, torch.float16: 0xFE00, torch.bfloat16: 0xFFC0}[dtype]], dtype)
    for i in (7, out.numel() // 3):                 # NaN with the sign bit set
        out.view(-1)[i : i + 1] = neg_nan
    assert int(bits_of(out.view(-1)[7:8])) >> (WIDTH[dtype] - 1) == 1
    if dtype == torch.float32:                      # a subnormal local maximum in a field of smaller negatives
        out.view(-1, H, W)[0, H // 3, W // 3] = 2.0 ** -145
    return out.to(DEV)


PEAK_SHAPES = [(2, 37, 53), (1, 2, 65, 64), (1, 1, 5, 2500), (2, 3, 9, 11)]


@pytest.mark.parametrize("dtype", HALF_FLOATS, ids=_name)
@pytest.mark.parametrize("shape", PEAK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_peaks_with_special_values(dtype, shape):
    heat = _special_map(shape, dtype, seed=sum(shape))
    group = shape[-1] * shape[-2]
    for kernel in (1, 3, 5, 7):
        for per_class in (False, True):
            for k in (1, 5, 40, min(300, group)):
                assert_peaks_match(heat, k, kernel=kernel, per_class=per_class)


@pytest.mark.parametrize("dtype", HALF_FLOATS, ids=_name)
def test_peaks_more_nans_than_k_come_first_by_index(dtype):
    from accvlab.draw_heatmap import heatmap_peaks

    heat = _special_map((1, 2, 40, 50), dtype, seed=3, n_nan=60)
    for kernel in (1, 3, 7):
        for per_class in (False, True):
            assert_peaks_match(heat, 16, kernel=kernel, per_class=per_class)
    got = heatmap_peaks(heat, 16, kernel=3)
    assert bool(torch.isnan(got.scores).all())
    flat = got.classes * 2000 + got.indices
    assert bool((flat[:, 1:] > flat[:, :-1]).all())


@pytest.mark.parametrize("dtype", HALF_FLOATS, ids=_name)
def test_peaks_all_minus_inf_and_all_nan_maps(dtype):
    for fill in (-math.inf, math.nan, math.inf):
        heat = torch.full((2, 2, 17, 33), fill, dtype=dtype, device=DEV)
        heat[1, 1, 4, 4] = 1.0
        for kernel in (1, 3, 7):
            for per_class in (False, True):
                assert_peaks_match(heat, 10, kernel=kernel, per_class=per_class)
    heat = torch.full((1, 1, 8, 8), -math.inf, dtype=dtype, device=DEV)
    assert_peaks_match(heat, 64)


@pytest.mark.parametrize("dtype", HALF_FLOATS, ids=_name)
def test_peaks_signed_zero_ties(dtype):
    # -0.0 and +0.0 plateaus with negative neighbours: every zero is a local maximum, they tie by index
    heat = -torch.rand((1, 1, 12, 12), generator=torch.Generator().manual_seed(1)).to(dtype)
    heat[0, 0, ::2, ::3] = -0.0
    heat[0, 0, 1::2, ::3] = 0.0
    heat = heat.to(DEV)
    for kernel in (1, 3, 5):
        assert_peaks_match(heat, 60, kernel=kernel)


# ---------------------------------------------------------------------------------------------------- gaussian_focal_loss
def focal_composition(logits, target, alpha=2.0, gamma=4.0, pos_weight=1.0, neg_weight=1.0, clamp_eps=1e-4, avg_factor=None):
    """the definition, in float64 with torch autograd (copy of test_heatmap_loss_gpu.composition)"""
    x = logits.detach().double().requires_grad_(True)
    t = target.double()
    p = x.sigmoid()
    if clamp_eps > 0:
        p = p.clamp(clamp_eps, 1 - clamp_eps)
    pos = t.eq(1)
    pos_loss = -(p + 1e-12).log() * (1 - p).pow(alpha) * pos
    neg_loss = -(1 - p + 1e-12).log() * p.pow(alpha) * (1 - t).pow(gamma)
    total = (pos_weight * pos_loss + neg_weight * neg_loss).sum()
    loss = total / (pos.sum().clamp(min=1) if avg_factor is None else avg_factor)
    loss.backward()
    return loss.detach(), x.grad


MANTISSA = {torch.float16: 10, torch.bfloat16: 7}


def assert_focal_grad(g, g64, dtype):
    """NaN where autograd has NaN; elsewhere the bar of test_heatmap_loss_gpu.assert_grad_close"""
    assert g.dtype == dtype and g.shape == g64.shape
    g, g64 = g.detach().cpu(), g64.detach().cpu()
    nan = torch.isnan(g64)
    assert torch.equal(torch.isnan(g), nan), f"NaN masks differ at {(torch.isnan(g) != nan).nonzero()[:5].tolist()}"
    g, g64 = g[~nan], g64[~nan]
    if dtype == torch.float32:
        err = (g.double() - g64).abs()
        tol = 1e-4 * g64.abs() + 1e-6 * g64.abs().max()
        assert bool((err <= tol).all()), f"max excess {float((err - tol).max()):.3e}"
    else:
        ref = g64.to(dtype).double()
        ulp = ref.abs() * 2.0 ** -MANTISSA[dtype] + (2.0 ** -24 if dtype == torch.float16 else 1e-38)
        err = (g.double() - ref).abs()
        assert bool((err <= ulp).all()), f"{int((err > ulp).sum())} elements off by more than one rounding"


def _focal_case(shape, dtype, seed, with_nan):
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    target = torch.rand(n, generator=g) * 0.9
    target[torch.randperm(n, generator=g)[: max(4, n // 20)]] = 1.0
    x = (torch.rand(n, generator=g) * 2 - 1) * 10
    pos = (target == 1).nonzero().flatten().tolist()
    neg = (target != 1).nonzero().flatten().tolist()
    specials = [math.inf, -math.inf, 0.0, -0.0] + ([math.nan] if with_nan else [])
    for i, v in enumerate(specials):       # each value at a positive and at a negative; the last elements are the tail
        x[pos[i % len(pos)]] = v
        x[neg[i]] = v
        x[neg[-1 - i]] = v
    return x.reshape(shape).to(dtype).to(DEV), target.reshape(shape).to(DEV)


FOCAL_PARAMS = [dict(), dict(clamp_eps=0.0), dict(alpha=1.5, gamma=3.0)]


@pytest.mark.parametrize("dtype", HALF_FLOATS, ids=_name)
@pytest.mark.parametrize("shape", [(4, 48, 64), (3, 5, 9)], ids=["vectorised", "scalar_tail"])
@pytest.mark.parametrize("kw", FOCAL_PARAMS, ids=["defaults", "no_clamp", "alpha1.5_gamma3"])
@pytest.mark.parametrize("with_nan", [False, True], ids=["inf_zero", "nan"])
def test_focal_loss_with_special_logits(dtype, shape, kw, with_nan):
    from accvlab.draw_heatmap import gaussian_focal_loss

    logits, target = _focal_case(shape, dtype, seed=len(shape) + shape[-1], with_nan=with_nan)
    x = logits.detach().clone().requires_grad_(True)
    loss = gaussian_focal_loss(x, target, **kw)
    loss.backward()
    loss = loss.detach()
    ref, g64 = focal_composition(logits, target, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    if with_nan:
        assert math.isnan(float(loss)) and math.isnan(float(ref))
    else:
        assert math.isfinite(float(ref))
        assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
        # the denominator: max(#positives, 1) counted on the device, the same sum divided by a given factor of 1
        npos = int((target == 1).sum())
        raw = gaussian_focal_loss(logits, target, avg_factor=1.0, **kw)
        assert abs(float(raw) - float(loss) * max(npos, 1)) <= 1e-6 * abs(float(raw))
    assert_focal_grad(x.grad, g64, dtype)
    if with_nan:
        assert bool(torch.isnan(x.grad).any()) and bool(torch.isfinite(x.grad[~torch.isnan(logits)]).all())


# ---------------------------------------------------------------------------------------------------- matched_pair_loss_sum
def _iou_loss_torch(g, p, eps):       # the example's formulation (copy of test_matched_pair_loss_gpu._iou_loss_torch)
    areas_g = torch.prod(g[..., 2:4] - g[..., 0:2], axis=-1)
    areas_p = torch.prod(p[..., 2:4] - p[..., 0:2], axis=-1)
    size = torch.min(g[..., 2:4], p[..., 2:4]) - torch.max(g[..., 0:2], p[..., 0:2])
    size = size.clone()
    size[size < 0.0] = 0.0
    inter = torch.prod(size, axis=-1)
    union = areas_g + areas_p - inter
    union = union.clone()
    union[union < eps] = eps
    return 1.0 - inter / union


def _pair_loss(ga, gb, kind, beta, eps, C):
    if kind == "l1":
        return (ga - gb).abs().sum(-1)
    if kind == "l2":
        return ((ga - gb) * (ga - gb)).sum(-1)
    if kind == "smooth_l1":
        return F.smooth_l1_loss(ga, gb, beta=beta, reduction="none").sum(-1)
    if kind == "iou_xyxy":
        return _iou_loss_torch(ga, gb, eps)
    onehot = (torch.arange(C, device=ga.device)[None, :] == ga[:, None]).double()
    return (onehot - gb).abs().sum(-1)


_MTOL = {torch.float32: 1e-5, torch.float64: 1e-12, torch.float16: 2e-3, torch.bfloat16: 2e-2}


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
@pytest.mark.parametrize("kind", ["l1", "l2", "smooth_l1", "iou_xyxy", "onehot_l1"])
def test_matched_pair_loss_with_special_values(kind, dtype):
    """NaN / ±inf in matched rows of a, b and the weights; NaN in every row no pair reads (unmatched rows, and the rows the
    index slots past the counts point at).  Reference: autograd in float64 over the valid pairs only."""
    import accvlab.batching_helpers as bh

    nan, inf = math.nan, math.inf
    g = torch.Generator().manual_seed(11)
    B, NA, NB, K, C = 3, 9, 11, 6, 5
    beta, eps = 0.5, 1e-6
    row = 4 if kind in ("iou_xyxy",) else (C if kind == "onehot_l1" else 3)
    counts = [5, 0, 3]
    ia = torch.zeros(B, K, dtype=torch.int64)
    ib = torch.zeros(B, K, dtype=torch.int64)
    for i in range(B):
        ia[i] = torch.randperm(NA, generator=g)[:K]
        ib[i] = torch.randperm(NB, generator=g)[:K]
    ib[0, 1] -= NB                                              # a negative index wraps once
    if kind == "iou_xyxy":
        def boxes(n):
            tl = torch.rand(B, n, 2, generator=g, dtype=torch.float64) * 60
            return torch.cat([tl, tl + 2 + torch.rand(B, n, 2, generator=g, dtype=torch.float64) * 40], -1)
        a, b = boxes(NA), boxes(NB)
    else:
        a = torch.randn(B, NA, row, generator=g, dtype=torch.float64)
        b = torch.randn(B, NB, row, generator=g, dtype=torch.float64)
    if kind == "onehot_l1":
        a = torch.randint(0, C, (B, NA), generator=g)
        b = torch.rand(B, NB, C, generator=g, dtype=torch.float64)
    w = 0.2 + torch.rand(B, NA, generator=g, dtype=torch.float64) * 1.8
    used_a = torch.zeros(B, NA, dtype=torch.bool)
    used_b = torch.zeros(B, NB, dtype=torch.bool)
    for i in range(B):
        for j in range(counts[i]):
            used_a[i, ia[i, j]] = True
            used_b[i, ib[i, j] % NB] = True
    # special values in matched rows (sample 0 pairs 0..2, sample 2 pair 1); coordinates of boxes get NaN only: the
    # reference's prod / masked-assignment gradients at an infinite box edge are NaN by a rule the kernel does not mirror
    m0a, m1a, m2a = int(ia[0, 0]), int(ia[0, 1]), int(ia[2, 1])
    m0b, m1b = int(ib[0, 0]), int(ib[0, 2]) % NB
    if kind == "iou_xyxy":
        a[0, m0a, 2] = nan
        b[0, m1b, 1] = nan
    elif kind == "onehot_l1":
        b[0, m0b, 1] = nan
        b[0, m1b, 0] = inf
        b[0, m1b, 3] = -inf
    else:
        a[0, m0a, 0] = nan
        a[0, m1a, 1] = inf
        b[0, m0b, 2] = -inf
        b[0, m1b, 0] = inf
        a[0, int(ia[0, 2]), 0] = inf                             # inf - inf = NaN
        b[0, m1b, 2] = -0.0
    w[2, m2a] = inf
    w[0, m1a] = -inf if kind != "iou_xyxy" else w[0, m1a]
    w[0, int(ia[0, 3])] = nan
    # poison what no pair reads
    if kind != "onehot_l1":
        a[~used_a] = nan
    b[~used_b] = nan
    w[~used_a] = nan
    ta = a.to(DEV) if kind == "onehot_l1" else a.to(dtype).to(DEV).requires_grad_(True)
    tb = b.to(dtype).to(DEV).requires_grad_(True)
    tw = w.to(dtype).to(DEV).requires_grad_(True)
    ra = bh.RaggedBatch(ia.to(DEV), sample_sizes=torch.tensor(counts, device=DEV))
    rb = bh.RaggedBatch(ib.to(DEV), sample_sizes=torch.tensor(counts, device=DEV))
    out = bh.matched_pair_loss_sum(ta, tb, ra, rb, tw, kind=kind, beta=beta, eps=eps)
    up = torch.linspace(0.5, 1.5, B, device=DEV, dtype=out.dtype)
    (out * up).sum().backward()

    # reference: the pairs j < counts[i] only, in float64 on the dtype-rounded inputs
    ca = a.clone() if kind == "onehot_l1" else ta.detach().double().cpu().requires_grad_(True)
    cb = tb.detach().double().cpu().requires_grad_(True)
    cw = tw.detach().double().cpu().requires_grad_(True)
    si = torch.tensor([i for i in range(B) for _ in range(counts[i])], dtype=torch.int64)
    ja = torch.tensor([int(ia[i, j]) for i in range(B) for j in range(counts[i])], dtype=torch.int64)
    jb = torch.tensor([int(ib[i, j]) % NB for i in range(B) for j in range(counts[i])], dtype=torch.int64)
    per = _pair_loss(ca[si, ja], cb[si, jb], kind, beta, eps, C) * cw[si, ja]
    ref = torch.zeros(B, dtype=torch.float64).index_add(0, si, per)
    (ref * up.detach().cpu().double()).sum().backward()

    fwd_tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert_nan_aware(out, ref, rtol=fwd_tol, atol=fwd_tol, what="forward")
    assert math.isnan(float(out[0])) and out[1].item() == 0.0      # the poisoned rows leave an empty sample at 0
    tol = _MTOL[dtype]
    grads = [("b", tb.grad, cb.grad, used_b), ("w", tw.grad, cw.grad, used_a)]
    if kind != "onehot_l1":
        grads.insert(0, ("a", ta.grad, ca.grad, used_a))
    for name, got, exp, used in grads:
        assert got.dtype == dtype
        fin = exp[torch.isfinite(exp)]
        scale = max(1.0, float(fin.abs().max())) if fin.numel() else 1.0
        assert_nan_aware(got, exp, atol=tol * scale, what=f"grad {name}")
        assert bool((got.cpu()[~used] == 0).all()), f"grad {name}: rows no pair reads must get exactly 0"
