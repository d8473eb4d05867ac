"""The fused Gaussian focal loss (accvlab.draw_heatmap.gaussian_focal_loss) against its definition, the torch composition
below evaluated in float64 with torch autograd from the same input values; targets drawn by draw_heatmap_batched."""
import math

import pytest
import torch

import bench_workloads as wl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
PARAMS = [
    dict(),
    dict(clamp_eps=0.0),
    dict(alpha=1.5, gamma=3.0),
    dict(pos_weight=2.5, neg_weight=0.75),
]
MANTISSA = {torch.float16: 10, torch.bfloat16: 7}


def composition(logits, target, alpha=2.0, gamma=4.0, pos_weight=1.0, neg_weight=1.0, clamp_eps=1e-4, avg_factor=None):
    """the definition, in float64 with torch autograd: (loss, d loss / d logits)"""
    x = logits.detach().double().requires_grad_(True)
    t = target.double()
    p = x.sigmoid()
    if clamp_eps > 0:
        p = p.clamp(clamp_eps, 1 - clamp_eps)
    pos = t.eq(1)
    pos_loss = -(p + 1e-12).log() * (1 - p).pow(alpha) * pos
    neg_loss = -(1 - p + 1e-12).log() * p.pow(alpha) * (1 - t).pow(gamma)
    total = (pos_weight * pos_loss + neg_weight * neg_loss).sum()
    if isinstance(avg_factor, torch.Tensor):
        avg_factor = avg_factor.double()
    loss = total / (pos.sum().clamp(min=1) if avg_factor is None else avg_factor)
    loss.backward()
    return loss.detach(), x.grad


def drawn_target(shape, seed):
    """a heat map drawn by draw_heatmap_batched(..., clear=True) on random objects: [B, H, W] or class-wise [B, C, H, W]"""
    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import draw_heatmap_batched

    classes = shape[1] if len(shape) == 4 else 0
    B, H, W = shape[0], shape[-2], shape[-1]
    objs = wl.heatmap_objects(B, H, W, 1, 24, "A", seed=seed, n_classes=classes)
    centers = combine_data(list(objs[0]), device=DEV)
    radii = combine_data(list(objs[1]), device=DEV, other_with_same_sample_sizes=centers)
    labels = combine_data(list(objs[2]), device=DEV, other_with_same_sample_sizes=centers) if classes else None
    hm = torch.empty(shape, device=DEV)
    draw_heatmap_batched(hm, centers, radii, 6.0, 1.0, labels, clear=True)
    assert (hm == 1).sum() > 0, "the positive branch must be covered"
    return hm


def random_logits(shape, dtype, seed, bound=10.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = (torch.rand(shape, device=DEV, generator=g) * 2 - 1) * bound
    return x.to(dtype)


def fused(logits, target, **kw):
    from accvlab.draw_heatmap import gaussian_focal_loss

    x = logits.detach().clone().requires_grad_(True)
    loss = gaussian_focal_loss(x, target, **kw)
    loss.backward()
    return loss.detach(), x.grad


def assert_grad_close(g, g64, dtype):
    assert g.dtype == dtype and g.shape == g64.shape
    if dtype == torch.float32:
        err = (g.double() - g64).abs()
        tol = 1e-4 * g64.abs() + 1e-6 * g64.abs().max()
        assert bool((err <= tol).all()), f"max excess {float((err - tol).max()):.3e}"
    else:
        ref = g64.to(dtype).double()
        ulp = ref.abs() * 2.0 ** -MANTISSA[dtype] + (2.0 ** -24 if dtype == torch.float16 else 1e-38)
        err = (g.double() - ref).abs()
        assert bool((err <= ulp).all()), f"{int((err > ulp).sum())} elements off by more than one rounding"


SHAPES = [(4, 270, 480), (2, 10, 37, 53), (1, 1, 7), (3, 5, 9)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kw", PARAMS, ids=["defaults", "no_clamp", "alpha1.5_gamma3", "weights"])
def test_forward_and_gradient_parity(shape, dtype, kw):
    target = drawn_target(shape, seed=sum(shape))
    logits = random_logits(shape, dtype, seed=len(shape) * 1000 + shape[-1])
    loss, g = fused(logits, target, **kw)
    ref, g64 = composition(logits, target, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert_grad_close(g, g64, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_gradient_is_zero_where_the_clamp_holds(dtype):
    shape = (2, 64, 96)
    target = drawn_target(shape, seed=5)
    logits = random_logits(shape, dtype, seed=6, bound=10.0)
    flat = logits.view(-1)
    flat[:8] = torch.tensor([9.5, -9.5, 10.0, -10.0, 9.75, -9.75, 9.3, -9.3], device=DEV).to(dtype)
    loss, g = fused(logits, target)
    ref, g64 = composition(logits, target)
    s = logits.double().sigmoid()
    clamped = (s < 1e-4) | (s > 1 - 1e-4)
    assert int(clamped.sum()) > 8
    assert bool((g[clamped] == 0).all())
    assert bool((g[~clamped] != 0).any())
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert_grad_close(g, g64, dtype)


def test_unaligned_inputs_take_the_scalar_path():
    """contiguous views that start 4 bytes into their storage: no 16-byte vectors possible"""
    shape = (2, 33, 65)
    n = 2 * 33 * 65
    target = torch.empty(n + 1, device=DEV)
    target[1:] = drawn_target(shape, seed=8).view(-1)
    logits = torch.empty(n + 1, device=DEV)
    logits[1:] = random_logits((n,), torch.float32, seed=9)
    t, x = target[1:].view(shape), logits[1:].view(shape)
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    loss, g = fused(x, t)
    ref, g64 = composition(x, t)
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert_grad_close(g, g64, torch.float32)


def test_avg_factor_forms():
    from accvlab.draw_heatmap import gaussian_focal_loss

    shape = (4, 270, 480)
    target = drawn_target(shape, seed=11)
    logits = random_logits(shape, torch.float32, seed=12)
    num_pos = int((target == 1).sum())
    assert num_pos > 0
    default = gaussian_focal_loss(logits, target)
    assert torch.equal(default, gaussian_focal_loss(logits, target, avg_factor=float(max(num_pos, 1))))
    as_float = gaussian_focal_loss(logits, target, avg_factor=37.5)
    as_tensor = gaussian_focal_loss(logits, target, avg_factor=torch.tensor(37.5, device=DEV))
    assert torch.equal(as_float, as_tensor)
    ref, _ = composition(logits, target, avg_factor=37.5)
    assert abs(float(as_float) - float(ref)) <= 1e-5 * abs(float(ref))
    # gradients through the tensor form
    _, g = fused(logits, target, avg_factor=torch.tensor(37.5, device=DEV))
    _, g64 = composition(logits, target, avg_factor=37.5)
    assert_grad_close(g, g64, torch.float32)
    # an all-zero target has no positives: the sum is divided by 1
    zero = torch.zeros(shape, device=DEV)
    loss0 = gaussian_focal_loss(logits, zero)
    assert torch.equal(loss0, gaussian_focal_loss(logits, zero, avg_factor=1.0))
    ref0, _ = composition(logits, zero)
    assert abs(float(loss0) - float(ref0)) <= 1e-5 * abs(float(ref0))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_runs_are_bitwise_reproducible(dtype):
    shape = (4, 270, 480)
    target = drawn_target(shape, seed=13)
    logits = random_logits(shape, dtype, seed=14)
    l1, g1 = fused(logits, target)
    l2, g2 = fused(logits, target)
    assert torch.equal(l1, l2)
    assert torch.equal(g1, g2)


def test_no_host_synchronisation():
    from accvlab.draw_heatmap import gaussian_focal_loss

    shape = (2, 10, 37, 53)
    target = drawn_target(shape, seed=15)
    x = random_logits(shape, torch.bfloat16, seed=16).requires_grad_(True)
    avg = torch.tensor(3.0, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = gaussian_focal_loss(x, target)
        loss.backward()
        loss2 = gaussian_focal_loss(x, target, avg_factor=avg)
        loss2.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert x.grad is not None and x.grad.dtype == torch.bfloat16


def test_input_errors_on_the_device():
    from accvlab.draw_heatmap import gaussian_focal_loss

    x = torch.zeros(2, 8, 8, device=DEV)
    t = torch.zeros(2, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="shape"):
        gaussian_focal_loss(x, torch.zeros(2, 8, 9, device=DEV))
    with pytest.raises(RuntimeError, match="target must be float32"):
        gaussian_focal_loss(x, t.half())
    with pytest.raises(RuntimeError, match="logits must be"):
        gaussian_focal_loss(x.double(), t)
    with pytest.raises(RuntimeError, match="CUDA"):
        gaussian_focal_loss(x, t.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        gaussian_focal_loss(x.transpose(1, 2), t)
    with pytest.raises(RuntimeError, match="alpha"):
        gaussian_focal_loss(x, t, alpha=0.5)
    with pytest.raises(RuntimeError, match="gamma"):
        gaussian_focal_loss(x, t, gamma=-1.0)
    with pytest.raises(RuntimeError, match="target"):
        gaussian_focal_loss(x, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="avg_factor"):
        gaussian_focal_loss(x, t, avg_factor=torch.ones(1, device=DEV))


def test_empty_input_returns_zero():
    from accvlab.draw_heatmap import gaussian_focal_loss

    x = torch.zeros(0, 8, device=DEV, requires_grad=True)
    loss = gaussian_focal_loss(x, torch.zeros(0, 8, device=DEV))
    assert loss.dim() == 0 and float(loss.detach()) == 0.0
    loss.backward()
    assert x.grad.shape == x.shape


def test_indices_beyond_2_pow_31():
    """bf16 logits of one constant value, more than 2^31 elements; a zero target with exact 1.0 entries past 2^31"""
    from accvlab.draw_heatmap import gaussian_focal_loss

    n = 2 ** 31 + 8 * 1000 + 3
    c = 0.5
    pos_idx = torch.tensor([2 ** 31 + 1, 2 ** 31 + 7777, n - 1], device=DEV)
    target = torch.zeros(n, device=DEV)
    target[pos_idx] = 1.0
    x = torch.full((n,), c, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    loss = gaussian_focal_loss(x, target)
    loss.backward()
    k = len(pos_idx)
    p = 1 / (1 + math.exp(-c))
    neg = -math.log(1 - p + 1e-12) * p * p
    pos = -math.log(p + 1e-12) * (1 - p) ** 2
    expect = ((n - k) * neg + k * pos) / k   # the three positives past 2^31 are counted: denominator 3
    loss = float(loss.detach())
    assert abs(loss - expect) <= 2e-6 * expect, (loss, expect)
    ds = p * (1 - p)
    g_pos = (-(1 - p) ** 2 / (p + 1e-12) + 2 * (1 - p) * math.log(p + 1e-12)) * ds / k
    g_neg = (p * p / (1 - p + 1e-12) - 2 * p * math.log(1 - p + 1e-12)) * ds / k
    g = x.grad
    for idx, want in ((int(pos_idx[0]), g_pos), (int(pos_idx[1]), g_pos), (n - 1, g_pos), (0, g_neg), (2 ** 31, g_neg),
                      (n - 2, g_neg)):
        ref = float(torch.tensor(want).to(torch.bfloat16))
        assert abs(float(g[idx]) - ref) <= abs(ref) * 2.0 ** -7, (idx, float(g[idx]), want)
    del x, g, target


def test_full_size_against_float64():
    """configs[1] shape (64 x 1080 x 1920), target from bench_workloads' seed-42 rule-A objects, f32 logits"""
    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import draw_heatmap_batched, gaussian_focal_loss

    B, H, W = 64, 1080, 1920
    centers_l, radii_l = wl.heatmap_objects(B, H, W, 1, 128, "A", seed=42)
    centers = combine_data(centers_l, device=DEV)
    radii = combine_data(radii_l, device=DEV, other_with_same_sample_sizes=centers)
    target = torch.empty((B, H, W), device=DEV)
    draw_heatmap_batched(target, centers, radii, 6.0, 1.0, clear=True)
    assert (target == 1).sum() > 0
    logits = random_logits((B, H, W), torch.float32, seed=42)
    loss = gaussian_focal_loss(logits, target)
    with torch.no_grad():
        x, t = logits.double(), target.double()
        p = x.sigmoid().clamp(1e-4, 1 - 1e-4)
        pos = t.eq(1)
        total = (-(p + 1e-12).log() * (1 - p).pow(2) * pos).sum()
        total += (-(1 - p + 1e-12).log() * p.pow(2) * (1 - t).pow(4)).sum()
        ref = float(total / pos.sum().clamp(min=1))
    assert abs(float(loss) - ref) <= 1e-4 * abs(ref), (float(loss), ref)
