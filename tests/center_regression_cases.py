"""Float64 oracle and inputs of the centre-point regression tests (test_center_regression_cpu.py,
test_center_regression_gpu.py) and of scripts/bench_center_regression.py: the torch composition that defines
accvlab.draw_heatmap.gather_at_centers and center_regression_loss, evaluated on the device of its inputs."""
import torch
import torch.nn.functional as F

MANTISSA = {torch.float16: 10, torch.bfloat16: 7}


def ragged(tensor, sizes, size_dtype=torch.int64):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=torch.as_tensor(sizes, dtype=size_dtype, device=tensor.device))


def valid_and_index(xy, sizes, H, W):
    """(valid [B, N] bool, ind [B, N] int64 clamped into the plane) of int centres [B, N, 2] as (x, y)"""
    B, N = xy.shape[:2]
    x, y = xy[..., 0].long(), xy[..., 1].long()
    slot = torch.arange(N, device=xy.device).view(1, N)
    valid = (slot < sizes.long().view(B, 1)) & (0 <= x) & (x < W) & (0 <= y) & (y < H)
    ind = (y * W + x).clamp(0, max(H * W - 1, 0))
    return valid, ind


def _gather(f, valid, ind):
    B, C, H, W = f.shape
    rows = f.permute(0, 2, 3, 1).reshape(B, H * W, C)
    zero = rows.new_zeros(())
    if H * W == 0:
        return rows.new_zeros(B, ind.shape[1], C)
    return torch.where(valid[..., None], rows.gather(1, ind[..., None].expand(-1, -1, C)), zero)


def oracle_gather(feats, xy, sizes):
    """gather_at_centers with ragged centres, float64 [B, N, C]"""
    f = torch.cat([m.detach().double() for m in feats], 1)
    valid, ind = valid_and_index(xy, sizes, f.shape[2], f.shape[3])
    return _gather(f, valid, ind)


def oracle_gather_indices(feats, indices):
    """gather_at_centers with int64 in-plane indices [B, K], float64 [B, K, C]"""
    f = torch.cat([m.detach().double() for m in feats], 1)
    hw = f.shape[2] * f.shape[3]
    valid = (indices >= 0) & (indices < hw)
    return _gather(f, valid, indices.clamp(0, max(hw - 1, 0)))


def pointwise(d, kind, beta):
    zero = torch.zeros_like(d)
    if kind == "l1":
        return F.l1_loss(d, zero, reduction="none")
    assert kind == "smooth_l1"
    return F.smooth_l1_loss(d, zero, reduction="none", beta=beta)


def oracle_loss(feats, xy, sizes, targets, weights=None, kind="l1", beta=1.0, avg_factor=None, grad_out=1.0):
    """(loss, [d loss / d feats[i]]) in float64 by torch autograd; grad_out scales the backward"""
    leaves = [m.detach().double().requires_grad_(True) for m in feats]
    f = torch.cat(leaves, 1)
    valid, ind = valid_and_index(xy, sizes, f.shape[2], f.shape[3])
    g = _gather(f, valid, ind)
    zero = g.new_zeros(())
    w = torch.ones_like(g) if weights is None else (weights.double() if weights.dim() == 3 else weights.double()[..., None])
    per = pointwise(g - targets.double(), kind, beta) * w
    if avg_factor is None:
        denom = valid.sum().clamp(min=1).double()
    elif isinstance(avg_factor, torch.Tensor):
        denom = avg_factor.detach().double()
    else:
        denom = float(avg_factor)
    loss = torch.where(valid[..., None], per, zero).sum() / denom
    (loss * grad_out).backward()
    return loss.detach(), [m.grad if m.grad is not None else torch.zeros_like(m) for m in leaves]


def composition_loss(feats, xy, sizes, targets, weights=None, kind="l1", beta=1.0):
    """the float32 form of the oracle as a head writes it today (what scripts/bench_center_regression.py times against):
    cat of the heads, permute + contiguous, gather, loss, masked sum; differentiable w.r.t. feats"""
    f = torch.cat(list(feats), 1) if len(feats) > 1 else feats[0]
    B, C, H, W = f.shape
    rows = f.permute(0, 2, 3, 1).contiguous().view(B, H * W, C)
    valid, ind = valid_and_index(xy, sizes, H, W)
    g = rows.gather(1, ind[..., None].expand(-1, -1, C)).float()
    w = valid[..., None].float() if weights is None else torch.where(
        valid[..., None], weights if weights.dim() == 3 else weights[..., None], g.new_zeros(()))
    per = pointwise(g - targets, kind, beta) * w
    return torch.where(valid[..., None], per, g.new_zeros(())).sum() / valid.sum().clamp(min=1)


def loop_loss(feats, xy, sizes, targets, weights=None, kind="l1", beta=1.0, avg_factor=None):
    """the same loss and gradients as a plain per-object Python loop over float64 values (pins the oracle itself)"""
    f = torch.cat([m.detach().double() for m in feats], 1)
    B, C, H, W = f.shape
    grad = torch.zeros_like(f)
    total, count = 0.0, 0
    hits = []
    for b in range(B):
        for n in range(min(int(sizes[b]), xy.shape[1])):
            x, y = int(xy[b, n, 0]), int(xy[b, n, 1])
            if not (0 <= x < W and 0 <= y < H):
                continue
            count += 1
            for c in range(C):
                d = float(f[b, c, y, x]) - float(targets[b, n, c])
                w = 1.0 if weights is None else float(weights[b, n, c] if weights.dim() == 3 else weights[b, n])
                if kind == "l1":
                    l, dl = abs(d), (d > 0) - (d < 0)
                else:
                    l, dl = (0.5 * d * d / beta, d / beta) if abs(d) < beta else (abs(d) - 0.5 * beta, (d > 0) - (d < 0))
                total += w * l
                hits.append((b, c, y, x, w * dl))
    denom = float(max(count, 1)) if avg_factor is None else float(avg_factor)
    for b, c, y, x, v in hits:
        grad[b, c, y, x] += v / denom
    return total / denom, list(grad.split([m.shape[1] for m in feats], 1))


def make_maps(B, channels, H, W, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, c, H, W, generator=g, dtype=torch.float64) * 3.0).to(dtype).to(device) for c in channels]


def make_centers(B, N, H, W, sizes, device, seed=0, margin=0, wild_padding=True):
    """int32 [B, N, 2] (x, y): valid slots inside the map grown by `margin` cells on every side (so some lie outside),
    padded slots at wild coordinates"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randint(-margin, max(W + margin, 1 - margin), (B, N), generator=g)
    y = torch.randint(-margin, max(H + margin, 1 - margin), (B, N), generator=g)
    xy = torch.stack([x, y], -1).to(torch.int32)
    if wild_padding:
        wild = torch.tensor([[2 ** 31 - 1, -(2 ** 31) + 1], [-(2 ** 31) + 1, 2 ** 31 - 1], [-1, -1], [7, -(2 ** 31) + 1]],
                            dtype=torch.int32)
        for b in range(B):
            for n in range(int(sizes[b]), N):
                xy[b, n] = wild[(b + n) % len(wild)]
    return xy.to(device)


def assert_grad_close(g, g64, dtype, what=""):
    """the bars of the heat-map loss: f32 within 1e-4 |g| + 1e-6 max|g|; f16 / bf16 within one rounding of the
    float64 gradient cast to the dtype; and the pattern of zeros is exact"""
    assert g.dtype == dtype and g.shape == g64.shape, (g.dtype, g.shape, g64.shape, what)
    zeros = g64 == 0
    assert int(torch.count_nonzero(g[zeros])) == 0, f"{what}: non-zero gradient where the oracle has none"
    assert not bool(torch.signbit(g[zeros]).any()), f"{what}: -0.0 where the oracle's gradient is 0"
    if dtype == torch.float32:
        err = (g.double() - g64).abs()
        tol = 1e-4 * g64.abs() + 1e-6 * g64.abs().max()
        assert bool((err <= tol).all()), f"{what}: max excess {float((err - tol).max()):.3e}"
    else:
        ref = g64.to(dtype).double()
        ulp = ref.abs() * 2.0 ** -MANTISSA[dtype] + (2.0 ** -24 if dtype == torch.float16 else 1e-38)
        err = (g.double() - ref).abs()
        assert bool((err <= ulp).all()), f"{what}: {int((err > ulp).sum())} elements off by more than one rounding"


def assert_loss_close(loss, ref, what=""):
    assert loss.dtype == torch.float32 and loss.dim() == 0, what
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref), what)
