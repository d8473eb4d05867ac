"""The centre-point regression operators (accvlab.draw_heatmap.gather_at_centers, center_regression_loss) against their
definition: the torch composition of center_regression_cases.py, evaluated in float64 on the same device with torch
autograd from the same input values."""
import ctypes

import numpy as np
import pytest
import torch

import bench_workloads as wl
import center_regression_cases as cr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
_ids = lambda d: str(d).split(".")[-1]  # noqa: E731
# channel counts of the maps of a call: one map; 2, 5 and 8 maps with unequal counts and a 1-channel map; the channel cap
MAPS = {"one": [4], "two": [2, 1], "five": [2, 1, 3, 2, 2], "eight": [1, 5, 2, 1, 3, 1, 2, 1], "cap": [32, 31, 1]}
NAN = float("nan")
INF = float("inf")


def border_centers(xy, sizes, H, W):
    """puts centres on all four borders and one cell outside on each side into the leading slots of frame 0"""
    pts = [(0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1), (0, 0), (W - 1, H - 1),
           (-1, H // 2), (W, H // 2), (W // 2, -1), (W // 2, H), (-1, -1), (W, H)]
    n = min(len(pts), int(sizes[0]))
    if n == 0:
        return xy
    xy[0, :n] = torch.tensor(pts[:n], dtype=torch.int32, device=xy.device)
    return xy


def unaligned(maps):
    """the same values, each map a slice of a larger buffer that starts one element off its alignment"""
    out = []
    for m in maps:
        buf = torch.empty(m.numel() + 9, dtype=m.dtype, device=m.device)
        v = buf[1:1 + m.numel()].view(m.shape)
        v.copy_(m)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        out.append(v)
    return out


def run_loss(maps, centers, targets, weights=None, grad_out=None, **kw):
    from accvlab.draw_heatmap import center_regression_loss

    leaves = [m.detach().clone().requires_grad_(True) for m in maps]
    loss = center_regression_loss(leaves if len(leaves) > 1 else leaves[0], centers, targets, weights, **kw)
    (loss if grad_out is None else loss * grad_out).backward()
    return loss.detach(), [m.grad for m in leaves]


def problem(B, N, H, W, channels, dtype, sizes, seed, margin=2):
    maps = cr.make_maps(B, channels, H, W, dtype, DEV, seed=seed)
    sizes = torch.as_tensor(sizes)
    xy = border_centers(cr.make_centers(B, N, H, W, sizes, DEV, seed=seed, margin=margin), sizes, H, W)
    g = torch.Generator().manual_seed(seed + 2)
    C = sum(channels)
    targets = (torch.randn(B, N, C, generator=g) * 3.0).to(DEV)
    return maps, xy, sizes.to(DEV), targets, g


# ------------------------------------------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("maps_id", sorted(MAPS))
@pytest.mark.parametrize("size_dtype", [torch.int64, torch.int32], ids=_ids)
def test_gather_parity_ragged_centers(dtype, maps_id, size_dtype):
    from accvlab.draw_heatmap import gather_at_centers

    B, N, H, W = 4, 40, 37, 53   # W is not a multiple of 4
    maps, xy, sizes, _, _ = problem(B, N, H, W, MAPS[maps_id], dtype, [N, 0, 17, 1], seed=len(maps_id))
    if maps_id in ("two", "eight"):
        maps = unaligned(maps)
    centers = cr.ragged(xy, sizes.cpu(), size_dtype)
    got = gather_at_centers(maps if len(maps) > 1 else maps[0], centers)
    want = cr.oracle_gather(maps, xy, sizes).to(dtype)
    assert got.tensor.dtype == dtype and got.tensor.shape == (B, N, sum(MAPS[maps_id]))
    assert got.sample_sizes is centers.sample_sizes
    assert torch.equal(got.tensor, want)
    valid, _ = cr.valid_and_index(xy, sizes, H, W)
    assert int(valid.sum()) > 0 and int((~valid[0, :12]).sum()) == 6, "six leading centres of frame 0 lie outside"
    assert int(torch.count_nonzero(got.tensor[~valid])) == 0 and not bool(torch.signbit(got.tensor[~valid]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("maps_id", ["one", "five"])
def test_gather_parity_peak_indices(dtype, maps_id):
    from accvlab.draw_heatmap import gather_at_centers

    B, K, H, W = 3, 33, 19, 30
    maps = cr.make_maps(B, MAPS[maps_id], H, W, dtype, DEV, seed=11)
    g = torch.Generator().manual_seed(12)
    ind = torch.randint(0, H * W, (B, K), generator=g)
    ind[0, :6] = torch.tensor([0, H * W - 1, -1, H * W, 2 ** 62, -(2 ** 62)])
    ind = ind.to(DEV)
    got = gather_at_centers(maps if len(maps) > 1 else maps[0], ind)
    assert isinstance(got, torch.Tensor) and got.dtype == dtype
    assert torch.equal(got, cr.oracle_gather_indices(maps, ind).to(dtype))
    assert int(torch.count_nonzero(got[0, 2:6])) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_gather_and_gradient_with_many_objects(dtype):
    """Nmax of 2500 (beyond the cells the backward caches per frame), a full frame, an empty one and a short one; many
    objects share cells at this density"""
    from accvlab.draw_heatmap import gather_at_centers

    B, N, H, W, channels = 3, 2500, 23, 31, [2, 3]
    maps, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [N, 0, 1100], seed=21, margin=1)
    centers = cr.ragged(xy, sizes.cpu())
    got = gather_at_centers(maps, centers)
    assert torch.equal(got.tensor, cr.oracle_gather(maps, xy, sizes).to(dtype))
    weights = torch.rand(B, N, generator=g).to(DEV)
    loss, grads = run_loss(maps, centers, targets, weights, kind="smooth_l1", beta=2.0)
    ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights, "smooth_l1", 2.0)
    cr.assert_loss_close(loss, ref)
    for i, (a, b) in enumerate(zip(grads, ref_grads)):
        cr.assert_grad_close(a, b, dtype, f"map {i}")


# --------------------------------------------------------------------------------------------------- 2. loss and gradient
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["l1", "smooth_l1"])
@pytest.mark.parametrize("weights", ["none", "object", "channel"])
@pytest.mark.parametrize("avg", ["default", "number", "tensor"])
def test_loss_and_gradient_parity(dtype, kind, weights, avg):
    B, N, H, W, channels = 4, 40, 37, 53, [2, 1, 3, 2, 2]
    C = sum(channels)
    maps, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [N, 0, 17, 1], seed=31)
    w = {"none": None, "object": torch.rand(B, N, generator=g).to(DEV), "channel": torch.rand(B, N, C, generator=g).to(DEV)}[weights]
    avg_factor = {"default": None, "number": 37.5, "tensor": torch.tensor(21.0, device=DEV)}[avg]
    centers = cr.ragged(xy, sizes.cpu())
    loss, grads = run_loss(maps, centers, cr.ragged(targets, sizes.cpu()) if avg == "number" else targets, w, kind=kind,
                           beta=1.7, avg_factor=avg_factor, grad_out=0.75)
    ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, w, kind, 1.7, avg_factor, grad_out=0.75)
    cr.assert_loss_close(loss, ref)
    assert float(ref) > 0
    for i, (a, b) in enumerate(zip(grads, ref_grads)):
        assert int(torch.count_nonzero(b)) > 0
        cr.assert_grad_close(a, b, dtype, f"map {i}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_default_denominator_with_no_valid_object(dtype):
    B, N, H, W = 3, 5, 9, 11
    maps, xy, _, targets, _ = problem(B, N, H, W, [2, 2], dtype, [0, 0, 0], seed=41)
    xy[1] = torch.tensor([W, 0], dtype=torch.int32, device=DEV)   # sized below, but every centre outside the map
    sizes = torch.tensor([0, N, 0], device=DEV)
    loss, grads = run_loss(maps, cr.ragged(xy, sizes.cpu()), targets)
    assert float(loss) == 0.0
    for gmap in grads:
        assert int(torch.count_nonzero(gmap)) == 0 and not bool(torch.isnan(gmap).any())


def test_only_some_maps_need_a_gradient_and_empty_shapes():
    from accvlab.draw_heatmap import center_regression_loss, gather_at_centers

    B, N, H, W = 2, 6, 8, 12
    maps, xy, sizes, targets, _ = problem(B, N, H, W, [2, 0, 3], torch.float32, [6, 3], seed=43)
    assert maps[1].shape[1] == 0
    leaves = [maps[0].clone().requires_grad_(True), maps[1], maps[2].clone()]
    centers = cr.ragged(xy, sizes.cpu())
    center_regression_loss(leaves, centers, targets).backward()
    _, ref = cr.oracle_loss(maps, xy, sizes, targets)
    cr.assert_grad_close(leaves[0].grad, ref[0], torch.float32)
    assert leaves[2].grad is None
    # B == 0, Nmax == 0: forward returns 0 / empty, backward writes all-zero gradients
    empty = torch.zeros(0, 3, H, W, device=DEV, requires_grad=True)
    none = cr.ragged(torch.zeros(0, 4, 2, dtype=torch.int32, device=DEV), [])
    loss = center_regression_loss(empty, none, torch.zeros(0, 4, 3, device=DEV))
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert empty.grad.shape == empty.shape
    assert gather_at_centers(empty, none).tensor.shape == (0, 4, 3)
    m = torch.randn(B, 3, H, W, device=DEV, requires_grad=True)
    zero_n = cr.ragged(torch.zeros(B, 0, 2, dtype=torch.int32, device=DEV), [0, 0])
    loss = center_regression_loss(m, zero_n, torch.zeros(B, 0, 3, device=DEV))
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert int(torch.count_nonzero(m.grad)) == 0 and not bool(torch.isnan(m.grad).any())
    rows = gather_at_centers(m, zero_n)
    assert rows.tensor.shape == (B, 0, 3)
    rows.tensor.sum().backward()


# ------------------------------------------------------------------------------------------------------------ 3. duplicates
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_duplicates_add_in_slot_order(dtype):
    """2, 3 and 5 objects of frame 0 on one cell each, one of the cells used again in frame 1: the gradient there is the
    f32 sum, in ascending slot order, of (w * sign(d)) * (grad_out / denom), rounded once"""
    B, N, H, W, C = 2, 12, 6, 9, 3
    cells = {"a": (2, 1), "b": (7, 4), "c": (0, 5)}   # (x, y)
    order = ["c", "a", "b", "c", "c", "b", "a", "c", "b", "c"] + [None, None]   # slot -> cell, the last two elsewhere
    xy = torch.zeros(B, N, 2, dtype=torch.int32)
    for n, key in enumerate(order):
        xy[0, n] = torch.tensor(cells[key] if key else (4 + n % 2, 2))
    xy[1, 0] = torch.tensor(cells["a"])
    sizes = torch.tensor([N, 1])
    maps = cr.make_maps(B, [C], H, W, dtype, DEV, seed=51)
    g = torch.Generator().manual_seed(52)
    targets = torch.randn(B, N, C, generator=g) * 3.0
    weights = torch.exp(torch.randn(B, N, generator=g) * 3.0)   # spread over orders of magnitude: the order of the sum shows
    avg = 3.0
    go = 0.7
    xy_d, sizes_d = xy.to(DEV), sizes.to(DEV)
    _, grads = run_loss(maps, cr.ragged(xy_d, sizes), targets.to(DEV), weights.to(DEV), avg_factor=avg,
                        grad_out=torch.tensor(go, device=DEV))
    got = grads[0].cpu()
    x = maps[0].float().cpu().numpy()
    t, w = targets.numpy(), weights.numpy()
    scale = np.float32(go) / np.float32(avg)
    want = np.zeros((B, C, H, W), np.float32)
    for b in range(B):
        for n in range(int(sizes[b])):
            cx, cy = int(xy[b, n, 0]), int(xy[b, n, 1])
            for c in range(C):
                d = np.float32(x[b, c, cy, cx]) - np.float32(t[b, n, c])
                v = np.float32(np.float32(w[b, n]) * np.float32(np.sign(d))) * scale
                want[b, c, cy, cx] = np.float32(want[b, c, cy, cx] + v)
    want_t = torch.from_numpy(want).to(dtype)
    for key, count in (("a", 2), ("b", 3), ("c", 5)):
        assert order.count(key) == count
    assert torch.equal(got, want_t), (got - want_t).abs().max()
    _, ref = cr.oracle_loss(maps, xy_d, sizes_d, targets.to(DEV), weights.to(DEV), avg_factor=avg, grad_out=go)
    cr.assert_grad_close(grads[0], ref[0], dtype)


# -------------------------------------------------------------------------------------------------------- 4. complete write
def _inside(shape, dtype, poison, pad=257, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad + offset,), poison, dtype=dtype, device=DEV)
    return buf, buf[pad + offset: pad + offset + n].view(shape), pad + offset, n


def _margins_hold(buf, start, n, poison):
    same = torch.isnan if poison != poison else (lambda v: v == poison)
    return bool(same(buf[:start]).all()) and bool(same(buf[start + n:]).all())


def _direct_loss_bwd(maps, grads, xy, sizes, targets, weights, kind, beta, grad_out, denom):
    from accvlab import _amd_native as nat

    n = len(maps)
    mp = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
    gp = (ctypes.c_void_p * n)(*[m.data_ptr() for m in grads])
    ch = (ctypes.c_int * n)(*[m.shape[1] for m in maps])
    params = nat.CenterRegressionParams({"l1": nat.CR_L1, "smooth_l1": nat.CR_SMOOTH_L1}[kind], 0, beta, 0.0)
    B, _, H, W = maps[0].shape
    flags = (nat.CR_COUNTS_I64 if sizes.dtype == torch.int64 else 0) | \
        (nat.CR_WEIGHTS_PER_CHANNEL if weights is not None and weights.dim() == 3 else 0)
    dtype = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[maps[0].dtype]
    nat.check(nat.lib().accv_center_regression_loss_bwd(
        ctypes.addressof(mp), ctypes.addressof(gp), ctypes.addressof(ch), n, dtype, B, H, W, xy.data_ptr(), sizes.data_ptr(),
        xy.shape[1], flags, targets.data_ptr(), None if weights is None else weights.data_ptr(), ctypes.addressof(params),
        grad_out.data_ptr(), denom.data_ptr(), nat.stream_ptr(DEV)), "direct backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("H,W", [(37, 53), (16, 128), (5, 7), (1, 1), (50, 1924)])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_backward_writes_every_element_and_nothing_else(dtype, H, W, offset):
    """the C-ABI backward on gradient buffers full of NaN, embedded in larger NaN buffers off their alignment: afterwards
    no NaN is left inside, the values are those of the autograd path, and the bands around them are untouched"""
    B, N, channels = 3, 9, [2, 1, 3]
    maps, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [N, 0, 4], seed=H + W)
    weights = torch.rand(B, N, sum(channels), generator=g).to(DEV)
    centers = cr.ragged(xy, sizes.cpu())
    loss, want = run_loss(maps, centers, targets, weights, kind="smooth_l1", beta=1.2)
    valid, _ = cr.valid_and_index(xy, sizes, H, W)
    denom = valid.sum().clamp(min=1).float()
    carved = [_inside(m.shape, dtype, NAN, offset=offset) for m in maps]
    _direct_loss_bwd(maps, [c[1] for c in carved], xy, sizes, targets, weights, "smooth_l1", 1.2,
                     torch.ones((), device=DEV), denom)
    torch.cuda.synchronize()
    for (buf, view, start, n), ref in zip(carved, want):
        assert not bool(torch.isnan(view).any()), "an element of the gradient was not written"
        assert torch.equal(view, ref)
        assert _margins_hold(buf, start, n, NAN), "wrote outside the gradient map"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("H,W", [(37, 53), (5, 7), (33, 260)])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_gather_and_its_backward_stay_inside_their_buffers(dtype, H, W, offset):
    from accvlab import _amd_native as nat
    from accvlab.draw_heatmap import gather_at_centers

    SENT = -12345.0
    B, N, channels = 3, 9, [1, 4]
    C = sum(channels)
    plain, xy, sizes, _, g = problem(B, N, H, W, channels, dtype, [N, 0, 4], seed=H * W)
    # the maps inside poisoned buffers: a read outside them would put the poison into a row
    maps = []
    for m in plain:
        _, view, _, _ = _inside(m.shape, dtype, NAN, offset=offset)
        view.copy_(m)
        maps.append(view)
    leaves = [m.detach().requires_grad_(True) for m in maps]
    rows = gather_at_centers(leaves, cr.ragged(xy, sizes.cpu())).tensor
    assert torch.equal(rows, cr.oracle_gather(plain, xy, sizes).to(dtype))
    upstream = torch.randn(B, N, C, generator=g).to(dtype).to(DEV)
    rows.backward(upstream)
    # the two C-ABI entries on carved outputs
    n = len(maps)
    mp = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
    ch = (ctypes.c_int * n)(*channels)
    code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype]
    geometry = (ctypes.addressof(ch), n, code, B, H, W, xy.data_ptr(), sizes.data_ptr(), N, nat.CR_COUNTS_I64)
    buf, out, start, cnt = _inside((B, N, C), dtype, SENT, offset=offset)
    nat.check(nat.lib().accv_gather_at_centers(ctypes.addressof(mp), *geometry, out.data_ptr(), nat.stream_ptr(DEV)), "gather")
    carved = [_inside(m.shape, dtype, NAN, offset=offset) for m in maps]
    gp = (ctypes.c_void_p * n)(*[c[1].data_ptr() for c in carved])
    nat.check(nat.lib().accv_scatter_at_centers(ctypes.addressof(gp), *geometry, upstream.data_ptr(), nat.stream_ptr(DEV)),
              "scatter")
    torch.cuda.synchronize()
    assert torch.equal(out, rows.detach()) and _margins_hold(buf, start, cnt, SENT)
    for (gbuf, view, gstart, gn), leaf in zip(carved, leaves):
        assert not bool(torch.isnan(view).any()), "an element of the gradient was not written"
        assert torch.equal(view, leaf.grad)
        assert _margins_hold(gbuf, gstart, gn, NAN)
    # and the gradient is the oracle's: the sum of the upstream rows of the valid slots of a cell
    f = torch.cat([m.detach().double() for m in plain], 1).requires_grad_(True)
    valid, ind = cr.valid_and_index(xy, sizes, H, W)
    (cr._gather(f, valid, ind) * upstream.double()).sum().backward()
    for leaf, ref in zip(leaves, f.grad.split(channels, 1)):
        cr.assert_grad_close(leaf.grad, ref, dtype)


# --------------------------------------------------------------------------------- 5. reproducibility, no synchronisation
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_reproducible_and_free_of_host_synchronisation(dtype):
    from accvlab.draw_heatmap import gather_at_centers

    B, N, H, W, channels = 8, 300, 45, 80, [2, 1, 3]
    maps, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [300, 0, 17, 1, 256, 257, 299, 64], seed=61)
    weights = torch.rand(B, N, generator=g).to(DEV)
    centers = cr.ragged(xy, sizes)   # device sample sizes
    avg = torch.tensor(100.0, device=DEV)
    upstream = torch.randn(B, N, sum(channels), generator=g).to(dtype).to(DEV)

    def once():
        loss, grads = run_loss(maps, centers, targets, weights, kind="smooth_l1", avg_factor=avg)
        leaves = [m.detach().clone().requires_grad_(True) for m in maps]
        rows = gather_at_centers(leaves, centers).tensor
        rows.backward(upstream)
        return [loss, rows.detach(), *grads, *[m.grad for m in leaves]]

    first = once()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = once()
        third = run_loss(maps, centers, targets, None)   # default denominator: counted on the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(third[0]))
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------- 6. special values
def _assert_same_special(got, want, dtype, what):
    """NaN and infinities exactly where the float64 result has them; the finite rest within the bars"""
    want_c = want.to(dtype)
    assert torch.equal(torch.isnan(got), torch.isnan(want_c)), f"{what}: NaN pattern"
    inf = torch.isinf(want_c)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want_c[inf]), f"{what}: infinities"
    fin = torch.isfinite(want_c)
    cr.assert_grad_close(torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, want, torch.zeros_like(want)), dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["l1", "smooth_l1"])
@pytest.mark.parametrize("where", ["cell", "target", "weight"])
@pytest.mark.parametrize("value", [NAN, INF, -INF, -0.0], ids=["nan", "inf", "-inf", "-0"])
def test_special_values_follow_float64_autograd(dtype, kind, where, value):
    B, N, H, W, channels = 2, 6, 7, 9, [2, 2]
    maps, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [6, 3], seed=71, margin=0)
    xy[0, 0] = torch.tensor([4, 3], dtype=torch.int32)
    xy[0, 1] = torch.tensor([4, 3], dtype=torch.int32)      # a second object on the special cell
    weights = torch.rand(B, N, sum(channels), generator=g).to(DEV) + 0.5
    if where == "cell":
        maps[0][0, 1, 3, 4] = value
    elif where == "target":
        targets[0, 0, 1] = value
    else:
        weights[0, 0, 1] = value
    centers = cr.ragged(xy, sizes.cpu())
    loss, grads = run_loss(maps, centers, targets, weights, kind=kind, beta=1.0, avg_factor=5.0)
    ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights, kind, 1.0, 5.0)
    if bool(torch.isfinite(ref)):
        cr.assert_loss_close(loss, ref)
    else:
        assert torch.equal(loss.double(), ref.to(torch.float32).double()) or (bool(torch.isnan(loss)) and bool(torch.isnan(ref)))
    for i, (a, b) in enumerate(zip(grads, ref_grads)):
        _assert_same_special(a, b, dtype, f"map {i}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["l1", "smooth_l1"])
def test_nan_in_everything_unread_reaches_nothing(dtype, kind):
    from accvlab.draw_heatmap import gather_at_centers

    B, N, H, W, channels = 3, 8, 9, 13, [3, 1]
    clean, xy, sizes, targets, g = problem(B, N, H, W, channels, dtype, [8, 0, 3], seed=81)
    weights = torch.rand(B, N, generator=g).to(DEV) + 0.5
    valid, ind = cr.valid_and_index(xy, sizes, H, W)
    targets[~valid] = NAN
    weights[~valid] = NAN
    read = torch.zeros(B, H * W, dtype=torch.bool, device=DEV)
    read.view(-1)[(torch.arange(B, device=DEV).view(B, 1) * (H * W) + ind)[valid]] = True
    maps = [torch.where(read.view(B, 1, H, W), m, torch.full_like(m, NAN)) for m in clean]
    centers = cr.ragged(xy, sizes.cpu())
    loss, grads = run_loss(maps, centers, targets, weights, kind=kind)
    ref, ref_grads = cr.oracle_loss(clean, xy, sizes, torch.nan_to_num(targets), torch.nan_to_num(weights), kind)
    cr.assert_loss_close(loss, ref)
    for a, b in zip(grads, ref_grads):
        assert bool(torch.isfinite(a).all())
        cr.assert_grad_close(a, b, dtype)
    rows = gather_at_centers(maps, centers).tensor
    assert bool(torch.isfinite(rows).all()) and torch.equal(rows, cr.oracle_gather(clean, xy, sizes).to(dtype))


# -------------------------------------------------------------------------------------------------------------------- 7. sizes
def test_map_beyond_2_31_elements():
    """one bf16 map of more than 2^31 elements, three objects in the last frame: their elements lie past 2^31"""
    from accvlab.draw_heatmap import gather_at_centers

    B, C, H, W = 3, 3, 16400, 16400
    assert B * C * H * W > 2 ** 31 and H * W < 2 ** 31
    m = torch.empty(B, C, H, W, dtype=torch.bfloat16, device=DEV)
    m.view(-1)[:] = 0.5
    xy = torch.zeros(B, 4, 2, dtype=torch.int32)
    pts = [(W - 1, H - 1), (17, H - 2), (W - 3, 16000)]
    xy[2, :3] = torch.tensor(pts, dtype=torch.int32)
    xy[2, 3] = torch.tensor([5, 5], dtype=torch.int32)   # beyond the sample size
    sizes = torch.tensor([0, 0, 3])
    vals = torch.arange(1, 10, dtype=torch.float32).view(3, 3)   # [object, channel]
    for n, (x, y) in enumerate(pts):
        for c in range(C):
            assert ((2 * C + c) * H + y) * W + x > 2 ** 31 or c < 2
            m[2, c, y, x] = vals[n, c]
    m.requires_grad_(True)
    centers = cr.ragged(xy.to(DEV), sizes)
    rows = gather_at_centers(m, centers).tensor
    want = torch.zeros(B, 4, C)
    want[2, :3] = vals
    assert torch.equal(rows.detach().float().cpu(), want)
    up = torch.zeros(B, 4, C)
    up[2] = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0], [100.0, 100.0, 100.0]])
    up[0] = 55.0   # frames without objects
    rows.backward(up.to(torch.bfloat16).to(DEV))
    assert int(torch.count_nonzero(m.grad)) == 9
    for n, (x, y) in enumerate(pts):
        assert torch.equal(m.grad[2, :, y, x].float().cpu(), up[2, n])
    del rows
    m.grad = None
    from accvlab.draw_heatmap import center_regression_loss
    targets = torch.zeros(B, 4, C, device=DEV)
    loss = center_regression_loss(m, centers, targets, avg_factor=2.0)
    assert float(loss.detach()) == float(vals.sum()) / 2.0
    loss.backward()
    assert int(torch.count_nonzero(m.grad)) == 9
    for x, y in pts:
        assert torch.equal(m.grad[2, :, y, x].float().cpu(), torch.full((C,), 0.5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_headline_geometry(dtype):
    from accvlab.batching_helpers import combine_data
    from accvlab.draw_heatmap import gather_at_centers

    B, H, W, channels = 64, 270, 480, [2, 2]
    centers_l, _ = wl.heatmap_objects(B, H, W)
    centers = combine_data([c.to(DEV) for c in centers_l])
    xy, sizes = centers.tensor, centers.sample_sizes
    N = xy.shape[1]
    maps = cr.make_maps(B, channels, H, W, dtype, DEV, seed=91)
    g = torch.Generator().manual_seed(92)
    targets = (torch.randn(B, N, 4, generator=g) * 3.0).to(DEV)
    weights = torch.rand(B, N, generator=g).to(DEV)
    assert torch.equal(gather_at_centers(maps, centers).tensor, cr.oracle_gather(maps, xy, sizes).to(dtype))
    loss, grads = run_loss(maps, centers, targets, weights)
    ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights)
    cr.assert_loss_close(loss, ref)
    for a, b in zip(grads, ref_grads):
        cr.assert_grad_close(a, b, dtype)


# --------------------------------------------------------------------------------------------------------------- 8. round trip
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_round_trip_with_drawing_and_peaks(dtype):
    from accvlab.draw_heatmap import draw_heatmap_batched, gather_at_centers, heatmap_peaks

    B, H, W, k, channels = 4, 60, 90, 25, [2, 3]
    g = torch.Generator().manual_seed(101)
    xy = torch.empty(B, k, 2, dtype=torch.int32)
    for b in range(B):   # distinct nodes of a 3-cell grid: at least three cells apart in x or y
        nodes = torch.randperm((H // 3) * (W // 3), generator=g)[:k]
        xy[b, :, 0] = (nodes % (W // 3)) * 3 + 1
        xy[b, :, 1] = (nodes // (W // 3)) * 3 + 1
    sizes = torch.full((B,), k)
    centers = cr.ragged(xy.to(DEV), sizes.to(DEV))
    radii = cr.ragged(torch.ones(B, k, dtype=torch.int32, device=DEV), sizes.to(DEV))
    hm = torch.empty(B, H, W, device=DEV)
    draw_heatmap_batched(hm, centers, radii, 6.0, 1.0, clear=True)
    ind = (xy[..., 1].long() * W + xy[..., 0].long()).to(DEV)
    # the precondition: every centre is 1, every other cell below 1
    assert bool((hm.view(B, -1).gather(1, ind) == 1).all()) and int((hm == 1).sum()) == B * k and float(hm.max()) == 1.0
    peaks = heatmap_peaks(hm.view(B, 1, H, W), k)
    assert torch.equal(peaks.indices.sort(1).values, ind.sort(1).values)
    maps = cr.make_maps(B, channels, H, W, dtype, DEV, seed=102)
    by_peaks = gather_at_centers(maps, peaks.indices)
    by_centers = gather_at_centers(maps, centers).tensor
    op, oc = peaks.indices.argsort(1), ind.argsort(1)
    C = sum(channels)
    assert torch.equal(by_peaks.gather(1, op[..., None].expand(-1, -1, C)), by_centers.gather(1, oc[..., None].expand(-1, -1, C)))
    assert int(torch.count_nonzero(by_centers)) > 0


# ------------------------------------------------------------------------------------------------------------------- 9. errors
def test_refusals_raise_runtime_error():
    from types import SimpleNamespace

    from accvlab.draw_heatmap import center_regression_loss, gather_at_centers

    B, N, H, W = 2, 5, 8, 12
    m = torch.zeros(B, 4, H, W, device=DEV)
    xy = torch.zeros(B, N, 2, dtype=torch.int32, device=DEV)
    sizes = torch.tensor([5, 2], device=DEV)
    centers = cr.ragged(xy, sizes)
    tg = torch.zeros(B, N, 4, device=DEV)
    rb = lambda t, s=sizes: SimpleNamespace(tensor=t, sample_sizes=s)  # noqa: E731
    bad_feats = {
        "non-contiguous": m.transpose(2, 3), "3-d": m[0], "float64": m.double(), "int": m.int(),
        "mixed dtype": [m, m.half()], "mixed shape": [m, torch.zeros(B, 4, H, W + 1, device=DEV)],
        "mixed batch": [m, torch.zeros(B + 1, 4, H, W, device=DEV)], "mixed device": [m, m.cpu()], "empty list": [],
        "nine maps": [m] * 9, "65 channels": [torch.zeros(B, 33, H, W, device=DEV), torch.zeros(B, 32, H, W, device=DEV)],
    }
    for what, feats in bad_feats.items():
        with pytest.raises(RuntimeError, match="gather_at_centers"):
            gather_at_centers(feats, centers)
        if what not in ("65 channels",):
            with pytest.raises(RuntimeError, match="center_regression_loss"):
                center_regression_loss(feats, centers, tg)
    with pytest.raises(RuntimeError, match="at most 64 channels"):
        gather_at_centers(bad_feats["65 channels"], centers)
    bad_where = {
        "float centres": rb(xy.float()), "int64 centres": rb(xy.long()), "wrong last dim": rb(xy[..., :1].contiguous()),
        "wrong batch": rb(xy[:1], sizes[:1]), "cpu centres": rb(xy.cpu()), "cpu sizes": rb(xy, sizes.cpu()),
        "float sizes": rb(xy, sizes.float()), "sizes shape": rb(xy, sizes[:1]), "non-contiguous": rb(xy.repeat(1, 2, 1)[:, ::2]),
    }
    for what, where in bad_where.items():
        with pytest.raises(RuntimeError, match="gather_at_centers"):
            gather_at_centers(m, where)
        with pytest.raises(RuntimeError, match="center_regression_loss"):
            center_regression_loss(m, where, tg)
    for where in (xy[..., 0].contiguous(), torch.zeros(B, 3, dtype=torch.int64), torch.zeros(B + 1, 3, dtype=torch.int64, device=DEV),
                  torch.zeros(B, 3, 1, dtype=torch.int64, device=DEV), torch.zeros(B, 6, dtype=torch.int64, device=DEV)[:, ::2], 5):
        with pytest.raises(RuntimeError, match="gather_at_centers"):
            gather_at_centers(m, where)
    with pytest.raises(RuntimeError, match="RaggedBatch"):
        center_regression_loss(m, torch.zeros(B, 3, dtype=torch.int64, device=DEV), tg)   # the loss takes ragged centres only
    bad_loss = [
        dict(targets=tg.double()), dict(targets=tg[..., :3].contiguous()), dict(targets=tg.cpu()), dict(targets=None),
        dict(targets=tg.clone().requires_grad_(True)), dict(targets=torch.zeros(B, N, 8, device=DEV)[..., ::2]),
        dict(weights=torch.zeros(B, N, 2, device=DEV)), dict(weights=torch.zeros(B, N, device=DEV).double()),
        dict(weights=torch.zeros(B, N).requires_grad_(True).to(DEV)), dict(weights=torch.zeros(B, N)),
        dict(kind="l2"), dict(kind="smooth_l1", beta=0.0), dict(kind="smooth_l1", beta=-1.0),
        dict(avg_factor=torch.tensor(1.0)), dict(avg_factor=torch.ones(1, device=DEV)),
        dict(avg_factor=torch.tensor(1.0, device=DEV, dtype=torch.float64)),
    ]
    for kw in bad_loss:
        kw = dict(kw)
        targets = kw.pop("targets", tg)
        with pytest.raises(RuntimeError, match="center_regression_loss"):
            center_regression_loss(m, centers, targets, kw.pop("weights", None), **kw)
    # the accepted forms still work after all of that
    loss = center_regression_loss(m, centers, tg, torch.ones(B, N, device=DEV), kind="smooth_l1", beta=0.5)
    assert float(loss) == 0.0
