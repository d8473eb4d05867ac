"""Gradients of the lane_helpers polyline operators on CPU tensors (the host backward accv_polyline_grad_host behind
torch autograd).  The reference is float64 torch autograd of the definition: the query's segment found by the kernel's
own binary search (no grad), then differentiable ops for the branch it took."""
import pytest
import torch

from accvlab.batching_helpers import RaggedBatch


def _poly():
    from accvlab.lane_helpers import polyline
    return polyline


# ---------------------------------------------------------------- float64 reference
def _search(acc, n, d):
    """the kernel's search: last index with acc <= d (an exact hit stops at the index it met), -1 before the start,
    n - 1 at / beyond the end; acc [B, P], n [B], d [B, Q]"""
    b, q = d.shape
    last = (n - 1).clamp(min=0).view(b, 1).expand(b, q)
    first_v = acc[:, :1].expand(b, q)
    last_v = acc.gather(1, last)
    mn = torch.zeros_like(last)
    mx = last.clone()
    while True:
        active = (mx - mn) > 1
        if not bool(active.any()):
            break
        c = (mn + mx) // 2
        v = acc.gather(1, c)
        lt, gt = v < d, v > d
        eq = ~lt & ~gt
        mn = torch.where(active & (lt | eq), c, mn)
        mx = torch.where(active & (gt | eq), c, mx)
    idx = torch.where(first_v > d, torch.full_like(mn, -1), torch.where(last_v < d, last, mn))
    return idx


def ref_sample(points, distances, n=None, relative=False, eps=None):
    """(samples [B, Q, D], lengths [B]) in float64, differentiable w.r.t. points and distances"""
    b, pmax, dims = points.shape
    q = distances.shape[1] if distances is not None else 0
    dev = points.device
    n = torch.full((b,), pmax, dtype=torch.int64, device=dev) if n is None else n.to(torch.int64).to(dev)
    eps = torch.finfo(points.dtype).eps if eps is None else eps
    if pmax > 1:
        seg = torch.linalg.vector_norm(points[:, 1:] - points[:, :-1], dim=2)
        valid = torch.arange(pmax - 1, device=dev).unsqueeze(0) < (n - 1).unsqueeze(1)
        seg = seg * valid
        acc = torch.cat([torch.zeros((b, 1), dtype=points.dtype, device=dev), torch.cumsum(seg, 1)], 1)
    else:
        seg = torch.zeros((b, 1), dtype=points.dtype, device=dev)
        acc = torch.zeros((b, max(pmax, 1)), dtype=points.dtype, device=dev)
    total = acc.gather(1, (n - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
    lengths = torch.where(n == 0, torch.full_like(total, float("nan")), total)
    if distances is None:
        return None, lengths
    d = distances * total.unsqueeze(1) if relative else distances
    with torch.no_grad():
        idx = _search(acc.detach(), n, d.detach())
        last = (n - 1).clamp(min=0).unsqueeze(1)
        inside = (idx >= 0) & (idx < last)
        i = idx.clamp(min=0, max=max(pmax - 2, 0))
        i1 = (i + 1).clamp(max=max(pmax - 1, 0))
        ln = acc.detach().gather(1, i1) - acc.detach().gather(1, i)
        interp = inside & (ln >= eps)
        j = torch.where(idx < 0, torch.zeros_like(idx), idx.minimum(last))
    c_i = acc.gather(1, i)
    l_i = torch.where(interp, seg.gather(1, i.clamp(max=seg.shape[1] - 1)), torch.ones_like(c_i))
    w1 = torch.where(interp, (d - c_i) / l_i, torch.zeros_like(c_i)).unsqueeze(-1)
    if pmax == 0:
        return torch.full((b, q, dims), float("nan"), dtype=points.dtype, device=dev), lengths
    pi = points.gather(1, i.unsqueeze(-1).expand(b, q, dims))
    pi1 = points.gather(1, i1.unsqueeze(-1).expand(b, q, dims))
    pj = points.gather(1, j.unsqueeze(-1).expand(b, q, dims))
    out = torch.where(interp.unsqueeze(-1), pi + w1 * (pi1 - pi), pj)
    out = torch.where((n == 0).view(b, 1, 1), torch.full_like(out, float("nan")), out)
    return out, lengths


def ref_grads(points, distances, grad_out=None, grad_lengths=None, p_sizes=None, d_sizes=None, relative=False, eps=None):
    """float64 gradients (points, distances) of <samples, grad_out> + <lengths, grad_lengths>, padded entries masked"""
    p = points.detach().double().requires_grad_()
    d = distances.detach().double().requires_grad_() if distances is not None else None
    out, lens = ref_sample(p, d, p_sizes, relative, eps)
    b = p.shape[0]
    terms = []
    if grad_out is not None:
        g = grad_out.double()
        if d_sizes is not None:
            live = torch.arange(g.shape[1], device=g.device).unsqueeze(0) < d_sizes.to(g.device).unsqueeze(1)
            g = g * live.unsqueeze(-1)
        n = p_sizes.to(g.device) if p_sizes is not None else torch.full((b,), p.shape[1], device=g.device)
        g = torch.where((n == 0).view(b, 1, 1), torch.zeros_like(g), g)
        terms.append((torch.nan_to_num(out, nan=0.0) * g).sum())
    if grad_lengths is not None:
        gl = grad_lengths.double()
        terms.append((torch.nan_to_num(lens, nan=0.0) * gl).sum())
    inputs = [p] + ([d] if d is not None else [])
    grads = torch.autograd.grad(sum(terms), inputs, allow_unused=True)
    gp = grads[0] if grads[0] is not None else torch.zeros_like(p)
    gd = None
    if d is not None:
        gd = grads[1] if grads[1] is not None else torch.zeros_like(d)
    return gp, gd


def _general(b, pmax, q, dims=2, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn((b, pmax, dims), generator=g, dtype=torch.float64).cumsum(1)
    fr = torch.rand((b, q), generator=g, dtype=torch.float64) * 1.2 - 0.1
    return pts.to(dtype), fr.to(dtype)


def _close(got, ref, rtol=1e-9, atol_frac=1e-12):
    got = got.double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = (got - ref).abs()
    bound = rtol * ref.abs() + atol_frac * scale + 1e-300
    assert bool((err <= bound).all()), f"max err {float(err.max()):.3e}, worst ratio {float((err / bound).max()):.3e}"


# ---------------------------------------------------------------- the feature exists
def test_interpolate_and_lengths_backward_fill_grad():
    poly = _poly()
    p = torch.tensor([[[0.0, 0.0], [3.0, 0.0], [3.0, 4.0]]], requires_grad=True)
    d = torch.tensor([[1.0, 5.0]])
    poly.interpolate(p, d).sum().backward()
    assert p.grad is not None and torch.isfinite(p.grad).all()
    q = p.detach().clone().requires_grad_()
    poly.lengths(q).sum().backward()
    # d T / d points: -e0, e0 - e1, e1
    assert torch.equal(q.grad, torch.tensor([[[-1.0, 0.0], [1.0, -1.0], [0.0, 1.0]]]))


# ---------------------------------------------------------------- gradcheck (float64, general position, off knots)
@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("dims", [2, 3, 5])
def test_gradcheck_fixed(relative, dims):
    poly = _poly()
    p, fr = _general(3, 9, 13, dims, seed=dims)
    if not relative:
        fr = fr * poly.lengths(p).unsqueeze(1)
    p.requires_grad_()
    fr.requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: poly.interpolate(a, b, relative=relative), (p, fr))
    assert torch.autograd.gradcheck(poly.lengths, (p,))


@pytest.mark.parametrize("relative", [False, True])
def test_gradcheck_ragged(relative):
    poly = _poly()
    p, fr = _general(4, 10, 12, 2, seed=7)
    ps = torch.tensor([10, 6, 2, 1])
    qs = torch.tensor([12, 5, 7, 0])
    if not relative:
        fr = fr * poly.lengths_var_size_batch(RaggedBatch(p, sample_sizes=ps)).nan_to_num().unsqueeze(1)
    p.requires_grad_()
    fr.requires_grad_()

    def f(a, b):
        out = poly.interpolate_var_size_batch(RaggedBatch(a, sample_sizes=ps), RaggedBatch(b, sample_sizes=qs),
                                              relative=relative)
        live = (torch.arange(12).unsqueeze(0) < qs.unsqueeze(1)).unsqueeze(-1)
        # padded samples are unspecified memory (possibly NaN / inf): selected away, not multiplied by 0
        return torch.where(live, out.tensor, torch.zeros_like(out.tensor))

    assert torch.autograd.gradcheck(f, (p, fr))
    assert torch.autograd.gradcheck(lambda a: poly.lengths_var_size_batch(RaggedBatch(a, sample_sizes=ps)), (p,))


# ---------------------------------------------------------------- branch cases, gradients derived by hand
L3 = [[0.0, 0.0], [3.0, 0.0], [3.0, 4.0]]   # segments 3 (along x) and 4 (along y), T = 7


def _grads(points, dist, g, relative=False):
    poly = _poly()
    p = torch.tensor([points], dtype=torch.float64, requires_grad=True)
    d = torch.tensor([dist], dtype=torch.float64, requires_grad=True)
    out = poly.interpolate(p, d, relative=relative)
    out.backward(torch.tensor([g], dtype=torch.float64))
    return p.grad[0], d.grad[0]


@pytest.mark.parametrize("dist,exp_p,exp_d", [
    (-1.0, [[1, 2], [0, 0], [0, 0]], 0.0),         # before the start: a copy of p0
    (8.0, [[0, 0], [0, 0], [1, 2]], 0.0),          # beyond T: a copy of p2
    (0.0, [[1, 2], [0, 0], [0, 0]], 1.0),          # exactly 0: segment 0 with w1 = 0, d/dd = g . e0
    (7.0, [[2, 0], [-2, 2], [1, 0]], 2.0),         # exactly T: segment 1 with w1 = 1
    (3.0, [[2, 0], [-1, 2], [0, 0]], 2.0),         # exactly on the interior knot: segment 1 with w1 = 0
    (1.5, [[1, 1], [0, 1], [0, 0]], 1.0),          # inside segment 0, w1 = 1/2: g / 2 each, lambda_0 = -s / 2 along x
])
def test_branch_cases_by_hand(dist, exp_p, exp_d):
    gp, gd = _grads(L3, [dist], [[1.0, 2.0]])
    assert torch.allclose(gp, torch.tensor(exp_p, dtype=torch.float64), atol=1e-12, rtol=0), gp
    assert abs(float(gd[0]) - exp_d) <= 1e-12


def test_zero_length_segment():
    pts = [[0.0, 0.0], [2.0, 0.0], [2.0, 0.0], [2.0, 3.0]]   # C = 0, 2, 2, 5
    # d = 2 stops on knot 1 (the zero-length segment): a copy of p1, no distance gradient
    gp, gd = _grads(pts, [2.0], [[1.0, 2.0]])
    assert torch.equal(gp, torch.tensor([[0.0, 0.0], [1.0, 2.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64))
    assert float(gd[0]) == 0.0
    # d = 3.5: segment 2 with w1 = 1/2, s = g_y = 2: lambda_2 = -1 (moves p2, p3 along y), lambda_1 none (zero length),
    # lambda_0 = -2 (moves p0 +2 x, p1 -2 x)
    gp, gd = _grads(pts, [3.5], [[1.0, 2.0]])
    exp = [[2.0, 0.0], [-2.0, 0.0], [0.5, 1.0 + 1.0], [0.5, 1.0 - 1.0]]
    assert torch.allclose(gp, torch.tensor(exp, dtype=torch.float64), atol=1e-12, rtol=0), gp
    assert float(gd[0]) == 2.0
    # lengths: the zero-length segment passes nothing (zero subgradient of the norm)
    poly = _poly()
    p = torch.tensor([pts], dtype=torch.float64, requires_grad=True)
    poly.lengths(p).backward(torch.ones(1, dtype=torch.float64))
    assert torch.equal(p.grad[0], torch.tensor([[-1.0, 0.0], [1.0, 0.0], [0.0, -1.0], [0.0, 1.0]], dtype=torch.float64))


def test_zero_one_two_point_polylines():
    poly = _poly()
    p = torch.tensor([[[5.0, 1.0], [9.0, 9.0], [9.0, 9.0]], [[1.0, 1.0], [4.0, 5.0], [7.0, 7.0]],
                      [[2.0, 2.0], [2.0, 6.0], [7.0, 7.0]]], dtype=torch.float64, requires_grad=True)
    ps = torch.tensor([0, 1, 2])
    d = torch.tensor([[1.0, 2.0], [1.0, 2.0], [1.0, 5.0]], dtype=torch.float64, requires_grad=True)
    qs = torch.tensor([2, 2, 2])
    out = poly.interpolate_var_size_batch(RaggedBatch(p, sample_sizes=ps), RaggedBatch(d, sample_sizes=qs))
    assert torch.isnan(out.tensor[0]).all()
    out.tensor.backward(torch.ones_like(out.tensor))   # NaN samples of the empty polyline: zero gradient
    exp_p = torch.zeros_like(p)
    exp_p[1, 0] = 2.0                                  # one point: both samples are copies of it
    # two points, e0 = (0, 1): d = 1 inside with w1 = 1/4 and s = 1 -> 3/4 g, 1/4 g and lambda_0 = -1/4, which moves
    # p1 by (0, -1/4) and p0 by (0, +1/4); d = 5 beyond the end -> a copy of p1
    exp_p[2, 0] = torch.tensor([0.75, 0.75 + 0.25])
    exp_p[2, 1] = torch.tensor([0.25 + 1.0, 0.25 - 0.25 + 1.0])
    assert torch.allclose(p.grad, exp_p, atol=1e-12), p.grad
    assert torch.equal(d.grad, torch.tensor([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]], dtype=torch.float64))
    q = p.detach().clone().requires_grad_()
    ln = poly.lengths_var_size_batch(RaggedBatch(q, sample_sizes=ps))
    assert torch.isnan(ln[0]) and float(ln[1].detach()) == 0.0 and float(ln[2].detach()) == 4.0
    ln.backward(torch.ones(3, dtype=torch.float64))
    exp_q = torch.zeros_like(q)
    exp_q[2, 0] = torch.tensor([0.0, -1.0])
    exp_q[2, 1] = torch.tensor([0.0, 1.0])
    assert torch.equal(q.grad, exp_q)


def test_relative_with_zero_total_length():
    # T = 0: every fraction maps to d = 0; the search stops on the middle knot, a zero-length segment: a copy of p1
    gp, gd = _grads([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]], [0.5, 0.0], [[1.0, 2.0], [3.0, 4.0]], relative=True)
    assert torch.equal(gp, torch.tensor([[0.0, 0.0], [4.0, 6.0], [0.0, 0.0]], dtype=torch.float64))
    assert torch.equal(gd, torch.zeros(2, dtype=torch.float64))


# ---------------------------------------------------------------- against the float64 reference, host backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("relative", [False, True])
def test_host_backward_matches_reference(dtype, relative):
    poly = _poly()
    p, fr = _general(6, 40, 50, 2, seed=11, dtype=dtype)
    ps = torch.tensor([40, 17, 2, 1, 0, 33])
    qs = torch.tensor([50, 20, 7, 3, 5, 0])
    if not relative:
        fr = (fr.double() * poly.lengths_var_size_batch(RaggedBatch(p, sample_sizes=ps)).double().nan_to_num()
              .unsqueeze(1)).to(dtype)
    g = torch.randn((6, 50, 2), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype)
    gl = torch.randn(6, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(dtype)
    pr = p.clone().requires_grad_()
    dr = fr.clone().requires_grad_()
    out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps), RaggedBatch(dr, sample_sizes=qs),
                                          relative=relative)
    assert out.tensor.dtype == dtype
    ln = poly.lengths_var_size_batch(RaggedBatch(pr, sample_sizes=ps))
    torch.autograd.backward([out.tensor, ln], [g, gl])
    # host arithmetic is double for both dtypes: the reference on the same (dtype-valued) inputs
    rp, rd = ref_grads(p, fr, g, gl, ps, qs, relative, eps=torch.finfo(torch.float64).eps)
    rtol = 1e-9 if dtype == torch.float64 else 2 * torch.finfo(torch.float32).eps
    _close(pr.grad, rp, rtol=rtol, atol_frac=rtol)
    _close(dr.grad, rd, rtol=rtol, atol_frac=rtol)
    assert torch.equal(pr.grad[4], torch.zeros_like(pr.grad[4]))
    assert torch.equal(pr.grad[2, 2:], torch.zeros_like(pr.grad[2, 2:]))   # behind the point count: exactly 0


def test_padded_grad_out_is_ignored_and_needs_input_grad():
    poly = _poly()
    p, fr = _general(3, 12, 9, 2, seed=5)
    ps = torch.tensor([12, 5, 8])
    qs = torch.tensor([9, 4, 1])

    def run(fill, want_d=True):
        pr = p.clone().requires_grad_()
        dr = fr.clone().requires_grad_(want_d)
        out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps), RaggedBatch(dr, sample_sizes=qs),
                                              relative=True)
        g = torch.ones_like(out.tensor)
        live = (torch.arange(9).unsqueeze(0) < qs.unsqueeze(1)).unsqueeze(-1)
        g = torch.where(live, g, torch.full_like(g, fill))
        out.tensor.backward(g)
        return pr.grad, dr.grad

    gp0, gd0 = run(0.0)
    gp1, gd1 = run(float("nan"))
    gp2, gd2 = run(1e30)
    assert torch.equal(gp0, gp1) and torch.equal(gp0, gp2)
    assert torch.equal(gd0, gd1) and torch.equal(gd0, gd2)
    assert torch.equal(gd0[1, 4:], torch.zeros(5, dtype=torch.float64))
    gp3, gd3 = run(0.0, want_d=False)
    assert gd3 is None and torch.equal(gp3, gp0)


def test_forward_is_bitwise_the_same_with_and_without_grad():
    poly = _poly()
    for dtype in (torch.float32, torch.float64):
        p, fr = _general(4, 30, 40, 3, seed=9, dtype=dtype)
        a = poly.interpolate(p, fr, relative=True)
        b = poly.interpolate(p.clone().requires_grad_(), fr, relative=True)
        assert b.requires_grad and torch.equal(a, b.detach())
        assert torch.equal(poly.lengths(p), poly.lengths(p.clone().requires_grad_()).detach())
        with torch.no_grad():
            c = poly.interpolate(p.clone().requires_grad_(), fr, relative=True)
        assert not c.requires_grad and torch.equal(a, c)


def test_host_entry_point_rejects_other_dtypes():
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    assert lib.accv_polyline_grad_host(None, None, None, None, None, None, None, None, 1, 2, 2, 2, 2, 0, 0, 0) == -1
    assert b"float32 / float64" in lib.accv_last_error()
    assert lib.accv_polyline_grad_host(None, None, None, None, None, None, None, None, -1, 2, 2, 2, 0, 0, 0, 0) == -1
    assert lib.accv_polyline_grad(None, None, None, None, None, None, None, None, 1, 2, 2, 2, 7, 0, 0, None, 0,
                                  None) == -1
    # too small a workspace is refused before any launch
    need = lib.accv_polyline_grad_workspace_bytes(4, 9000, 100, 2, 0)
    assert need > 0
    dummy = 4096
    assert lib.accv_polyline_grad(dummy, dummy, None, None, dummy, None, dummy, None, 4, 9000, 100, 2, 0, 0, 0,
                                  dummy, need - 1, None) == -3
