"""Gradients of the lane_helpers polyline operators on the GPU (the HIP backward accv_polyline_grad behind torch
autograd), against float64 torch autograd of the definition: the query's segment found by the kernel's own binary search
(no grad), then differentiable ops for the branch it took.

float32 data sit on an integer lattice with axis-parallel segments: segment lengths, arc lengths and the relative query
positions (fractions k / 1024) are then exact in float32, so the kernel and the float64 reference take the same branch
and the comparison measures the backward alone (rounding of w1 and of the accumulation), not the conditioning of a long
float32 prefix sum."""
import pytest
import torch

from accvlab.batching_helpers import RaggedBatch

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _lattice(b, pmax, q, dims=2, relative=False, seed=0, max_step=3):
    """float64 lattice points [b, pmax, dims] and queries [b, q] (fractions k / 1024 or float32 arc lengths)"""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.cat([torch.eye(dims), -torch.eye(dims)]).double()
    k = torch.randint(0, 2 * dims, (b, max(pmax - 1, 0)), generator=g)
    steps = dirs[k] * torch.randint(1, max_step + 1, (b, max(pmax - 1, 0), 1), generator=g).double()
    start = torch.randint(-16, 17, (b, 1, dims), generator=g).double()
    pts = torch.cat([start, start + steps.cumsum(1)], 1)[:, :pmax]
    if relative:
        fr = torch.randint(-64, 1024 + 64, (b, q), generator=g).double() / 1024
    else:
        tot = steps.abs().sum((1, 2)) if pmax > 1 else torch.zeros(b, dtype=torch.float64)
        fr = ((torch.rand((b, q), generator=g, dtype=torch.float64) * 1.2 - 0.1) * tot.unsqueeze(1)).float().double()
    return pts, fr


def _gout(shape, seed, dtype):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def _check(got, ref, rtol, atol_frac, what):
    got = got.double().cpu()
    ref = ref.double().cpu()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = (got - ref).abs()
    bound = rtol * ref.abs() + atol_frac * scale
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} outside, max err {float(err.max()):.3e}, "
                                 f"worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3e}, max |ref| {scale:.3e}")


def _run(p, fr, relative, dtype, ps=None, qs=None, seed=1, terms=("samples", "lengths")):
    """GPU gradients of <interpolate, g> + <lengths, gl> (the terms named) and their float64 reference on the dtype-rounded
    inputs"""
    poly = _poly()
    pd, fd = p.to(dtype), fr.to(dtype)
    g = _gout(pd.shape[:1] + fd.shape[1:] + pd.shape[2:], seed, dtype)
    gl = _gout(pd.shape[:1], seed + 1, dtype)
    pr = pd.to(DEV).requires_grad_()
    dr = fd.to(DEV).requires_grad_()
    if ps is None:
        out = poly.interpolate(pr, dr, relative=relative)
        ln = poly.lengths(pr)
    else:
        out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps.to(DEV)), RaggedBatch(dr, sample_sizes=qs.to(DEV)),
                                              relative=relative).tensor
        ln = poly.lengths_var_size_batch(RaggedBatch(pr, sample_sizes=ps.to(DEV)))
    assert out.dtype == dtype and ln.dtype == dtype
    g = g if "samples" in terms else None
    gl = gl if "lengths" in terms else None
    torch.autograd.backward([t for t, w in ((out, g), (ln, gl)) if w is not None],
                            [w.to(DEV) for w in (g, gl) if w is not None])
    assert pr.grad.dtype == dtype
    gd = dr.grad if dr.grad is not None else torch.zeros_like(dr)
    assert gd.dtype == dtype
    eps = torch.finfo(torch.float64 if dtype == torch.float64 else torch.float32).eps
    rp, rd = ref_grads(pd.to(DEV), fd.to(DEV), None if g is None else g.to(DEV), None if gl is None else gl.to(DEV),
                       None if ps is None else ps.to(DEV), None if qs is None else qs.to(DEV), relative, eps=eps)
    return pr.grad, gd, rp, rd


# ---------------------------------------------------------------- the feature exists
def test_interpolate_and_lengths_backward_fill_grad():
    poly = _poly()
    p = torch.tensor([[[0.0, 0.0], [3.0, 0.0], [3.0, 4.0]]], device=DEV, requires_grad=True)
    d = torch.tensor([[1.0, 5.0]], device=DEV)
    poly.interpolate(p, d).sum().backward()
    # d = 1: w1 = 1/3 on segment 0; d = 5: w1 = 1/2 on segment 1; lambda_0 = -1/3 - 1, lambda_1 = -1/2
    exp = torch.tensor([[[2.0, 2.0 / 3], [-0.5, 4.0 / 3], [0.5, 0.0]]])
    assert p.grad is not None and torch.allclose(p.grad.cpu(), exp, atol=1e-6, rtol=0), p.grad
    q = p.detach().clone().requires_grad_()
    poly.lengths(q).sum().backward()
    assert torch.equal(q.grad.cpu(), torch.tensor([[[-1.0, 0.0], [1.0, -1.0], [0.0, 1.0]]]))


# ---------------------------------------------------------------- float32 against the float64 reference
SHAPES = [   # (batch, points, queries, dims, relative): the benchmark's shapes and a few more
    (256, 24, 256, 2, True),      # config-3 lanes: 32 frames x 8 lanes
    (64, 100, 100, 2, False),
    (64, 100, 100, 3, True),
    (64, 5000, 5000, 2, True),
    (1, 5000, 5000, 2, False),
    (1, 5000, 5000, 3, True),
    (8, 37, 300, 4, True),        # run-time number of coordinates
    (5, 30, 0, 2, False),         # no queries: lengths only
]


@pytest.mark.parametrize("b,npnt,nq,dims,relative", SHAPES)
def test_f32_matches_float64_reference(b, npnt, nq, dims, relative):
    p, fr = _lattice(b, npnt, nq, dims, relative, seed=npnt + nq + dims)
    gp, gd, rp, rd = _run(p, fr, relative, torch.float32)
    _check(gp, rp, 1e-4, 1e-6, "grad points")
    _check(gd, rd, 1e-4, 1e-6, "grad distances")


def test_f32_long_polyline_takes_the_workspace_path():
    from accvlab import _amd_native as nat

    import polyline_edges_cases as pc   # the launch plan restated (imports this module: not at the top)

    b, npnt, nq = 3, 9000, 3000
    # 1024 threads, three chunks of 1024 queries: accumulators of 9000 * (2 + 2) floats per polyline and chunk, and the slab
    plan = pc.plan(b, npnt, nq, 2, torch.float32)
    assert plan.use_ws and (plan.threads, plan.chunks, plan.q_chunk) == (1024, 3, 1024)
    assert plan.ws_acc == pc.align256(npnt * 4 * 4) * b * 3 and plan.ws_slab == pc.align256(3 * b * npnt * 2 * 4)
    assert nat.lib().accv_polyline_grad_workspace_bytes(b, npnt, nq, 2, 0) == plan.ws_acc + plan.ws_slab
    p, fr = _lattice(b, npnt, nq, 2, True, seed=5, max_step=1)
    ps, qs = torch.tensor([9000, 4000, 1]), torch.tensor([3000, 2999, 17])
    gp, gd, rp, rd = _run(p, fr, True, torch.float32, ps, qs)
    _check(gp, rp, 1e-4, 1e-6, "grad points")
    _check(gd, rd, 1e-4, 1e-6, "grad distances")


@pytest.mark.parametrize("npnt,nq", [(10, 3000), (600, 5000), (3000, 4100), (2048, 9000)])
@pytest.mark.parametrize("relative", [False, True])
def test_f32_chunked_queries(npnt, nq, relative):
    """the forward's chunking shapes (test_lane_helpers.py): several workgroups per polyline, partial rows summed"""
    p, fr = _lattice(3, npnt, nq, 2, relative, seed=npnt + nq)
    ps = torch.tensor([npnt, max(1, npnt // 3), 0])
    qs = torch.tensor([nq, nq // 2 + 7, nq - 1])
    gp, gd, rp, rd = _run(p, fr, relative, torch.float32, ps, qs)
    _check(gp, rp, 1e-4, 1e-6, "grad points")
    _check(gd, rd, 1e-4, 1e-6, "grad distances")
    assert torch.equal(gp[2].cpu(), torch.zeros_like(gp[2].cpu()))                 # empty polyline
    assert torch.equal(gp[1, npnt // 3:].cpu(), torch.zeros_like(gp[1, npnt // 3:].cpu()))


def test_f32_general_position():
    """random (non-lattice) points: float32 prefix sums differ from float64 ones, so this checks at a looser bound"""
    g = torch.Generator().manual_seed(3)
    p = torch.randn((64, 100, 2), generator=g, dtype=torch.float64).cumsum(1)
    fr = torch.rand((64, 100), generator=g, dtype=torch.float64) * 1.2 - 0.1
    gp, gd, rp, rd = _run(p, fr, True, torch.float32)
    _check(gp, rp, 1e-3, 1e-4, "grad points")
    _check(gd, rd, 1e-3, 1e-4, "grad distances")


# ---------------------------------------------------------------- half precision: accumulate in f32, write once
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("b,npnt,nq,relative", [(256, 24, 256, True), (64, 100, 100, False), (64, 100, 100, True)])
def test_half_matches_reference_on_rounded_inputs(dtype, b, npnt, nq, relative):
    # each backward rounds its f32 result into the dtype once (<= eps / 2 relative); bound eps plus 1e-4 max|g| of f32
    # accumulation slack.  The samples' and the lengths' gradients are checked one by one: summed by autograd in the dtype
    # they would carry three roundings.
    p, fr = _lattice(b, npnt, nq, 2, relative, seed=npnt + nq + 1)
    eps = torch.finfo(dtype).eps
    for terms in (("samples",), ("lengths",)):
        gp, gd, rp, rd = _run(p, fr, relative, dtype, terms=terms)
        _check(gp, rp, eps, 1e-4, f"grad points ({terms[0]})")
        _check(gd, rd, eps, 1e-4, f"grad distances ({terms[0]})")


# ---------------------------------------------------------------- float64: GPU against the host backward
@pytest.mark.parametrize("relative", [False, True])
def test_f64_gpu_matches_host_backward(relative):
    poly = _poly()
    g = torch.Generator().manual_seed(8)
    p = torch.randn((16, 700, 3), generator=g, dtype=torch.float64).cumsum(1)
    fr = torch.rand((16, 900), generator=g, dtype=torch.float64) * 1.2 - 0.1
    if not relative:
        fr = fr * poly.lengths(p).unsqueeze(1)
    ps = torch.randint(0, 701, (16,), generator=g)
    qs = torch.randint(0, 901, (16,), generator=g)
    go = _gout((16, 900, 3), 2, torch.float64)
    grads = []
    for dev in ("cpu", DEV):
        pr = p.to(dev, copy=True).requires_grad_()
        dr = fr.to(dev, copy=True).requires_grad_()
        out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps.to(dev)), RaggedBatch(dr, sample_sizes=qs.to(dev)),
                                              relative=relative)
        out.tensor.backward(go.to(dev))
        grads.append((pr.grad.cpu(), dr.grad.cpu()))
    _check(grads[1][0], grads[0][0], 1e-9, 1e-12, "grad points")
    _check(grads[1][1], grads[0][1], 1e-9, 1e-12, "grad distances")
    rp, rd = ref_grads(p, fr, go, None, ps, qs, relative)
    _check(grads[1][0], rp, 1e-9, 1e-12, "grad points vs reference")


# ---------------------------------------------------------------- branch cases on the GPU (hand-derived values)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_branch_cases(dtype):
    poly = _poly()
    pts = torch.tensor([[[0.0, 0.0], [3.0, 0.0], [3.0, 4.0]]] * 6, dtype=dtype, device=DEV, requires_grad=True)
    d = torch.tensor([[-1.0], [8.0], [0.0], [7.0], [3.0], [1.5]], dtype=dtype, device=DEV, requires_grad=True)
    out = poly.interpolate(pts, d)
    out.backward(torch.tensor([[1.0, 2.0]], dtype=dtype, device=DEV).expand(6, 1, 2))
    exp_p = torch.tensor([[[1, 2], [0, 0], [0, 0]], [[0, 0], [0, 0], [1, 2]], [[1, 2], [0, 0], [0, 0]],
                          [[2, 0], [-2, 2], [1, 0]], [[2, 0], [-1, 2], [0, 0]], [[1, 1], [0, 1], [0, 0]]], dtype=dtype)
    assert torch.equal(pts.grad.cpu(), exp_p)
    assert torch.equal(d.grad.cpu(), torch.tensor([[0.0], [0.0], [1.0], [2.0], [2.0], [1.0]], dtype=dtype))
    # zero-length segment, T = 0 with relative queries, 0 / 1 / 2 points
    z = torch.tensor([[[0.0, 0.0], [2.0, 0.0], [2.0, 0.0], [2.0, 3.0]]] * 2, dtype=dtype, device=DEV, requires_grad=True)
    dz = torch.tensor([[2.0], [3.5]], dtype=dtype, device=DEV)
    poly.interpolate(z, dz).backward(torch.tensor([[1.0, 2.0]], dtype=dtype, device=DEV).expand(2, 1, 2))
    assert torch.equal(z.grad.cpu(), torch.tensor([[[0, 0], [1, 2], [0, 0], [0, 0]], [[2, 0], [-2, 0], [0.5, 2], [0.5, 0]]],
                                                  dtype=dtype))
    c = torch.ones((1, 3, 2), dtype=dtype, device=DEV, requires_grad=True)
    dc = torch.tensor([[0.5, 0.0]], dtype=dtype, device=DEV, requires_grad=True)
    poly.interpolate(c, dc, relative=True).backward(torch.tensor([[[1.0, 2.0], [3.0, 4.0]]], dtype=dtype, device=DEV))
    assert torch.equal(c.grad.cpu(), torch.tensor([[[0, 0], [4, 6], [0, 0]]], dtype=dtype))
    assert torch.equal(dc.grad.cpu(), torch.zeros((1, 2), dtype=dtype))
    e = torch.tensor([[[5.0, 1.0], [9.0, 9.0], [9.0, 9.0]], [[1.0, 1.0], [4.0, 5.0], [7.0, 7.0]],
                      [[2.0, 2.0], [2.0, 6.0], [7.0, 7.0]]], dtype=dtype, device=DEV, requires_grad=True)
    de = torch.tensor([[1.0, 2.0], [1.0, 2.0], [1.0, 5.0]], dtype=dtype, device=DEV, requires_grad=True)
    ps = torch.tensor([0, 1, 2], device=DEV)
    out = poly.interpolate_var_size_batch(RaggedBatch(e, sample_sizes=ps), RaggedBatch(de, sample_sizes=torch.tensor([2, 2, 2], device=DEV)))
    assert torch.isnan(out.tensor[0]).all()
    out.tensor.backward(torch.ones_like(out.tensor))     # NaN samples of the empty polyline: zero gradient
    exp_e = torch.zeros((3, 3, 2), dtype=dtype)
    exp_e[1, 0] = 2.0
    exp_e[2, 0] = torch.tensor([0.75, 1.0])
    exp_e[2, 1] = torch.tensor([1.25, 1.0])
    assert torch.equal(e.grad.cpu(), exp_e)
    assert torch.equal(de.grad.cpu(), torch.tensor([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]], dtype=dtype))
    e2 = e.detach().clone().requires_grad_()
    poly.lengths_var_size_batch(RaggedBatch(e2, sample_sizes=ps)).backward(torch.ones(3, dtype=dtype, device=DEV))
    exp_l = torch.zeros((3, 3, 2), dtype=dtype)
    exp_l[2, 0, 1], exp_l[2, 1, 1] = -1.0, 1.0
    assert torch.equal(e2.grad.cpu(), exp_l)


# ---------------------------------------------------------------- padding, laziness, forward, synchronisation
def test_padded_grad_out_is_ignored_and_needs_input_grad():
    poly = _poly()
    p, fr = _lattice(3, 12, 9, 2, True, seed=4)
    p, fr = p.float().to(DEV), fr.float().to(DEV)
    ps = torch.tensor([12, 5, 8], device=DEV)
    qs = torch.tensor([9, 4, 1], device=DEV)

    def run(fill, want_p=True, want_d=True):
        pr = p.clone().requires_grad_(want_p)
        dr = fr.clone().requires_grad_(want_d)
        out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps), RaggedBatch(dr, sample_sizes=qs),
                                              relative=True)
        live = (torch.arange(9, device=DEV).unsqueeze(0) < qs.unsqueeze(1)).unsqueeze(-1)
        g = torch.where(live, torch.ones_like(out.tensor), torch.full_like(out.tensor, fill))
        out.tensor.backward(g)
        return pr.grad, dr.grad

    gp0, gd0 = run(0.0)
    for fill in (float("nan"), 1e30):
        gp1, gd1 = run(fill)
        assert torch.equal(gp0, gp1) and torch.equal(gd0, gd1)
    assert torch.equal(gp0[1, 5:].cpu(), torch.zeros((7, 2)))
    assert torch.equal(gd0[1, 4:].cpu(), torch.zeros(5))
    gp2, gd2 = run(0.0, want_d=False)
    assert gd2 is None and torch.equal(gp2, gp0)
    gp3, gd3 = run(0.0, want_p=False)
    assert gp3 is None and torch.equal(gd3, gd0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_forward_is_bitwise_the_same_with_and_without_grad(dtype):
    poly = _poly()
    g = torch.Generator().manual_seed(6)
    p = torch.randn((32, 200, 2), generator=g, dtype=torch.float64).cumsum(1).to(dtype).to(DEV)
    fr = (torch.rand((32, 3000), generator=g, dtype=torch.float64) * 1.2 - 0.1).to(dtype).to(DEV)
    a = poly.interpolate(p, fr, relative=True)
    b = poly.interpolate(p.clone().requires_grad_(), fr, relative=True)
    c = poly.interpolate(p, fr.clone().requires_grad_(), relative=True)
    assert b.requires_grad and c.requires_grad
    assert torch.equal(a, b.detach()) and torch.equal(a, c.detach())
    assert torch.equal(poly.lengths(p), poly.lengths(p.clone().requires_grad_()).detach())


def test_no_host_synchronisation():
    poly = _poly()
    p, fr = _lattice(64, 100, 300, 2, True, seed=2)
    p, fr = p.float().to(DEV), fr.float().to(DEV)
    ps = torch.full((64,), 77, device=DEV)
    qs = torch.full((64,), 250, device=DEV)
    pr = p.clone().requires_grad_()
    dr = fr.clone().requires_grad_()
    out = poly.interpolate_var_size_batch(RaggedBatch(pr, sample_sizes=ps), RaggedBatch(dr, sample_sizes=qs),
                                          relative=True)   # (its size check reads back, as without grad)
    ln = poly.lengths_var_size_batch(RaggedBatch(pr, sample_sizes=ps))
    go = torch.ones_like(out.tensor)
    gl = torch.ones_like(ln)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.autograd.backward([out.tensor, ln], [go, gl])
        q = p.clone().requires_grad_()
        e = fr.clone().requires_grad_()
        loss = poly.interpolate(q, e, relative=True).sum() + poly.lengths(q).sum()
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert pr.grad is not None and q.grad is not None and e.grad is not None
