"""batched_polyline_matching_cost, batched_polyline_hungarian_match and matched_polyline_loss on the device (the kernels of
csrc/polyline_match.hip) against the float64 definition of tests/polyline_match_cases.py and against the host path:
values, gradients, the edges of the kernels' work partition, strided input, padding, guard bands, reproducibility, graph
capture, no synchronisation, special values, the end-to-end criterion."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from polyline_match_cases import (DTYPES, PAIRS, SIZES, assert_close_nan_aware, bits, check_cost, check_grad, check_losses,  # noqa: E402
                                  compare, cost_definition, definition, make_case, name, ragged, run, to_host, tolerance)

from accvlab.batching_helpers import RaggedBatch, batched_linear_sum_assignment  # noqa: E402
from accvlab.lane_helpers.polyline import (batched_polyline_hungarian_match, batched_polyline_matching_cost,  # noqa: E402
                                           matched_polyline_loss)

pytestmark = pytest.mark.gpu

DEV = "cuda"
mpl = matched_polyline_loss
cost_op = batched_polyline_matching_cost


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "polyline_match.hip")).read()
WAVE = int(_constant(_SRC, "kWave"))                       # ground-truth lines per LDS chunk, one per lane
THREADS = int(_constant(_SRC, "kThreads"))
QUERIES_PER_WAVE = int(_constant(_SRC, "kQueriesPerWave"))
TILE = THREADS // WAVE * QUERIES_PER_WAVE                  # kQueryTile: queries per workgroup of the cost kernel
CHUNK = int(_constant(_SRC, "kLossQueries"))               # queries per workgroup of the loss kernels
assert (WAVE, TILE, CHUNK) == (64, 16, 64)


def both(inp, what="", host=True, **kw):
    """loss on the device against the definition and (host=True) the host path on the same inputs"""
    out, grad = compare(mpl, inp, what + " device", **kw)
    assert out.is_cuda and grad.is_cuda
    if host:
        hkw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        compare(mpl, to_host(inp), what + " host", **hkw)
    return out, grad


# ---------------------------------------------------------------------------------------------------- definition match
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("P,D", [(2, 2), (5, 3), (20, 2)])
@pytest.mark.parametrize("closed", ["open", "closed", "mixed"])
@pytest.mark.parametrize("reversible", [True, False])
def test_device_and_host_match_definition(reversible, closed, P, D, dtype):
    inp = make_case(5, 7, P, D, SIZES, PAIRS, dtype, seed=P + D, closed=closed, reversible=reversible, device=DEV)
    g = torch.Generator().manual_seed(1)
    both(inp, f"{name(dtype)}/P{P}/D{D}/{closed}/rev{reversible}", reversible=reversible,
         grad_out=torch.rand(2, 5, generator=g) + 0.5)
    kw = dict(reversible=reversible, pts_weight=1.5, filler=-7.25)
    cost = cost_op(inp[0], inp[1], gt_closed=inp[4], **kw)
    check_cost(cost, inp, "cost device", **kw)
    h = to_host(inp)
    check_cost(cost_op(h[0], h[1], gt_closed=h[4], **kw), h, "cost host", **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms_dir_off_and_index_dtypes(dtype):
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, dtype, seed=7, index_dtype=torch.int32, closed_dtype=torch.int32, device=DEV)
    for factor in (None, 1.0, 3.7, torch.tensor(2.5, device=DEV)):
        both(inp, f"avg_factor {factor}", host=False, avg_factor=factor)
    out, _ = both(inp, "dir off", host=False, dir_loss=False)
    assert bool((out[1] == 0).all())
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4]), inp, "int32 closed")


@pytest.mark.parametrize("kind", ["one_minus_prob", "neg_prob", "focal"])
def test_cost_with_class_term(kind):
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, torch.float32, seed=3, device=DEV)
    g = torch.Generator().manual_seed(2)
    raw = torch.randn(5, 7, 4, generator=g, dtype=torch.float64) * 3
    scores = (raw if kind == "focal" else raw.softmax(-1)).float().to(DEV)
    labels = ragged(torch.randint(0, 4, (5, 5), generator=g).to(DEV), SIZES)
    labels.tensor[2, 1] = 9
    kw = dict(class_cost=kind, class_weight=2.0, pts_weight=5.0)
    check_cost(cost_op(inp[0], inp[1], scores, labels, gt_closed=inp[4], **kw), inp, kind, scores=scores, labels=labels, **kw)
    only_cls = cost_op(None, None, scores, labels, pts_weight=0.0, class_cost=kind, class_weight=2.0)
    want, _, mag = cost_definition(None, None, scores, labels, pts_weight=0.0, class_cost=kind, class_weight=2.0)
    assert_close_nan_aware(only_cls.tensor, want, tolerance(torch.float32), "class only", scale=mag)


# ------------------------------------------------------------------------------------------------------ partition edges
@pytest.mark.parametrize("Q", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_cost_queries_across_query_tiles(Q):
    inp = make_case(2, Q, 5, 2, [3, 6], [0, 0], torch.float32, seed=Q, device=DEV)
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4], filler=3.0), inp, f"Q {Q}", filler=3.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
@pytest.mark.parametrize("G", [WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 5])
def test_cost_lines_across_the_wave_width_and_lds_chunks(G, dtype):
    """G past WAVE takes a second LDS chunk; the frame with fewer lines ends inside a chunk"""
    inp = make_case(2, TILE + 2, 3, 2, [G, G // 2], [0, 0], dtype, seed=G, device=DEV)
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4], filler=-1.0), inp, f"G {G}", filler=-1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
@pytest.mark.parametrize("P", [2, 64, 128])
def test_long_closed_lines(P, dtype):
    """closed lines: V = 2 P orders, 256 at the limit of P, where the LDS budget also shortens the chunk (D = 3, float64:
    five lines per chunk, so G = 7 takes two)"""
    inp = make_case(2, 5, P, 3, [7, 2], [3, 2], dtype, seed=P, closed="closed", device=DEV)
    both(inp, f"P {P}", host=False)
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4]), inp, f"cost P {P}")


@pytest.mark.parametrize("Q", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_loss_queries_across_workgroup_chunks(Q):
    """pairs on both sides of every chunk boundary: the first and the last query of the frame are matched"""
    n = [6, 0, 5]
    inp = make_case(3, Q, 5, 2, [6, 5, 5], n, torch.float32, seed=Q, device=DEV)
    # move the matched predictions to the edge queries: swap rows so that the case stays a small perturbation of its line
    edge = [0, Q - 1, min(CHUNK - 1, Q - 2), min(CHUNK, Q - 3), 5, 7]
    for b, k in enumerate(n):
        for j in range(k):
            old, new = int(inp[2].tensor[b, j]), edge[j]
            if old != new and new not in inp[2].tensor[b, :k].tolist():
                inp[0][b, [old, new]] = inp[0][b, [new, old]]
                inp[2].tensor[b, j] = new
    both(inp, f"Q {Q}")


@pytest.mark.parametrize("K", [63, 64, 65, 130])
def test_slot_counts_across_waves(K):
    inp = make_case(2, 300, 3, 2, [K, K], [K, K - 1], torch.float32, seed=K, closed="open", device=DEV)
    both(inp, f"K {K}", host=False)
    # a query named in the first and in the last slot: the first one is its pair, whichever wave reads it
    inp[2].tensor[0, K - 1] = inp[2].tensor[0, 0]
    both(inp, f"K {K} duplicate", host=False)


# ------------------------------------------------------------------------------------------------- strides and padding
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_strided_lines_equal_their_contiguous_copy(dtype):
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, dtype, seed=9, width=13, device=DEV)
    assert not inp[0].is_contiguous()
    out, grad = both(inp, "strided", host=False)
    out_c, grad_c = run(mpl, inp[0].contiguous(), *inp[1:4], gt_closed=inp[4])
    assert torch.equal(bits(out), bits(out_c)) and torch.equal(bits(grad), bits(grad_c))
    cost, cost_c = cost_op(inp[0], inp[1], gt_closed=inp[4]), cost_op(inp[0].contiguous(), inp[1], gt_closed=inp[4])
    assert torch.equal(bits(cost.tensor), bits(cost_c.tensor))
    # B = 1 / Q = 1 with arbitrary strides in the dimensions of extent 1
    one = make_case(1, 1, 5, 2, [2], [1], dtype, seed=10, device=DEV)
    odd = torch.as_strided(one[0].clone(), (1, 1, 5, 2), (3, 7, 2, 1))
    out_o, grad_o = run(mpl, odd, *one[1:4], gt_closed=one[4])
    out_c, grad_c = run(mpl, one[0], *one[1:4], gt_closed=one[4])
    assert torch.equal(bits(out_o), bits(out_c)) and torch.equal(bits(grad_o), bits(grad_c))
    assert torch.equal(bits(cost_op(odd, one[1]).tensor), bits(cost_op(one[0], one[1]).tensor))


@pytest.mark.parametrize("filler", [0.0, -0.0, float("inf"), 1e30])
def test_padded_columns_are_bitwise_the_filler(filler):
    inp = make_case(5, 2 * TILE + 1, 5, 2, SIZES, PAIRS, torch.float32, seed=2, device=DEV)
    check_cost(cost_op(inp[0], inp[1], gt_closed=inp[4], filler=filler), inp, f"filler {filler}", filler=filler)


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", [(3, 7, 5, 2), (2, CHUNK + 3, 3, 3)])
def test_guard_bands_around_cost_outputs_gradient_and_workspace(shape, dtype):
    from accvlab import _amd_native as nat

    B, Q, P, D = shape
    sizes = [5] * B
    lines, gt, pind, gind, closed = make_case(B, Q, P, D, sizes, sizes, dtype, seed=4, closed_dtype=torch.uint8, device=DEV)
    lib = nat.ctypes_lib()
    out_dtype = torch.float64 if dtype == torch.float64 else torch.float32
    osize = 8 if dtype == torch.float64 else 4
    pad = 512

    def banded(nbytes, as_dtype):
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        inner = buf[pad: pad + nbytes]
        inner.view(as_dtype).fill_(float("nan"))
        return buf, inner

    G, K = gt.tensor.shape[1], pind.tensor.shape[1]
    ws_bytes = lib.accv_matched_polyline_loss_workspace_bytes(B, Q)
    cost_buf, cost_in = banded(B * Q * G * osize, out_dtype)
    out_buf, out_in = banded(2 * B * osize, out_dtype)
    den_buf, den_in = banded(8, torch.float64)
    ws_buf, ws_in = banded(ws_bytes, torch.float64)
    grad_buf, grad_in = banded(B * Q * P * D * lines.element_size(), dtype)
    p = nat.PolylineMatchParams()
    p.pts_weight, p.dir_eps, p.avg_mode, p.dir_loss = 1.0, 1e-12, nat.FL_AVG_NUM_POS, 1
    p.pred_stride_b, p.pred_stride_q, p.gt_closed = Q * P * D, P * D, closed.tensor.data_ptr()
    counts = pind.sample_sizes.to(torch.int64)
    gcounts = gt.sample_sizes.to(torch.int64)
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}[dtype]
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    assert lib.accv_polyline_matching_cost(lines.data_ptr(), gt.tensor.data_ptr(), None, None, gcounts.data_ptr(), dt,
                                           nat.PM_REVERSIBLE, B, Q, G, P, D, 0, 0, 0, ctypes.addressof(p), cost_in.data_ptr(),
                                           stream) == 0, lib.accv_last_error()
    common = (lines.data_ptr(), gt.tensor.data_ptr(), pind.tensor.data_ptr(), gind.tensor.data_ptr(), counts.data_ptr())
    shape_args = (dt, nat.PM_IDX_I64 | nat.PM_REVERSIBLE, B, Q, G, P, D, K, ctypes.addressof(p))
    assert lib.accv_matched_polyline_loss(*common, *shape_args, out_in.data_ptr(), den_in.data_ptr(), ws_in.data_ptr(),
                                          ws_bytes, stream) == 0, lib.accv_last_error()
    go = torch.ones(2, B, dtype=out_dtype, device=DEV)
    assert lib.accv_matched_polyline_loss_bwd(*common, go[0].data_ptr(), go[1].data_ptr(), den_in.data_ptr(), *shape_args,
                                              grad_in.data_ptr(), stream) == 0, lib.accv_last_error()
    torch.cuda.synchronize()
    for buf, inner in ((cost_buf, cost_in), (out_buf, out_in), (den_buf, den_in), (ws_buf, ws_in), (grad_buf, grad_in)):
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + inner.numel():] == 0xA5).all())
    grad = grad_in.view(dtype).view(B, Q, P, D)
    assert bool(torch.isfinite(grad).all()), "the NaN-filled gradient buffer was not written completely"
    out = out_in.view(out_dtype).view(2, B)
    cost = cost_in.view(out_dtype).view(B, Q, G)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cost).all()), "outputs were not written completely"
    want, gwant, factor, _ = definition(lines, gt, pind, gind, gt_closed=closed)
    check_losses(out, want, dtype)
    check_grad(grad.clone(), gwant, dtype)
    assert float(den_in.view(torch.float64)) == factor
    check_cost(RaggedBatch(cost.clone(), sample_sizes=gt.sample_sizes, non_uniform_dim=2), (lines, gt, None, None, closed))


# -------------------------------------------------------------------------- reproducibility, no synchronisation, graphs
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_bitwise_reproducible_and_completely_written(dtype):
    sizes = [0, 12, 7, 12, 3, 9]
    inp = make_case(6, 150, 20, 2, sizes, sizes, dtype, seed=2, device=DEV)
    first = run(mpl, *inp[:4], gt_closed=inp[4])
    cost = cost_op(inp[0], inp[1], gt_closed=inp[4]).tensor
    for _ in range(3):
        poison = torch.full(inp[0].shape, float("nan"), dtype=dtype, device=DEV)
        del poison
        again = run(mpl, *inp[:4], gt_closed=inp[4])
        assert torch.equal(bits(again[0]), bits(first[0])) and torch.equal(bits(again[1]), bits(first[1]))
        assert torch.equal(bits(cost_op(inp[0], inp[1], gt_closed=inp[4]).tensor), bits(cost))
    assert bool(torch.isfinite(first[1]).all())


def test_no_synchronisation():
    sizes = [0, 12, 7, 12, 3, 9]
    inp = make_case(6, 150, 20, 2, sizes, sizes, torch.float32, seed=3, device=DEV)
    avg = torch.tensor(17.0, device=DEV)
    x = inp[0].detach().requires_grad_(True)
    go = torch.ones(6, device=DEV)
    torch.autograd.grad(mpl(x, *inp[1:4], gt_closed=inp[4]), x, (go, go))    # warm-up: library load, allocator
    cost_op(inp[0], inp[1], gt_closed=inp[4])
    batched_polyline_hungarian_match(inp[0], inp[1], gt_closed=inp[4], check=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in ({}, {"avg_factor": avg}, {"avg_factor": 3.0, "dir_loss": False, "reversible": False}):
            grad, = torch.autograd.grad(mpl(x, *inp[1:4], gt_closed=inp[4], **kw), x, (go, go))
        cost = cost_op(inp[0], inp[1], gt_closed=inp[4])
        pind, gind, status = batched_polyline_hungarian_match(inp[0], inp[1], gt_closed=inp[4], check=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(cost.tensor).all()) and bool((status == 0).all())


def test_graph_capture_and_replay_with_changed_lines_and_matches():
    sizes = [0, 12, 7, 12, 3, 9]
    a = make_case(6, 150, 20, 2, sizes, sizes, torch.float32, seed=5, device=DEV)
    b = make_case(6, 150, 20, 2, sizes[::-1], sizes[::-1], torch.float32, seed=6, device=DEV)
    assert a[2].tensor.shape == b[2].tensor.shape and a[1].tensor.shape == b[1].tensor.shape
    x = a[0].clone().requires_grad_(True)
    gt, pind, gind, closed = (ragged(rb.tensor.clone(), [0] * 6) for rb in a[1:5])
    for rb, src in zip((gt, pind, gind, closed), a[1:5]):
        rb.sample_sizes.copy_(src.sample_sizes)
    go = torch.ones(6, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            pts, dr = mpl(x, gt, pind, gind, gt_closed=closed)
            grad, = torch.autograd.grad((pts, dr), x, (go, go))
            cost = cost_op(x.detach(), gt, gt_closed=closed)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pts, dr = mpl(x, gt, pind, gind, gt_closed=closed)
        grad, = torch.autograd.grad((pts, dr), x, (go, go))
        cost = cost_op(x.detach(), gt, gt_closed=closed)
    for case in (b, a):
        with torch.no_grad():
            x.copy_(case[0])
        for rb, src in zip((gt, pind, gind, closed), case[1:5]):
            rb.tensor.copy_(src.tensor)
            rb.sample_sizes.copy_(src.sample_sizes)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(mpl, *case[:4], gt_closed=case[4])
        out = torch.stack([pts, dr])
        assert torch.equal(bits(out), bits(eager[0])) and torch.equal(bits(grad), bits(eager[1]))
        assert torch.equal(bits(cost.tensor), bits(cost_op(case[0], case[1], gt_closed=case[4]).tensor))
        want, gwant, _, _ = definition(*case[:4], gt_closed=case[4])
        check_losses(out, want, torch.float32, "replay")
        check_grad(grad.clone(), gwant, torch.float32, "replay")


# -------------------------------------------------------------------------------------------------------- special values
def test_special_values_device_and_host_agree():
    inp = make_case(5, 7, 5, 2, SIZES, PAIRS, torch.float32, seed=17, device=DEV)
    lines, gt, pind, gind, closed = inp
    clean = run(mpl, lines, gt, pind, gind, gt_closed=closed)
    matched = torch.zeros(5, 7, dtype=torch.bool, device=DEV)
    for b, n in enumerate(PAIRS):
        matched[b, pind.tensor[b, :n]] = True
    # NaN in unmatched rows, and slots past n_b that point at them: the loss never reads them
    junk = lines.clone()
    junk[~matched] = float("nan")
    junk_p = pind.tensor.clone()
    for b, n in enumerate(PAIRS):
        junk_p[b, n:] = (~matched[b]).nonzero().flatten()[0]
    out, grad = run(mpl, junk, gt, ragged(junk_p, PAIRS), gind, gt_closed=closed)
    assert torch.equal(bits(out), bits(clean[0])) and torch.equal(bits(grad), bits(clean[1]))
    assert bool((bits(grad)[~matched] == 0).all())   # exactly +0
    # a NaN coordinate in one prediction: only that query's costs; matched: its frame's losses and its gradient
    q = int(pind.tensor[4, 1])
    bad = lines.clone()
    bad[4, q, 2, 1] = float("nan")
    cost = cost_op(bad, gt, gt_closed=closed).tensor
    want = torch.zeros_like(cost, dtype=torch.bool)
    want[4, q, :SIZES[4]] = True
    assert torch.equal(torch.isnan(cost), want)
    out, grad = run(mpl, bad, gt, pind, gind, gt_closed=closed)
    assert bool(torch.isnan(out[:, 4]).all()) and bool(torch.isfinite(out[:, :4]).all())
    nan = torch.isnan(grad)
    assert bool(nan[4, q, 2, 1]) and int(nan.sum()) == int(nan[4, q].sum())
    h = to_host((bad, gt, pind, gind, closed))
    hout, hgrad = run(mpl, *h[:4], gt_closed=h[4])
    assert torch.equal(torch.isnan(out).cpu(), torch.isnan(hout)) and torch.equal(nan.cpu(), torch.isnan(hgrad))
    # a zero-length predicted segment: cosine 0, the finite gradient of the formula
    flat = lines.clone()
    flat[4, q, 3] = flat[4, q, 2]
    case = (flat, gt, pind, gind, closed)
    want, gwant, _, _ = definition(*case[:4], gt_closed=closed)
    out, grad = run(mpl, *case[:4], gt_closed=closed)
    check_losses(out, want, torch.float32, "zero-length segment")
    check_grad(grad, gwant, torch.float32, "zero-length segment")
    assert bool(torch.isfinite(grad).all())


def test_empty_extents():
    for B, Q, n in ((0, 6, 0), (3, 0, 0), (3, 6, 0)):
        inp = make_case(B, Q, 5, 2, [2] * B, [n] * B, torch.float32, seed=1, device=DEV)
        out, grad = run(mpl, *inp[:4])
        assert out.shape == (2, B) and bool((out == 0).all()) and grad.shape == (B, Q, 5, 2) and bool((bits(grad) == 0).all())
        assert tuple(cost_op(inp[0], inp[1]).tensor.shape) == (B, Q, 2 if B else 0)


# ----------------------------------------------------------------------------------------------------------- end to end
def test_hungarian_match_total_cost_equals_the_host_solver_on_the_definition():
    inp = make_case(4, 40, 5, 2, [4, 0, 6, 9], [0, 0, 0, 0], torch.float32, seed=6, device=DEV)
    pind, gind = batched_polyline_hungarian_match(inp[0], inp[1], gt_closed=inp[4])
    want, _, _ = cost_definition(inp[0], inp[1], gt_closed=inp[4])
    rp, rg = batched_linear_sum_assignment(RaggedBatch(want, sample_sizes=inp[1].sample_sizes.cpu(), non_uniform_dim=2))
    assert torch.equal(pind.sample_sizes.cpu(), rp.sample_sizes)
    for b in range(4):
        n = int(rp.sample_sizes[b])
        got = want[b, pind.tensor[b, :n].cpu(), gind.tensor[b, :n].cpu()].sum()
        ref = want[b, rp.tensor[b, :n], rg.tensor[b, :n]].sum()
        assert abs(float(got - ref)) <= 1e-5 * (1 + abs(float(ref)))


def test_example_criterion_equals_its_torch_composition():
    """in float64, where the composition's own rounding (its 1 - cos cancels in float32) does not blur the comparison"""
    import lane_set_prediction as lsp

    data = lsp.make_inputs(4, 30, 3, 8, 10, DEV, seed=3, dtype=torch.float64)
    matching = lsp.match(*data)
    assert int(matching[0].sample_sizes.sum()) == int(data[2].sample_sizes.sum()) > 0
    la, xa = data[0].clone().requires_grad_(True), data[1].clone().requires_grad_(True)
    lb, xb = data[0].clone().requires_grad_(True), data[1].clone().requires_grad_(True)
    fused = lsp.criterion_fused(la, xa, *data[2:], matching=matching)
    composed = lsp.criterion_composed(lb, xb, *data[2:], matching=matching)
    torch.testing.assert_close(fused, composed, rtol=1e-10, atol=0)
    fused.sum().backward()
    composed.sum().backward()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-9, atol=1e-12 * float(xb.grad.abs().max()))
    torch.testing.assert_close(la.grad, lb.grad, rtol=1e-9, atol=1e-12 * float(lb.grad.abs().max()))
