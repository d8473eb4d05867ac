"""Batched linear sum assignment on the GPU (the HIP kernel of csrc/linear_assignment.hip) against the host solver: the
same algorithm, tie rule and f64 operation sequence, so every output must be bitwise equal — on tie-rich matrices too —
and therefore equal to scipy wherever tests/test_linear_assignment_cpu.py says the host solver is."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
DEV = torch.device("cuda", 0)
SHAPES = [(1, 1), (5, 3), (3, 5), (900, 100), (100, 300), (300, 300)]


def lsa(cost, **kw):
    from accvlab.batching_helpers import batched_linear_sum_assignment

    return batched_linear_sum_assignment(cost, **kw)


def ragged(tensor, sizes, dim):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=torch.as_tensor(sizes, dtype=torch.int64, device=tensor.device),
                       non_uniform_dim=dim)


def cpu_form(cost):
    from accvlab.batching_helpers import RaggedBatch

    if isinstance(cost, RaggedBatch):
        return ragged(cost.tensor.cpu(), cost.sample_sizes.cpu(), cost.non_uniform_dim)
    return cost.cpu()


def assert_same_as_host(cost, **kw):
    """GPU result == host result, bit for bit (indices, sizes, status); returns the GPU result"""
    got = lsa(cost, check=False, **kw)
    want = lsa(cpu_form(cost), check=False, **kw)
    for g, w in zip(got, want):
        gt = g.tensor if hasattr(g, "tensor") else g
        wt = w.tensor if hasattr(w, "tensor") else w
        assert gt.device.type == "cuda"
        assert torch.equal(gt.cpu(), wt), (gt.cpu(), wt)
    if hasattr(got[0], "sample_sizes"):
        assert torch.equal(got[0].sample_sizes.cpu(), want[0].sample_sizes)
        assert torch.equal(got[1].sample_sizes.cpu(), want[0].sample_sizes)
    return got


@pytest.mark.parametrize("threads", [None, 64, 1024])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_random_bitwise_host_and_scipy(shape, dtype, threads):
    g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
    cost = torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)
    r, c, st = assert_same_as_host(cost.to(DEV), _threads=threads)
    er, ec = linear_sum_assignment(cost.double().numpy())
    np.testing.assert_array_equal(r.cpu().numpy(), er)
    np.testing.assert_array_equal(c.cpu().numpy(), ec)
    assert int(st) == 0
    assert_same_as_host(cost.to(DEV), maximize=True, _threads=threads)


@pytest.mark.parametrize("shape", [(6, 6), (9, 4), (4, 9), (60, 20), (20, 60), (100, 100), (900, 100)])
@pytest.mark.parametrize("threads", [None, 64, 1024])
def test_tie_rich_bitwise(shape, threads):
    for seed in range(3):
        g = torch.Generator().manual_seed(seed)
        cost = torch.randint(0, 4, (4,) + shape, generator=g).float()
        r, c, st = assert_same_as_host(cost.to(DEV), _threads=threads)
        assert_same_as_host(cost.to(DEV), maximize=True, _threads=threads)
        for b in range(4):
            er, ec = linear_sum_assignment(cost[b].numpy())
            rr, cc = r.tensor[b].cpu(), c.tensor[b].cpu()
            assert float(cost[b][rr, cc].double().sum()) == float(cost[b].numpy()[er, ec].sum())


def test_special_entries_and_status():
    inf = float("inf")
    g = torch.Generator().manual_seed(11)
    cost = torch.rand(5, 8, 6, generator=g, dtype=torch.float64)
    cost[0, :, 1] = inf               # a forbidden column, still feasible (8 rows > 6 columns)
    cost[0, 3, 1] = 0.5
    cost[1, 2, 2] = float("nan")
    cost[2] = inf
    cost[2, 0, 0] = 1.0                # infeasible
    cost[3, 4, 4] = -inf               # invalid when minimising
    r, c, st = assert_same_as_host(cost.to(DEV))
    assert st.tolist() == [0, 2, 1, 2, 0]
    assert r.sample_sizes.tolist() == [6, 0, 0, 0, 6]
    for b in (0, 4):
        er, ec = linear_sum_assignment(cost[b].numpy())
        np.testing.assert_array_equal(r.tensor[b].cpu().numpy(), er)
        np.testing.assert_array_equal(c.tensor[b].cpu().numpy(), ec)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        lsa(cost.to(DEV))
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        lsa(cost[2:3].to(DEV))
    # maximize: -inf forbids, +inf is invalid
    m = -cost[4:5].clone()
    m[0, 0, 0] = -inf
    assert_same_as_host(m.to(DEV), maximize=True)
    m[0, 1, 1] = inf
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        lsa(m.to(DEV), maximize=True)


def test_input_forms_and_views():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(6, 40, 25, generator=g).to(DEV)
    assert_same_as_host(ragged(x, [25, 0, 4, 17, 1, 25], 2))
    assert_same_as_host(ragged(x, [40, 0, 3, 25, 26, 7], 1))
    assert_same_as_host(x)
    assert_same_as_host(x.transpose(1, 2))
    assert_same_as_host(x[:, ::2, 3:])
    assert_same_as_host(x[2])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 8, 64])
def test_half_precision_and_batch_sizes(dtype, B):
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 300, 50, generator=g).to(dtype).to(DEV)
    sizes = torch.randint(0, 51, (B,), generator=g)
    assert_same_as_host(ragged(x, sizes, 2))
    r, c = lsa(ragged(x, sizes, 2))
    r64, c64 = lsa(ragged(x.double(), sizes, 2))
    assert torch.equal(r.tensor, r64.tensor) and torch.equal(c.tensor, c64.tensor)


def test_limit_frame_and_more_targets_than_queries():
    g = torch.Generator().manual_seed(2)
    big = torch.rand(1, 4096, 1024, generator=g)
    r, c, st = assert_same_as_host(big.to(DEV))
    assert int(st[0]) == 0 and r.sample_sizes.tolist() == [1024]
    wide = torch.rand(3, 100, 300, generator=g)
    assert_same_as_host(ragged(wide.to(DEV), [300, 120, 99], 2))
    with pytest.raises(ValueError, match="exceed the limit"):
        lsa(torch.zeros(1, 4097, 2, device=DEV))


def test_example_matcher_and_losses():
    import matched_loss as ml

    import accvlab.batching_helpers as bh

    inp = ml.make_inputs(8, 900, 10, 100, DEV, seed=0)
    gt_boxes = bh.combine_data(inp[0])
    gt_labels = bh.combine_data(inp[1], other_with_same_sample_sizes=gt_boxes)
    want = ml.match_batched(gt_boxes, gt_labels, inp[3], inp[4])
    got = ml.match_batched_on_device(gt_boxes, gt_labels, inp[3], inp[4])
    for w, g in zip(want, got):
        assert g.tensor.device.type == "cuda"
        assert torch.equal(w.sample_sizes, g.sample_sizes)
        m = w.mask
        assert torch.equal(w.tensor[m], g.tensor[:, :w.tensor.shape[1]][m])

    for fused in (False, True):
        a = [t.clone().requires_grad_(True) for t in inp[3:]]
        b = [t.clone().requires_grad_(True) for t in inp[3:]]
        la = ml.run_batched(*inp[:3], *a, fused=fused)
        lb = ml.run_batched_on_device(*inp[:3], *b, fused=fused)
        torch.testing.assert_close(lb, la, atol=1e-5, rtol=1e-5)
        la.sum().backward()
        lb.sum().backward()
        for ta, tb in zip(a, b):
            torch.testing.assert_close(tb.grad, ta.grad, atol=1e-5, rtol=1e-5)


def test_side_stream_graph_and_determinism():
    g = torch.Generator().manual_seed(9)
    x = torch.rand(8, 300, 60, generator=g).to(DEV)
    sizes = torch.randint(0, 61, (8,), generator=g).to(DEV)
    eager = lsa(ragged(x, sizes, 2), check=False)
    again = lsa(ragged(x, sizes, 2), check=False)
    for e, a in zip(eager[:2], again[:2]):
        assert torch.equal(e.tensor, a.tensor)
    assert torch.equal(eager[2], again[2])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = x * 1.0                      # produced on the side stream, consumed there
        on_side = lsa(ragged(y, sizes, 2), check=False)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(on_side[0].tensor, eager[0].tensor) and torch.equal(on_side[1].tensor, eager[1].tensor)

    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lsa(ragged(static, sizes, 2), check=False)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = lsa(ragged(static, sizes, 2), check=False)
    for seed in (1, 2):
        new = torch.rand(8, 300, 60, generator=torch.Generator().manual_seed(seed)).to(DEV)
        static.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        ref = lsa(ragged(new, sizes, 2), check=False)
        assert torch.equal(captured[0].tensor, ref[0].tensor)
        assert torch.equal(captured[1].tensor, ref[1].tensor)
        assert torch.equal(captured[2], ref[2])


def test_outputs_stay_in_their_extent():
    """the launch writes row_ind / col_ind [B, W], sizes [B] and status [B] exactly: guard bands around each stay intact"""
    from accvlab import _amd_native as nat

    lib = nat.lib()
    g = torch.Generator().manual_seed(4)
    B, R, C = 5, 70, 30
    x = torch.rand(B, R, C, generator=g).to(DEV)
    counts = torch.tensor([30, 0, 12, 29, 30], dtype=torch.int64, device=DEV)
    guard, sentinel = 4096, -7
    W = min(R, C)

    def banded(n, dtype):
        buf = torch.full((guard + n + guard,), sentinel, dtype=dtype, device=DEV)
        return buf, buf[guard:guard + n]

    (rb, row), (cb, col), (sb, sizes), (tb, status) = (banded(B * W, torch.int64), banded(B * W, torch.int64),
                                                       banded(B, torch.int64), banded(B, torch.int32))
    need = lib.accv_linear_assignment_workspace_bytes(B, R, C, 0)
    wb = torch.full((guard + need + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    ws = wb[guard:guard + need]
    nat.check(lib.accv_linear_assignment(x.data_ptr(), 0, B, R, C, *x.stride(), 0, counts.data_ptr(), 0,
                                         row.data_ptr(), col.data_ptr(), sizes.data_ptr(), status.data_ptr(),
                                         ws.data_ptr(), need, nat.stream_ptr(DEV)), "linear_assignment")
    torch.cuda.synchronize()
    for buf in (rb, cb, sb, tb):
        assert (buf[:guard] == sentinel).all() and (buf[-guard:] == sentinel).all()
    assert (wb[:guard] == 0x5A).all() and (wb[-guard:] == 0x5A).all()
    want = lsa(ragged(x.cpu(), counts.cpu(), 2), check=False)
    assert torch.equal(row.view(B, W).cpu(), want[0].tensor)
    assert torch.equal(col.view(B, W).cpu(), want[1].tensor)
    assert torch.equal(sizes.cpu(), want[0].sample_sizes) and torch.equal(status.cpu(), want[2])
