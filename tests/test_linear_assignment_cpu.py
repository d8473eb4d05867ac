"""Batched linear sum assignment (accvlab.batching_helpers.batched_linear_sum_assignment) on CPU tensors — the host solver,
the same algorithm and tie rule as the HIP kernel — against scipy.optimize.linear_sum_assignment, plus the C-ABI's
argument validation.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

SHAPES = [(1, 1), (5, 3), (3, 5), (900, 100), (100, 300), (300, 300)]


def lsa(cost, **kw):
    from accvlab.batching_helpers import batched_linear_sum_assignment

    return batched_linear_sum_assignment(cost, **kw)


def rb(tensor, sizes, dim):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=torch.as_tensor(sizes, dtype=torch.int64), non_uniform_dim=dim)


def frames(row_rb, col_rb):
    sizes = row_rb.sample_sizes.tolist()
    assert torch.equal(row_rb.sample_sizes, col_rb.sample_sizes)
    return [(row_rb.tensor[b, :n].numpy(), col_rb.tensor[b, :n].numpy()) for b, n in enumerate(sizes)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_random_matches_scipy_exactly(shape, dtype):
    g = torch.Generator().manual_seed(shape[0] * 1000 + shape[1])
    cost = torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)
    r, c = lsa(cost)
    er, ec = linear_sum_assignment(cost.double().numpy())
    assert r.dtype == c.dtype == torch.int64
    np.testing.assert_array_equal(r.numpy(), er)
    np.testing.assert_array_equal(c.numpy(), ec)
    rm, cm = lsa(cost, maximize=True)
    er, ec = linear_sum_assignment(cost.double().numpy(), maximize=True)
    np.testing.assert_array_equal(rm.numpy(), er)
    np.testing.assert_array_equal(cm.numpy(), ec)


@pytest.mark.parametrize("shape", [(6, 6), (9, 4), (4, 9), (60, 20), (20, 60), (100, 100)])
@pytest.mark.parametrize("maximize", [False, True])
def test_tie_rich_optimum_exact(shape, maximize):
    for seed in range(5):
        g = torch.Generator().manual_seed(seed)
        cost = torch.randint(0, 4, shape, generator=g).double()
        r, c = lsa(cost, maximize=maximize)
        n = min(shape)
        assert r.numel() == c.numel() == n
        assert len(set(r.tolist())) == n and len(set(c.tolist())) == n
        assert r.tolist() == sorted(r.tolist())
        er, ec = linear_sum_assignment(cost.numpy(), maximize=maximize)
        assert float(cost[r, c].sum()) == float(cost.numpy()[er, ec].sum())


def test_forbidden_pairs_feasible_and_infeasible():
    inf = float("inf")
    cost = torch.tensor([[inf, 1.0, 2.0], [3.0, inf, 1.0], [1.0, 2.0, inf]])
    r, c = lsa(cost)
    er, ec = linear_sum_assignment(cost.numpy())
    np.testing.assert_array_equal(r.numpy(), er)
    np.testing.assert_array_equal(c.numpy(), ec)
    bad = torch.tensor([[inf, 1.0], [inf, 2.0]])
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        linear_sum_assignment(bad.numpy())
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        lsa(bad)
    # maximize: -inf forbids, +inf is invalid
    m = -cost
    r, c = lsa(m, maximize=True)
    er, ec = linear_sum_assignment(m.numpy(), maximize=True)
    np.testing.assert_array_equal(c.numpy(), ec)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        lsa(torch.tensor([[inf, 1.0], [0.0, 2.0]]), maximize=True)


@pytest.mark.parametrize("value", [float("nan"), float("-inf")])
def test_invalid_entries(value):
    cost = torch.rand(4, 6, dtype=torch.float64)
    cost[2, 3] = value
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        linear_sum_assignment(cost.numpy())
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        lsa(cost)


def test_status_without_check_keeps_other_frames():
    g = torch.Generator().manual_seed(3)
    cost = torch.rand(4, 7, 5, generator=g, dtype=torch.float64)
    cost[1, :, 2] = float("nan")
    cost[2, :, :] = float("inf")
    cost[2, 0, 0] = 1.0          # one finite entry: no complete matching
    r, c, st = lsa(cost, check=False)
    assert st.dtype == torch.int32 and st.tolist() == [0, 2, 1, 0]
    assert r.sample_sizes.tolist() == [5, 0, 0, 5]
    for b in (0, 3):
        er, ec = linear_sum_assignment(cost[b].numpy())
        np.testing.assert_array_equal(r.tensor[b].numpy(), er)
        np.testing.assert_array_equal(c.tensor[b].numpy(), ec)
    assert not r.tensor[1:3].any() and not c.tensor[1:3].any()
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        lsa(cost)


def test_ragged_forms_dense_and_views():
    g = torch.Generator().manual_seed(5)
    B, R, C = 5, 12, 9
    x = torch.rand(B, R, C, generator=g)
    col_sizes = [9, 0, 4, 12 - 3, 1]
    r, c = lsa(rb(x, col_sizes, 2))
    assert tuple(r.tensor.shape) == (B, min(R, C))
    assert r.sample_sizes.tolist() == [min(R, s) for s in col_sizes]
    for b, (rr, cc) in enumerate(frames(r, c)):
        er, ec = linear_sum_assignment(x[b, :, :col_sizes[b]].numpy())
        np.testing.assert_array_equal(rr, er)
        np.testing.assert_array_equal(cc, ec)
        assert not r.tensor[b, len(rr):].any() and not c.tensor[b, len(rr):].any()
    row_sizes = [12, 0, 3, 9, 7]
    r, c = lsa(rb(x, row_sizes, 1))
    assert r.sample_sizes.tolist() == [min(s, C) for s in row_sizes]
    for b, (rr, cc) in enumerate(frames(r, c)):
        er, ec = linear_sum_assignment(x[b, :row_sizes[b]].numpy())
        np.testing.assert_array_equal(rr, er)
        np.testing.assert_array_equal(cc, ec)
    # dense 3-D, and a transposed (non-contiguous) view
    xt = x.transpose(1, 2)
    assert not xt.is_contiguous()
    for t in (x, xt):
        r, c = lsa(t)
        for b in range(B):
            er, ec = linear_sum_assignment(t[b].numpy())
            np.testing.assert_array_equal(r.tensor[b].numpy(), er)
            np.testing.assert_array_equal(c.tensor[b].numpy(), ec)


def test_half_precision_inputs_are_widened():
    g = torch.Generator().manual_seed(8)
    x = torch.rand(3, 20, 30, generator=g)
    for dt in (torch.float16, torch.bfloat16):
        h = x.to(dt)
        r, c = lsa(h)
        r64, c64 = lsa(h.double())
        assert torch.equal(r.tensor, r64.tensor) and torch.equal(c.tensor, c64.tensor)


def test_limits_and_empty():
    with pytest.raises(ValueError, match="exceed the limit"):
        lsa(torch.zeros(1, 4097, 10))
    with pytest.raises(ValueError, match="exceed the limit"):
        lsa(torch.zeros(1, 1025, 1025))
    assert lsa(torch.zeros(1, 4096, 1))[0].tensor.shape == (1, 1)
    r, c = lsa(torch.zeros(0, 5, 3))
    assert r.tensor.shape == (0, 3) and r.sample_sizes.numel() == 0
    for shape in [(3, 0, 5), (3, 5, 0)]:
        r, c, st = lsa(torch.zeros(shape), check=False)
        assert r.tensor.shape == (3, 0) and r.sample_sizes.tolist() == [0, 0, 0] and st.tolist() == [0, 0, 0]
    r, c = lsa(torch.zeros(0, 4))
    assert r.numel() == 0 and c.numel() == 0
    with pytest.raises(TypeError):
        lsa(torch.zeros(2, 3, 3, dtype=torch.int32))


def test_cabi_validation():
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    out = [torch.zeros(4, dtype=torch.int64) for _ in range(3)] + [torch.zeros(1, dtype=torch.int32)]
    cost = torch.rand(1, 2, 2)
    ptrs = [t.data_ptr() for t in out]
    args = lambda dtype, p=cost.data_ptr(): (p, dtype, 1, 2, 2, 4, 2, 1, None, None, 0, *ptrs)   # noqa: E731
    assert lib.accv_linear_assignment_host(*args(0)) == nat.OK
    assert lib.accv_linear_assignment_host(*args(7)) == -1        # ACCV_EINVAL: unknown dtype
    assert lib.accv_linear_assignment_host(*args(0, None)) == -1  # null cost
    assert lib.accv_linear_assignment_workspace_bytes(1, 2, 2, 7) == 0
    assert lib.accv_linear_assignment_workspace_bytes(1, 5000, 2, 0) == 0
    assert lib.accv_linear_assignment_workspace_bytes(2, 3, 5, 0) >= 2 * 3 * 5 * 8
    dev = (cost.data_ptr(), 0, 1, 2, 2, 4, 2, 1, None, None, 0, *ptrs)
    # refused before the device is touched: oversized, null output, short workspace
    assert lib.accv_linear_assignment(cost.data_ptr(), 0, 1, 5000, 2, 4, 2, 1, None, None, 0, *ptrs, None, 0, None) == -1
    assert lib.accv_linear_assignment(cost.data_ptr(), 0, 1, 2, 2, 4, 2, 1, None, None, 0, None, ptrs[1], ptrs[2], ptrs[3],
                                      None, 0, None) == -1
    assert lib.accv_linear_assignment(*dev, None, 0, None) == -3  # ACCV_EWORKSPACE
    assert lib.accv_linear_assignment(*dev, ptrs[0], 8, None) == -3


def test_example_matcher_matches_scipy_loop():
    import matched_loss as ml

    import accvlab.batching_helpers as bh

    inp = ml.make_inputs(8, 900, 10, 100, torch.device("cpu"), seed=0)
    gt_boxes = bh.combine_data(inp[0])
    gt_labels = bh.combine_data(inp[1], other_with_same_sample_sizes=gt_boxes)
    want = ml.match_batched(gt_boxes, gt_labels, inp[3], inp[4])
    got = ml.match_batched_on_device(gt_boxes, gt_labels, inp[3], inp[4])
    for w, g in zip(want, got):
        assert torch.equal(w.sample_sizes, g.sample_sizes)
        m = w.mask
        assert torch.equal(w.tensor[m], g.tensor[:, :w.tensor.shape[1]][m])
