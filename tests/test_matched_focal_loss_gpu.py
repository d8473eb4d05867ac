"""matched_focal_loss on the device (accv_matched_focal_loss / _bwd) against the float64 definition of
tests/matched_focal_loss_cases.py and against the host path: values, gradients, reproducibility, complete writes, guard
bands, no synchronisation, graph capture, special values."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matched_focal_loss_cases import (DTYPES, bits, check_grad, check_loss, deep_tail_case, definition, end_to_end,  # noqa: E402
                                      make_case, ragged, run, shape_case)

from accvlab.batching_helpers import matched_focal_loss as mfl  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [0, 6, 3, 1, 6]
PAIRS = [0, 6, 2, 1, 6]
SHAPES = {"a": (8, 900, 10, 100), "b": (16, 300, 91, 40), "c": (48, 900, 80, 60)}
name = lambda d: str(d).split(".")[-1]


def to_host(inp):
    logits, labels, pind, gind, w = inp
    cpu = lambda rb: ragged(rb.tensor.cpu(), rb.sample_sizes.cpu().tolist())
    return logits.cpu(), cpu(labels), cpu(pind), cpu(gind), None if w is None else w.cpu()


def compare(inp, what="", grad_out=None, host=True, **kw):
    """device against the float64 definition and (host=True) the host path against it on the same inputs"""
    logits, labels, pind, gind, w = inp
    ref = dict(kw)
    if isinstance(ref.get("avg_factor"), torch.Tensor):
        ref["avg_factor"] = float(ref["avg_factor"])
    want, gwant, _ = definition(logits, labels, pind, gind, grad_out=grad_out, query_weights=w, **ref)
    out, grad = run(mfl, logits, labels, pind, gind, grad_out=None if grad_out is None else grad_out.to(DEV),
                    query_weights=w, **kw)
    assert out.is_cuda and grad.is_cuda and grad.is_contiguous()
    check_loss(out, want, logits.dtype, what + " device")
    check_grad(grad, gwant, logits.dtype, what + " device")
    if host:
        h = to_host(inp)
        hkw = dict(kw)
        if isinstance(hkw.get("avg_factor"), torch.Tensor):
            hkw["avg_factor"] = hkw["avg_factor"].cpu()
        hout, hgrad = run(mfl, *h[:4], grad_out=grad_out, query_weights=h[4], **hkw)
        check_loss(hout, want, logits.dtype, what + " host")
        check_grad(hgrad, gwant, logits.dtype, what + " host")
    return out, grad


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("gamma", [2.0, 0.0, 1.5])
@pytest.mark.parametrize("alpha", [0.25, -1.0])
@pytest.mark.parametrize("weights", [False, True])
def test_device_and_host_match_definition(weights, alpha, gamma, dtype):
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=3, weights=weights, device=DEV)
    g = torch.Generator().manual_seed(1)
    compare(inp, f"{name(dtype)}/a{alpha}/g{gamma}/w{weights}", grad_out=torch.rand(5, generator=g) + 0.5, alpha=alpha,
            gamma=gamma)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_realistic_shapes(shape, dtype):
    B, Q, C, objects = SHAPES[shape]
    compare(shape_case(B, Q, C, objects, dtype, seed=B, device=DEV, weights=shape == "b"), f"({shape}) {name(dtype)}")


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("label_dtype", [torch.int32, torch.int64], ids=name)
def test_index_and_label_dtypes(label_dtype, index_dtype):
    compare(make_case(5, 9, 4, SIZES, PAIRS, torch.float32, seed=5, index_dtype=index_dtype, label_dtype=label_dtype,
                      device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms(dtype):
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=7, device=DEV)
    for factor in (None, 1.0, 3.7, torch.tensor(2.5, device=DEV)):
        compare(inp, f"avg_factor {factor}", avg_factor=factor)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("C,width", [(11, 16), (8, 12), (3, 7), (1, 2), (300, 301)])
def test_strided_and_misaligned_logits(C, width, dtype):
    """x[..., :C] of a wider tensor (scalar path), and contiguous logits whose base is not 16-byte aligned (the vector
    path with a head and a tail) against the contiguous copy bit for bit"""
    inp = make_case(5, 7, C, SIZES, PAIRS, dtype, seed=9, width=width, weights=True, device=DEV)
    out, grad = compare(inp, host=False)
    out_c, grad_c = run(mfl, inp[0].contiguous(), *inp[1:4], query_weights=inp[4])
    assert torch.equal(bits(grad), bits(grad_c))
    check_loss(out, out_c.cpu().double(), torch.float64 if dtype == torch.float64 else torch.float32)
    flat = torch.empty(5 * 7 * C + 3, dtype=dtype, device=DEV)
    shifted = flat[3:].view(5, 7, C)
    shifted.copy_(inp[0])
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    out_s, grad_s = run(mfl, shifted, *inp[1:4], query_weights=inp[4])
    assert torch.equal(bits(grad_s), bits(grad_c))
    check_loss(out_s, out_c.cpu().double(), torch.float64 if dtype == torch.float64 else torch.float32)


def test_corners_on_the_device():
    """labels outside the classes, indices outside their range, a query named twice, junk past the sample sizes: the device
    follows the definition and the host path"""
    logits, labels, pind, gind, _ = make_case(3, 6, 5, [4, 4, 4], [3, 3, 3], torch.float32, seed=11, device=DEV)
    labels.tensor[1, int(gind.tensor[1, 0])] = 2 ** 31 + 7
    labels.tensor[1, int(gind.tensor[1, 1])] = -1
    pind.tensor[2, 1] = -1
    gind.tensor[2, 2] = 10 ** 6
    pind.tensor[0] = torch.tensor([4, 2, 4])
    compare((logits, labels, pind, gind, None), "corners")
    out, grad = run(mfl, logits, labels, pind, gind)
    n = [2, 1, 3]
    junk_p, junk_g = pind.tensor.clone(), gind.tensor.clone()
    for b, k in enumerate(n):
        junk_p[b, k:] = 2 ** 40
        junk_g[b, k:] = -7
    small = run(mfl, logits, labels, ragged(pind.tensor, n), ragged(gind.tensor, n))
    junk = run(mfl, logits, labels, ragged(junk_p, n), ragged(junk_g, n))
    assert torch.equal(bits(small[0]), bits(junk[0])) and torch.equal(bits(small[1]), bits(junk[1]))
    assert not torch.equal(bits(small[1]), bits(grad))


def test_empty_extents_and_frames_without_pairs():
    for B, Q, C in ((0, 6, 5), (3, 0, 5), (3, 6, 0)):
        logits, labels, pind, gind, _ = make_case(B, Q, C, [2] * B, [0] * B, torch.float32, seed=1, device=DEV)
        out, grad = run(mfl, logits, labels, pind, gind)
        assert out.shape == (B,) and bool((out == 0).all()) and grad.shape == (B, Q, C)
    inp = make_case(3, 6, 5, [4, 0, 4], [0, 0, 0], torch.float32, seed=15, device=DEV)
    assert inp[2].tensor.shape == (3, 0)
    compare(inp, "K = 0")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_bitwise_reproducible_and_completely_written(dtype):
    inp = shape_case(16, 300, 91, 40, dtype, seed=2, device=DEV, weights=True)
    first = run(mfl, *inp[:4], query_weights=inp[4])
    for _ in range(5):
        # the allocator hands the freed block of a same-size tensor to the next gradient: NaN in every element
        poison = torch.full(inp[0].shape, float("nan"), dtype=dtype, device=DEV)
        del poison
        again = run(mfl, *inp[:4], query_weights=inp[4])
        assert torch.equal(bits(again[0]), bits(first[0])) and torch.equal(bits(again[1]), bits(first[1]))
    assert bool(torch.isfinite(first[1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("shape", [(3, 7, 11), (2, 130, 80), (1, 5, 2500)])
def test_guard_bands_around_output_gradient_and_workspace(shape, dtype):
    from accvlab import _amd_native as nat

    B, Q, C = shape
    sizes = [min(Q, 5)] * B
    logits, labels, pind, gind, w = make_case(B, Q, C, sizes, sizes, dtype, seed=4, device=DEV, weights=True)
    lib = nat.ctypes_lib()
    out_dtype = torch.float64 if dtype == torch.float64 else torch.float32
    pad = 512

    def banded(nbytes):
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[pad: pad + nbytes]

    ws_bytes = lib.accv_matched_focal_loss_workspace_bytes(B, Q, C)
    out_buf, out_in = banded(B * (8 if dtype == torch.float64 else 4))
    den_buf, den_in = banded(8)
    ws_buf, ws_in = banded(ws_bytes)
    grad_buf, grad_in = banded(B * Q * C * logits.element_size())
    grad_in.view(dtype).fill_(float("nan"))
    p = nat.MatchedFocalParams(0.25, 2.0, 0.0, nat.FL_AVG_NUM_POS, None)
    counts = pind.sample_sizes.to(torch.int64)
    flags = nat.MF_IDX_I64 | nat.MF_LABELS_I64
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}[dtype]
    common = (logits.data_ptr(), labels.tensor.data_ptr(), pind.tensor.data_ptr(), gind.tensor.data_ptr(), counts.data_ptr(),
              w.data_ptr())
    shape_args = (dt, flags, B, Q, C, labels.tensor.shape[1], pind.tensor.shape[1], Q * C, C, ctypes.addressof(p))
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    assert lib.accv_matched_focal_loss(*common, *shape_args, out_in.data_ptr(), den_in.data_ptr(), ws_in.data_ptr(), ws_bytes,
                                       stream) == 0, lib.accv_last_error()
    go = torch.ones(B, dtype=out_dtype, device=DEV)
    assert lib.accv_matched_focal_loss_bwd(*common, go.data_ptr(), den_in.data_ptr(), *shape_args, grad_in.data_ptr(),
                                           stream) == 0, lib.accv_last_error()
    torch.cuda.synchronize()
    for buf, inner in ((out_buf, out_in), (den_buf, den_in), (ws_buf, ws_in), (grad_buf, grad_in)):
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + inner.numel():] == 0xA5).all())
    grad = grad_in.view(dtype).view(B, Q, C)
    assert bool(torch.isfinite(grad).all()), "the NaN-filled gradient buffer was not written completely"
    want, gwant, factor = definition(logits, labels, pind, gind, query_weights=w)
    check_loss(out_in.view(out_dtype), want, dtype)
    check_grad(grad.clone(), gwant, dtype)
    assert float(den_in.view(torch.float64)) == factor


def test_no_synchronisation_forward_and_backward():
    inp = shape_case(8, 900, 10, 100, torch.float32, seed=3, device=DEV, weights=True)
    avg = torch.tensor(17.0, device=DEV)
    x = inp[0].detach().requires_grad_(True)
    go = torch.ones(8, device=DEV)
    mfl(x, *inp[1:4]).backward(go)    # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in ({}, {"avg_factor": avg}, {"avg_factor": 3.0, "query_weights": inp[4], "gamma": 1.5}):
            x.grad = None
            mfl(x, *inp[1:4], **kw).backward(go)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x.grad).all())


def test_graph_capture_and_replay_with_changed_inputs():
    a = shape_case(8, 300, 20, 30, torch.float32, seed=5, device=DEV)
    b = shape_case(8, 300, 20, 30, torch.float32, seed=6, device=DEV)
    assert a[2].tensor.shape == b[2].tensor.shape and a[1].tensor.shape == b[1].tensor.shape
    x = a[0].clone().requires_grad_(True)
    labels, pind, gind = (ragged(rb.tensor.clone(), [0] * 8) for rb in a[1:4])
    for rb, src in zip((labels, pind, gind), a[1:4]):
        rb.sample_sizes.copy_(src.sample_sizes)
    go = torch.ones(8, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            out = mfl(x, labels, pind, gind)
            grad, = torch.autograd.grad(out, x, go)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mfl(x, labels, pind, gind)
        grad, = torch.autograd.grad(out, x, go)
    for case in (b, a):
        with torch.no_grad():
            x.copy_(case[0])
        for rb, src in zip((labels, pind, gind), case[1:4]):
            rb.tensor.copy_(src.tensor)
            rb.sample_sizes.copy_(src.sample_sizes)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(mfl, *case[:4])
        assert torch.equal(bits(out), bits(eager[0])) and torch.equal(bits(grad), bits(eager[1]))
        want, gwant, _ = definition(*case[:4])
        check_loss(out, want, torch.float32, "replay")
        check_grad(grad.clone(), gwant, torch.float32, "replay")


def test_nan_logit_stays_in_its_frame_and_element():
    logits, labels, pind, gind, _ = make_case(3, 6, 5, [4, 4, 4], [3, 3, 3], torch.float32, seed=11, device=DEV)
    logits[1, 2, 3] = float("nan")
    for gamma in (2.0, 1.5, 0.0):
        out, grad = run(mfl, logits, labels, pind, gind, gamma=gamma)
        assert bool(torch.isnan(out[1])) and bool(torch.isfinite(out[[0, 2]]).all())
        nan = torch.isnan(grad)
        assert bool(nan[1, 2, 3]) and int(nan.sum()) == 1 and bool(torch.isfinite(grad[~nan]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_infinite_logits_device_and_host_agree(dtype):
    inp = make_case(3, 6, 5, [4, 4, 4], [3, 3, 3], dtype, seed=11, device=DEV)
    logits, labels, pind, gind, _ = inp
    q = int(pind.tensor[0, 0])
    l = int(labels.tensor[0, int(gind.tensor[0, 0])])
    logits[0] = 0.0
    logits[0, q, l] = float("inf")
    logits[0, q, (l + 1) % 5] = float("inf")
    logits[0, (q + 1) % 6] = float("-inf")
    q2 = int(pind.tensor[1, 0])
    logits[1, q2, int(labels.tensor[1, int(gind.tensor[1, 0])])] = float("-inf")
    h = to_host(inp)
    for gamma in (2.0, 0.0, 1.5):
        out, grad = run(mfl, logits, labels, pind, gind, gamma=gamma, avg_factor=1.0)
        hout, hgrad = run(mfl, *h[:4], gamma=gamma, avg_factor=1.0)
        assert float(out[0]) == float("inf") and float(out[1]) == float("inf") and bool(torch.isfinite(out[2]))
        assert torch.equal(torch.isinf(out.cpu()), torch.isinf(hout))
        assert float(grad[0, q, l]) == 0.0 and float(grad[0, q, (l + 1) % 5]) == 0.75
        assert bool(torch.isfinite(grad).all())
        if dtype in (torch.float16, torch.bfloat16):
            check_grad(grad, hgrad.double(), dtype, "device vs host")
        else:
            torch.testing.assert_close(grad.cpu(), hgrad, rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=0)


def test_end_to_end_chain_equals_the_composition():
    end_to_end(DEV, ragged_ops=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("gamma", [0.0, 1.0, 1.5, 2.0])
@pytest.mark.parametrize("alpha", [0.25, -1.0])
@pytest.mark.parametrize("sigma", [8.0, 16.0])
def test_deep_tail_logits_device_and_host_match_definition(sigma, alpha, gamma, dtype):
    """logits of sigma 8 and 16: most sigmoids saturated, the tails that matched_focal_arith.h keeps cancellation-free
    (the float64 definition is cancellation-free as well: tests/matched_focal_loss_cases.py::elementwise_stable)"""
    inp = deep_tail_case(dtype, sigma, device=DEV)
    compare(inp, f"sigma {sigma} {name(dtype)}/a{alpha}/g{gamma}", alpha=alpha, gamma=gamma)
