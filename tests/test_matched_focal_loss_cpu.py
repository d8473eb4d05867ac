"""matched_focal_loss on the host path (accv_matched_focal_loss_host / _bwd_host) against the float64 definition of
tests/matched_focal_loss_cases.py, its corners, the end-to-end chain of examples/matched_loss.py and the argument
checks.  Needs no GPU."""
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

SIZES = [0, 6, 3, 1, 6]   # ragged, an empty frame, full ones
PAIRS = [0, 6, 2, 1, 6]   # K = 6: frames 1 and 4 have n_b = K
name = lambda d: str(d).split(".")[-1]


def compare(inp, what="", grad_out=None, **kw):
    logits, labels, pind, gind, w = inp
    kw = dict(kw, query_weights=w)
    out, grad = run(mfl, logits, labels, pind, gind, grad_out=grad_out, **kw)
    ref = dict(kw)
    if isinstance(ref.get("avg_factor"), torch.Tensor):
        ref["avg_factor"] = float(ref["avg_factor"])
    want, gwant, _ = definition(logits, labels, pind, gind, grad_out=grad_out, **ref)
    assert out.dtype == (torch.float64 if logits.dtype == torch.float64 else torch.float32) and out.shape == want.shape
    assert grad.is_contiguous()
    check_loss(out, want, logits.dtype, what)
    check_grad(grad, gwant, logits.dtype, what)
    return out, grad


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("gamma", [2.0, 0.0, 1.5])
@pytest.mark.parametrize("alpha", [0.25, -1.0])
@pytest.mark.parametrize("weights", [False, True])
def test_host_matches_definition(weights, alpha, gamma, dtype):
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=3, weights=weights)
    g = torch.Generator().manual_seed(1)
    compare(inp, f"{name(dtype)}/a{alpha}/g{gamma}/w{weights}", grad_out=torch.rand(5, generator=g) + 0.5, alpha=alpha,
            gamma=gamma)


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("label_dtype", [torch.int32, torch.int64], ids=name)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=name)
def test_index_and_label_dtypes(dtype, label_dtype, index_dtype):
    compare(make_case(5, 9, 4, SIZES, PAIRS, dtype, seed=5, index_dtype=index_dtype, label_dtype=label_dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=name)
def test_avg_factor_forms(dtype):
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=7)
    out_none, _ = compare(inp)
    out_raw, _ = compare(inp, avg_factor=1.0)
    out_num, _ = compare(inp, avg_factor=3.7)
    out_dev, _ = compare(inp, avg_factor=torch.tensor(2.5))
    check_loss(out_none * float(sum(PAIRS)), out_raw.double(), torch.float32)
    check_loss(out_num * 3.7, out_raw.double(), torch.float32)
    check_loss(out_dev * 2.5, out_raw.double(), torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_strided_logits(dtype):
    """x[..., :C] of a wider tensor is read in place and equals its contiguous copy bit for bit"""
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=9, width=16, weights=True)
    assert not inp[0].is_contiguous()
    out, grad = compare(inp)
    out_c, grad_c = run(mfl, inp[0].contiguous(), *inp[1:4], query_weights=inp[4])
    assert torch.equal(bits(out), bits(out_c)) and torch.equal(bits(grad), bits(grad_c))
    sliced = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=9)[0][:, 1:6]   # a query slice: free query / batch strides
    compare((sliced, *inp[1:4], None))


@pytest.mark.parametrize("shape", [(8, 900, 10, 100), (16, 300, 91, 40), (4, 50, 3, 20)])
def test_shapes_of_the_issue_float32(shape):
    B, Q, C, objects = shape
    compare(shape_case(B, Q, C, objects, torch.float32, seed=B), f"{B}x{Q}x{C}")


# ------------------------------------------------------------------------------------------------------------- corners
def _small(dtype=torch.float32, **kw):
    return make_case(3, 6, 5, [4, 4, 4], [3, 3, 3], dtype, seed=11, **kw)


def test_label_outside_the_classes_is_background():
    logits, labels, pind, gind, _ = _small()
    for bad in (5, -1, 2 ** 31 + 7, -2 ** 40):
        labels.tensor[1, int(gind.tensor[1, 0])] = bad
        out, grad = compare((logits, labels, pind, gind, None))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    # and equals the same case without that pair
    keep = [0, 2, 1]
    pind2 = ragged(pind.tensor.clone(), [3, 2, 3])
    pind2.tensor[1, :2] = pind.tensor[1, 1:3]
    gind2 = ragged(gind.tensor.clone(), [3, 2, 3])
    gind2.tensor[1, :2] = gind.tensor[1, 1:3]
    out2, grad2 = run(mfl, logits, labels, pind2, gind2, avg_factor=1.0)
    out1, grad1 = run(mfl, logits, labels, pind, gind, avg_factor=1.0)
    assert torch.equal(bits(out1), bits(out2)) and torch.equal(bits(grad1), bits(grad2)) and keep


@pytest.mark.parametrize("which", ["pred", "gt"])
@pytest.mark.parametrize("value", [-1, 10 ** 6, -2 ** 40])
def test_indices_outside_their_range_are_skipped_not_wrapped(which, value):
    logits, labels, pind, gind, _ = _small()
    (pind if which == "pred" else gind).tensor[2, 1] = value
    out, grad = compare((logits, labels, pind, gind, None), avg_factor=1.0)
    # the same as the matching without slot 1 of frame 2
    pind2, gind2 = ragged(pind.tensor.clone(), [3, 3, 2]), ragged(gind.tensor.clone(), [3, 3, 2])
    pind2.tensor[2, 1], gind2.tensor[2, 1] = pind.tensor[2, 2], gind.tensor[2, 2]
    out2, grad2 = run(mfl, logits, labels, pind2, gind2, avg_factor=1.0)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))


def test_query_named_twice_takes_the_lowest_slot():
    logits, labels, pind, gind, _ = _small()
    labels.tensor[0] = torch.tensor([0, 1, 2, 3])
    pind.tensor[0] = torch.tensor([4, 2, 4])
    gind.tensor[0] = torch.tensor([1, 0, 3])       # query 4: label 1 (slot 0), not label 3 (slot 2)
    out, grad = compare((logits, labels, pind, gind, None), avg_factor=1.0)
    gind.tensor[0, 2] = 2                          # what the later pair says changes nothing
    out2, grad2 = run(mfl, logits, labels, pind, gind, avg_factor=1.0)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))
    assert float(grad[0, 4, 1]) < 0 < float(grad[0, 4, 3])
    # a lower slot with a label outside the classes still owns the query: its row stays background
    labels.tensor[0, 1] = 77
    _, grad3 = compare((logits, labels, pind, gind, None), avg_factor=1.0)
    assert bool((grad3[0, 4] > 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=name)
def test_slots_at_or_past_the_sample_size_are_never_read(dtype):
    inp = make_case(5, 7, 11, SIZES, PAIRS, dtype, seed=13, weights=True)
    logits, labels, pind, gind, w = inp
    out, grad = run(mfl, logits, labels, pind, gind, query_weights=w)
    junk_p, junk_g, junk_l = pind.tensor.clone(), gind.tensor.clone(), labels.tensor.clone()
    for b, n in enumerate(PAIRS):
        junk_p[b, n:] = torch.tensor([3, -5, 2 ** 40, 0, 1, 2 ** 62])[: 6 - n]
        junk_g[b, n:] = torch.tensor([2 ** 50, 0, -1, 1, 2 ** 31, 0])[: 6 - n]
    for b, n in enumerate(SIZES):
        junk_l[b, n:] = 2 ** 45    # labels of padded objects: no pair points at them
    out2, grad2 = run(mfl, logits, ragged(junk_l, SIZES), ragged(junk_p, PAIRS), ragged(junk_g, PAIRS), query_weights=w)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(grad), bits(grad2))
    compare((logits, ragged(junk_l, SIZES), ragged(junk_p, PAIRS), ragged(junk_g, PAIRS), w))


def test_frames_without_pairs_are_all_background():
    logits, labels, pind, gind, _ = make_case(3, 6, 5, [4, 0, 4], [0, 0, 0], torch.float32, seed=15)
    assert pind.tensor.shape == (3, 0)             # K = 0
    out, grad = compare((logits, labels, pind, gind, None))
    assert bool((grad > 0).all())
    logits, labels, pind, gind, _ = make_case(3, 6, 5, [4, 0, 4], [2, 0, 0], torch.float32, seed=15)
    compare((logits, labels, pind, gind, None))


@pytest.mark.parametrize("shape", [(0, 6, 5), (3, 0, 5), (3, 6, 0)])
def test_empty_extents_give_zeros(shape):
    B, Q, C = shape
    sizes = [min(2, Q)] * B
    logits, labels, pind, gind, _ = make_case(B, Q, C, [2] * B, sizes if C else [0] * B, torch.float32, seed=1)
    out, grad = run(mfl, logits, labels, pind, gind)
    assert out.shape == (B,) and out.dtype == torch.float32 and bool((out == 0).all())
    assert grad.shape == (B, Q, C)


def test_nan_logit_stays_in_its_frame_and_element():
    logits, labels, pind, gind, _ = _small()
    logits[1, 2, 3] = float("nan")
    for gamma in (2.0, 1.5, 0.0):
        out, grad = run(mfl, logits, labels, pind, gind, gamma=gamma)
        assert bool(torch.isnan(out[1])) and bool(torch.isfinite(out[[0, 2]]).all())
        nan = torch.isnan(grad)
        assert bool(nan[1, 2, 3]) and int(nan.sum()) == 1 and bool(torch.isfinite(grad[~nan]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_infinite_logits_give_the_documented_limits(dtype):
    logits, labels, pind, gind, _ = _small(dtype)
    q = int(pind.tensor[0, 0])
    l = int(labels.tensor[0, int(gind.tensor[0, 0])])
    other = (l + 1) % 5
    cases = {(float("inf"), l): (0.0, 0.0), (float("inf"), other): (float("inf"), 0.75),
             (float("-inf"), l): (float("inf"), -0.25), (float("-inf"), other): (0.0, 0.0)}
    for (value, c), (loss, g) in cases.items():
        x = logits.clone()
        x[0] = 0.0
        x[0, q, c] = value
        base = x.clone()
        base[0, q, c] = 0.0
        for gamma in (2.0, 0.0, 1.5):
            out, grad = run(mfl, x, labels, pind, gind, gamma=gamma, avg_factor=1.0)
            out0, _ = run(mfl, base, labels, pind, gind, gamma=gamma, avg_factor=1.0)
            if loss == 0.0:   # the element contributes nothing: the frame's sum is the others'
                el = 0.25 * 0.5 ** gamma * 0.6931471805599453 if c == l else 0.75 * 0.5 ** gamma * 0.6931471805599453
                assert abs(float(out[0]) - (float(out0[0]) - el)) <= 2e-3 * abs(float(out0[0]))
            else:
                assert float(out[0]) == loss
            assert float(grad[0, q, c]) == g, (value, c, gamma, float(grad[0, q, c]))
            assert int((~torch.isfinite(grad)).sum()) == 0 and bool(torch.isfinite(out[1:]).all())


# ---------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_chain_equals_the_composition():
    """the ragged gathers have no host path (as in the reference): here the composition is spelled with torch indexing;
    the GPU suite runs the chain with focal_class_loss_composed and matched_pair_loss_sum"""
    end_to_end("cpu", ragged_ops=False)


# ------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_name_the_operator():
    logits, labels, pind, gind, w = _small(weights=True)
    ok = dict(query_weights=w)
    bad = [
        (lambda: mfl(logits.to(torch.int32), labels, pind, gind), TypeError),
        (lambda: mfl(logits[0], labels, pind, gind), ValueError),
        (lambda: mfl(logits.transpose(1, 2), labels, pind, gind), ValueError),
        (lambda: mfl(logits, labels.tensor, pind, gind), TypeError),
        (lambda: mfl(logits, ragged(labels.tensor.float(), [4, 4, 4]), pind, gind), TypeError),
        (lambda: mfl(logits, labels, ragged(pind.tensor.to(torch.int32), [3, 3, 3]), gind), TypeError),
        (lambda: mfl(logits, labels, ragged(pind.tensor[:, :2], [2, 2, 2]), gind), ValueError),
        (lambda: mfl(logits, ragged(labels.tensor[:2], [4, 4]), pind, gind), ValueError),
        (lambda: mfl(logits, labels, pind, gind, gamma=-0.5), ValueError),
        (lambda: mfl(logits, labels, pind, gind, gamma=float("nan")), ValueError),
        (lambda: mfl(logits, labels, pind, gind, query_weights=w[:, :3]), ValueError),
        (lambda: mfl(logits, labels, pind, gind, query_weights=w.double()), TypeError),
        (lambda: mfl(logits, labels, pind, gind, avg_factor=torch.tensor([2.0])), ValueError),
        (lambda: mfl(logits, labels, pind, gind, avg_factor=torch.tensor(2.0, dtype=torch.float64)), ValueError),
        (lambda: mfl(logits.to("meta"), labels, pind, gind), (RuntimeError, ValueError)),
    ]
    for call, exc in bad:
        with pytest.raises(exc, match="matched_focal_loss"):
            call()
    assert mfl(logits, labels, pind, gind, **ok).shape == (3,)


def test_c_abi_argument_validation():
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    p = nat.MatchedFocalParams(0.25, 2.0, 1.0, nat.FL_AVG_NUM_POS, None)
    d = ctypes.c_void_p(64)
    fwd = lambda *, params=ctypes.addressof(p), dtype=0, flags=0, B=2, Q=3, C=4, sq=4, logits=d, ws=d, nbytes=1 << 20: \
        lib.accv_matched_focal_loss(logits, d, d, d, d, None, dtype, flags, B, Q, C, 5, 2, 12, sq, params, d, d, ws, nbytes, None)
    assert fwd(params=None) == -1 and b"null params" in lib.accv_last_error()
    assert fwd(dtype=4) == -1 and fwd(flags=8) == -1 and fwd(B=-1) == -1
    assert fwd(sq=3) == -1 and b"stride" in lib.accv_last_error()
    assert fwd(logits=None) == -1
    assert fwd(logits=ctypes.c_void_p(66)) == -1 and b"aligned" in lib.accv_last_error()
    assert fwd(nbytes=8) == -3 and fwd(ws=None) == -3
    assert fwd(B=0) == 0 and fwd(Q=0) == 0 and fwd(C=0) == 0
    p.gamma = -1.0
    assert fwd() == -1 and b"gamma" in lib.accv_last_error()
    p.gamma, p.avg_mode = 2.0, 7
    assert fwd() == -1 and b"avg_factor mode" in lib.accv_last_error()
    p.avg_mode = nat.FL_AVG_DEVICE
    assert fwd() == -1 and b"avg_factor pointer" in lib.accv_last_error()
    assert lib.accv_matched_focal_loss_workspace_bytes(8, 900, 10) >= 8 * 8
    assert lib.accv_matched_focal_loss_workspace_bytes(0, 900, 10) == 0


# -------------------------------------------------------------------------------------- the definition and the deep tails
from matched_focal_loss_cases import elementwise_stable, elementwise_textbook  # noqa: E402

GAMMAS = [0.0, 1.0, 1.5, 2.0]


def _element_and_gradient(form, x, t, alpha, gamma):
    x = x.clone().requires_grad_(True)
    loss = form(x, t, alpha, gamma)
    grad, = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), grad


# measured over the grid below: worst relative disagreement 7.90e-7 on losses (gamma = 2; 7.61e-7 already at gamma = 0),
# 5.26e-7 on gradients (gamma = 2), all at |x| close to 20.  The gradient figure is the expected 2^-53 / p = 5e-8 per
# cancelling term times the few terms of the product rule; the loss figure is larger because torch evaluates
# binary_cross_entropy_with_logits as (1 - t) x - logsigmoid(x), which for a saturated easy element is 20 - (20 - 2e-9):
# half a unit in the last place of 20 (1.8e-15) against a value of 2e-9.  The bound is ten times the measured worst.
TEXTBOOK_AGREEMENT = 7.9e-6


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("alpha", [0.25, -1.0])
def test_stable_and_textbook_definitions_agree_up_to_20(alpha, gamma):
    """for |x| <= 20 (p >= 2e-9) the textbook form is accurate to about 2^-53 / p per cancelling term: both forms are
    the same function there, on losses and gradients, for both targets"""
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.linspace(-20, 20, 4001, dtype=torch.float64), torch.rand(4000, generator=g, dtype=torch.float64) * 40 - 20])
    worst = [0.0, 0.0]
    for target in (0.0, 1.0):
        t = torch.full_like(x, target)
        a, b = _element_and_gradient(elementwise_stable, x, t, alpha, gamma), _element_and_gradient(elementwise_textbook, x, t, alpha, gamma)
        for k in range(2):
            worst[k] = max(worst[k], float(((a[k] - b[k]).abs() / a[k].abs()).max()))
    print(f"alpha {alpha} gamma {gamma}: worst relative disagreement {worst[0]:.3e} (loss), {worst[1]:.3e} (gradient); "
          f"bound {TEXTBOOK_AGREEMENT:g}")
    assert max(worst) <= TEXTBOOK_AGREEMENT


@pytest.mark.parametrize("gamma", GAMMAS)
def test_stable_definition_against_50_digits_in_the_deep_tails(gamma):
    """a dozen logits in +-[20, 60], both targets, alpha on and off: the float64 stable form and its autograd gradient
    against a 50-digit evaluation of L = c ln(1 + e^-z) (1 + e^z)^-gamma, z = +-x, and of its closed-form derivative, within
    float64 rounding (1e-13 relative)"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    xs = [20.0, 23.5, 28.0, 31.0, 36.75, 44.0, 52.5, 60.0, -20.0, -27.25, -31.0, -38.5, -47.0, -60.0]
    x = torch.tensor(xs, dtype=torch.float64)
    worst = 0.0
    for alpha in (0.25, -1.0):
        for target in (0.0, 1.0):
            loss, grad = _element_and_gradient(elementwise_stable, x, torch.full_like(x, target), alpha, gamma)
            coeff = mp.mpf(1) if alpha < 0 else (mp.mpf(alpha) if target else 1 - mp.mpf(alpha))
            for i, v in enumerate(xs):
                sign = 1 if target else -1
                z = mp.mpf(v) * sign
                sp, s = mp.log1p(mp.exp(-z)), 1 / (1 + mp.exp(z))            # softplus(-z), sigmoid(-z)
                want = coeff * sp * s ** gamma
                # d/dz: softplus(-z)' = -sigmoid(-z); sigmoid(-z)' = -sigmoid(-z) sigmoid(z)
                dz = coeff * (-s * s ** gamma - sp * gamma * s ** gamma * (1 - s))
                want_g = dz * sign
                for got, ref in ((float(loss[i]), want), (float(grad[i]), want_g)):
                    rel = float(abs((mp.mpf(got) - ref) / ref))
                    worst = max(worst, rel)
                    assert rel <= 1e-13, f"x {v} target {target} alpha {alpha} gamma {gamma}: {got!r} vs {mp.nstr(ref, 20)} ({rel:.2e})"
    print(f"gamma {gamma}: worst relative error against 50 digits {worst:.3e} (bound 1e-13)")


def test_textbook_definition_loses_the_gradient_in_the_deep_tails():
    """what the stable form is for: at x = -31 on a negative element (p = 3.4e-14) the textbook float64 gradient is off
    by more than a percent, the stable one agrees with the closed form p^2 (2 softplus(x) (1 - p) + p) to float64 rounding"""
    x = torch.tensor([-31.0], dtype=torch.float64)
    t = torch.zeros_like(x)
    _, g_stable = _element_and_gradient(elementwise_stable, x, t, -1.0, 2.0)
    _, g_text = _element_and_gradient(elementwise_textbook, x, t, -1.0, 2.0)
    p = float(torch.exp(x))                      # sigmoid(-31) = e^-31 (1 - 3.4e-14)
    closed = p * p * (2.0 * p + p)               # softplus(x) = p to first order, 1 - p = 1 to first order
    assert abs(float(g_stable) - closed) <= 1e-12 * closed
    assert abs(float(g_text) - closed) > 5e-3 * closed


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("alpha", [0.25, -1.0])
@pytest.mark.parametrize("sigma", [8.0, 16.0])
def test_deep_tail_logits_host_matches_definition(sigma, alpha, gamma, dtype):
    """logits of sigma 8 and 16: most sigmoids saturated, the tails that matched_focal_arith.h keeps cancellation-free"""
    inp = deep_tail_case(dtype, sigma)
    compare(inp, f"sigma {sigma} {name(dtype)}/a{alpha}/g{gamma}", alpha=alpha, gamma=gamma)
