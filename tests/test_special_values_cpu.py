"""Filler conversion of the ragged ops on the host: ``element_bits`` (the bytes every GPU fill writes) and the CPU pad fill
against ``static_cast<scalar_t>(double)`` as torch spells it, ``torch.tensor(v, dtype=float64).to(dtype)``: round to
nearest even, out of range -> ±inf, NaN stays NaN, -0.0 stays -0.0.  Also pins that the cached conversion does not
depend on call order (-0.0 and 0.0 compare and hash equal).

The shared f16 / bf16 conversions of csrc/accv_numeric.h (software flavour) have no entry point of their own; they are
pinned through ``accv_matched_focal_loss_bwd_host``, whose gradient can be made to equal a chosen float32 exactly."""
import math
import struct

import pytest
import torch

FLOATS = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}
WIDTH = {torch.float32: 32, torch.float64: 64, torch.float16: 16, torch.bfloat16: 16}

# ±0, NaN, ±inf, the usual mask sentinels, one value beyond every finite range
COMMON = [0.0, -0.0, math.nan, math.inf, -math.inf, 1e6, -1e9, 1e300, -1e300, 1.0, -2.5]
# largest finite, first value that rounds to inf, smallest subnormal; round-to-nearest-even ties (exact in float32, so
# no double rounding is involved) for the two half types
PER_TYPE = {
    torch.float16: [65504.0, -65504.0, 65520.0, -65520.0, 65519.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -25,
                    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, 2051.0],
    torch.bfloat16: [3.3895313892515355e38, 3.3961775292304e38, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -134,
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 257.0, 259.0],
    torch.float32: [3.4028234663852886e38, 3.4028235677973366e38, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -150],
    torch.float64: [1.7976931348623157e308, 5e-324, -5e-324],
}
CASES = [(dt, v) for dt in FLOATS for v in COMMON + PER_TYPE[dt]]


def _id(case):
    dt, v = case
    return f"{str(dt).split('.')[-1]}-{v!r}"


def reference_bits(value, dtype):
    x = torch.tensor(float(value), dtype=torch.float64).to(dtype)
    return int(x.view(INT_VIEW[dtype]).item()) & ((1 << WIDTH[dtype]) - 1)


def element_bits(value, dtype):
    from accvlab.batching_helpers.batched_indexing_access_cuda import element_bits as f

    return f(value, dtype)


def test_reference_conversion_is_static_cast():
    """the yardstick itself: out of range gives ±inf, ties go to even, NaN is NaN, the sign of zero survives"""
    assert reference_bits(1e6, torch.float16) == 0x7C00 and reference_bits(-1e9, torch.float16) == 0xFC00
    assert reference_bits(65520.0, torch.float16) == 0x7C00 and reference_bits(65519.0, torch.float16) == 0x7BFF
    assert reference_bits(1e300, torch.float32) == 0x7F800000 and reference_bits(-1e300, torch.bfloat16) == 0xFF80
    assert reference_bits(1 + 2.0 ** -11, torch.float16) == 0x3C00 and reference_bits(1 + 3 * 2.0 ** -11, torch.float16) == 0x3C02
    assert reference_bits(1 + 2.0 ** -8, torch.bfloat16) == 0x3F80 and reference_bits(1 + 3 * 2.0 ** -8, torch.bfloat16) == 0x3F82
    assert reference_bits(2.0 ** -24, torch.float16) == 0x0001 and reference_bits(2.0 ** -25, torch.float16) == 0x0000
    assert reference_bits(-0.0, torch.float16) == 0x8000 and reference_bits(-0.0, torch.float64) == 1 << 63
    assert reference_bits(math.nan, torch.float16) & 0x7C00 == 0x7C00 and reference_bits(math.nan, torch.float16) & 0x3FF


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_element_bits_is_static_cast(case):
    dtype, v = case
    assert element_bits(v, dtype) == reference_bits(v, dtype), hex(reference_bits(v, dtype))


@pytest.mark.parametrize("dtype", FLOATS, ids=lambda d: str(d).split(".")[-1])
def test_signed_zero_does_not_depend_on_call_order(dtype):
    from accvlab.batching_helpers import batched_indexing_access_cuda as m

    neg = 1 << (WIDTH[dtype] - 1)
    m._element_bits.cache_clear()
    assert element_bits(0.0, dtype) == 0
    assert element_bits(-0.0, dtype) == neg
    m._element_bits.cache_clear()
    assert element_bits(-0.0, dtype) == neg
    assert element_bits(0.0, dtype) == 0
    assert element_bits(0, dtype) == 0 and element_bits(-0.0, dtype) == neg
    # numpy and 0-dim tensor fillers normalise to the same python float, sign included
    assert element_bits(torch.tensor(-0.0), dtype) == neg and element_bits(torch.tensor(0.0), dtype) == 0


@pytest.mark.parametrize("dtype,bits", [(torch.int8, 8), (torch.uint8, 8), (torch.int16, 16), (torch.int32, 32),
                                        (torch.int64, 64)], ids=lambda x: str(x).split(".")[-1])
def test_integer_fillers_truncate_toward_zero(dtype, bits):
    mask = (1 << bits) - 1
    for v, want in [(0, 0), (-0.0, 0), (5, 5), (-1, -1), (1.7, 1), (-1.7, -1), (0.999, 0), (-0.999, 0), (100.5, 100)]:
        assert element_bits(v, dtype) == want & mask, (v, dtype)
    lo = -(1 << (bits - 1)) if dtype != torch.uint8 else 0
    hi = (1 << (bits - 1)) - 1 if dtype != torch.uint8 else 255
    assert element_bits(lo, dtype) == lo & mask and element_bits(hi, dtype) == hi & mask


def test_bool_filler_is_nonzero():
    for v, want in [(0, 0), (0.0, 0), (-0.0, 0), (1, 1), (True, 1), (False, 0), (0.5, 1), (-2.0, 1), (math.nan, 1),
                    (math.inf, 1)]:
        assert element_bits(v, torch.bool) == want, v


def _pad_fill_cpu(dtype, value):
    from accvlab.batching_helpers import RaggedBatch

    data = torch.arange(2 * 4 * 3, dtype=torch.float64).reshape(2, 4, 3).to(dtype)
    sizes = torch.tensor([1, 3])
    rb = RaggedBatch(data.clone(), sample_sizes=sizes)
    out = rb.with_padded_set_to(value).tensor
    pad = torch.arange(4)[None, :] >= sizes[:, None]
    return data, out, pad


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cpu_pad_fill_writes_the_same_bits(case):
    dtype, v = case
    data, out, pad = _pad_fill_cpu(dtype, v)
    iv = INT_VIEW[dtype]
    got = out.view(iv)[pad].long() & ((1 << WIDTH[dtype]) - 1) if WIDTH[dtype] < 64 else out.view(iv)[pad]
    want = reference_bits(v, dtype)
    if WIDTH[dtype] == 64:
        want = struct.unpack("<q", struct.pack("<Q", want))[0]
    assert bool((got == want).all()), (hex(want), got.unique().tolist())
    assert torch.equal(out.view(iv)[~pad], data.view(iv)[~pad])          # the valid entries keep their bits


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16, torch.uint8], ids=lambda d: str(d).split(".")[-1])
def test_cpu_pad_fill_integer_and_bool(dtype):
    for v, want in [(7, 7), (-1.7, -1), (2.9, 2)]:
        if dtype == torch.uint8 and want < 0:
            continue
        data, out, pad = _pad_fill_cpu(dtype, v)
        assert bool((out[pad] == want).all()) and torch.equal(out[~pad], data[~pad])
    from accvlab.batching_helpers import RaggedBatch

    b = RaggedBatch(torch.zeros(2, 3, dtype=torch.bool), sample_sizes=torch.tensor([0, 2]))
    assert b.with_padded_set_to(0.5).tensor.tolist() == [[True, True, True], [False, False, True]]


# ---- the shared f16 / bf16 conversions (csrc/accv_numeric.h), through the host twin of the matched focal loss --------------
# One frame per value, Q = C = 1, no pair (all background), logit +inf, gamma = 0, no alpha blend, avg_factor = 1: the
# element's derivative is sigmoid(+inf) = 1 exactly, so the gradient written is narrow((w * 1) * grad_out[b]) with grad_out
# float32 and w the query weight widened from the logits dtype (1 without weights).
HALVES = [torch.float16, torch.bfloat16]


def _host_gradient(dtype, grad_out, weights=None):
    from accvlab.batching_helpers import RaggedBatch, matched_focal_loss

    B = grad_out.numel()
    empty = lambda dt: RaggedBatch(torch.zeros((B, 1), dtype=dt), sample_sizes=torch.zeros((B,), dtype=torch.int64))
    logits = torch.full((B, 1, 1), math.inf, dtype=dtype, requires_grad=True)
    out = matched_focal_loss(logits, empty(torch.int64), empty(torch.int64), empty(torch.int64), alpha=-1.0, gamma=0.0,
                             query_weights=weights, avg_factor=1.0)
    out.backward(grad_out)
    return logits.grad.reshape(B)


def _narrowing_inputs(dtype):
    vals = [v for v in COMMON + PER_TYPE[dtype] if not math.isnan(v) and abs(v) < 3.5e38 or math.isinf(v)]
    x = torch.tensor(vals, dtype=torch.float64).to(torch.float32)
    # every float32 around the boundaries: subnormal / normal, largest finite / infinity, and ties between neighbours
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (200000,), generator=g, dtype=torch.int64).to(torch.int32)
    rnd = bits.view(torch.float32)
    tiny = torch.tensor(6.5e-5 if dtype == torch.float16 else 2.4e-38) * torch.rand(50000, generator=g)   # subnormal results
    ulp = torch.arange(-40, 41, dtype=torch.int32)
    edge = torch.tensor([65504.0, 65520.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 3.3895313892515355e38,
                         3.3961775292304e38, 2.0 ** -126, 1.0 + 2.0 ** -8], dtype=torch.float32)
    near = (edge.view(torch.int32)[:, None] + ulp[None, :]).reshape(-1).view(torch.float32)
    x = torch.cat([x, rnd, tiny, -tiny, near, -near])
    return x[~torch.isnan(x)]


@pytest.mark.parametrize("dtype", HALVES, ids=["float16", "bfloat16"])
def test_shared_narrowing_is_the_torch_cast(dtype):
    x = _narrowing_inputs(dtype)
    got = _host_gradient(dtype, x)
    want = x.to(dtype)
    assert not torch.isnan(want).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    for v in (0.0, -0.0, 65504.0, 65519.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11):   # named cases
        one = _host_gradient(dtype, torch.tensor([v], dtype=torch.float32))
        assert one.view(torch.int16).item() == torch.tensor([v], dtype=torch.float32).to(dtype).view(torch.int16).item(), v


@pytest.mark.parametrize("dtype", HALVES, ids=["float16", "bfloat16"])
def test_shared_narrowing_keeps_nan(dtype):
    nans = torch.tensor([0x7fc00000, -0x400000, 0x7f800001, 0x7fffffff, -1, 0x7f80ffff, 0x7f810000],
                        dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert torch.isnan(nans).all()
    assert torch.isnan(_host_gradient(dtype, nans).float()).all()


@pytest.mark.parametrize("dtype", HALVES, ids=["float16", "bfloat16"])
def test_shared_widening_is_exact(dtype):
    """Every 16-bit pattern as a query weight: widen, times 1, narrow gives the pattern back (NaN: some NaN)."""
    w = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(dtype)
    got = _host_gradient(dtype, torch.ones(w.numel(), dtype=torch.float32), weights=w.reshape(-1, 1))
    nan = torch.isnan(w.float())
    assert torch.equal(got.view(torch.int16)[~nan], w.view(torch.int16)[~nan])
    assert torch.isnan(got.float()[nan]).all()
    assert torch.equal(got.float()[~nan], w.float()[~nan])   # and torch widens to the same float32
