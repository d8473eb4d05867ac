"""The polyline sampler and its backward (csrc/polyline.hip) in every launch regime: two workgroup sizes, LDS or scratch
arc lengths, LDS or workspace accumulators, one or many query chunks with the slab and the summing launch, compile-time or
run-time coordinate count, four storage types — at the shapes of polyline_edges_cases.py, which sit on both sides of every
threshold of the launch plan (DESIGN.md §9k lists each decision and loop next to the case that crosses it).

Every case first asserts the regime it names through the two workspace entry points.  The forward is compared with the
float64 definition (test_polyline_grad_gpu.ref_sample) at the bounds of polyline_edges_cases.check_forward, the backward
through _run / ref_grads / _check of test_polyline_grad_gpu.py at that file's own tolerances."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import polyline_edges_cases as pc  # noqa: E402
# modules, so that their tests are not collected here
import test_guard_bands_gpu as gb  # noqa: E402
import test_polyline_grad_gpu as pg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _dev(t):
    return None if t is None else t.to(DEV)


def _grad_tolerance(dtype):
    """test_polyline_grad_gpu.py: f32 1e-4 relative and 1e-6 of scale, half eps and 1e-4 of scale, f64 1e-9 / 1e-12"""
    if dtype == pc.F64:
        return 1e-9, 1e-12
    return (1e-4, 1e-6) if dtype == pc.F32 else (torch.finfo(dtype).eps, 1e-4)


def _assert_padding_is_zero(row, gp, gd, ps, qs, what):
    if ps is None:
        return
    for b in range(row.batch):
        n, q = int(ps[b]), int(qs[b])
        assert pc.bitwise_zero(gp[b, n:]), f"{what}: gradient rows behind the point count of polyline {b}"
        assert pc.bitwise_zero(gd[b, q if n else 0:]), f"{what}: grad_distances behind the query count of polyline {b}"


# ------------------------------------------------------------------------------------------------- forward and backward
@pytest.mark.parametrize("which,dtype", pc.RUNS, ids=pc.RUN_IDS)
def test_forward_and_backward_in_the_named_regime(which, dtype):
    row = pc.CASES[which]
    pc.assert_regime(which, dtype)
    for relative in pc.relatives(which, dtype):
        p, fr, ps, qs = pc.inputs(which, relative)
        what = f"{which} {pc.name(dtype)} {'relative' if relative else 'absolute'}"
        pd, fd = p.to(dtype).to(DEV), fr.to(dtype).to(DEV)          # half types: compared on the rounded inputs, as _run does
        ref, ref_lens = pg.ref_sample(pd.double(), fd.double(), _dev(ps), relative, pc.acc_eps(dtype, DEV))
        out, lens = pc.forward(pd, fd, ps, qs, relative)
        assert out.dtype == dtype and lens.dtype == dtype
        pc.check_forward(out, lens, ref, ref_lens, qs, dtype, what)
        if ps is not None:                                          # int32 counts: the same kernel, the same bits
            out32, lens32 = pc.forward(pd, fd, ps, qs, relative, counts=torch.int32)
            live = pc.live_mask(qs, row.batch, row.Q, DEV)
            assert torch.equal(out32[live].view(torch.uint8), out[live].view(torch.uint8))
            assert torch.equal(lens32.view(torch.uint8), lens.view(torch.uint8))
        rtol, afrac = _grad_tolerance(dtype)
        # the half types: the samples' and the lengths' gradients one by one (test_half_matches_reference_on_rounded_inputs)
        for terms in ((("samples",), ("lengths",)) if dtype in pc.HALF else (("samples", "lengths"),)):
            gp, gd, rp, rd = pg._run(p, fr, relative, dtype, ps, qs, terms=terms)
            pg._check(gp, rp, rtol, afrac, f"{what} grad points ({'+'.join(terms)})")
            pg._check(gd, rd, rtol, afrac, f"{what} grad distances ({'+'.join(terms)})")
            _assert_padding_is_zero(row, gp, gd, ps, qs, what)
        if dtype == pc.F64:     # test_f64_gpu_matches_host_backward: the host backward as the second witness
            g = pg._gout(tuple(out.shape), 1, dtype)
            gl = pg._gout((row.batch,), 2, dtype)
            hp, hd = pc.api_grads(pd.cpu(), fd.cpu(), ps, qs, relative, g, gl)
            dp, dd = pc.api_grads(pd, fd, ps, qs, relative, g.to(DEV), gl.to(DEV))
            pg._check(dp, hp, 1e-9, 1e-12, f"{what} grad points against the host backward")
            pg._check(dd, hd, 1e-9, 1e-12, f"{what} grad distances against the host backward")


# -------------------------------------------------------------------------------------------------------------- chunks
CHUNKED = [(w, d) for w, d in pc.RUNS if pc.CASES[w].regimes[d]["fwd_chunks"] > 1]


@pytest.mark.parametrize("which,dtype", CHUNKED, ids=[f"{w}-{pc.name(d)}" for w, d in CHUNKED])
def test_forward_chunks_are_independent(which, dtype):
    """every chunk repeats the same scan: the samples of a chunked launch are the bits of the same polylines launched with the
    queries of one chunk alone (a slice of `threads` queries is one workgroup per polyline; a longer one may be cut again,
    into other chunks, and the bits still agree)"""
    row = pc.CASES[which]
    pl = pc.assert_regime(which, dtype)
    relative = pc.relatives(which, dtype)[-1]
    p, fr, ps, qs = pc.inputs(which, relative)
    pd, fd = p.to(dtype).to(DEV), fr.to(dtype).to(DEV)
    out, _ = pc.forward(pd, fd, ps, qs, relative)
    live = pc.live_mask(qs, row.batch, row.Q, DEV)
    n = pl.fwd_chunks
    for c in (range(n) if n <= 64 else (0, 1, n // 2, n - 2, n - 1)):
        lo, hi = c * pl.fwd_q_chunk, min(row.Q, (c + 1) * pl.fwd_q_chunk)
        qc = None if qs is None else (qs - lo).clamp(0, hi - lo)
        part, _ = pc.forward(pd, fd[:, lo:hi].contiguous(), ps, qc, relative)
        m = live[:, lo:hi]
        assert torch.equal(part[m].view(torch.uint8), out[:, lo:hi][m].view(torch.uint8)), f"chunk {c} of {n}"


SLICED = [(w, d) for w, d in pc.RUNS if pc.CASES[w].sliced and d not in pc.HALF]


@pytest.mark.parametrize("which,dtype", SLICED, ids=[f"{w}-{pc.name(d)}" for w, d in SLICED])
def test_chunked_gradient_equals_the_sum_over_single_chunk_launches(which, dtype):
    """the slab and the summing launch against the same inputs cut so that one chunk results: slices of `threads` queries per
    polyline, run one at a time, the point gradients summed in float64.  (f32 and f64 only: a half-type launch rounds its
    row once, the sum of twenty such launches twenty times.)"""
    row = pc.CASES[which]
    pl = pc.assert_regime(which, dtype)
    assert pl.chunks > 1 and pc.plan(row.batch, row.P, pl.threads, row.D, dtype).chunks == 1
    relative = pc.relatives(which, dtype)[-1]
    p, fr, ps, qs = pc.inputs(which, relative)
    pd, fd = p.to(dtype).to(DEV), fr.to(dtype).to(DEV)
    g = pg._gout((row.batch, row.Q, row.D), 3, dtype).to(DEV)
    gl = pg._gout((row.batch,), 4, dtype).to(DEV)
    gp, gd = pc.api_grads(pd, fd, ps, qs, relative, g, gl)
    sp, sd = pc.sliced_grads(pd, fd, ps, qs, relative, g, gl, pl.threads)
    rtol, afrac = _grad_tolerance(dtype)
    pg._check(gp, sp, rtol, afrac, f"{which} grad points, chunked against sliced")
    pg._check(gd, sd, rtol, afrac, f"{which} grad distances, chunked against sliced")
    if ps is not None:
        for b in range(row.batch):
            if int(ps[b]) == 0:       # an empty polyline: zero from every chunk, and from every slice
                assert pc.bitwise_zero(gp[b]) and pc.bitwise_zero(sp[b]) and pc.bitwise_zero(gd[b])


# ---------------------------------------------------------------------------------------------------------- guard bands
def _carved(shape, dtype, offset=0):
    """gb._inside with the buffer NaN-filled: (buffer, view, start, count)"""
    buf, view, start, n = gb._inside(shape, dtype=dtype, pad=256, offset=offset)
    buf.fill_(NAN)
    return buf, view, start, n


def _margins_are_nan(buf, start, n):
    return bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + n:]).all())


@pytest.mark.parametrize("which,dtype", pc.RUNS, ids=pc.RUN_IDS)
def test_outputs_and_workspace_stay_inside_their_extent(which, dtype):
    """the C entry points writing into outputs, scratch and workspace carved out of NaN-filled buffers (the outputs one
    element off their alignment): every live element is written, nothing outside the extents changes"""
    from accvlab import _amd_native as nat

    row = pc.CASES[which]
    pl = pc.assert_regime(which, dtype)
    relative = pc.relatives(which, dtype)[-1]
    p, fr, ps, qs = pc.inputs(which, relative)
    pd, fd = p.to(dtype).to(DEV), fr.to(dtype).to(DEV)
    B, P, Q, D = row.batch, row.P, row.Q, row.D
    code, lib, stream = pc.CODE[dtype], nat.lib(), nat.stream_ptr(torch.device(DEV, 0))
    psd, qsd = _dev(ps), _dev(qs)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    sb, wb = pc.entry_points(B, P, Q, D, dtype)
    out_b = _carved((B, Q, D), dtype, offset=1)
    len_b = _carved((B,), dtype, offset=1)
    scr_b = _carved((max(sb // 4, 1),), torch.float32)
    nat.check(lib.accv_polyline_sample(pd.data_ptr(), fd.data_ptr(), ptr(psd), ptr(qsd), out_b[1].data_ptr(), len_b[1].data_ptr(),
                                       B, P, Q, D, code, 1, int(relative), scr_b[1].data_ptr() if sb else None, sb, stream),
              "polyline")
    torch.cuda.synchronize()
    ref_out, ref_len = pc.forward(pd, fd, ps, qs, relative)
    live = pc.live_mask(qs, B, Q, DEV)
    assert torch.equal(out_b[1][live].view(torch.uint8), ref_out[live].view(torch.uint8))
    assert torch.equal(len_b[1].view(torch.uint8), ref_len.view(torch.uint8))
    for buf, _, start, n in (out_b, len_b, scr_b):
        assert _margins_are_nan(buf, start, n), "the sampler wrote outside an extent"
    if sb == 0:
        assert bool(torch.isnan(scr_b[1]).all())
    # backward
    g = pg._gout((B, Q, D), 5, dtype).to(DEV)
    # (the half types without the lengths' term: autograd adds the two operators' gradients in the type, three roundings
    # where this one launch has one)
    gl = None if dtype in pc.HALF else pg._gout((B,), 6, dtype).to(DEV)
    gp_b = _carved((B, P, D), dtype, offset=1)
    gd_b = _carved((B, Q), dtype, offset=1)
    ws_b = _carved((max(wb // 4, 1),), torch.float32)
    assert wb % 256 == 0 and ws_b[1].data_ptr() % 256 == 0
    nat.check(lib.accv_polyline_grad(pd.data_ptr(), fd.data_ptr(), ptr(psd), ptr(qsd), g.data_ptr(), ptr(gl),
                                     gp_b[1].data_ptr(), gd_b[1].data_ptr(), B, P, Q, D, code, 1, int(relative),
                                     ws_b[1].data_ptr() if wb else None, wb, stream), "polyline backward")
    torch.cuda.synchronize()
    for buf, _, start, n in (gp_b, gd_b, ws_b):
        assert _margins_are_nan(buf, start, n), "the backward wrote outside an extent"
    assert not bool(torch.isnan(gp_b[1]).any()) and not bool(torch.isnan(gd_b[1]).any()), "a gradient element was not written"
    if wb == 0:
        assert bool(torch.isnan(ws_b[1]).all())
    _assert_padding_is_zero(row, gp_b[1], gd_b[1], ps, qs, which)
    ap, ad = pc.api_grads(pd, fd, ps, qs, relative, g, gl)
    rtol, afrac = _grad_tolerance(dtype)
    # (two runs of the same float atomics: the sums may differ in their last bits)
    pg._check(gp_b[1], ap, rtol, afrac, f"{which} carved grad points against the operator's")
    pg._check(gd_b[1], ad, rtol, afrac, f"{which} carved grad distances against the operator's")


# ---------------------------------------------------------------------------------------------------------- group boxes
@pytest.mark.parametrize("which,samples", [("wg256_p2047", 1000), ("wg1024_p2048", 2100)])
def test_group_boxes_of_a_chunked_launch_with_a_partial_last_group(which, samples):
    """sample_lanes with group boxes at a per-lane sample count that is no multiple of 64: the entry point accepts it and
    writes ceil(samples / 64) boxes per lane, the last over the samples there are (1000 = 15 * 64 + 40, four chunks of 256
    at 256 threads; 2100 = 32 * 64 + 52, three chunks of 1024 at 1024 threads).  With boxes the query loop runs whole waves
    to the end of the chunk; the samples are the bits of the launch without boxes."""
    from accvlab.draw_heatmap import sample_lanes

    row = pc.CASES[which]
    pl = pc.assert_plan_matches_library(row.batch, row.P, samples, 2, pc.F32)
    assert pl.fwd_chunks > 1 and pl.threads == row.regimes[pc.F32]["threads"] and samples % 64
    p, _, ps, _ = pc.inputs(which, True)
    lanes = p.float().view(1, row.batch, row.P, 2).to(DEV)
    counts = ps.view(1, row.batch).to(DEV)
    groups = -(-samples // 64)
    box_b = _carved((row.batch * groups, 4), torch.float32)
    assert box_b[1].data_ptr() % 16 == 0
    got = sample_lanes(lanes, samples, num_points=counts, group_boxes_ptr=box_b[1].data_ptr())
    torch.cuda.synchronize()
    plain = sample_lanes(lanes, samples, num_points=counts)
    assert torch.equal(got.view(torch.uint8), plain.view(torch.uint8))
    assert _margins_are_nan(box_b[0], box_b[2], box_b[3]), "the sampler wrote outside the group boxes"
    s = got.view(row.batch, samples, 2)
    pad = torch.full((row.batch, groups * 64 - samples, 2), NAN, device=DEV)
    grp = torch.cat([s, pad], 1).view(row.batch * groups, 64, 2)
    inf = float("inf")
    missing = torch.isnan(grp)                              # an empty lane (NaN samples): (inf, inf, -inf, -inf)
    lo = torch.where(missing, torch.full_like(grp, inf), grp).min(1).values
    hi = torch.where(missing, torch.full_like(grp, -inf), grp).max(1).values
    assert torch.equal(box_b[1], torch.cat([lo, hi], 1))
    for b in range(row.batch):
        assert bool((torch.isnan if int(ps[b]) == 0 else torch.isfinite)(s[b]).all())
