"""The launch plan of csrc/polyline.hip restated in Python (polyline_edges_cases.plan) against the library's two workspace
entry points — on every row of the case table and on a sweep around every threshold — and the host path (CPU tensors) on the
small rows against the float64 definition.  The first keeps the restatement honest, so that the GPU cases of
test_polyline_edges_gpu.py name their regime truthfully; the host path has no regimes and is the second witness there.
Needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import polyline_edges_cases as pc  # noqa: E402
import test_polyline_grad_gpu as pg  # noqa: E402  (a module: its reference and comparison, its tests are not collected here)


@pytest.mark.parametrize("which,dtype", pc.RUNS, ids=pc.RUN_IDS)
def test_every_row_is_in_the_regime_it_names(which, dtype):
    pc.assert_regime(which, dtype)


def test_plan_restatement_equals_the_entry_points_around_every_threshold():
    shapes = pc.sweep_shapes()
    assert len(shapes) > 5000
    for shape in shapes:
        pc.assert_plan_matches_library(*shape)


def test_the_sweep_and_the_table_stand_on_both_sides_of_every_threshold():
    """the sweep would prove nothing if it stayed on one side: every decision of the plan takes both values in it"""
    plans = [pc.plan(*s) for s in pc.sweep_shapes()] + [pc.plan(r.batch, r.P, r.Q, r.D, d) for r in pc.CASES.values()
                                                        for d in r.dtypes]
    for key in ("threads", "spread", "use_scratch", "use_ws"):
        assert len({getattr(p, key) for p in plans}) == 2, key
    assert {p.chunks > 1 for p in plans} == {False, True}
    assert {p.fwd_chunks != p.chunks for p in plans} == {False, True}           # scratch: the forward alone keeps one chunk
    assert {p.chunks > 1 and p.sum_count > pc.K_SUM_GRID for p in plans} == {False, True}   # the summing kernel's second trip
    assert {p.use_ws and p.threads == 256 for p in plans} == {False, True}
    assert pc.plan(2047, 260, 512, 2, pc.F32).sum_count == 1064440


def test_q_chunk_cap_below_int_max_shows_in_the_slab_term():
    assert pc.plan(2048, 30, pc.INT_MAX, 2, pc.F32).chunks == 2 and pc.plan(2048, 30, pc.INT_MAX - 256, 2, pc.F32).chunks == 1
    pc.assert_plan_matches_library(2048, 30, pc.INT_MAX, 2, pc.F32)


def test_refusals_are_decided_before_a_launch():
    """the error returns of the three device entry points: nothing here gets as far as the GPU"""
    import ctypes

    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    d = ctypes.c_void_p(64)
    err = lambda: lib.accv_last_error() or b""  # noqa: E731
    sample = lambda *a: lib.accv_polyline_sample_boxes(*a)  # noqa: E731
    # (points, distances, point counts, query counts, samples, lengths, boxes, B, P, Q, D, dtype, i64, relative, scratch, bytes, stream)
    assert sample(d, d, None, None, d, None, None, -1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"negative" in err()
    assert sample(d, d, None, None, d, None, None, 1, 4, 4, -2, 0, 0, 0, None, 0, None) == -1 and b"negative" in err()
    assert sample(d, d, None, None, d, None, None, 1, 4, 4, 2, 4, 0, 0, None, 0, None) == -1 and b"dtype" in err()
    assert sample(None, d, None, None, d, None, None, 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"null points" in err()
    assert sample(d, None, None, None, d, None, None, 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"null distances" in err()
    for dtype, dims in ((1, 2), (0, 3)):
        assert sample(d, d, None, None, d, None, d, 1, 4, 4, dims, dtype, 0, 0, None, 0, None) == -1 and b"group boxes need float32" in err()
    assert sample(d, d, None, None, None, d, d, 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"group boxes need float32" in err()
    assert sample(d, d, None, None, d, None, ctypes.c_void_p(68), 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"alignment" in err()
    # the scratch path without (enough) scratch
    need = lib.accv_polyline_scratch_bytes(2, 12289, 0)
    assert need == 2 * 12289 * 4
    assert sample(d, d, None, None, d, None, None, 2, 12289, 4, 2, 0, 0, 0, None, 0, None) == -3 and b"scratch" in err()
    assert sample(d, d, None, None, d, None, None, 2, 12289, 4, 2, 0, 0, 0, d, need - 1, None) == -3
    # nothing to do: no error, no launch
    assert sample(None, None, None, None, None, None, None, 0, 4, 4, 2, 0, 0, 0, None, 0, None) == 0
    assert sample(d, d, None, None, None, None, None, 3, 4, 4, 2, 0, 0, 0, None, 0, None) == 0
    grad = lambda *a: lib.accv_polyline_grad(*a)  # noqa: E731
    # (points, distances, counts, counts, grad_out, grad_lengths, grad_points, grad_distances, B, P, Q, D, dtype, i64, relative, ws, bytes, stream)
    assert grad(d, d, None, None, d, None, d, d, 1, -4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"negative" in err()
    assert grad(d, d, None, None, d, None, d, d, 1, 4, 4, 2, -1, 0, 0, None, 0, None) == -1 and b"dtype" in err()
    assert grad(None, d, None, None, d, None, d, d, 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"null points" in err()
    assert grad(d, None, None, None, d, None, d, d, 1, 4, 4, 2, 0, 0, 0, None, 0, None) == -1 and b"null distances" in err()
    need = lib.accv_polyline_grad_workspace_bytes(3, 2047, 600, 2, 0)      # chunked: the slab
    assert need > 0
    assert grad(d, d, None, None, d, None, d, d, 3, 2047, 600, 2, 0, 0, 0, None, 0, None) == -3 and b"workspace" in err()
    assert grad(d, d, None, None, d, None, d, d, 3, 2047, 600, 2, 0, 0, 0, d, need - 1, None) == -3
    assert grad(d, d, None, None, d, None, None, None, 3, 2047, 600, 2, 0, 0, 0, None, 0, None) == 0
    assert grad(None, None, None, None, None, None, d, d, 0, 4, 4, 2, 0, 0, 0, None, 0, None) == 0
    assert lib.accv_polyline_grad_workspace_bytes(-1, 4, 4, 2, 0) == 0 and lib.accv_polyline_grad_workspace_bytes(1, 4, 4, 2, 7) == 0
    assert lib.accv_polyline_scratch_bytes(0, 20000, 0) == 0


HOST_RUNS = [(w, d, r) for w, d in pc.RUNS if pc.CASES[w].host and d in (pc.F32, pc.F64) for r in pc.CASES[w].relative]


@pytest.mark.parametrize("which,dtype,relative", HOST_RUNS, ids=[f"{w}-{pc.name(d)}-{'rel' if r else 'abs'}" for w, d, r in HOST_RUNS])
def test_host_path_meets_the_definition_at_the_edge_shapes(which, dtype, relative):
    row = pc.CASES[which]
    p, fr, ps, qs = pc.inputs(which, relative)
    pd, fd = p.to(dtype), fr.to(dtype)
    what = f"{which} {pc.name(dtype)} host"
    eps = pc.acc_eps(dtype, "cpu")
    ref, ref_lens = pg.ref_sample(pd.double(), fd.double(), ps, relative, eps)
    out, lens = pc.forward(pd, fd, ps, qs, relative)
    pc.check_forward(out, lens, ref, ref_lens, qs, dtype, what)
    g = pg._gout(tuple(out.shape), 1, dtype)
    gl = pg._gout((row.batch,), 2, dtype)
    gp, gd = pc.api_grads(pd, fd, ps, qs, relative, g, gl)
    rp, rd = pg.ref_grads(pd, fd, g, gl, ps, qs, relative, eps=eps)
    rtol, afrac = (1e-9, 1e-12) if dtype == pc.F64 else (1e-4, 1e-6)
    pg._check(gp, rp, rtol, afrac, f"{what} grad points")
    pg._check(gd, rd, rtol, afrac, f"{what} grad distances")
    if ps is not None:
        for b in range(row.batch):
            assert pc.bitwise_zero(gp[b, int(ps[b]):]) and pc.bitwise_zero(gd[b, int(qs[b]) if int(ps[b]) else 0:])


@pytest.mark.parametrize("which", ["wg256_p2047", "chunk_borders"])
@pytest.mark.parametrize("relative", [False, True])
def test_float64_definition_agrees_with_the_oracle(which, relative):
    """the reference the edge cases are compared with (test_polyline_grad_gpu.ref_sample) against oracle/lane.py, which is
    pinned to the reference implementation's own vectors"""
    from oracle import lane as oracle

    p, fr, ps, qs = pc.inputs(which, relative)
    ref, ref_lens = pg.ref_sample(p, fr, ps, relative)
    for b in range(p.shape[0]):
        n, q = int(ps[b]), int(qs[b])
        want = oracle.sample(p[b, :n].numpy(), fr[b, :q].numpy(), relative=relative)
        assert np.allclose(ref[b, :q].numpy(), want, atol=1e-9, rtol=0, equal_nan=True)
        assert np.allclose(float(ref_lens[b]), oracle.length(p[b, :n].numpy()), atol=0, rtol=0, equal_nan=True)
