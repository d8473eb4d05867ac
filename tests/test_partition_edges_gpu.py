"""The loss-side kernels at the edges of their own work partition: deterministic shapes derived from the constants of the
``.hip`` files (DESIGN.md §9k lists every host-side geometry decision and shape-dependent device loop next to the test that
crosses it).  Every case is compared with the operator's float64 definition at the tolerance its own test file states, and
with the host path where there is one; nothing here adds or changes a tolerance.  A case asserts the regime it names through
the workspace entry points (partition_edges_cases.py) or, where no entry shows it, documents the arithmetic at the shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import center_regression_cases as cr  # noqa: E402
import matched_box_loss_cases as mb  # noqa: E402
import matched_focal_loss_cases as mf  # noqa: E402
import matching_cost_cases as mc  # noqa: E402
import partition_edges_cases as pe  # noqa: E402
# the device-and-host comparisons of the operators' own GPU test files (modules, so that their tests are not collected here)
import test_center_regression_gpu as crg  # noqa: E402
import test_heatmap_loss_gpu as hlg  # noqa: E402
import test_heatmap_peaks_gpu as hpg  # noqa: E402
import test_matched_box_loss_gpu as mbg  # noqa: E402
import test_matched_focal_loss_gpu as mfg  # noqa: E402
import test_matching_cost_gpu as mcg  # noqa: E402

from accvlab.batching_helpers import matched_box_loss as mbl  # noqa: E402
from accvlab.batching_helpers import matched_focal_loss as mfl  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------ matched_focal_loss
FOCAL_RUNS = [(which, dtype) for which in pe.FOCAL for dtype in pe.FOCAL[which][5]]


@pytest.mark.parametrize("which,dtype", FOCAL_RUNS, ids=[f"{w}-{pe.name(d)}" for w, d in FOCAL_RUNS])
def test_matched_focal_loss_partition_edges(which, dtype):
    B, Q, C, nqb, qpb, _ = pe.FOCAL[which]
    pe.assert_focal_partition(B, Q, C, nqb, qpb)
    inp, go, notes = pe.focal_case(which, dtype, device=DEV)
    logits, labels, pind, gind, w = inp
    out, grad = mfg.compare(inp, f"{which} {pe.name(dtype)}", grad_out=go)
    if which == "more_than_1024_frames":
        # the default denominator (in `compare` against the definition's) is the number of pairs the finish kernel
        # counts over all 1030 frames: the same bits as with that number given
        factor = float(sum(b % 3 for b in range(B)))
        fixed = mf.run(mfl, logits, labels, pind, gind, grad_out=go.to(DEV), query_weights=w, avg_factor=factor)
        assert torch.equal(mf.bits(out), mf.bits(fixed[0])) and torch.equal(mf.bits(grad), mf.bits(fixed[1]))
    if "twice" in notes:
        # slot 3 (first trip of the slot loop) owns the query, whatever slot 290 (second trip) says
        b, q, first, later, slot = notes["twice"]
        assert float(grad[b, q, first]) < 0 < float(grad[b, q, later])
        other = mf.run(mfl, logits, labels, pind, pe.say_something_else(gind, b, slot, 300), grad_out=go.to(DEV),
                       query_weights=w)
        assert torch.equal(mf.bits(out), mf.bits(other[0])) and torch.equal(mf.bits(grad), mf.bits(other[1]))


# -------------------------------------------------------------------------------------------------------- matched_box_loss
BOX_RUNS = [(which, dtype, kind) for which in pe.BOX for dtype, kind in pe.BOX_RUNS]


@pytest.mark.parametrize("which,dtype,kind", BOX_RUNS, ids=[f"{w}-{pe.name(d)}-{k}" for w, d, k in BOX_RUNS])
def test_matched_box_loss_partition_edges(which, dtype, kind):
    B, Q, D, nqb = pe.BOX[which]
    pe.assert_box_partition(B, Q, D, nqb)
    inp, go, notes = pe.box_case(which, dtype, device=DEV)
    out, grad = mbg.compare(inp, f"{which} {pe.name(dtype)} {kind}", grad_out=go, box_format="cxcywh", iou_kind=kind)
    if "twice" in notes:
        b, q, slot = notes["twice"]
        boxes, gt, pind, gind, w = inp
        other = mb.run(mbl, boxes, gt, pind, pe.say_something_else(gind, b, slot, 300), grad_out=go, query_weights=w,
                       box_format="cxcywh", iou_kind=kind)
        assert bool((grad[b, q] != 0).any())
        assert torch.equal(mb.bits(out), mb.bits(other[0])) and torch.equal(mb.bits(grad), mb.bits(other[1]))


# ------------------------------------------------------------------------------------------------------- centre regression
# band_geometry() of csrc/center_regression.hip, with row_bytes = W * esize * C:
#   lo = ceil(16384 / row_bytes), hi = max(65536 / row_bytes, lo), rows = clamp(H * B / 2048, lo, hi),
#   band_rows = min(rows, H), bands = ceil(H / band_rows).
# There is no entry point that shows the bands: the arithmetic of every shape is written out next to it.
def _points(xy, b, pts):
    if pts:
        xy[b, :len(pts)] = torch.tensor(pts, dtype=torch.int32)


def _row_per_band():
    # f32: row_bytes = 1924 * 4 * 9 = 69264 > 65536 -> lo = 1, hi = max(0, 1) = 1, rows = 1: five bands of one row
    B, N, H, W, channels, sizes = 2, 8, 5, 1924, [2, 3, 4], [8, 3]
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=41)
    _points(xy, 0, [(0, 0), (1923, 0), (5, 4), (1923, 4), (700, 2), (700, 2), (0, 4)])   # rows 0 and 4; two objects on a cell
    _points(xy, 1, [(1923, 4), (0, 0), (700, 2)])
    return B, N, H, W, channels, sizes, xy


def _rows_between_lo_and_hi():
    # f32: row_bytes = 64 * 4 * 1 = 256 -> lo = 64, hi = 256, H * B / 2048 = 134400 / 2048 = 65: lo < 65 < hi.
    # bands = ceil(2100 / 65) = 33; bands 1 and 2 are rows [65, 130) and [130, 195); the last band [2080, 2100) has 20 rows
    B, N, H, W, channels = 64, 8, 2100, 64, [1]
    sizes = [(8, 0, 4, 8)[b % 4] for b in range(B)]
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=42)
    for b in range(B):
        _points(xy, b, [(b, 65), (63 - b, 129), (b, 130), (63 - b, 194), (0, 2080), (63, 2099), (b, 0), (b, 64)][:sizes[b]])
    return B, N, H, W, channels, sizes, xy


def _rows_clamped_to_hi():
    # f32: row_bytes = 64 * 4 * 16 = 4096 -> lo = 4, hi = 16, H * B / 2048 = 35200 / 2048 = 17 > hi: bands of 16 rows,
    # 138 of them, the last [2192, 2200) of 8 rows
    B, N, H, W, channels = 16, 6, 2200, 64, [16]
    sizes = [(6, 0, 3)[b % 3] for b in range(B)]
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=46)
    for b in range(B):
        _points(xy, b, [(b, 15), (63 - b, 16), (b, 2192), (b, 2199), (0, 31), (63, 32)][:sizes[b]])
    return B, N, H, W, channels, sizes, xy


def _band_rows_clamped_to_h():
    # row_bytes = 40 * esize * 2 = 320 (f32) / 160 (bf16) -> lo = 52 / 103 > H = 3: band_rows = H, one band per frame
    B, N, H, W, channels, sizes = 3, 5, 3, 40, [2], [5, 0, 2]
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=43)
    _points(xy, 0, [(0, 0), (39, 2), (39, 0), (0, 2)])
    return B, N, H, W, channels, sizes, xy


def _more_than_256_frames():
    # loss_finish_kernel walks the 300 per-frame partials with i += 256: a second trip.  One band per frame (lo >= 512 > H)
    B, N, H, W, channels = 300, 2, 4, 4, [2]
    sizes = [b % 3 for b in range(B)]
    return B, N, H, W, channels, sizes, cr.make_centers(B, N, H, W, sizes, "cpu", seed=44)


def _slot_loops_across_a_trip():
    # 600 and 257 slots: the cull loop of the scatter kernel (base += 256) takes 3 and 2 trips, the loss kernel's lane loop
    # 600 * 3 / 256.  f32: row_bytes = 768 -> lo = 22, rows = 22: bands of 22, 22 and 20 rows, each with fewer slots than
    # the 2048 its list holds.  Cells named by slots on both sides of 256:
    B, N, H, W, channels, sizes = 2, 600, 64, 64, [3], [600, 257]
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=45, wild_padding=True)
    for n in (3, 250, 256, 300, 599):
        xy[0, n] = torch.tensor([10, 20], dtype=torch.int32)
    for n in (255, 257):
        xy[0, n] = torch.tensor([63, 63], dtype=torch.int32)
    for n in (255, 256):
        xy[1, n] = torch.tensor([33, 7], dtype=torch.int32)
    return B, N, H, W, channels, sizes, xy


CENTER = {
    "row_per_band": (_row_per_band, [torch.float32]),
    "rows_between_lo_and_hi": (_rows_between_lo_and_hi, [torch.float32]),
    "rows_clamped_to_hi": (_rows_clamped_to_hi, [torch.float32]),
    "band_rows_clamped_to_h": (_band_rows_clamped_to_h, [torch.float32, torch.bfloat16]),
    "more_than_256_frames": (_more_than_256_frames, [torch.float32, torch.bfloat16]),
    "slot_loops_across_a_trip": (_slot_loops_across_a_trip, [torch.float32, torch.bfloat16]),
}
CENTER_RUNS = [(which, dtype, kind) for which in CENTER for dtype in CENTER[which][1] for kind in ("l1", "smooth_l1")]


def _center_inputs(which, dtype, spread=False):
    B, N, H, W, channels, sizes, xy = CENTER[which][0]()
    C = sum(channels)
    maps = cr.make_maps(B, channels, H, W, dtype, DEV, seed=B + H)
    g = torch.Generator().manual_seed(B + W)
    targets = torch.randn(B, N, C, generator=g) * 3.0
    # spread: weights over orders of magnitude, so that the order of a sum shows in its last bits
    weights = torch.exp(torch.randn(B, N, generator=g) * 3.0) if spread else torch.rand(B, N, generator=g) + 0.25
    upstream = (torch.randn(B, N, C, generator=g) * (torch.exp(torch.randn(B, N, 1, generator=g) * 3.0) if spread else 1.0))
    return maps, xy, torch.as_tensor(sizes), targets, weights, upstream.to(dtype), channels


def _report(what, got, ref):
    err = (got.double() - ref).abs()
    print(f"{what}: max error {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")


@pytest.mark.parametrize("which,dtype,kind", CENTER_RUNS, ids=[f"{w}-{pe.name(d)}-{k}" for w, d, k in CENTER_RUNS])
def test_center_regression_partition_edges(which, dtype, kind):
    """gather and its backward, the loss and its backward against the float64 oracle, and the complete write of the loss
    backward into NaN-filled gradient maps carved out of larger buffers off their alignment"""
    from accvlab.draw_heatmap import gather_at_centers

    maps, xy, sizes, targets, weights, upstream, channels = _center_inputs(which, dtype)
    xy, sizes, targets, weights, upstream = (t.to(DEV) for t in (xy, sizes, targets, weights, upstream))
    H, W = maps[0].shape[2:]
    centers = cr.ragged(xy, sizes.cpu())
    valid, ind = cr.valid_and_index(xy, sizes, H, W)
    assert int(valid.sum()) > 0
    what = f"{which} {pe.name(dtype)} {kind}"
    # gather, and the scatter of its backward
    leaves = [m.detach().requires_grad_(True) for m in maps]
    rows = gather_at_centers(leaves if len(leaves) > 1 else leaves[0], centers).tensor
    assert torch.equal(rows, cr.oracle_gather(maps, xy, sizes).to(dtype))
    rows.backward(upstream)
    f = torch.cat([m.detach().double() for m in maps], 1).requires_grad_(True)
    (cr._gather(f, valid, ind) * upstream.double()).sum().backward()
    for i, (leaf, ref) in enumerate(zip(leaves, f.grad.split(channels, 1))):
        _report(f"{what} gather backward map {i}", leaf.grad, ref)
        cr.assert_grad_close(leaf.grad, ref, dtype, f"gather backward map {i}")
    # loss and its backward
    loss, grads = crg.run_loss(maps, centers, targets, weights, kind=kind, beta=1.3, grad_out=0.75)
    ref, ref_grads = cr.oracle_loss(maps, xy, sizes, targets, weights, kind, 1.3, grad_out=0.75)
    print(f"{what} loss: relative error {abs(float(loss) - float(ref)) / abs(float(ref)):.3e} (bound 1e-05)")
    assert float(ref) > 0
    cr.assert_loss_close(loss, ref, what)
    for i, (a, b) in enumerate(zip(grads, ref_grads)):
        assert int(torch.count_nonzero(b)) > 0
        _report(f"{what} loss backward map {i}", a, b)
        cr.assert_grad_close(a, b, dtype, f"loss backward map {i}")
    # the complete write
    denom = valid.sum().clamp(min=1).float()
    carved = [crg._inside(m.shape, dtype, NAN, offset=1) for m in maps]
    crg._direct_loss_bwd(maps, [c[1] for c in carved], xy, sizes, targets, weights, kind, 1.3,
                         torch.full((), 0.75, device=DEV), denom)
    torch.cuda.synchronize()
    for (buf, view, start, n), want in zip(carved, grads):
        assert not bool(torch.isnan(view).any()), "an element of the gradient was not written"
        assert torch.equal(view, want)
        assert crg._margins_hold(buf, start, n, NAN), "wrote outside the gradient map"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=pe.name)
def test_center_regression_slot_order_across_the_slot_loop_trip(dtype):
    """cells named by slots below and above 256 (and many random pairs among 600 slots on 4096 cells): the gradient of a
    cell is the f32 sum of its slots' contributions in ascending slot order, rounded once — for the loss backward
    ((w * sign(d)) * (grad_out / denom), as test_duplicates_add_in_slot_order) and for the rows of the gather backward"""
    from accvlab.draw_heatmap import gather_at_centers

    maps, xy, sizes, targets, weights, upstream, channels = _center_inputs("slot_loops_across_a_trip", dtype, spread=True)
    B, N = xy.shape[:2]
    C, H, W = maps[0].shape[1:]
    avg, go = 3.0, 0.7
    centers = cr.ragged(xy.to(DEV), sizes)
    _, grads = crg.run_loss(maps, centers, targets.to(DEV), weights.to(DEV), avg_factor=avg,
                            grad_out=torch.tensor(go, device=DEV))
    leaf = maps[0].detach().requires_grad_(True)
    gather_at_centers(leaf, centers).tensor.backward(upstream.to(DEV))
    x = maps[0].float().cpu().numpy()
    t, w, up = targets.numpy(), weights.numpy(), upstream.float().numpy()
    scale = np.float32(go) / np.float32(avg)
    want = np.zeros((B, C, H, W), np.float32)
    want_rows = np.zeros((B, C, H, W), np.float32)
    shared = 0
    for b in range(B):
        seen = set()
        for n in range(int(sizes[b])):
            cx, cy = int(xy[b, n, 0]), int(xy[b, n, 1])
            shared += (cx, cy) in seen
            seen.add((cx, cy))
            for c in range(C):
                d = np.float32(x[b, c, cy, cx]) - np.float32(t[b, n, c])
                v = np.float32(np.float32(w[b, n]) * np.float32(np.sign(d))) * scale
                want[b, c, cy, cx] = np.float32(want[b, c, cy, cx] + v)
                want_rows[b, c, cy, cx] = np.float32(want_rows[b, c, cy, cx] + np.float32(up[b, n, c]))
    assert shared > 8
    assert torch.equal(grads[0].cpu(), torch.from_numpy(want).to(dtype))
    assert torch.equal(leaf.grad.cpu(), torch.from_numpy(want_rows).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=pe.name)
def test_gather_grid_stride_second_trip(dtype):
    """accv_gather_at_centers launches ceil(B * N * C / 256) workgroups, at most 8192: above 8192 * 256 = 2097152 output
    elements the kernel's grid-stride loop takes a second trip.  B * N * C = 2 * 16400 * 64 = 2099200.  (Forward only: that
    many slots on one band would put the backward on its quadratic path for thousands of slots.)"""
    from accvlab.draw_heatmap import gather_at_centers

    B, N, H, W, channels = 2, 16400, 8, 8, [32, 31, 1]
    assert 8192 * 256 < B * N * sum(channels) < 2 * 8192 * 256
    sizes = torch.tensor([N, N - 300])
    maps = cr.make_maps(B, channels, H, W, dtype, DEV, seed=7)
    xy = cr.make_centers(B, N, H, W, sizes, DEV, seed=7, margin=1)
    got = gather_at_centers(maps, cr.ragged(xy, sizes)).tensor
    assert torch.equal(got, cr.oracle_gather(maps, xy, sizes.to(DEV)).to(dtype))
    assert int(torch.count_nonzero(got[1, N - 300:])) == 0 and int(torch.count_nonzero(got[:, -400:])) > 0


# ---------------------------------------------------------------------------------------------------------- matching cost
@pytest.mark.parametrize("G", [64, 65, 128, 129, 256, 257])
def test_matching_cost_column_tile_boundaries(G):
    """launch() of csrc/matching_cost.hip picks a tile of 64, 128 or 256 columns at G <= 64, <= 128 and above, with 32, 16
    or 8 queries per workgroup; G = 257 adds a second column tile of one column.  Q = 33 leaves a last query block of one
    row at every tile size (33 = 32 + 1 = 2 * 16 + 1 = 4 * 8 + 1)."""
    kw, D = mc.term_kwargs("one_minus_prob", "l1_iou_giou_cxcywh")
    inp = mc.make_case(2, 33, 5, [G, G - 1], "one_minus_prob", D, kw["box_format"], torch.float32, seed=G, device=mcg.DEV)
    mcg.check_against_host(inp, kw, torch.float32, f"G {G}")


# ---------------------------------------------------------------------------------------------------- Gaussian focal loss
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (1, 4097, 4099)), (torch.bfloat16, (1, 5793, 5795))],
                         ids=["float32", "bfloat16"])
def test_gaussian_focal_loss_grid_caps(dtype, shape):
    """csrc/heatmap_loss.hip: the forward grid is capped at kMaxBlocks = 2048 workgroups above 2048 * 2048 elements (the
    grid-stride loop then takes several trips, the finish kernel's i += 256 eight); the backward grid at 4 * kMaxBlocks
    workgroups of 2 * 256 vectors, that is above 8192 * 2048 f32 or 8192 * 4096 bf16 elements.  Both sizes are odd, so
    the last vector is followed by a scalar tail."""
    from accvlab import _amd_native as nat

    numel = shape[0] * shape[1] * shape[2]
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    assert nat.ctypes_lib().accv_gaussian_focal_loss_workspace_bytes(numel) == 2048 * 16   # the forward cap
    assert nat.ctypes_lib().accv_gaussian_focal_loss_workspace_bytes(2048 * 2048) == 2048 * 16
    assert nat.ctypes_lib().accv_gaussian_focal_loss_workspace_bytes(2047 * 2048) == 2047 * 16
    assert 8192 * 256 * vec * 2 < numel < 2 * 8192 * 256 * vec * 2 and numel % vec   # the backward cap, second trip, tail
    target = hlg.drawn_target(shape, seed=shape[1])
    logits = hlg.random_logits(shape, dtype, seed=shape[2])
    loss, g = hlg.fused(logits, target)
    ref, g64 = hlg.composition(logits, target)
    print(f"{pe.name(dtype)} loss: relative error {abs(float(loss) - float(ref)) / abs(float(ref)):.3e} (bound 1e-05)")
    _report(f"{pe.name(dtype)} gradient", g, g64)
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    hlg.assert_grad_close(g, g64, dtype)


# ---------------------------------------------------------------------------------------------------------- heat-map peaks
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=pe.name)
def test_heatmap_peaks_middle_column_tile_and_candidate_loop_trip(dtype):
    """geometry() of csrc/heatmap_peaks.hip at H x W = 5 x 4100: column tiles of 2048, 2048 and 4 columns, two rows per
    chunk and a last chunk row of one.  The middle tile has a halo on both sides: with kernel 7 its 2 x (2048 + 6) values
    fill the LDS tile (kTileElems) to the last element.  Nine chunks x k = 1024 candidates are more than the 8192 the group
    kernel reads per trip of its candidate loop."""
    from accvlab import _amd_native as nat

    shape = (1, 1, 5, 4100)
    assert nat.ctypes_lib().accv_heatmap_peaks_workspace_bytes(*shape, 1024) == 3 * 3 * 1024 * 8
    heat = hpg.seeded(shape, dtype, seed=4100)
    # the largest value of the map lies in the last chunk (row 4 of the 4-column tile), whose candidates are the ones the
    # second trip reads; the second largest in the middle tile's last column, next to the halo and four rows away (outside
    # the 7 x 7 window of the first)
    heat[0, 0, 4, 4098] = 9.0
    heat[0, 0, 0, 4095] = 8.0
    for kernel in (3, 7):
        for k in (7, 1024):
            got = hpg.assert_matches(heat, k, kernel=kernel)
            assert got.scores[0, :2].tolist() == [9.0, 8.0] and got.indices[0, :2].tolist() == [4 * 4100 + 4098, 4095]
