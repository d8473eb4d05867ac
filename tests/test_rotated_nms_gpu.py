"""rotated_nms_bev and rotated_iou_bev on the GPU: the kernels against the float64 world-coordinate definition of
rotated_nms_cases.py and against the host entries, at the edges of their work partition (wave block, chunk of kThreads slots,
IoU tile, the two cuts), keep decisions ON the threshold across those edges, guard bands, reproducibility, graph capture, no
host synchronisation, a non-default stream, and the path heatmap_peaks -> center_point_decode -> rotated_nms_bev; the
hard-geometry families of rotated_iou_hard_cases.py against the definition and the host.  The largest IoU error seen against
the definition, per case, goes to profiles/rotated_nms_accuracy.log."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rotated_nms_cases import (BAR, BEV, BIG, CHAIN, CHAIN_THR, SMALL, Case, assert_margin, check, definition, iou64, kept_slots,  # noqa: E402
                               make_case, pick_threshold, placed_case, ragged5, random_boxes, share)

import rotated_iou_hard_cases as hard  # noqa: E402

from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import (CenterPointDetections, center_point_decode, gather_at_centers, heatmap_peaks, rotated_iou_bev,  # noqa: E402
                                  rotated_nms_bev)

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = rotated_nms_bev


def _constant(text, ident):
    return re.search(rf"constexpr \w+ {ident} = ([^;]+);", text).group(1)


_SRC = open(os.path.join(ROOT, "accv-lab_amd", "csrc", "rotated_nms.hip")).read()
WAVE = int(_constant(_SRC, "kWave"))
THREADS = int(_constant(_SRC, "kThreads"))          # slots per chunk
TILE = int(_constant(_SRC, "kTile"))
assert (WAVE, THREADS, TILE) == (64, 256, 64)
BELOW = float(np.nextafter(np.float32(0.25), np.float32(0)))
# comparisons of rotated_iou_bev with the definition in this module: four matrix shapes, three box kinds and the families of
# rotated_iou_hard_cases.py
IOU_CASES = 7 + len(hard.NAMES)


def both(case, thr, what="", **kw):
    """`case` lives on the host: the device against the definition, and against the host path on the same inputs"""
    thr_list = thr if isinstance(thr, list) else [thr] * len(case.tasks)
    if kw.pop("margin", True):       # off only where a test puts a pair ON the threshold, with exact arithmetic
        assert_margin(case, thr_list)
    got = op(case.to(DEV).detections(), thr, **kw)
    assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for r in got for x in r)
    want = definition(case, thr_list, kw.get("pre_max_size"), kw.get("post_max_size"))
    check(got, want, case, what + " device")
    host = op(case.detections(), thr, **kw)
    for t, (d, h) in enumerate(zip(got, host)):
        assert torch.equal(d.boxes.sample_sizes.cpu(), h.boxes.sample_sizes), f"{what} task {t}: sizes, device against host"
        for x, y in zip(d, h):
            assert torch.equal(x.tensor.cpu().view(torch.uint8), y.tensor.view(torch.uint8)), f"{what} task {t}: device against host"
    return got, want


# ---------------------------------------------------------------------------------------------------------- accuracy log
@pytest.fixture(scope="module")
def accuracy():
    """every IoU comparison of this module records its largest error here; written out once the module is through"""
    seen = []
    yield seen
    if len(seen) < IOU_CASES:      # a partial run (-k, -x) must not leave a log that covers a subset
        return
    worst = max(e for _, _, _, e in seen)
    lines = [f"rotated_iou_bev on {torch.cuda.get_device_name(0)}: largest absolute IoU error against the float64 world-coordinate "
             f"definition (tests/rotated_nms_cases.py), bar {BAR:g}"]
    lines += [f"  {name}: {pairs} pairs, {over} overlapping, max abs err {err:.3e}" for name, pairs, over, err in seen]
    lines.append(f"max over all cases: {worst:.3e}")
    try:
        with open(os.path.join(ROOT, "profiles", "rotated_nms_accuracy.log"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:      # a read-only checkout: the figures were asserted all the same
        pass


# --------------------------------------------------------------------------------------------- the kernel's work partition
@pytest.mark.parametrize("D", [7, 9])
@pytest.mark.parametrize("B", [0, 1, 3])
@pytest.mark.parametrize("N", [1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1, 1024])
def test_slot_counts_across_wave_blocks_and_chunks(N, B, D):
    case = make_case(B, N, 3, D, seed=1)
    thr = [pick_threshold(case, 0, 0.2), None, pick_threshold(case, 2, 0.5)]
    got, want = both(case, thr, f"B={B} N={N} D={D}")
    assert all(r.boxes.tensor.shape == (B, N, D) for r in got)
    if B and N >= WAVE - 1:
        kept, dead, total = share(want, case, thr)
        assert kept >= total / 10 and dead >= total / 10, f"the case shows nothing: {kept} kept, {dead} suppressed of {total}"


# ------------------------------------------------------------------------------------------- decisions across boundaries
@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_iou_equal_to_the_threshold_keeps_and_one_ulp_below_suppresses_across_a_boundary(edge):
    N = edge + WAVE
    for first, second in ((BIG, SMALL), (SMALL, BIG)):
        case = placed_case(N, {edge - 1: first, edge: second})
        got, _ = both(case, 0.25, "equal", margin=False)
        assert kept_slots(got) == list(range(N))
        got, _ = both(case, BELOW, "one ulp below", margin=False)
        assert kept_slots(got) == [k for k in range(N) if k != edge]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
@pytest.mark.parametrize("first", [-2, -1])
def test_a_suppressed_box_suppresses_nothing_across_a_boundary(first, edge):
    """A kills B, only B would kill C: C survives — with A and B before the boundary and C behind it, and with only A before it"""
    N = edge + WAVE
    a = edge + first
    case = placed_case(N, {a: CHAIN[0], a + 1: CHAIN[1], a + 2: CHAIN[2]})
    got, _ = both(case, CHAIN_THR, "chain")
    assert kept_slots(got) == [k for k in range(N) if k != a + 1]


@pytest.mark.parametrize("edge", [WAVE, THREADS])
def test_a_degenerate_box_between_two_overlapping_ones_suppresses_nothing(edge):
    N = edge + WAVE
    flat = (CHAIN[1][0], CHAIN[1][1], 4.0, 0.0, 0.0)
    nan = (CHAIN[1][0], CHAIN[1][1], 4.0, 2.0, float("nan"))
    for bad in (flat, nan):
        case = placed_case(N, {edge - 1: CHAIN[0], edge: bad, edge + 1: CHAIN[2]})
        got, _ = both(case, CHAIN_THR, "degenerate between")
        assert kept_slots(got) == list(range(N))
    case = placed_case(N, {edge - 1: BIG, edge: (BIG[0], BIG[1], -1.0, 4.0, 0.0), edge + 1: SMALL})
    got, _ = both(case, 0.2, "degenerate between a pair")
    assert kept_slots(got) == [k for k in range(N) if k != edge + 1]


@pytest.mark.parametrize("N", [WAVE + 1, THREADS + 1, 1024])
def test_identical_boxes_leave_one_survivor(N):
    box = (-50.0, -60.0, 4.5, 1.9, 0.7)
    case = placed_case(N, {k: box for k in range(N)})
    got, _ = both(case, 0.2, "identical", margin=False)
    assert kept_slots(got) == [0]
    got, _ = both(case, float(np.nextafter(np.float32(1), np.float32(0))), "identical, threshold below one", margin=False)
    assert kept_slots(got) == [0]
    got, _ = both(case, 1.0, "identical, threshold one", margin=False)        # iou = 1 is not > 1
    assert kept_slots(got) == list(range(N))


@pytest.mark.parametrize("cut", [1, WAVE - 1, WAVE, WAVE + 1, 2000])
def test_the_two_cuts_at_the_edges_of_a_wave_block(cut):
    N = 2 * THREADS + 9
    case = make_case(3, N, 2, 9, seed=17)
    thr = [pick_threshold(case, 0, 0.2), pick_threshold(case, 1, 0.3)]
    M = min(N, cut)
    got, want = both(case, thr, f"post_max_size={cut}", post_max_size=cut)
    assert all(r.boxes.tensor.shape == (3, M, 9) for r in got)
    if 1 < cut <= WAVE + 1:
        assert (want[0]["sizes"] == M).all() and all(k[M - 1] > M - 1 for k in want[0]["kept"]), "the cut falls on a slot: it shows nothing"
    got, want = both(case, thr, f"pre_max_size={cut}", pre_max_size=cut)
    assert all(r.boxes.tensor.shape == (3, M, 9) for r in got)
    both(case, thr, f"pre_max_size={cut} post_max_size=40", pre_max_size=cut, post_max_size=40)


def test_per_task_thresholds_and_tasks_do_not_see_each_others_boxes():
    N = THREADS + 2
    case = placed_case(N, {THREADS - 1: BIG, THREADS: SMALL}, T=3)
    got, _ = both(case, [0.2, 0.3, None], "per task")
    assert kept_slots(got, 0) == [k for k in range(N) if k != THREADS]
    assert kept_slots(got, 1) == list(range(N)) and kept_slots(got, 2) == list(range(N))


# ---------------------------------------------------------------------------------------------------- the IoU operator
def _iou_inputs(Na, Nb, B=3, seed=0):
    rng = np.random.default_rng(seed + Na)
    boxes = np.stack([random_boxes(rng, Na + Nb, f) for f in range(B)])
    sizes_a = [Na, 0, max(Na - 3, 1)][:B]
    sizes_b = [Nb, Nb // 2, 0][:B]
    return boxes[:, :Na].copy(), boxes[:, Na:].copy(), sizes_a, sizes_b


def _iou_want(a, b, sizes_a, sizes_b):
    want = np.zeros((a.shape[0], a.shape[1], b.shape[1]))
    for f, (na, nb) in enumerate(zip(sizes_a, sizes_b)):
        want[f, :na, :nb] = iou64(a[f, :na], b[f, :nb])
    return want


@pytest.mark.parametrize("Na,Nb", [(1, 1), (WAVE - 1, WAVE + 1), (TILE, TILE), (130, 257)])
def test_iou_matrix_against_the_definition_with_ragged_sizes_and_guard_bands(Na, Nb, accuracy):
    from accvlab import _amd_native as nat

    a, b, sizes_a, sizes_b = _iou_inputs(Na, Nb)
    B = a.shape[0]
    want = _iou_want(a, b, sizes_a, sizes_b)
    ra, rb = ragged5(a, sizes_a, DEV), ragged5(b, sizes_b, DEV)
    got = rotated_iou_bev(ra, rb)
    assert got.tensor.is_cuda and got.sample_sizes is ra.sample_sizes and tuple(got.tensor.shape) == (B, Na, Nb)
    g = got.tensor.cpu().numpy()
    err = float(np.abs(g - want).max())
    accuracy.append((f"Na={Na} Nb={Nb} B={B}", int(sum(x * y for x, y in zip(sizes_a, sizes_b))), int((want > 0).sum()), err))
    assert err <= BAR, f"IoU off by {err:.3e} (bar {BAR})"
    inside = np.zeros((B, Na, Nb), bool)
    for f, (na, nb) in enumerate(zip(sizes_a, sizes_b)):
        inside[f, :na, :nb] = True
    assert not g.view(np.uint32)[~inside].any(), "a pair beyond a size is not +0"
    assert Na == 1 or (want > 0.01).sum() > 20
    host = rotated_iou_bev(ragged5(a, sizes_a), ragged5(b, sizes_b)).tensor.numpy()
    assert np.abs(g - host).max() <= BAR, "device against host"
    # the same call through the raw C-ABI into a sentinel-filled buffer with bands around it
    pad = 512
    nbytes = B * Na * Nb * 4
    buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    inner = buf[pad: pad + nbytes].view(torch.float32).view(B, Na, Nb)
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    status = nat.ctypes_lib().accv_rotated_iou_bev(ra.tensor.data_ptr(), ra.sample_sizes.data_ptr(), rb.tensor.data_ptr(), rb.sample_sizes.data_ptr(),
                                                   B, Na, Nb, inner.data_ptr(), stream)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + nbytes:] == 0xA5).all()), "wrote outside the output"
    assert torch.equal(inner.view(torch.uint8), got.tensor.view(torch.uint8)), "an element kept the sentinel, or two runs differ"


def test_iou_of_a_frame_of_nms_size_and_the_closed_forms_on_the_device(accuracy):
    """the IoU that the NMS kernel decides on: every pair of a 300-box frame of each kind, through the matrix operator"""
    worst = 0.0
    for kind in range(3):
        boxes = random_boxes(np.random.default_rng(40 + kind), 300, kind)[None]
        want = iou64(boxes[0], boxes[0])
        r = ragged5(boxes, [300], DEV)
        g = rotated_iou_bev(r, r).tensor[0].cpu().numpy()
        err = float(np.abs(g - want).max())
        accuracy.append((f"kind {kind} N=300", 300 * 300, int((want > 0).sum()), err))
        worst = max(worst, err)
    assert worst <= BAR
    lit = ragged5([[BIG, SMALL, (3.0, 4.0, 10.0, 2.8, 1e-4), (2.0, 1.0, 4.0, 2.0, 0.0), (6.0, 1.0, 4.0, 2.0, 0.0)]], [5], DEV)
    g = rotated_iou_bev(lit, lit).tensor[0].cpu().numpy()
    assert g[0, 1] == 0.25 and g[1, 0] == 0.25 and (np.diag(g) == 1.0).all() and g[3, 4] == 0.0 and g[4, 3] == 0.0


# ------------------------------------------------------------------------------------- boxes off the dataset-like range
@pytest.mark.parametrize("name", hard.NAMES)
def test_hard_geometry_family_on_the_device(name, accuracy):
    """yaws many turns out, strips, quarter-turn and axis yaws, far centres: against the definition, against the host entry (the
    same operations but the platform's cosf / sinf), and iou(a, b) against iou(b, a)"""
    a, b, want = hard.family(name)
    got = hard.op_pairs(a, b, DEV)
    err = float(np.abs(got - want).max())
    accuracy.append((name, len(want), int((want > hard.OVERLAP).sum()), err))
    assert err <= BAR, f"{name}: IoU off by {err:.3e} (bar {BAR})"
    host = float(np.abs(got - hard.op_pairs(a, b)).max())
    assert host <= BAR, f"{name}: device against host {host:.3e}"
    sym = float(np.abs(got - hard.op_pairs(b, a, DEV)).max())
    assert sym <= BAR, f"{name}: iou(a, b) and iou(b, a) differ by {sym:.3e}"


def test_closed_forms_and_rewritten_rectangles_on_the_device():
    for form in (hard.crossing_strips, hard.box_inside_box):
        a, b, want = form()
        assert np.abs(hard.op_pairs(a, b, DEV) - want).max() <= BAR, form.__name__
        assert np.abs(hard.op_pairs(b, a, DEV) - want).max() <= BAR, form.__name__
    r, q, third = hard.rewritten_rectangles()
    assert hard.op_pairs(r, q, DEV).min() >= 1 - BAR and hard.op_pairs(q, r, DEV).min() >= 1 - BAR
    assert np.abs(hard.op_pairs(r, third, DEV) - hard.op_pairs(q, third, DEV)).max() <= BAR
    assert np.abs(hard.op_pairs(third, r, DEV) - hard.op_pairs(third, q, DEV)).max() <= BAR


def test_strips_moved_along_their_length_stay_within_the_bar_plus_the_rotation_of_the_centre_offset():
    """what the bar does not cover, pinned to the bound its cause gives (rotated_iou_hard_cases.py)"""
    a, b, want, bound = hard.shifted_strips()
    for got in (hard.op_pairs(a, b, DEV), hard.op_pairs(b, a, DEV)):
        err = np.abs(got - want)
        print(f"strips moved along their length: largest error {err.max():.3e}, largest error / bound {(err / bound).max():.3f}, bound up to {bound.max():.2e}")
        assert (err <= bound).all(), f"{(err / bound).max():.3f} of the bound"


def test_many_turns_out_identical_boxes_give_one_exactly_and_beyond_the_domain_a_finite_value():
    same = np.float32([[10.0, 20.0, 4.5, 1.9, 628.3], [-37.25, 48.5, 50.0, 0.02, -4084.5], [1.0, 2.0, 4.5, 1.9, hard.YAW_DOMAIN]])
    assert (hard.op_pairs(same, same, DEV) == 1.0).all()
    a = np.float32([[1.0, 2.0, 4.5, 1.9, 2 * np.pi * 1e5 + 0.3], [1.0, 2.0, 4.5, 1.9, 3e38], [1.0, 2.0, 50.0, 0.02, -1e9], [1.0, 2.0, 4.5, 1.9, 0.3]])
    b = a.copy()
    b[:, 4] = np.float32([0.3, -3e38, 1e9, -2 * np.pi * 1e5])
    r = ragged5(a[None], [4], DEV), ragged5(b[None], [4], DEV)
    m = rotated_iou_bev(*r).tensor.cpu().numpy()
    assert np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()


@pytest.mark.parametrize("edge", [WAVE, THREADS])
@pytest.mark.parametrize("k", range(len(hard.FROZEN)))
def test_keep_decisions_that_one_float32_subtraction_of_the_yaws_got_wrong_across_a_boundary(k, edge):
    """the threshold lies 2e-5 from the float64 IoU, twice the margin, on the side where the old arithmetic's value was"""
    a, b, want, was = hard.FROZEN[k]
    thr = hard.frozen_threshold(want, was)
    N = edge + WAVE
    case = placed_case(N, {edge - 1: b, edge: a})
    got, _ = both(case, thr, f"frozen pair {k}")
    assert kept_slots(got) == [s for s in range(N) if s != edge or want <= thr]


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B,N,pre,M,D", [(3, 70, 70, 70, 9), (2, THREADS + 3, 200, 83, 7), (1, 5, 5, 1, 16)])
def test_guard_bands_and_complete_write_of_all_four_outputs_and_the_sizes(B, N, pre, M, D):
    from accvlab import _amd_native as nat

    T, pad = 3, 512
    host_case = make_case(B, N, T, D, seed=5)
    thr = [pick_threshold(host_case, 0, 0.2), None, pick_threshold(host_case, 2, 0.5)]
    case = host_case.to(DEV)

    def banded(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV)      # the sentinel fills the inside too
        return buf, buf[pad: pad + nbytes].view(dtype).view(shape)

    shapes = dict(boxes=((T, B, M, D), torch.float32), scores=((T, B, M), torch.float32), labels=((T, B, M), torch.int64),
                  source=((T, B, M), torch.int32), sizes=((T, B), torch.int64))
    bands = {k: banded(*v) for k, v in shapes.items()}
    p = nat.RotatedNmsParams()
    for t, (bx, sc, lb, src, sizes) in enumerate(case.tasks):
        p.boxes[t], p.scores[t], p.labels[t], p.source[t], p.sizes[t] = (x.data_ptr() for x in (bx, sc, lb, src, sizes))
        p.has_threshold[t], p.iou_threshold[t] = (0, 0.0) if thr[t] is None else (1, thr[t])
    p.num_tasks = T
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device()))
    status = nat.ctypes_lib().accv_rotated_nms_bev(ctypes.addressof(p), B, N, D, pre, M,
                                                   *(bands[k][1].data_ptr() for k in ("boxes", "scores", "labels", "source", "sizes")), stream)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    torch.cuda.synchronize()
    for name, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{name}: wrote outside its buffer"
    # every slot inside was written: the pre-filled sentinel is gone wherever the definition has a value, padding included
    got = [CenterPointDetections(*(RaggedBatch(bands[k][1][t].clone(), sample_sizes=sizes) for k in ("boxes", "scores", "labels", "source")))
           for t, sizes in enumerate(bands["sizes"][1].clone().unbind(0))]
    check(got, definition(host_case, thr, pre, M), host_case, "banded")


# -------------------------------------------------------------- reproducibility, no synchronisation, graphs, other streams
FULL = dict(pre_max_size=400, post_max_size=83)


def _full(seed, N=2 * THREADS + 1):
    host = make_case(3, N, 3, 9, seed=seed)
    return host, [pick_threshold(host, 0, 0.2), None, pick_threshold(host, 2, 0.5)]


def _flat(result):
    return [x.tensor for r in result for x in r] + [r.boxes.sample_sizes for r in result]


def test_two_runs_are_bitwise_identical():
    host, thr = _full(8)
    det = host.to(DEV).detections()
    first = _flat(op(det, thr, **FULL))
    for _ in range(2):
        for a, b in zip(first, _flat(op(det, thr, **FULL))):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_no_host_synchronisation():
    host, thr = _full(9, 70)
    det = host.to(DEV).detections()
    ra = ragged5(host.tasks[0][0][..., BEV].numpy(), host.tasks[0][4].tolist(), DEV)
    op(det, thr, **FULL), rotated_iou_bev(ra, ra)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = op(det, thr, **FULL)
        m = rotated_iou_bev(ra, ra)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    check(got, definition(host, thr, **FULL), host)
    assert tuple(m.tensor.shape) == (3, 70, 70)


def test_a_non_default_stream():
    host, thr = _full(10, THREADS + 9)
    det = host.to(DEV).detections()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = op(det, thr, **FULL)
    stream.synchronize()
    check(got, definition(host, thr, **FULL), host, "side stream")


def test_graph_capture_and_replay_equal_eager():
    N = THREADS + 9
    (a, thr_a), (b, thr_b) = _full(12, N), _full(13, N)
    thr = [max(thr_a[0], thr_b[0]), None, max(thr_a[2], thr_b[2])]
    assert_margin(a, thr), assert_margin(b, thr)
    live = a.to(DEV)
    det = live.detections()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            op(det, thr, **FULL)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(det, thr, **FULL)
    for case in (b, a):
        live.copy_(case.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        eager = op(case.to(DEV).detections(), thr, **FULL)
        for x, y in zip(_flat(out), _flat(eager)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        check(out, definition(case, thr, **FULL), case, "replay")


def test_wrong_devices_are_refused():
    host = make_case(2, 6, 2, 9, seed=6)
    dev = host.to(DEV)
    det = dev.detections()
    mixed = [det[0], host.detections()[1]]
    with pytest.raises(RuntimeError, match=r"rotated_nms_bev: detections\[1\].boxes is \(2, 6, 9\) on cpu, detections\[0\].boxes \(2, 6, 9\) on cuda"):
        op(mixed, 0.2)
    d = det[0]
    bad = CenterPointDetections(d.boxes, RaggedBatch(d.scores.tensor.cpu(), sample_sizes=d.scores.sample_sizes), d.labels, d.source)
    with pytest.raises(RuntimeError, match=r"rotated_nms_bev: detections\[0\].scores must be \(2, 6\) on cuda:0, got \(2, 6\) on cpu"):
        op(bad, 0.2)
    bad = CenterPointDetections(RaggedBatch(d.boxes.tensor, sample_sizes=d.boxes.sample_sizes.cpu()), d.scores, d.labels, d.source)
    with pytest.raises(RuntimeError, match=r"rotated_nms_bev: the sample_sizes of detections\[0\].boxes must be an int64 tensor \(2,\) on cuda:0"):
        op(bad, 0.2)
    a = ragged5(np.zeros((2, 3, 5)), [3, 3], DEV)
    with pytest.raises(RuntimeError, match=r"rotated_iou_bev: boxes_a is on cuda:0, boxes_b on cpu"):
        rotated_iou_bev(a, ragged5(np.zeros((2, 3, 5)), [3, 3]))


# ------------------------------------------------------------------------------------------------------------ end to end
def test_peaks_decode_and_rotated_nms_on_a_small_head():
    """heatmap_peaks -> center_point_decode(nms_threshold=None) -> rotated_nms_bev against the definition applied to the
    decode's own output; `source` still indexes the peaks, so gather_at_centers finds the kept detections' cells"""
    tasks = ((0,), (1, 2))
    B, H, W, K = 2, 32, 32, 96
    g = torch.Generator().manual_seed(11)
    cfg = dict(pc_range=[-12.8, -12.8], voxel_size=[0.1, 0.1], out_size_factor=8)          # cells of 0.8 m: neighbouring boxes overlap
    logits, heads = [], []
    for ids in tasks:
        logits.append((torch.randn(B, len(ids), H, W, generator=g) - 1.0).to(DEV))
        ang = (torch.rand(B, 1, H, W, generator=g) * 2 - 1) * np.pi
        heads.append([t.contiguous().to(DEV) for t in (torch.rand(B, 2, H, W, generator=g), torch.rand(B, 1, H, W, generator=g),
                                                       torch.rand(B, 3, H, W, generator=g) * 0.8 + 0.4, torch.cat([ang.sin(), ang.cos()], 1))])
    peaks = [heatmap_peaks(lg, K, kernel=1) for lg in logits]
    dets = center_point_decode(peaks, heads, tasks, **cfg, scores_are_logits=True, score_threshold=0.1, nms_threshold=None)
    case = Case([tuple(x.tensor.cpu() for x in d) + (d.boxes.sample_sizes.cpu(),) for d in dets])
    thr = [pick_threshold(case, 0, 0.2), pick_threshold(case, 1, 0.2)]
    got = op(dets, thr, post_max_size=40)
    want = definition(case, thr, None, 40)
    check(got, want, case, "end to end")
    kept, dead, total = share(definition(case, thr), case, thr)         # without the cut: what the NMS alone suppresses
    assert dead >= total / 10 and kept >= total / 10, (kept, dead, total)
    for t, d in enumerate(got):
        n = d.source.sample_sizes
        rank = d.source.tensor.clamp(min=0).long()
        assert bool(((d.source.tensor >= 0) == (torch.arange(d.source.tensor.shape[1], device=DEV)[None] < n[:, None])).all())
        cells = peaks[t].indices.gather(1, rank)
        rows = gather_at_centers(heads[t], cells)                       # [B, M, 8]: (off_x, off_y, z, d0, d1, d2, sin, cos)
        rows = rows.tensor if hasattr(rows, "tensor") else rows
        valid = (d.source.tensor >= 0)
        assert torch.equal(rows[..., 2][valid], d.boxes.tensor[..., 2][valid]), "z is a bit copy of the map at the kept detection's cell"
