"""Inputs at the edges of the loss kernels' own work partition, shared by test_partition_edges_cpu.py (host path) and
test_partition_edges_gpu.py (device and host path).  Every shape is derived from a constant of the operator's ``.hip`` file
(DESIGN.md §9k has the table); definitions and comparison rules are those of matched_focal_loss_cases.py and
matched_box_loss_cases.py, unchanged.

A case proves from outside that it is in the regime it names: the workspace entry points publish the number of workgroups
per frame (``nqb``),

    accv_matched_focal_loss_workspace_bytes(B, Q, C) == align16(8 * B * nqb)
    accv_matched_box_loss_workspace_bytes(B, Q, D)   == align16(16 * B * nqb)

and the queries per workgroup (``qpb``) of the focal kernel are the largest Q that still gives one workgroup per frame at
that C: ``nqb(Q = qpb) == 1`` and ``nqb(Q = qpb + 1) == 2``.  (``ceil(Q / nqb)`` is qpb only where the ranges are even; the
probe holds for every case.)  geometry() is not restated here.
"""
import torch

import matched_box_loss_cases as mb
import matched_focal_loss_cases as mf

name = lambda d: str(d).split(".")[-1]  # noqa: E731


def align16(n):
    return (n + 15) // 16 * 16


def _lib():
    from accvlab import _amd_native as nat

    return nat.ctypes_lib()


def assert_focal_partition(B, Q, C, nqb, qpb=None):
    """the case has `nqb` workgroups per frame and (where given) `qpb` queries per workgroup"""
    lib = _lib()
    assert lib.accv_matched_focal_loss_workspace_bytes(B, Q, C) == align16(8 * B * nqb), (B, Q, C, nqb)
    # B == 2 rows of the same geometry make the product even, so that the 16-byte padding cannot hide one workgroup
    assert lib.accv_matched_focal_loss_workspace_bytes(2, Q, C) == 16 * nqb, (Q, C, nqb)
    if qpb is not None:
        assert lib.accv_matched_focal_loss_workspace_bytes(2, qpb, C) == 16, (C, qpb)
        assert lib.accv_matched_focal_loss_workspace_bytes(2, qpb + 1, C) == 32, (C, qpb)
        assert nqb == -(-Q // qpb)


def assert_box_partition(B, Q, D, nqb):
    assert _lib().accv_matched_box_loss_workspace_bytes(B, Q, D) == align16(16 * B * nqb), (B, Q, D, nqb)


def place(pind, b, n, edges, Q, seed):
    """slots [0, n) of frame b: `edges` first, then distinct random queries outside them"""
    g = torch.Generator().manual_seed(seed)
    rest = [int(q) for q in torch.randperm(Q, generator=g) if int(q) not in edges][: n - len(edges)]
    assert len(edges) + len(rest) == n
    pind.tensor[b, :n] = torch.tensor(list(edges) + rest, dtype=pind.tensor.dtype, device=pind.tensor.device)


def grad_out(shape, seed=1):
    """random in [0.5, 1.5]"""
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) + 0.5


# ------------------------------------------------------------------------------------------------------ matched_focal_loss
# name -> (B, Q, C, nqb, qpb or None, dtypes).  Constants of csrc/matched_focal.hip: kTargetElems = 8192, kMaxQ = 1024,
# kThreads = 256, kFinishThreads = 1024 (csrc/matched_pairs.h; 16 waves of 64), V = 16 / element size.
FOCAL = {
    # 8192 / 8 = 1024 = kMaxQ: the cap is reached, ranges [0, 1024) and [1024, 1030)
    "maxq_two_ranges": (2, 1030, 8, 2, 1024, mf.DTYPES),
    # 8192 / C > kMaxQ: capped; ranges [0, 1024), [1024, 2048), [2048, 2051).  C = 3: every 16-byte vector straddles queries
    "maxq_c1": (2, 2051, 1, 3, 1024, mf.DTYPES),
    "maxq_c3": (2, 2051, 3, 3, 1024, mf.DTYPES),
    # 8192 / 4100 = 1 query per workgroup, 70 > 64 partials per frame: the finish kernel's lane loop takes a second trip
    "qpb1_finish_second_trip": (2, 70, 4100, 70, 1, mf.DTYPES),
    # C > kTargetElems: one query per workgroup and more elements than aimed at; C > 256 * V for every dtype (dq == 0)
    "range_longer_than_target": (1, 3, 8200, 3, 1, mf.DTYPES),
    "range_longer_than_target_odd": (1, 3, 8201, 3, 1, mf.DTYPES),   # rows of 8201: no range but the first starts aligned
    # C = 2049 > 256 * 8: walk()'s dq == 0 for f64 (V = 2), f32 (4) and f16 / bf16 (8); 3 queries per workgroup
    "dq0_every_dtype": (2, 5, 2049, 2, 3, mf.DTYPES),
    # C = 513 > 256 * 2: dq == 0 for f64 only; 8192 / 513 = 15 >= Q, one workgroup
    "dq0_f64": (2, 5, 513, 1, None, [torch.float64]),
    # one workgroup per frame (819 >= 600) reads 300 and 257 slots: build_table's slot loop takes a second trip
    "more_than_256_pairs": (2, 600, 10, 1, None, mf.DTYPES),
    # 8192 / 10 = 819: ranges [0, 819) and [819, 900)
    "range_boundaries": (3, 900, 10, 2, 819, mf.DTYPES),
    # the pair count of the finish kernel: b += 1024 takes a second trip; a wave adds frames wave, wave + 16, ...
    "more_than_1024_frames": (1030, 2, 3, 1, None, mf.DTYPES),
}


def focal_case(which, dtype, device="cpu"):
    """-> (inputs of make_case, grad_out [B], notes) with the pairs the regime asks for"""
    B, Q, C, nqb, qpb, _ = FOCAL[which]
    notes = {}
    if which == "maxq_two_ranges":
        n = [40, 30]
        inp = mf.make_case(B, Q, C, [40, 40], n, dtype, seed=21, weights=True)
        for b in range(B):
            place(inp[2], b, n[b], [0, 1023, 1024, 1029], Q, seed=b)
    elif which in ("maxq_c1", "maxq_c3"):
        n = [50, 20]
        inp = mf.make_case(B, Q, C, [50, 20], n, dtype, seed=22 + C, weights=True)
        for b in range(B):
            place(inp[2], b, n[b], [0, 1023, 1024, 2047, 2048, 2050], Q, seed=b)
    elif which == "qpb1_finish_second_trip":
        inp = mf.make_case(B, Q, C, [70, 0], [70, 0], dtype, seed=23, weights=True)
    elif which.startswith("range_longer_than_target"):
        inp = mf.make_case(B, Q, C, [3], [2], dtype, seed=24, weights=True)
    elif which in ("dq0_every_dtype", "dq0_f64"):
        inp = mf.make_case(B, Q, C, [4, 2], [4, 1], dtype, seed=25, weights=True)
        place(inp[2], 0, 4, [0, 2, 3, 4], Q, seed=0)      # both sides of the range boundary at query 3
    elif which == "more_than_256_pairs":
        inp = mf.make_case(B, Q, C, [300, 257], [300, 257], dtype, seed=26, weights=True)
        _, labels, pind, gind, _ = inp
        pind.tensor[0, 290] = pind.tensor[0, 3]            # one query in slot 3 and in slot 290: slot 3 is its pair
        labels.tensor[0, int(gind.tensor[0, 3])] = 1
        labels.tensor[0, int(gind.tensor[0, 290])] = 2
        notes["twice"] = (0, int(pind.tensor[0, 3]), 1, 2, 290)   # frame, query, label of slot 3, label of slot 290, slot
    elif which == "range_boundaries":
        inp = mf.make_case(B, Q, C, [5, 2, 0], [3, 1, 0], dtype, seed=27, weights=True)
        inp[2].tensor[0, :3] = torch.tensor([818, 819, 899])
        inp[2].tensor[1, :1] = torch.tensor([819])
    else:
        assert which == "more_than_1024_frames"
        n = [b % 3 for b in range(B)]
        inp = mf.make_case(B, Q, C, [2] * B, n, dtype, seed=28, weights=True)
    logits, labels, pind, gind, w = inp
    move = lambda rb: mf.ragged(rb.tensor.to(device), rb.sample_sizes.tolist())  # noqa: E731
    return (logits.to(device), move(labels), move(pind), move(gind), w.to(device)), grad_out((B,)), notes


# -------------------------------------------------------------------------------------------------------- matched_box_loss
# name -> (B, Q, D, nqb).  Constants of csrc/matched_box.hip: kThreads = 256 queries per workgroup; kFinishThreads = 1024 (csrc/matched_pairs.h).
BOX = {
    "finish_second_trip": (1, 16400, 4, 65),        # ceil(16400 / 256) = 65 > 64 partials: the lane loop's second trip
    "more_than_1024_frames": (1030, 5, 4, 1),       # the pair count's b += 1024 takes a second trip
    "more_than_256_pairs": (2, 700, 4, 3),          # every workgroup reads 300 / 257 slots: the slot loop's second trip
}
BOX_RUNS = [(torch.float32, "giou"), (torch.float32, None), (torch.bfloat16, "giou"), (torch.bfloat16, None),
            (torch.float64, "giou")]


def box_case(which, dtype, device="cpu"):
    """-> (inputs of make_case, grad_out [2, B], notes); boxes in cxcywh"""
    B, Q, D, _ = BOX[which]
    notes = {}
    if which == "finish_second_trip":
        inp = mb.make_case(B, Q, D, [40], [40], dtype, seed=31, box_format="cxcywh", weights=True)
        place(inp[2], 0, 40, [0, 255, 256, 16383, 16384, 16399], Q, seed=0)
    elif which == "more_than_1024_frames":
        n = [b % 4 for b in range(B)]
        inp = mb.make_case(B, Q, D, [3] * B, n, dtype, seed=32, box_format="cxcywh", weights=True)
    else:
        inp = mb.make_case(B, Q, D, [300, 257], [300, 257], dtype, seed=33, box_format="cxcywh", weights=True)
        inp[2].tensor[0, 290] = inp[2].tensor[0, 3]       # one query in slot 3 and in slot 290: slot 3 is its pair
        notes["twice"] = (0, int(inp[2].tensor[0, 3]), 290)
    boxes, gt, pind, gind, w = inp
    move = lambda rb: mb.ragged(rb.tensor.to(device), rb.sample_sizes.tolist())  # noqa: E731
    return (boxes.to(device), move(gt), move(pind), move(gind), w.to(device)), grad_out((2, B)), notes


def say_something_else(rb, b, slot, limit):
    """a copy of ragged indices whose entry (b, slot) names another object"""
    t = rb.tensor.clone()
    t[b, slot] = (t[b, slot] + 1) % limit
    return mf.ragged(t, rb.sample_sizes.tolist())
