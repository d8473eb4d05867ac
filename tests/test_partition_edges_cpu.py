"""The host paths of matched_focal_loss and matched_box_loss on the partition-edge shapes of partition_edges_cases.py,
against the float64 definitions at their stated tolerances.  The host path has no partition: it is the second witness of
test_partition_edges_gpu.py, and here it shows that the definition's bars hold at these shapes before any kernel is
involved.  Needs no GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import matched_box_loss_cases as mb  # noqa: E402
import matched_focal_loss_cases as mf  # noqa: E402
import partition_edges_cases as pe  # noqa: E402

from accvlab.batching_helpers import matched_box_loss as mbl  # noqa: E402
from accvlab.batching_helpers import matched_focal_loss as mfl  # noqa: E402

FOCAL_RUNS = [(which, dtype) for which in pe.FOCAL for dtype in pe.FOCAL[which][5]]


@pytest.mark.parametrize("which,dtype", FOCAL_RUNS, ids=[f"{w}-{pe.name(d)}" for w, d in FOCAL_RUNS])
def test_focal_host_path_meets_the_definition_at_the_edge_shapes(which, dtype):
    B, Q, C, nqb, qpb, _ = pe.FOCAL[which]
    pe.assert_focal_partition(B, Q, C, nqb, qpb)
    (logits, labels, pind, gind, w), go, notes = pe.focal_case(which, dtype)
    want, gwant, factor = mf.definition(logits, labels, pind, gind, grad_out=go, query_weights=w)
    out, grad = mf.run(mfl, logits, labels, pind, gind, grad_out=go, query_weights=w)
    mf.check_loss(out, want, dtype, f"{which} {pe.name(dtype)} host")
    mf.check_grad(grad, gwant, dtype, f"{which} {pe.name(dtype)} host")
    if which == "more_than_1024_frames":   # the default denominator is the definition's number of pairs
        assert factor == float(sum(b % 3 for b in range(B)))
        fixed = mf.run(mfl, logits, labels, pind, gind, grad_out=go, query_weights=w, avg_factor=factor)
        assert torch.equal(mf.bits(out), mf.bits(fixed[0])) and torch.equal(mf.bits(grad), mf.bits(fixed[1]))
    if "twice" in notes:
        b, q, first, later, slot = notes["twice"]
        assert float(grad[b, q, first]) < 0 < float(grad[b, q, later])
        other = mf.run(mfl, logits, labels, pind, pe.say_something_else(gind, b, slot, 300), grad_out=go, query_weights=w)
        assert torch.equal(mf.bits(out), mf.bits(other[0])) and torch.equal(mf.bits(grad), mf.bits(other[1]))


BOX_RUNS = [(which, dtype, kind) for which in pe.BOX for dtype, kind in pe.BOX_RUNS]


@pytest.mark.parametrize("which,dtype,kind", BOX_RUNS, ids=[f"{w}-{pe.name(d)}-{k}" for w, d, k in BOX_RUNS])
def test_box_host_path_meets_the_definition_at_the_edge_shapes(which, dtype, kind):
    B, Q, D, nqb = pe.BOX[which]
    pe.assert_box_partition(B, Q, D, nqb)
    inp, go, notes = pe.box_case(which, dtype)
    out, grad = mb.compare(mbl, inp, f"{which} {pe.name(dtype)} {kind} host", grad_out=go, box_format="cxcywh", iou_kind=kind)
    if "twice" in notes:
        b, q, slot = notes["twice"]
        boxes, gt, pind, gind, w = inp
        other = mb.run(mbl, boxes, gt, pind, pe.say_something_else(gind, b, slot, 300), grad_out=go, query_weights=w,
                       box_format="cxcywh", iou_kind=kind)
        assert bool((grad[b, q] != 0).any())
        assert torch.equal(mb.bits(out), mb.bits(other[0])) and torch.equal(mb.bits(grad), mb.bits(other[1]))
