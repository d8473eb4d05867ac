"""The three losses over matched pairs agree on which queries are matched (device kernels): one index set, the matched set
read off each gradient, against the pair rule of matched_box_loss_cases.pairs_of and against the host path's set.
Cases: tests/matched_pair_rule_cases.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matched_pair_rule_cases import expected, indices, matched_by_box, matched_by_focal, matched_by_polyline  # noqa: E402

from accvlab.batching_helpers import matched_box_loss, matched_focal_loss  # noqa: E402
from accvlab.lane_helpers.polyline import matched_polyline_loss  # noqa: E402

pytestmark = pytest.mark.gpu

LOSSES = [(matched_by_focal, matched_focal_loss), (matched_by_box, matched_box_loss),
          (matched_by_polyline, matched_polyline_loss)]


@pytest.mark.parametrize("index_dtype, dtype", [(torch.int32, torch.float32), (torch.int64, torch.float32),
                                                (torch.int64, torch.float16)], ids=["i32-f32", "i64-f32", "i64-f16"])
def test_three_losses_match_the_same_queries(index_dtype, dtype):
    pind, gind = indices(index_dtype, "cuda")
    hpind, hgind = indices(index_dtype)
    want = expected(hpind, hgind)
    for read, op in LOSSES:
        got = read(op, pind, gind, dtype, "cuda")
        assert got == want, op.__name__
        assert got == read(op, hpind, hgind, dtype), op.__name__ + " host"
