"""The three losses over matched pairs agree on which queries are matched (host path): one index set, the matched set read
off each gradient, against the pair rule of matched_box_loss_cases.pairs_of.  Cases: tests/matched_pair_rule_cases.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from matched_pair_rule_cases import expected, indices, matched_by_box, matched_by_focal, matched_by_polyline  # noqa: E402

from accvlab.batching_helpers import matched_box_loss, matched_focal_loss  # noqa: E402
from accvlab.lane_helpers.polyline import matched_polyline_loss  # noqa: E402


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_three_losses_match_the_same_queries(index_dtype):
    pind, gind = indices(index_dtype)
    want = expected(pind, gind)
    assert matched_by_focal(matched_focal_loss, pind, gind, torch.float32) == want
    assert matched_by_box(matched_box_loss, pind, gind, torch.float32) == want
    assert matched_by_polyline(matched_polyline_loss, pind, gind, torch.float32) == want
