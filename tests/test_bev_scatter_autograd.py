"""The autograd contract of DESIGN.md §9p for scatter_to_bev: the checks of autograd_contract_cases.py (imported, not
edited) on the smallest input that keeps both what the backward reads and what it ignores non-trivial: B = 2, a 5 x 7 map,
C = 3, six rows with one duplicate cell and one unplaced row.  The backward entry receives `coors` and the saved `index` (an
output of the forward, which the case publishes as t["index"]) and never `features`.  The gradient is a copy: the
comparison is torch.equal and the bound is zero."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autograd_contract_cases as acc  # noqa: E402

B, NY, NX, C = 2, 5, 7, 3
COORS = [[0, 0, 1, 2], [1, 3, 4, 6], [0, -2, 1, 2], [1, 0, 0, 0], [0, 0, 5, 0], [1, 9, 2, 3]]   # rows 0 and 2 share a cell; row 4: y == ny


class ScatterToBev(acc.Case):
    name = "scatter_to_bev"
    cfgs = ("i32",)          # coors are int32 only
    differentiable = ("features",)
    reads = (("coors", "index"), ("index", "index"))
    ignores = (("features", "float"),)

    def build(self, device, cfg):
        return {"features": torch.randn(len(COORS), C, generator=acc._gen(21)).to(device),
                "coors": torch.tensor(COORS, dtype=torch.int32, device=device)}

    def forward(self, t):
        from accvlab.point_cloud import scatter_to_bev

        canvas, index = scatter_to_bev(t["features"], t["coors"], grid_hw=(NY, NX), batch_size=B, return_index=True)
        t["index"] = index       # what the backward reads besides coors
        return (canvas,)

    def definition(self, t, gos):
        """from the coors and the index as they are in `t`: a row gets the gradient at its cell iff the index names it"""
        coors, go = t["coors"].long(), gos[0].double()
        index = t["index"].long()
        grad = torch.zeros(coors.shape[0], C, dtype=torch.float64)
        for r, (b, _, y, x) in enumerate(coors.tolist()):
            if 0 <= b < B and 0 <= y < NY and 0 <= x < NX and int(index[b, y, x]) == r:
                grad[r] = go[b, :, y, x]
        return {"features": grad}

    def bound(self, want):
        return torch.zeros_like(want)

    def check(self, name, got, want, device, what):
        assert torch.equal(got.detach().cpu().double(), want), what


CASE = ScatterToBev()


def test_the_case_is_what_its_text_says():
    t = CASE.build("cpu", "i32")
    canvas, = CASE.forward(t)
    assert t["index"][0, 1, 2] == 2 and int((t["index"] >= 0).sum()) == 4 and not t["index"].requires_grad
    assert torch.equal(canvas[0, :, 1, 2], t["features"][2]) and int((canvas != 0).sum()) == 4 * C


@pytest.mark.parametrize("check", acc.CHECKS, ids=lambda c: c.__name__)
def test_contract_on_the_host_path(check):
    check(CASE, "cpu", "i32")


@pytest.mark.gpu
@pytest.mark.parametrize("check", acc.CHECKS, ids=lambda c: c.__name__)
def test_contract_on_the_device_path(check):
    check(CASE, "cuda", "i32")
