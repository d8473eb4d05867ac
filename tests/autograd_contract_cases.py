"""The autograd contract of every public differentiable operator: the operators, their smallest
meaningful inputs, the float64 definitions of their gradients and the checks (the seven of §9p and one with saved-tensor
hooks) that test_autograd_contract_cpu.py (host path) and test_autograd_contract_gpu.py (device path) run on each of them.

A case lists every user-visible tensor of one call by name (``build``), says which of them take a gradient
(``differentiable``), which the backward entry point of the C header receives (``reads``: pointer arguments of the
``*_bwd`` / scatter / grad entry in include/accv_hip.h, operands behind the parameter structs included) and which it does
not (``ignores``).  Definitions and comparison rules are imported from the operator's own cases or test module and used
unchanged; the table below says which.  No tolerance is defined here.

    operator                              definition                                    comparison rule
    gaussian_focal_loss                   test_heatmap_loss_gpu.composition             test_heatmap_loss_gpu.assert_grad_close
    gather_at_centers                     center_regression_cases._gather (autograd)    center_regression_cases.assert_grad_close
    center_regression_loss                center_regression_cases.oracle_loss           center_regression_cases.assert_grad_close
    matched_pair_loss_sum                 the composition of its module text, float64   test_matched_pair_loss_gpu (1e-5 of max(1, |g|))
    matched_focal_loss                    matched_focal_loss_cases.definition           matched_focal_loss_cases.check_grad
    matched_box_loss                      matched_box_loss_cases.definition             matched_box_loss_cases.check_grad
    matched_polyline_loss                 polyline_match_cases.definition               polyline_match_cases.check_grad
    interpolate / lengths (+ var size)    test_polyline_grad_cpu.ref_grads              test_polyline_grad_cpu._close (host, float32 rule),
                                                                                        test_polyline_grad_gpu._check (device, float32 rule)
    batched_indexing_access, _inverse,    the indexed copy as a Python loop, float64    test_batching_helpers_gpu (index mapping: < 1e-5)
    _write, batched_index_mapping
    RaggedBatch.with_padded_set_to        torch.where on the mask, float64              test_batching_helpers_gpu (torch.equal)

Everything is float32: the wiring is under test, not the arithmetic.  ``cfg`` is ``"i64"`` or ``"i32"``: the dtype of the
sample sizes and, where the operator takes both, of index and label tensors.  With the native dtype the Python layer
passes the caller's storage on, with the other one it may convert (a copy); ``Case.copied`` names the tensors it copies.
"""
import gc
import itertools

import pytest
import torch

import center_regression_cases as cr
import matched_box_loss_cases as mb
import matched_focal_loss_cases as mf
import polyline_match_cases as pm
from test_polyline_grad_cpu import _close as polyline_close_host, ref_grads as polyline_ref_grads

CFGS = ("i64", "i32")
STALE = "modified by an inplace operation"
TWICE = "backward through the graph a second time"
ONCE = "once_differentiable|differentiate twice"
INT = {"i64": torch.int64, "i32": torch.int32}
F32 = torch.float32


def _rb(tensor, sizes):
    from accvlab.batching_helpers import RaggedBatch

    return RaggedBatch(tensor, sample_sizes=sizes)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cpu(t):
    return {k: v.detach().cpu() for k, v in t.items()}


def f32_bound(want):
    """the float32 gradient rule that matched_focal_loss_cases.check_grad, matched_box_loss_cases.check_grad,
    center_regression_cases.assert_grad_close, test_heatmap_loss_gpu.assert_grad_close and test_polyline_grad_gpu share"""
    return mb.grad_bound(want, F32)


class Case:
    """one operator; see the module text"""
    name = ""
    devices = ("cpu", "cuda")
    cfgs = CFGS
    differentiable = ()
    reads = ()       # (tensor name, "float" | "index" | "sizes")
    ignores = ()
    once = True      # the Function is marked @once_differentiable

    def build(self, device, cfg):
        raise NotImplementedError

    def forward(self, t):
        """-> tuple of output tensors"""
        raise NotImplementedError

    def definition(self, t, gos):
        """t: the input values on the CPU, gos: one upstream gradient per output on the CPU -> {name: float64 gradient}"""
        raise NotImplementedError

    def check(self, name, got, want, device, what):
        mb.check_grad(got, want, F32, what)

    def bound(self, want):
        return f32_bound(want)

    def copied(self, name, cfg):
        """whether the Python layer hands the backward a private copy of this tensor (a dtype conversion)"""
        return False

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ the matched operators
B, Q, G, K, C, D, P = 2, 6, 4, 3, 3, 4, 5
OBJECTS, PAIRS = [4, 3], [3, 2]


class _Matched(Case):
    """pred, a ragged ground truth and the two index batches; `pred_ind.sample_sizes` is the only size tensor read"""
    pred, gt = "", ""

    def copied(self, name, cfg):
        return name == "pred_ind.sample_sizes" and cfg == "i32"   # counts are passed as int64: .to(int64) copies

    def _common(self, t, pred, gt, pind, gind, device, cfg):
        it = INT[cfg]
        t[self.pred] = pred.to(device)
        t[self.gt] = gt.tensor.to(device)
        t[self.gt + ".sample_sizes"] = torch.tensor(OBJECTS, dtype=it, device=device)
        t["pred_ind"] = pind.tensor.to(it).to(device)
        t["pred_ind.sample_sizes"] = torch.tensor(PAIRS, dtype=it, device=device)
        t["gt_ind"] = gind.tensor.to(it).to(device)
        t["gt_ind.sample_sizes"] = torch.tensor(PAIRS, dtype=it, device=device)
        t["avg_factor"] = torch.tensor(3.5, device=device)
        return t

    def ragged(self, t):
        return (_rb(t[self.gt], t[self.gt + ".sample_sizes"]), _rb(t["pred_ind"], t["pred_ind.sample_sizes"]),
                _rb(t["gt_ind"], t["gt_ind.sample_sizes"]))


class MatchedFocal(_Matched):
    name, pred, gt = "matched_focal_loss", "pred_logits", "gt_labels"
    differentiable = ("pred_logits",)
    reads = (("pred_logits", "float"), ("gt_labels", "index"), ("pred_ind", "index"), ("gt_ind", "index"),
             ("pred_ind.sample_sizes", "sizes"), ("query_weights", "float"))
    ignores = (("avg_factor", "float"), ("gt_labels.sample_sizes", "sizes"), ("gt_ind.sample_sizes", "sizes"))

    def build(self, device, cfg):
        logits, labels, pind, gind, w = mf.make_case(B, Q, C, OBJECTS, PAIRS, F32, seed=3, weights=True)
        labels.tensor[:] = torch.tensor([[0, 1, 2, 1], [2, 0, 1, 0]])   # a shift along G changes every label
        t = self._common({}, logits, labels, pind, gind, device, cfg)
        t["gt_labels"] = t["gt_labels"].to(INT[cfg])
        t["query_weights"] = w.to(device)
        return t

    def forward(self, t):
        from accvlab.batching_helpers import matched_focal_loss

        return (matched_focal_loss(t["pred_logits"], *self.ragged(t), query_weights=t["query_weights"],
                                   avg_factor=t["avg_factor"]),)

    def definition(self, t, gos):
        _, grad, _ = mf.definition(t["pred_logits"], *self.ragged(t), query_weights=t["query_weights"],
                                   avg_factor=float(t["avg_factor"]), grad_out=gos[0])
        return {"pred_logits": grad}

    def check(self, name, got, want, device, what):
        mf.check_grad(got, want, F32, what)


class MatchedBox(_Matched):
    name, pred, gt = "matched_box_loss", "pred_boxes", "gt_boxes"
    differentiable = ("pred_boxes",)
    reads = (("pred_boxes", "float"), ("gt_boxes", "float"), ("pred_ind", "index"), ("gt_ind", "index"),
             ("pred_ind.sample_sizes", "sizes"), ("query_weights", "float"), ("code_weights", "float"))
    ignores = (("avg_factor", "float"), ("gt_boxes.sample_sizes", "sizes"), ("gt_ind.sample_sizes", "sizes"))

    def build(self, device, cfg):
        boxes, gt, pind, gind, w = mb.make_case(B, Q, D, OBJECTS, PAIRS, F32, seed=5, weights=True)
        t = self._common({}, boxes, gt, pind, gind, device, cfg)
        t["query_weights"] = w.to(device)
        t["code_weights"] = torch.tensor([1.0, 0.5, 2.0, 1.5], device=device)
        return t

    def forward(self, t):
        from accvlab.batching_helpers import matched_box_loss

        return matched_box_loss(t["pred_boxes"], *self.ragged(t), query_weights=t["query_weights"],
                                code_weights=t["code_weights"], avg_factor=t["avg_factor"])

    def definition(self, t, gos):
        _, grad, _ = mb.definition(t["pred_boxes"], *self.ragged(t), query_weights=t["query_weights"],
                                   code_weights=t["code_weights"], avg_factor=float(t["avg_factor"]),
                                   grad_out=torch.stack(list(gos)))
        return {"pred_boxes": grad}


class MatchedPolyline(_Matched):
    name, pred, gt = "matched_polyline_loss", "pred_lines", "gt_lines"
    differentiable = ("pred_lines",)
    reads = (("pred_lines", "float"), ("gt_lines", "float"), ("pred_ind", "index"), ("gt_ind", "index"),
             ("pred_ind.sample_sizes", "sizes"), ("gt_closed", "index"))
    ignores = (("avg_factor", "float"), ("gt_lines.sample_sizes", "sizes"), ("gt_ind.sample_sizes", "sizes"),
               ("gt_closed.sample_sizes", "sizes"))

    def build(self, device, cfg):
        lines, gt, pind, gind, closed = pm.make_case(B, Q, P, 2, OBJECTS, PAIRS, F32, seed=7, closed="mixed")
        t = self._common({}, lines, gt, pind, gind, device, cfg)
        t["gt_closed"] = closed.tensor.to(device)
        t["gt_closed.sample_sizes"] = torch.tensor(OBJECTS, dtype=INT[cfg], device=device)
        return t

    def forward(self, t):
        from accvlab.lane_helpers.polyline import matched_polyline_loss

        return matched_polyline_loss(t["pred_lines"], *self.ragged(t),
                                     gt_closed=_rb(t["gt_closed"], t["gt_closed.sample_sizes"]), avg_factor=t["avg_factor"])

    def definition(self, t, gos, margin=False):
        _, grad, _, m = pm.definition(t["pred_lines"], *self.ragged(t),
                                      gt_closed=_rb(t["gt_closed"], t["gt_closed.sample_sizes"]),
                                      avg_factor=float(t["avg_factor"]), grad_out=torch.stack(list(gos)))
        if margin:   # polyline_match_cases.compare: float32 and float64 must agree on the order
            assert m > pm.MARGIN, f"the best order leads by {m:.3e} only; pick another seed"
        return {"pred_lines": grad}


# --------------------------------------------------------------------------------------------------- the heat-map branch
class GaussianFocal(Case):
    devices = ("cuda",)
    cfgs = ("i64",)      # no integer input
    differentiable = ("logits",)
    reads = (("logits", "float"), ("target", "float"))
    ignores = (("avg_factor", "float"),)

    def __init__(self, shape, path):
        self.shape, self.name = shape, f"gaussian_focal_loss[{path}]"

    def build(self, device, cfg):
        g = _gen(sum(self.shape))
        target = torch.rand(self.shape, generator=g) * 0.98
        target.view(-1)[::17] = 1.0      # the positives
        logits = (torch.rand(self.shape, generator=g) * 2 - 1) * 6.0
        return {"logits": logits.to(device), "target": target.to(device), "avg_factor": torch.tensor(5.0, device=device)}

    def forward(self, t):
        from accvlab.draw_heatmap import gaussian_focal_loss

        return (gaussian_focal_loss(t["logits"], t["target"], avg_factor=t["avg_factor"]),)

    def definition(self, t, gos):
        from test_heatmap_loss_gpu import composition

        _, grad = composition(t["logits"], t["target"], avg_factor=t["avg_factor"])
        return {"logits": grad * gos[0].double()}

    def check(self, name, got, want, device, what):
        from test_heatmap_loss_gpu import assert_grad_close

        assert_grad_close(got.cpu(), want, F32)


MAPS, H, W, N = [2, 1], 5, 7, 4
CENTERS = [[[1, 2], [6, 4], [1, 2], [7, 1]],      # a duplicate cell, a centre one column outside the map
           [[0, 0], [3, 3], [5, 1], [2, 4]]]
COUNTS = [4, 3]


class _Centers(Case):
    devices = ("cuda",)
    differentiable = ("feats[0]", "feats[1]")

    def maps(self, device):
        m = cr.make_maps(B, MAPS, H, W, F32, device, seed=9)
        return {"feats[0]": m[0], "feats[1]": m[1]}

    def centers(self, t, device, cfg):
        t["centers"] = torch.tensor(CENTERS, dtype=torch.int32, device=device)
        t["centers.sample_sizes"] = torch.tensor(COUNTS, dtype=INT[cfg], device=device)
        return t

    def check(self, name, got, want, device, what):
        cr.assert_grad_close(got.cpu(), want, F32, what)


class GatherRagged(_Centers):
    name = "gather_at_centers[ragged centres]"
    reads = (("centers", "index"), ("centers.sample_sizes", "sizes"))
    ignores = (("feats[0]", "float"), ("feats[1]", "float"))

    def build(self, device, cfg):
        return self.centers(self.maps(device), device, cfg)

    def forward(self, t):
        from accvlab.draw_heatmap import gather_at_centers

        return (gather_at_centers([t["feats[0]"], t["feats[1]"]], _rb(t["centers"], t["centers.sample_sizes"])).tensor,)

    def valid(self, t):
        return cr.valid_and_index(t["centers"], t["centers.sample_sizes"], H, W)

    def definition(self, t, gos):
        leaves = [t[n].double().requires_grad_(True) for n in self.differentiable]
        out = cr._gather(torch.cat(leaves, 1), *self.valid(t))
        grads = torch.autograd.grad((out * gos[0].double()).sum(), leaves)
        return dict(zip(self.differentiable, grads))


class GatherIndices(GatherRagged):
    name = "gather_at_centers[peak indices]"
    cfgs = ("i64",)      # int64 in-plane indices only, no sample sizes
    reads = (("indices", "index"),)

    def build(self, device, cfg):
        t = self.maps(device)
        t["indices"] = torch.tensor([[15, 34, 15, -1], [0, 24, H * W, 30]], dtype=torch.int64, device=device)
        return t

    def forward(self, t):
        from accvlab.draw_heatmap import gather_at_centers

        return (gather_at_centers([t["feats[0]"], t["feats[1]"]], t["indices"]),)

    def valid(self, t):
        ind = t["indices"]
        return (ind >= 0) & (ind < H * W), ind.clamp(0, H * W - 1)


class CenterRegression(_Centers):
    name = "center_regression_loss"
    reads = (("feats[0]", "float"), ("feats[1]", "float"), ("centers", "index"), ("centers.sample_sizes", "sizes"),
             ("targets", "float"), ("weights", "float"))
    ignores = (("avg_factor", "float"),)

    def build(self, device, cfg):
        t = self.centers(self.maps(device), device, cfg)
        g = _gen(10)
        t["targets"] = (torch.randn(B, N, sum(MAPS), generator=g) * 3.0).to(device)
        t["weights"] = (0.25 + torch.rand(B, N, generator=g)).to(device)
        t["avg_factor"] = torch.tensor(3.0, device=device)
        return t

    def forward(self, t):
        from accvlab.draw_heatmap import center_regression_loss

        return (center_regression_loss([t["feats[0]"], t["feats[1]"]], _rb(t["centers"], t["centers.sample_sizes"]),
                                       t["targets"], t["weights"], kind="smooth_l1", beta=1.7, avg_factor=t["avg_factor"]),)

    def definition(self, t, gos):
        _, grads = cr.oracle_loss([t["feats[0]"], t["feats[1]"]], t["centers"], t["centers.sample_sizes"], t["targets"],
                                  t["weights"], "smooth_l1", 1.7, t["avg_factor"], grad_out=float(gos[0]))
        return dict(zip(self.differentiable, grads))


# --------------------------------------------------------------------------------------------------- the index operators
NB, NI = 6, 4            # b = 2 rows of n = 6, 4 indices
IDX_SIZES = [4, 3]


def _valid_slots(sizes, k):
    return [(b, j) for b in range(len(sizes)) for j in range(max(0, min(int(sizes[b]), k)))]


class MatchedPair(Case):
    name = "matched_pair_loss_sum"
    devices = ("cuda",)
    differentiable = ("data_a", "data_b", "weights")
    reads = (("data_a", "float"), ("data_b", "float"), ("indices_a", "index"), ("indices_b", "index"),
             ("indices_a.sample_sizes", "sizes"), ("weights", "float"))
    ignores = (("indices_b.sample_sizes", "sizes"),)

    def build(self, device, cfg):
        g, it = _gen(11), INT[cfg]
        return {"data_a": torch.randn(B, NB, 3, generator=g).to(device), "data_b": torch.randn(B, 5, 3, generator=g).to(device),
                "indices_a": torch.tensor([[5, 0, 2, 3], [1, 4, 0, 2]], dtype=it, device=device),
                "indices_b": torch.tensor([[4, 1, 0, 2], [3, 0, 2, 1]], dtype=it, device=device),
                "indices_a.sample_sizes": torch.tensor(IDX_SIZES, dtype=it, device=device),
                "indices_b.sample_sizes": torch.tensor(IDX_SIZES, dtype=it, device=device),
                "weights": (0.2 + 1.8 * torch.rand(B, NB, generator=g)).to(device)}

    def forward(self, t):
        from accvlab.batching_helpers import matched_pair_loss_sum

        return (matched_pair_loss_sum(t["data_a"], t["data_b"], _rb(t["indices_a"], t["indices_a.sample_sizes"]),
                                      _rb(t["indices_b"], t["indices_b.sample_sizes"]), t["weights"], kind="smooth_l1",
                                      beta=0.5),)

    def definition(self, t, gos):
        a, b, w = (t[n].double().requires_grad_(True) for n in self.differentiable)
        rows = [torch.zeros((), dtype=torch.float64) for _ in range(B)]
        for f, j in _valid_slots(t["indices_a.sample_sizes"], NI):
            ia, ib = int(t["indices_a"][f, j]), int(t["indices_b"][f, j])
            per = torch.nn.functional.smooth_l1_loss(a[f, ia], b[f, ib], beta=0.5, reduction="none").sum()
            rows[f] = rows[f] + per * w[f, ia]
        return dict(zip(self.differentiable, torch.autograd.grad((torch.stack(rows) * gos[0].double()).sum(), (a, b, w))))

    def bound(self, want):   # test_matched_pair_loss_gpu.py: 1e-5 * max(1, max |gradient of the composition|)
        return torch.full_like(want, 1e-5 * max(1.0, float(want.abs().max())))

    def check(self, name, got, want, device, what):
        err = (got.detach().cpu().double() - want).abs()
        assert bool((err <= self.bound(want)).all()), f"{what}: max error {float(err.max()):.3e}"


class _Indexed(Case):
    """the four ragged gather / scatter operators: the gradient is an indexed copy of the upstream gradient"""
    devices = ("cuda",)
    reads = (("indices", "index"), ("indices.sample_sizes", "sizes"))

    def indices(self, t, device, cfg):
        t["indices"] = torch.tensor([[5, 0, 2, 3], [1, 4, 0, 2]], dtype=INT[cfg], device=device)
        t["indices.sample_sizes"] = torch.tensor(IDX_SIZES, dtype=INT[cfg], device=device)
        return t

    def rb(self, t):
        return _rb(t["indices"], t["indices.sample_sizes"])

    def composed(self, t, leaves):
        raise NotImplementedError

    def definition(self, t, gos):
        leaves = {n: t[n].double().requires_grad_(True) for n in self.differentiable}
        out = self.composed(t, leaves)
        grads = torch.autograd.grad((out * gos[0].double()).sum(), list(leaves.values()), allow_unused=True)
        return {n: torch.zeros_like(leaves[n]) if g is None else g for n, g in zip(leaves, grads)}

    def bound(self, want):   # test_batching_helpers_gpu.py::test_index_mapping_random_and_backward: < 1e-5
        return torch.full_like(want, 1e-5)

    def check(self, name, got, want, device, what):
        err = (got.detach().cpu().double() - want).abs()
        assert bool((err < self.bound(want)).all()), f"{what}: max error {float(err.max()):.3e}"


class IndexingAccess(_Indexed):
    name = "batched_indexing_access"
    differentiable = ("input_data",)
    ignores = (("input_data", "float"),)

    def build(self, device, cfg):
        return self.indices({"input_data": torch.randn(B, NB, 3, generator=_gen(12)).to(device)}, device, cfg)

    def forward(self, t):
        from accvlab.batching_helpers import batched_indexing_access

        return (batched_indexing_access(t["input_data"], self.rb(t)).tensor,)

    def composed(self, t, x):
        out = torch.zeros(B, NI, 3, dtype=torch.float64)
        for f, j in _valid_slots(t["indices.sample_sizes"], NI):
            out[f, j] = x["input_data"][f, int(t["indices"][f, j])]
        return out


class InverseIndexingAccess(_Indexed):
    name = "batched_inverse_indexing_access"
    differentiable = ("input_data",)
    ignores = (("input_data", "float"),)

    def build(self, device, cfg):
        return self.indices({"input_data": torch.randn(B, NI, 3, generator=_gen(13)).to(device)}, device, cfg)

    def forward(self, t):
        from accvlab.batching_helpers import batched_inverse_indexing_access

        return (batched_inverse_indexing_access(t["input_data"], self.rb(t), NB),)

    def composed(self, t, x):
        out = torch.zeros(B, NB, 3, dtype=torch.float64)
        for f, j in _valid_slots(t["indices.sample_sizes"], NI):
            out[f, int(t["indices"][f, j])] = x["input_data"][f, j]
        return out


class IndexingWrite(_Indexed):
    name = "batched_indexing_write"
    differentiable = ("to_write", "to_write_into")
    ignores = (("to_write", "float"), ("to_write_into", "float"))

    def build(self, device, cfg):
        g = _gen(14)
        return self.indices({"to_write": torch.randn(B, NI, 3, generator=g).to(device),
                             "to_write_into": torch.randn(B, NB, 3, generator=g).to(device)}, device, cfg)

    def forward(self, t):
        from accvlab.batching_helpers import batched_indexing_write

        return (batched_indexing_write(t["to_write"], self.rb(t), t["to_write_into"]),)

    def composed(self, t, x):
        out = x["to_write_into"].clone()
        for f, j in _valid_slots(t["indices.sample_sizes"], NI):
            out[f, int(t["indices"][f, j])] = x["to_write"][f, j]
        return out


class IndexMapping(_Indexed):
    name = "batched_index_mapping"
    differentiable = ("source_data", "target_data")
    reads = (("source_indices", "index"), ("target_indices", "index"), ("source_indices.sample_sizes", "sizes"))
    ignores = (("source_data", "float"), ("target_data", "float"), ("target_indices.sample_sizes", "sizes"))

    def build(self, device, cfg):
        g, it = _gen(15), INT[cfg]
        return {"source_data": torch.randn(B, NB, 3, generator=g).to(device),
                "target_data": torch.randn(B, 5, 3, generator=g).to(device),
                "source_indices": torch.tensor([[5, 0, 5, 3], [1, 1, 0, 2]], dtype=it, device=device),   # sources repeat
                "target_indices": torch.tensor([[4, 1, 0, 2], [3, 0, 2, 1]], dtype=it, device=device),
                "source_indices.sample_sizes": torch.tensor(IDX_SIZES, dtype=it, device=device),
                "target_indices.sample_sizes": torch.tensor(IDX_SIZES, dtype=it, device=device)}

    def forward(self, t):
        from accvlab.batching_helpers import batched_index_mapping

        return (batched_index_mapping(t["source_data"], _rb(t["source_indices"], t["source_indices.sample_sizes"]),
                                      _rb(t["target_indices"], t["target_indices.sample_sizes"]), t["target_data"]),)

    def composed(self, t, x):
        out = x["target_data"].clone()
        for f, j in _valid_slots(t["source_indices.sample_sizes"], NI):
            out[f, int(t["target_indices"][f, j])] = x["source_data"][f, int(t["source_indices"][f, j])]
        return out


class PaddedSetTo(Case):
    name = "RaggedBatch.with_padded_set_to"
    differentiable = ("tensor",)
    reads = (("sample_sizes", "sizes"),)
    ignores = (("tensor", "float"),)
    once = False
    VALUE = 7.0

    def build(self, device, cfg):
        return {"tensor": torch.randn(B, 5, 3, generator=_gen(16)).to(device),
                "sample_sizes": torch.tensor([5, 3], dtype=INT[cfg], device=device)}

    def forward(self, t):
        return (_rb(t["tensor"], t["sample_sizes"]).with_padded_set_to(self.VALUE).tensor,)

    def composed(self, x, sizes):
        """the definition: differentiable any number of times"""
        live = (torch.arange(x.shape[1]).view(1, -1) < sizes.cpu().long().view(-1, 1)).unsqueeze(-1)
        return torch.where(live, x, torch.full_like(x, self.VALUE))

    def definition(self, t, gos):
        x = t["tensor"].double().requires_grad_(True)
        grad, = torch.autograd.grad((self.composed(x, t["sample_sizes"]) * gos[0].double()).sum(), x)
        return {"tensor": grad}

    def bound(self, want):   # test_batching_helpers_gpu.py compares this gradient with torch.equal
        return torch.zeros_like(want)

    def check(self, name, got, want, device, what):
        assert torch.equal(got.detach().cpu().double(), want), what


# ------------------------------------------------------------------------------------------------ the polyline operators
class Polyline(Case):
    """interpolate (relative) or lengths, fixed-size or ragged"""

    def __init__(self, op, var):
        self.op, self.var = op, var
        self.name = op + ("_var_size_batch" if var else "")
        self.cfgs = CFGS if var else ("i64",)
        self.differentiable = ("points", "distances") if op == "interpolate" else ("points",)
        reads = [("points", "float")] + ([("distances", "float")] if op == "interpolate" else [])
        if var:
            reads += [("points.sample_sizes", "sizes")] + ([("distances.sample_sizes", "sizes")] if op == "interpolate" else [])
        self.reads = tuple(reads)

    def build(self, device, cfg):
        g = _gen(17)
        t = {"points": torch.randn(B, 6, 2, generator=g, dtype=torch.float64).cumsum(1).float().to(device)}
        if self.op == "interpolate":
            t["distances"] = (torch.rand(B, 4, generator=g, dtype=torch.float64) * 0.9 + 0.05).float().to(device)
        if self.var:
            t["points.sample_sizes"] = torch.tensor([6, 4], dtype=INT[cfg], device=device)
            if self.op == "interpolate":
                t["distances.sample_sizes"] = torch.tensor([4, 3], dtype=INT[cfg], device=device)
        return t

    def forward(self, t):
        from accvlab.lane_helpers import polyline

        if self.op == "lengths":
            return (polyline.lengths_var_size_batch(_rb(t["points"], t["points.sample_sizes"])) if self.var
                    else polyline.lengths(t["points"]),)
        if self.var:
            return (polyline.interpolate_var_size_batch(_rb(t["points"], t["points.sample_sizes"]),
                                                        _rb(t["distances"], t["distances.sample_sizes"]), relative=True).tensor,)
        return (polyline.interpolate(t["points"], t["distances"], relative=True),)

    def definition(self, t, gos, device="cpu"):
        inter = self.op == "interpolate"
        eps = torch.finfo(torch.float64 if device == "cpu" else F32).eps   # the host path evaluates in double
        gp, gd = polyline_ref_grads(t["points"], t.get("distances"), gos[0] if inter else None, None if inter else gos[0],
                                    t.get("points.sample_sizes"), t.get("distances.sample_sizes"), True, eps=eps)
        return {"points": gp, "distances": gd} if inter else {"points": gp}

    def check(self, name, got, want, device, what):
        if device == "cpu":   # test_polyline_grad_cpu.py::test_host_backward_matches_reference, float32
            rtol = 2 * torch.finfo(F32).eps
            polyline_close_host(got.detach(), want, rtol=rtol, atol_frac=rtol)
        else:                 # test_polyline_grad_gpu.py::test_f32_matches_float64_reference
            from test_polyline_grad_gpu import _check

            _check(got.detach(), want, 1e-4, 1e-6, what)


CASES = [GaussianFocal((3, 5, 9), "scalar tail"), GaussianFocal((2, 8, 16), "vector path"), GatherRagged(), GatherIndices(),
         CenterRegression(), MatchedPair(), MatchedFocal(), MatchedBox(), MatchedPolyline(), Polyline("interpolate", False),
         Polyline("interpolate", True), Polyline("lengths", False), Polyline("lengths", True), IndexingAccess(),
         InverseIndexingAccess(), IndexingWrite(), IndexMapping(), PaddedSetTo()]


def params(device):
    """(case, cfg) of every operator that takes tensors of `device`"""
    return [pytest.param(c, cfg, id=f"{c.name}-{cfg}") for c in CASES if device in c.devices for cfg in c.cfgs]


# =============================================================================================================== checks
def set_leaves(case, t, subset=None):
    """fresh leaves for the differentiable inputs; only those in `subset` (default: all) require a gradient"""
    for n in case.differentiable:
        t[n] = t[n].detach().clone().requires_grad_(subset is None or n in subset)
    return t


def upstream(outs, seed=1):
    """one random upstream gradient in [0.5, 1.5] per output (partition_edges_cases.grad_out's range)"""
    g = _gen(seed)
    return tuple((torch.rand(o.shape, generator=g) + 0.5).to(o.dtype).to(o.device) for o in outs)


def gradients(case, t, outs, gos, **kw):
    names = [n for n in case.differentiable if t[n].requires_grad]
    return dict(zip(names, torch.autograd.grad(list(outs), [t[n] for n in names], list(gos), **kw)))


def wanted(case, t, gos, device, **kw):
    if isinstance(case, Polyline):
        kw["device"] = device
    return case.definition(_cpu(t), tuple(g.detach().cpu() for g in gos), **kw)


def compare(case, got, want, device, what):
    for n, g in got.items():
        case.check(n, g, want[n], device, f"{case.name} {what}: d/d {n}")


def mutate(tensor, kind):
    """other valid values in the same storage: float x -1.5, sizes - 1, index tensors shifted by one slot"""
    with torch.no_grad():
        if kind == "float":
            tensor.mul_(-1.5)
        elif kind == "sizes":
            tensor.sub_(1)
        else:
            tensor.copy_(tensor.roll(1, 1))


def prepared(case, device, cfg):
    """-> (inputs with fresh leaves, outputs, upstream gradients, the definition's gradients at these inputs)"""
    t = set_leaves(case, case.build(device, cfg))
    kw = {"margin": True} if isinstance(case, MatchedPolyline) else {}
    outs = case.forward(t)
    gos = upstream(outs)
    return t, outs, gos, wanted(case, t, gos, device, **kw)


def check_forward_backward(case, device, cfg):
    """the base line every other check builds on"""
    t, outs, gos, want = prepared(case, device, cfg)
    compare(case, gradients(case, t, outs, gos), want, device, "plain")


def check_stale_reads(case, device, cfg):
    """1. a tensor the backward reads is overwritten between forward and backward"""
    failures = []
    for name, kind in case.reads:
        t, outs, gos, want = prepared(case, device, cfg)
        mutate(t[name], kind)
        new = wanted(case, t, gos, device)
        assert any(bool(((new[n] - want[n]).abs() >= (100 * case.bound(want[n])).clamp_min(1e-300)).any()) for n in want), \
            f"{case.name}: overwriting {name} does not move the definition's gradient by 100 x the tolerance"
        try:
            got = gradients(case, t, outs, gos)
        except RuntimeError as e:
            if STALE not in str(e):
                failures.append(f"{name}: {type(e).__name__}: {e}")
            continue
        if not case.copied(name, cfg):
            failures.append(f"{name}: shares the caller's storage, backward must raise '{STALE}', it returned a gradient")
            continue
        try:
            compare(case, got, want, device, f"after overwriting {name}")
        except AssertionError as e:
            failures.append(f"{name}: gradient of the overwritten values: {e}")
    assert not failures, f"{case.name} [{cfg}, {device}]:\n  " + "\n  ".join(failures)


def check_unread_inputs(case, device, cfg):
    """2. a tensor the backward does not receive is overwritten between forward and backward"""
    failures = []
    for name, kind in case.ignores:
        t, outs, gos, want = prepared(case, device, cfg)
        mutate(t[name], kind)
        try:
            compare(case, gradients(case, t, outs, gos), want, device, f"after overwriting {name}")
        except (RuntimeError, AssertionError) as e:
            failures.append(f"{name}: {type(e).__name__}: {str(e).splitlines()[0]}")
    assert not failures, f"{case.name} [{cfg}, {device}]:\n  " + "\n  ".join(failures)


def check_inputs_die(case, device, cfg):
    """3. every reference to the read tensors is dropped after the forward and their memory handed out again"""
    t = case.build(device, cfg)
    leaves = {n: t[n].detach().clone().requires_grad_(True) for n in case.differentiable}
    for n, x in leaves.items():
        t[n] = x.clone()       # what the operator sees is not the leaf: it can be dropped
    outs = case.forward(t)
    gos = upstream(outs)
    want = wanted(case, {**t, **leaves}, gos, device, **({"margin": True} if isinstance(case, MatchedPolyline) else {}))
    specs = [(t[n].shape, t[n].dtype) for n, _ in case.reads]
    del t, n, x
    gc.collect()
    g = _gen(99)
    decoys = [(torch.randn(s, generator=g) * 3.0).to(d).to(device) if d.is_floating_point else
              torch.zeros(s, dtype=d, device=device) for s, d in specs for _ in range(2)]
    got = dict(zip(leaves, torch.autograd.grad(list(outs), list(leaves.values()), list(gos))))
    compare(case, got, want, device, "after its inputs died")
    assert len(decoys) == 2 * len(specs)


def check_backward_twice(case, device, cfg):
    """4. two retained backwards give the same bits; once the graph is released, another one raises torch's error"""
    t, outs, gos, want = prepared(case, device, cfg)
    first = gradients(case, t, outs, gos, retain_graph=True)
    second = gradients(case, t, outs, gos, retain_graph=True)
    for n in first:
        assert torch.equal(first[n], second[n]), f"{case.name}: two backwards differ in d/d {n}"
    compare(case, first, want, device, "first of two backwards")
    gradients(case, t, outs, gos)                      # without retain_graph: releases what was saved
    with pytest.raises(RuntimeError, match=TWICE):
        gradients(case, t, outs, gos)


def check_needs_input_grad(case, device, cfg):
    """5. every non-empty subset of the differentiable inputs requires a gradient; and none does"""
    names = case.differentiable
    for r in range(1, len(names) + 1):
        for subset in itertools.combinations(names, r):
            t = set_leaves(case, case.build(device, cfg), subset)
            outs = case.forward(t)
            gos = upstream(outs)
            want = wanted(case, t, gos, device)
            torch.autograd.backward(list(outs), list(gos))
            for n in names:
                if n not in subset:
                    assert t[n].grad is None, f"{case.name}: {n} needs no gradient and got one (subset {subset})"
            compare(case, {n: t[n].grad for n in subset}, want, device, f"subset {subset}")
    t = set_leaves(case, case.build(device, cfg), ())
    for o in case.forward(t):
        assert not o.requires_grad and o.grad_fn is None, f"{case.name}: no input requires a gradient, the output does"


def check_grad_out_layouts(case, device, cfg):
    """6. expanded (stride 0), non-contiguous and float64 upstream gradients"""
    for layout in ("expanded", "strided", "float64"):
        t = set_leaves(case, case.build(device, cfg))
        outs = case.forward(t)
        if layout == "expanded":      # what out.sum().backward() hands down
            gos = tuple(torch.full((), 0.75, dtype=o.dtype, device=o.device).expand(o.shape) for o in outs)
            assert all(o.dim() == 0 or set(g.stride()) == {0} for o, g in zip(outs, gos))
        else:
            gos = tuple(torch.stack([g, -g], -1)[..., 0] for g in upstream(outs, seed=2))
            assert all(o.dim() == 0 or not g.is_contiguous() for o, g in zip(outs, gos))
        want = wanted(case, t, gos, device)
        if layout == "float64":       # reaches the float32 output through .double()
            outs, gos = tuple(o.double() for o in outs), tuple(g.double() for g in gos)
        compare(case, gradients(case, t, outs, gos), want, device, f"{layout} grad_out")


def check_second_derivative(case, device, cfg):
    """7. a second derivative raises, or is right"""
    t = set_leaves(case, case.build(device, cfg))
    xs = [t[n] for n in case.differentiable]
    if case.once:
        # the upstream gradient of sum(out^2) depends on the inputs: the first derivative is part of the graph
        first = torch.autograd.grad(sum(o.square().sum() for o in case.forward(t)), xs, create_graph=True)
        with pytest.raises(RuntimeError, match=ONCE):   # backward(): every node below the sum runs
            torch.autograd.backward(sum(g.sum() for g in first))
        # that of sum(out) does not: either the same error or torch's own refusal, never a silent value
        first = torch.autograd.grad(sum(o.sum() for o in case.forward(t)), xs, create_graph=True)
        with pytest.raises(RuntimeError, match=ONCE + "|does not require grad"):
            torch.autograd.backward(sum(g.sum() for g in first))
        return
    # not marked: float64 autograd of the definition, through the inputs and through the upstream gradient
    assert isinstance(case, PaddedSetTo)
    sizes = t["sample_sizes"]
    gen = _gen(5)
    x0 = torch.randn(t["tensor"].shape, generator=gen, dtype=torch.float64)
    v0, w0 = (torch.rand(x0.shape, generator=gen, dtype=torch.float64) + 0.5 for _ in range(2))
    results = []
    for op, dev in ((lambda x: case.forward({"tensor": x, "sample_sizes": sizes})[0], device),
                    (lambda x: case.composed(x, sizes), "cpu")):
        x, v, w = (a.to(dev).requires_grad_(True) for a in (x0, v0, w0))
        first, = torch.autograd.grad((op(x) ** 3 * v).sum(), x, create_graph=True)
        results.append([g.cpu() for g in torch.autograd.grad((first * w).sum(), (x, v))])
        plain, = torch.autograd.grad(op(x), x, v, create_graph=True)       # the operator's own backward, differentiated
        results[-1].append(torch.autograd.grad((plain * w).sum(), v)[0].cpu())
    for got, want, what in zip(*results, ("d2/dx2", "d2/dx dv", "d backward / d grad_out")):
        assert float((got - want).abs().max()) <= 1e-10, f"{case.name}: {what} off by {float((got - want).abs().max()):.3e}"


def check_saved_tensor_hooks(case, device, cfg):
    """beyond the seven: under saved-tensor hooks that pack a private copy (as torch.autograd.graph.save_on_cpu does),
    the backward must read what torch unpacks, not a pointer remembered from the forward: every read tensor is
    overwritten, no version check applies to the copies, and the gradient must be that of the forward-time values"""
    t = set_leaves(case, case.build(device, cfg))
    with torch.autograd.graph.saved_tensors_hooks(lambda x: x.clone(), lambda x: x):
        outs = case.forward(t)
    gos = upstream(outs)
    want = wanted(case, t, gos, device)
    for name, kind in case.reads:
        mutate(t[name], kind)
    compare(case, gradients(case, t, outs, gos), want, device, "with packed copies, every read overwritten")


CHECKS = [check_forward_backward, check_stale_reads, check_unread_inputs, check_inputs_die, check_backward_twice,
          check_needs_input_grad, check_grad_out_layouts, check_second_derivative, check_saved_tensor_hooks]
