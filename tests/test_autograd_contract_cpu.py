"""The autograd contract of every differentiable operator that accepts CPU tensors, through its host
path: matched_focal_loss, matched_box_loss, matched_polyline_loss, the polyline operators and
RaggedBatch.with_padded_set_to.  Operators, definitions and checks are those of autograd_contract_cases.py; the
comparison rules are those of each operator's own test file.  Needs no GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autograd_contract_cases as ac  # noqa: E402

PARAMS = ac.params("cpu")


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_gradient_meets_the_definition(case, cfg):
    ac.check_forward_backward(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_stale_inputs_never_reach_the_gradient(case, cfg):
    ac.check_stale_reads(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_unread_inputs_may_change(case, cfg):
    ac.check_unread_inputs(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_inputs_may_die(case, cfg):
    ac.check_inputs_die(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_backward_twice(case, cfg):
    ac.check_backward_twice(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_only_some_inputs_need_a_gradient(case, cfg):
    ac.check_needs_input_grad(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_layouts_of_grad_out(case, cfg):
    ac.check_grad_out_layouts(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_second_derivatives_fail_loudly_or_are_right(case, cfg):
    ac.check_second_derivative(case, "cpu", cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_backward_reads_what_torch_unpacks(case, cfg):
    ac.check_saved_tensor_hooks(case, "cpu", cfg)
