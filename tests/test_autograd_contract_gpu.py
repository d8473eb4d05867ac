"""The autograd contract of every public differentiable operator on the device: what may change between
forward and backward, what may not, and what the backward does with the graph torch hands it.  Operators, definitions and
checks are those of autograd_contract_cases.py; the comparison rules are those of each operator's own test file."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autograd_contract_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAMS = ac.params("cuda")


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_gradient_meets_the_definition(case, cfg):
    ac.check_forward_backward(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_stale_inputs_never_reach_the_gradient(case, cfg):
    ac.check_stale_reads(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_unread_inputs_may_change(case, cfg):
    ac.check_unread_inputs(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_inputs_may_die(case, cfg):
    """no empty_cache(): freed blocks stay mapped, so a lifetime bug shows as a wrong value"""
    ac.check_inputs_die(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_backward_twice(case, cfg):
    ac.check_backward_twice(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_only_some_inputs_need_a_gradient(case, cfg):
    ac.check_needs_input_grad(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_layouts_of_grad_out(case, cfg):
    ac.check_grad_out_layouts(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_second_derivatives_fail_loudly_or_are_right(case, cfg):
    ac.check_second_derivative(case, DEV, cfg)


@pytest.mark.parametrize("case,cfg", PARAMS)
def test_backward_reads_what_torch_unpacks(case, cfg):
    ac.check_saved_tensor_hooks(case, DEV, cfg)
