"""The refusals of the two-backend operators, word for word: every bad-argument call of operand_errors_cases.py raises the
exception type and the message recorded in golden/operand_errors.json (made by golden/make_operand_errors.py), so a
reworded check, or two checks that change places, fails here.  CPU tensors only; every call is refused before any native
call."""
import json
import os

import pytest

import operand_errors_cases as cases
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "operand_errors.json")) as _f:
    TABLE = json.load(_f)
CASES = cases.cases()


def test_table_and_cases_name_the_same_calls():
    assert sorted(TABLE) == sorted(CASES)


@pytest.mark.parametrize("key", sorted(TABLE))
def test_refusal(key):
    assert cases.outcome(CASES[key]) == TABLE[key]
