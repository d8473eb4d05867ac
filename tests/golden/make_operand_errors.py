#!/usr/bin/env python3
"""Generates tests/golden/operand_errors.json: case id -> [exception type name, message] of every bad-argument call of
tests/operand_errors_cases.py, as the wrappers refuse it at the commit this is run on.  CPU tensors only; needs the built
library for the imports, calls no native entry.  Run it on the commit whose refusals are the reference, not after a change
to the wrappers: the table is what test_operand_errors_cpu.py holds later commits to."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path[:0] = [os.path.join(ROOT, "accv-lab_amd"), ROOT, os.path.join(ROOT, "tests")]

import operand_errors_cases as cases  # noqa: E402

table = {key: cases.outcome(call) for key, call in cases.cases().items()}
accepted = [key for key, (kind, _) in table.items() if not kind]
assert not accepted, f"not refused: {accepted}"
path = os.path.join(HERE, "operand_errors.json")
with open(path, "w") as f:
    json.dump(table, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", len(table), "cases", os.path.getsize(path), "bytes")
