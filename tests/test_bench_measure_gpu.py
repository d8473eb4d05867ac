"""scripts/measure.py on the device: the two timing schedules make their calls in exactly the order the recorded logs were
made with, the `prepare` hook runs outside every timed call, and the counters never report a measured zero for "saw
nothing".  Every callable appends its name to a list and enqueues one tiny add."""
import os
import sys

import pytest
import torch

sys.path.append(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))   # last: the root's bench_configs stays first

import measure  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def sides():
    x = torch.zeros(8, device="cuda")
    log = []

    def side(name):
        def f():
            log.append(name)
            torch.add(x, 1.0)
        return f

    return log, side("a"), side("b")


def test_window_schedule_alternates_windows_of_back_to_back_calls(sides):
    log, a, b = sides
    ms = measure.window_times({"a": a, "b": b}, warmup=2, iters=3, calls=2)
    assert log == ["a", "b"] * 2 + ["a", "a", "b", "b"] * 3
    assert list(ms) == ["a", "b"] and all(len(v) == 3 and all(t > 0 for t in v) for v in ms.values())


def test_window_schedule_with_one_side(sides):
    log, a, _ = sides
    ms = measure.window_times({"a": a}, warmup=2, iters=3, calls=2)
    assert log == ["a"] * 2 + ["a", "a"] * 3 and len(ms["a"]) == 3 and all(t > 0 for t in ms["a"])
    del log[:]
    s = measure.timed_windows(a, 2, 3, 2)
    assert log == ["a"] * 8 and list(s) == ["median_ms", "min_ms", "timed_s"] and 0 < s["min_ms"] <= s["median_ms"]


def test_per_call_schedule_takes_turns_inside_an_iteration(sides):
    log, a, b = sides
    ms = measure.call_times({"a": a, "b": b}, warmup=2, iters=3)
    assert log == ["a", "b"] * 5
    assert list(ms) == ["a", "b"] and all(len(v) == 3 and all(t > 0 for t in v) for v in ms.values())


def test_prepare_runs_before_every_call_and_hands_its_result_over(sides):
    log, a, _ = sides
    x = torch.zeros(8, device="cuda")
    made = []

    def prepare():
        log.append("prepare")
        made.append(object())
        return made[-1]

    def run(state):
        log.append(("run", state is made[-1]))
        torch.add(x, 1.0)

    run.prepare = prepare
    ms = measure.call_times({"a": a, "p": run}, warmup=2, iters=3)
    assert log == ["a", "prepare", ("run", True)] * 5 and len(made) == 5
    assert len(ms["p"]) == 3 and all(t > 0 for t in ms["p"])


def test_wall_times_makes_one_call_outside_the_timed_ones(sides):
    log, a, _ = sides
    ms = measure.wall_times(a, 3)
    assert log == ["a"] * 4 and len(ms) == 3 and all(t > 0 for t in ms)


def test_launches_counts_kernels_and_never_reports_zero():
    x = torch.zeros(8, device="cuda")

    def two_kernels():
        torch.mul(torch.add(x, 1.0), 2.0)

    assert measure.launches(two_kernels) in (2, None)
    assert measure.launches(lambda: None) is None             # no kernel event: "the profiler saw nothing", not a measured 0
    times = measure.kernel_times(two_kernels)
    assert times is None or (1 <= len(times) <= 2 and sum(times.values()) > 0)       # one name if both kernels share it


def test_round_trips_counts_synchronising_calls():
    x = torch.ones(8, device="cuda")
    n = measure.round_trips(lambda: x.sum().item())
    assert n is None or n >= 1
    assert measure.round_trips(lambda: torch.add(x, 1.0)) in (0, None)
