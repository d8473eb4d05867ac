"""scripts/measure.py on the host: `summary` is arithmetic on a list (the expected values are written out), and the shared
parser yields the defaults a script passes in."""
import os
import sys

import pytest

sys.path.append(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))   # last: the root's bench_configs stays first

import measure  # noqa: E402

ODD = [0.51234, 0.49876, 0.50557]
EVEN = [12.34562, 10.00004, 11.5, 13.25]


@pytest.mark.parametrize("ms, kwargs, want", [
    (ODD, dict(), dict(median_ms=0.50557, min_ms=0.49876, timed_s=0.002)),
    (ODD, dict(calls=7, digits=4), dict(median_ms=0.5056, min_ms=0.4988, timed_s=0.011)),
    (ODD, dict(digits=4, with_max=True), dict(median_ms=0.5056, min_ms=0.4988, max_ms=0.5123, timed_s=0.002)),
    (EVEN, dict(), dict(median_ms=11.92281, min_ms=10.00004, timed_s=0.047)),
    (EVEN, dict(calls=7, with_max=True), dict(median_ms=11.92281, min_ms=10.00004, max_ms=13.25, timed_s=0.33)),
    (EVEN, dict(calls=7, digits=4), dict(median_ms=11.9228, min_ms=10.0, timed_s=0.33)),
])
def test_summary_of_a_literal_list(ms, kwargs, want):
    got = measure.summary(list(ms), **kwargs)
    assert got == want and list(got) == list(want)          # the fields and their order are what the logs hold


def test_block_summary_is_the_median_of_block_medians_and_their_spread():
    blocks = [dict(median_ms=0.5, min_ms=0.4, timed_s=0.1), dict(median_ms=0.7, min_ms=0.3, timed_s=0.2),
              dict(median_ms=0.6, min_ms=0.5, timed_s=0.3)]
    assert measure.block_summary(blocks) == dict(block_medians_ms=[0.5, 0.7, 0.6], median_ms=0.6, min_ms=0.3, spread_ms=0.2, timed_s=0.6)


def test_parser_yields_the_defaults_it_was_given():
    args = measure.parser(warmup=3, iters=7, calls=2).parse_args([])
    assert (args.warmup, args.iters, args.calls, args.out) == (3, 7, 2, None)
    args = measure.parser(warmup=5, iters=30).parse_args([])
    assert (args.warmup, args.iters, args.out) == (5, 30, None) and not hasattr(args, "calls")
    args = measure.parser(warmup=3, iters=7, calls=2).parse_args(["--warmup", "1", "--iters", "4", "--calls", "9", "--out", "x.log"])
    assert (args.warmup, args.iters, args.calls, args.out) == (1, 4, 9, "x.log")


def test_shown_renders_only_none():
    assert measure.shown(None) == "not measured" and measure.shown(0) == 0 and measure.shown(3) == 3


def test_emit_prints_and_writes_the_same_lines(tmp_path, capsys):
    out = tmp_path / "sub" / "log.txt"
    measure.emit(["a", "b", "c"], str(out), printed=2)
    assert capsys.readouterr().out == "c\n" and out.read_text() == "a\nb\nc\n"
    measure.emit(["a", "b"])
    assert capsys.readouterr().out == "a\nb\n"
