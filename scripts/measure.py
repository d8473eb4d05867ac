"""What the per-operator scripts/bench_*.py share: two timing schedules between device events, a host-clock timer, three
counters through torch's own instruments, and the prologue and epilogue of a script.  The recorded logs under profiles/
were made with these schedules; a script's docstring says which one it uses and with which counts.

    window_times   `iters` windows of `calls` back-to-back calls between two device events; the sides alternate window by
                   window, one synchronisation per round of sides.  Per-call ms, one value per window.
    call_times     one call per event pair; the sides take turns inside an iteration; no synchronisation until the end.
    wall_times     the host clock around one call plus a synchronisation, for sides that take tens of milliseconds.
    summary        median / min [/ max] / total of such a list, rounded as the script prints it.

Importing this module puts the repository root, the package, examples/ and tests/ (the shared case builders) on sys.path.
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd"), os.path.join(ROOT, "examples"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def parser(warmup, iters, calls=None):
    """the options every script has, with the script's own defaults; `--calls` only for the window schedule"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--iters", type=int, default=iters, help="timed windows (window schedule) or calls (per-call schedule) per side")
    if calls is not None:
        ap.add_argument("--calls", type=int, default=calls, help="back-to-back calls per window")
    ap.add_argument("--out", default=None, help="also write what is printed to this file")
    return ap


def gpu():
    """cuda:0, or the exit every script takes on a machine without one"""
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(sys.argv[0])} measures on a GPU; none is visible")
    return torch.device("cuda", 0)


def emit(lines, out=None, printed=0):
    """print the lines (from `printed` on, for a script that showed the earlier ones as it went), also write all to `out`"""
    print("\n".join(lines[printed:]), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def shown(v):
    return v if v is not None else "not measured"


def window_times(fns, warmup, iters, calls):
    """{name: [ms per call, one per window]}: `warmup` rounds of every side, then `iters` rounds in which every side in turn
    makes `calls` back-to-back calls between two device events"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    events = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            events[k].append((a, b))
        torch.cuda.synchronize()          # keep the queue short: a window must not wait behind the other side's backlog
    return {k: [a.elapsed_time(b) / calls for a, b in v] for k, v in events.items()}


def call_times(fns, warmup, iters):
    """{name: [ms, one per call]}: the callables run one after the other inside every iteration, each between two device
    events of its own.  A callable with a `prepare` attribute gets `prepare()` run outside the timed interval (in warm-up
    too) and its result passed in."""
    for _ in range(warmup):
        for f in fns.values():
            pre = getattr(f, "prepare", None)
            f(pre()) if pre else f()
    torch.cuda.synchronize()
    events = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pre = getattr(f, "prepare", None)
            state = pre() if pre else None
            a.record()
            f(state) if pre else f()
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}


def wall_times(f, iters, warmup=1):
    """[ms, one per call] by the host clock around the call and a synchronisation"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def summary(ms, calls=1, digits=5, with_max=False):
    """median and minimum [and maximum] of the list, and the seconds its `calls`-call entries took together"""
    out = dict(median_ms=round(statistics.median(ms), digits), min_ms=round(min(ms), digits))
    if with_max:
        out["max_ms"] = round(max(ms), digits)
    out["timed_s"] = round(sum(ms) * calls / 1e3, 3)
    return out


def timed_windows(f, warmup, iters, calls):
    """`summary` of the window schedule with one side"""
    return summary(window_times({"f": f}, warmup, iters, calls)["f"], calls)


def block_summary(blocks):
    """a row timed in several blocks (a `summary` each): the median of the block medians, their max - min as the spread"""
    medians = [b["median_ms"] for b in blocks]
    return dict(block_medians_ms=medians, median_ms=round(statistics.median(medians), 5), min_ms=round(min(b["min_ms"] for b in blocks), 5),
                spread_ms=round(max(medians) - min(medians), 5), timed_s=round(sum(b["timed_s"] for b in blocks), 3))


def _device_events(f):
    """the profiler's device-side events of one call of f, after one call outside it"""
    from torch.profiler import ProfilerActivity, profile

    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    return [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]


def launches(f):
    """kernels on the device in one call (copies and memsets are not counted), or None when the profiler cannot tell: every
    timed callable launches at least one, so no kernel event means the profiler saw nothing"""
    try:
        return len([e for e in _device_events(f) if not e.name.lower().startswith(("memcpy", "memset"))]) or None
    except Exception:   # pragma: no cover - profiler builds differ
        return None


def kernel_times(f):
    """name -> device time in ms of every kernel of one call, or None when the profiler cannot tell"""
    try:
        out = {}
        for e in _device_events(f):
            out[e.name] = out.get(e.name, 0.0) + e.device_time / 1e3
        return out
    except Exception:   # pragma: no cover - profiler builds differ
        return None


def round_trips(f):
    """synchronisations of the host with the device in one call, as torch's sync debug mode reports them, or None when the
    debug mode cannot tell"""
    try:
        f()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                f()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return sum("synchroniz" in str(w.message).lower() for w in seen)
    except Exception:   # pragma: no cover - builds differ
        return None
