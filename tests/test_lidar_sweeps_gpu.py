"""The seeded sweeps of tests/lidar_sweep_cases.py on the GPU: the HIP kernels of the lidar branch (voxelize_points,
pillar_features, voxel_mean, scatter_to_bev with its backward, their chain, lidar_depth_targets) and of the two query
decoders against their definitions through the check functions of test_lidar_sweeps_cpu.py (the operators' own comparisons,
no tolerance added or moved), and against their host entries on every output of every draw, over random combinations of
shape, dtype, alignment, ragged sizes and flags that the hand-picked cases cross one at a time.  The
constants that the value lists straddle are read from the .hip sources here and held against the literals of the draws.
ACCV_FUZZ_SCALE=k runs k times as many seeds.  After a complete run the worst error seen per operator and dtype goes to
profiles/lidar_sweeps_accuracy.log; a partial run writes nothing."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lidar_sweep_cases as sw  # noqa: E402
import test_lidar_sweeps_cpu as host_checks  # noqa: E402
from test_lidar_sweeps_cpu import report_redraws, seeds  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = "exact"      # the dtype column of an operator whose outputs are compared bit for bit


def _constants(source, *names):
    text = open(os.path.join(ROOT, "accv-lab_amd", "csrc", source)).read()
    return text, tuple(int(re.search(rf"constexpr int {n} = (\d+);", text).group(1)) for n in names)


_PF, (PF_MAX_GROUP, PF_LDS_FLOATS) = _constants("pillar_features.hip", "kMaxGroup", "kLdsFloats")
assert (PF_MAX_GROUP, PF_LDS_FLOATS) == (sw.MAX_GROUP, sw.LDS_FLOATS)
assert "const long long fit = kLdsFloats / (T * D);" in _PF and "fit > kMaxGroup ? kMaxGroup : fit" in _PF      # group_of
_, (VX_SCAN_THREADS, VX_UNROLL) = _constants("voxelize.hip", "kScanThreads", "kUnroll")
assert VX_SCAN_THREADS * VX_UNROLL == sw.SCAN_CHUNK and {sw.SCAN_CHUNK - 1, sw.SCAN_CHUNK + 1} <= set(sw.VOX_P)
_BS, BS_CONSTANTS = _constants("bev_scatter.hip", "kThreads", "kTileW", "kChunk")
assert BS_CONSTANTS == (sw.THREADS, sw.TILE, sw.CHUNK)
assert "(a.C * esize) % 16 == 0 && (a.nx * esize) % 16 == 0" in _BS                                           # write_path_of
_, (QD_THREADS, QD_UNROLL) = _constants("query_decode.hip", "kThreads", "kUnroll")
assert (QD_THREADS, QD_UNROLL) == (sw.Q_THREADS, sw.Q_UNROLL) and QD_THREADS * QD_UNROLL in sw.DECODE_N


@pytest.fixture(scope="module")
def worst():
    """every sweep records its largest errors here; written out once every seed of every sweep of the module is through"""
    seen = sw.Worst()
    seen.done = set()
    yield seen
    if seen.done != {(op, s) for op in sw.SWEEPS for s in seeds(op)}:      # a partial run (-k, -x) leaves no log
        return
    lines = [f"lidar sweeps on {torch.cuda.get_device_name(0)} (tests/test_lidar_sweeps_gpu.py, ACCV_FUZZ_SCALE "
             f"{os.environ.get('ACCV_FUZZ_SCALE', '1')}): the largest error seen per operator and dtype.  Every output of every case",
             "is bit-equal between the device and the host entry (asserted), except where a 'vs_host' figure is listed.",
             "oracle_b: lidar_depth_targets against its float64 oracle (b) on placed cases without image transforms, as a share",
             "of its bar 6 x 2^-24 x largest intermediate (bound 1).  approx / approx_vs_host: the decoders' exp sizes, yaw and",
             "bottom z against float64 and against the host entry, absolute (bar 1e-5); score / score_vs_host: their sigmoid",
             "scores likewise.  The dtype of a decoder line is that of its scores."]
    lines += seen.lines()
    try:
        with open(os.path.join(ROOT, "profiles", "lidar_sweeps_accuracy.log"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:      # a read-only checkout: the figures were asserted all the same
        pass


def both_devices(op, seed):
    """the cases of one seed drawn on the device and on the host: (tag, device inputs, kwargs, host inputs, host kwargs)"""
    for (tag, inp, kw), (_, hinp, hkw) in zip(sw.sweep(op, seed, DEV), sw.sweep(op, seed, "cpu")):
        yield tag, inp, kw, hinp, hkw


def same_bits(a, b, what):
    assert a.is_cuda and not b.is_cuda and a.dtype == b.dtype and a.shape == b.shape, what
    view = {4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[a.element_size()]
    assert torch.equal(a.detach().contiguous().view(view).cpu(), b.detach().contiguous().view(view)), f"{what}: device and host entry differ"


# --------------------------------------------------------------------------------------- pillar_features and voxel_mean
@pytest.mark.parametrize("seed", seeds("pillar_features"))
def test_pillar_features_sweep(seed, worst):
    for tag, inp, kw, hinp, _ in both_devices("pillar_features", seed):
        got = host_checks.check_pillar_features(tag + " device", inp, kw)
        same_bits(got, host_checks.check_pillar_features(tag + " host", hinp, kw), tag)
        worst.add("pillar_features", EXACT)
    worst.done.add(("pillar_features", seed))


@pytest.mark.parametrize("seed", seeds("voxel_mean"))
def test_voxel_mean_sweep(seed, worst):
    for tag, inp, kw, hinp, _ in both_devices("voxel_mean", seed):
        got = host_checks.check_voxel_mean(tag + " device", inp, kw)
        same_bits(got, host_checks.check_voxel_mean(tag + " host", hinp, kw), tag)
        worst.add("voxel_mean", EXACT)
    worst.done.add(("voxel_mean", seed))


# ------------------------------------------------------------------------------------------------------- scatter_to_bev
@pytest.mark.parametrize("seed", seeds("scatter_to_bev"))
def test_scatter_to_bev_sweep(seed, worst):
    for tag, inp, kw, hinp, _ in both_devices("scatter_to_bev", seed):
        assert inp["features"].is_cuda and inp["grad"].is_cuda
        got = host_checks.check_scatter_to_bev(tag + " device", inp, kw)
        host = host_checks.check_scatter_to_bev(tag + " host", hinp, kw)
        for a, b, what in zip(got, host, ("canvas", "index", "grad_features")):
            same_bits(a, b, f"{tag}: {what}")
        worst.add("scatter_to_bev + backward", kw["dtype"])
    worst.done.add(("scatter_to_bev", seed))


# ------------------------------------------------------------------------------------------ voxelize_points, the chain
@pytest.mark.parametrize("seed", seeds("voxelize_points"))
def test_voxelize_points_sweep(seed, worst):
    import voxelize_cases as vx

    for tag, inp, kw, hinp, _ in both_devices("voxelize_points", seed):
        got = host_checks.check_voxelize_points(tag + " device", inp, kw)
        assert all(t.is_cuda for t in got)
        vx.check_equal(got, host_checks.check_voxelize_points(tag + " host", hinp, kw), tag + ": device against host entry")
        worst.add("voxelize_points", EXACT)
    worst.done.add(("voxelize_points", seed))


@pytest.mark.parametrize("seed", seeds("lidar_chain"))
def test_lidar_chain_sweep(seed, worst):
    stages = ("voxels", "coors", "num_points", "voxel_counts", "point_voxel", "pillar_features", "pillar_features, concatenated", "canvas",
              "index", "grad_features", "flat canvas", "flat index", "flat grad_features")
    for tag, inp, kw, hinp, _ in both_devices("lidar_chain", seed):
        got = host_checks.check_lidar_chain(tag + " device", inp, kw)
        host = host_checks.check_lidar_chain(tag + " host", hinp, kw)
        assert len(got) == len(host) == len(stages)
        for a, b, what in zip(got, host, stages):
            same_bits(a, b, f"{tag}: {what}")
        worst.add("voxelize_points -> pillar_features -> scatter_to_bev + backward", kw["dtype"])
    worst.done.add(("lidar_chain", seed))


# -------------------------------------------------------------------------------------------------- lidar_depth_targets
@pytest.mark.parametrize("seed", seeds("lidar_depth_targets"))
def test_lidar_depth_targets_sweep(seed, worst):
    for tag, inp, kw in sw.sweep("lidar_depth_targets", seed):
        got, share = host_checks.check_lidar_depth_targets(tag + " device", inp, kw, DEV)
        host, _ = host_checks.check_lidar_depth_targets(tag + " host", inp, kw, "cpu")
        same_bits(got.depth, host.depth, tag + ": depth")
        assert (got.bins is None) == (host.bins is None), tag
        if got.bins is not None:
            same_bits(got.bins, host.bins, tag + ": bins")
        if share is None:
            worst.add("lidar_depth_targets", EXACT)
        else:
            worst.add("lidar_depth_targets", torch.float32, oracle_b=share)
    worst.done.add(("lidar_depth_targets", seed))


# ------------------------------------------------------------------------------------------------------ the two decoders
def largest(got, want):
    """the largest absolute difference where both sides are finite (check has already matched NaN and infinities)"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(g) & np.isfinite(w)
    return float(np.abs(g[ok] - w[ok]).max()) if ok.any() else 0.0


def decoder_sweep(which, seed, worst):
    import query_decode_cases as qc

    from accvlab.draw_heatmap import query_box_decode_2d, query_box_decode_3d

    op = "query_box_decode_" + which
    fn = query_box_decode_3d if which == "3d" else query_box_decode_2d
    before, cases = sw.REDRAWS[op], 0
    for tag, inp, kw in sw.sweep(op, seed, DEV):
        cases += 1
        got, want = host_checks.check_query_decode(which, tag + " device", inp, kw)
        assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for x in got)
        cls, rows, M = inp
        host = fn(cls.cpu(), rows.cpu(), M, **{k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        qc.check_device_against_host(got, host, want["approx_channels"], want["logits"], tag + " device against host")
        figures, ch = {}, want["approx_channels"]
        boxes = got.boxes.tensor.cpu().numpy()
        if ch:
            figures.update(approx=largest(boxes[..., ch], want["approx"][..., ch]),
                           approx_vs_host=largest(boxes[..., ch], host.boxes.tensor.numpy()[..., ch]))
        if want["logits"]:
            figures.update(score=largest(got.scores.tensor.cpu().numpy(), want["score_approx"]),
                           score_vs_host=largest(got.scores.tensor.cpu().numpy(), host.scores.tensor.numpy()))
        worst.add(op, cls.dtype if figures else EXACT, **figures)
    report_redraws(op, cases, sw.REDRAWS[op] - before)
    worst.done.add((op, seed))


@pytest.mark.parametrize("seed", seeds("query_box_decode_3d"))
def test_query_box_decode_3d_sweep(seed, worst):
    decoder_sweep("3d", seed, worst)


@pytest.mark.parametrize("seed", seeds("query_box_decode_2d"))
def test_query_box_decode_2d_sweep(seed, worst):
    decoder_sweep("2d", seed, worst)
