"""The seeded sweeps of tests/lidar_sweep_cases.py through the host entries of the lidar branch (voxelize_points,
pillar_features, voxel_mean, scatter_to_bev with its backward, their chain, lidar_depth_targets) and of the two query
decoders, against their definitions — the same draws as test_lidar_sweeps_gpu.py, without a GPU: this is what shows that
the references hold over the swept ranges.  Every comparison goes through the operators' own case modules;
no tolerance is added or moved.  The check functions take the inputs on whatever device the draw put them, so the GPU file
runs the same functions on the device.  ACCV_FUZZ_SCALE=k runs k times as many seeds."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lidar_sweep_cases as sw  # noqa: E402
from test_fuzz_gpu import _seeds  # noqa: E402
from test_operator_sweeps_cpu import report_redraws  # noqa: E402


def seeds(op):
    return _seeds(sw.SWEEPS[op][1])


# --------------------------------------------------------------------------------------- pillar_features and voxel_mean
def check_pillar_features(tag, inp, kw):
    """the decoration against the numpy definition, bit for bit; -> the result"""
    import pillar_features_cases as pf

    from accvlab.point_cloud import pillar_features

    got = pillar_features(*inp["args"], **kw)
    first = inp["args"][0]
    assert got.device == (first if isinstance(first, torch.Tensor) else first.voxels).device, tag
    assert tuple(got.shape) == inp["lead"] + (inp["T"], inp["F"]), tag
    assert got.numel() == 0 or got.data_ptr() % 16 == 0, f"{tag}: the output is not 16-byte aligned"
    want = pf.definition(inp["vox"], inp["num"], inp["coors"], **kw)
    pf.assert_bits(got.reshape(want.shape), want, tag)
    return got


@pytest.mark.parametrize("seed", seeds("pillar_features"))
def test_pillar_features_host_sweep(seed):
    for tag, inp, kw in sw.sweep("pillar_features", seed):
        check_pillar_features(tag, inp, kw)


def check_voxel_mean(tag, inp, kw):
    import pillar_features_cases as pf

    from accvlab.point_cloud import voxel_mean

    got = voxel_mean(*inp["args"], **kw)
    want = pf.mean_definition(inp["vox"], inp["num"], kw["num_features"])
    assert tuple(got.shape) == inp["lead"] + (want.shape[-1],), tag
    pf.assert_bits(got.reshape(want.shape), want, tag)
    return got


@pytest.mark.parametrize("seed", seeds("voxel_mean"))
def test_voxel_mean_host_sweep(seed):
    for tag, inp, kw in sw.sweep("voxel_mean", seed):
        check_voxel_mean(tag, inp, kw)


def test_the_pillar_draws_enter_every_launch_of_the_decoration():
    """over the seeds of ACCV_FUZZ_SCALE = 1: 16-byte and 4-byte loads times 16-byte and 4-byte stores all occur, each also
    with the voxels 16-byte aligned, where the workgroup's range alone decides; the voxel mean takes both loads, the
    4-byte one on aligned voxels too"""
    seen, seen_aligned = set(), set()
    for seed in range(sw.SWEEPS["pillar_features"][1]):
        for tag, _, _ in sw.sweep("pillar_features", seed):
            loads, stores, aligned = sw.dispatch_of(tag)
            seen.add((loads, stores))
            if aligned:
                seen_aligned.add((loads, stores))
    every = {(16, 16), (16, 4), (4, 16), (4, 4)}
    assert seen == every, f"launches not drawn: {sorted(every - seen)}"
    assert seen_aligned == every, f"launches not drawn under aligned voxels: {sorted(every - seen_aligned)}"
    mean = set()
    for seed in range(sw.SWEEPS["voxel_mean"][1]):
        for tag, _, _ in sw.sweep("voxel_mean", seed):
            loads, _, aligned = sw.dispatch_of(tag)
            mean.add((loads, aligned))
    assert {(16, True), (4, True), (4, False)} <= mean, f"voxel_mean launches drawn: {sorted(mean)}"


# ------------------------------------------------------------------------------------------------------- scatter_to_bev
def check_scatter_to_bev(tag, inp, kw):
    """forward and backward against the sequential definition, bit for bit; -> (canvas, index, grad_features)"""
    import bev_scatter_cases as bs

    dev = inp["features"].device
    return bs.run_case(dev, kw["dtype"], inp["coors"], kw["B"], kw["ny"], kw["nx"], kw["C"], 0, tag, V=kw["V"], features=inp["features"],
                       grad=inp["grad"])


@pytest.mark.parametrize("seed", seeds("scatter_to_bev"))
def test_scatter_to_bev_host_sweep(seed):
    for tag, inp, kw in sw.sweep("scatter_to_bev", seed):
        check_scatter_to_bev(tag, inp, kw)


def test_the_scatter_draws_enter_both_write_launches_per_element_size():
    """over the seeds of ACCV_FUZZ_SCALE = 1: the vector and the element write launch for 2-byte and 4-byte elements, and
    on each of the two launches tiles without a row in a frame that has rows (the empty-tile path next to the copy)"""
    seen, with_empty = set(), set()
    for seed in range(sw.SWEEPS["scatter_to_bev"][1]):
        for tag, _, _ in sw.sweep("scatter_to_bev", seed):
            vector, es, empty_tiles = sw.write_path_of(tag)
            seen.add((vector, es))
            if empty_tiles:
                with_empty.add(vector)
    assert seen == {(True, 2), (True, 4), (False, 2), (False, 4)}, f"write launches drawn: {sorted(seen)}"
    assert with_empty == {True, False}, f"empty tiles in frames with rows only on vector = {sorted(with_empty)}"


# ------------------------------------------------------------------------------------------------------ voxelize_points
def check_voxelize_points(tag, inp, kw):
    """all five outputs against the sequential definition, bit for bit; -> the Voxels"""
    import voxelize_cases as vx

    from accvlab.point_cloud import voxelize_points

    got = voxelize_points(inp["ragged"], augmentation=inp["aug_t"], return_point_voxel=True, **kw)
    assert got.voxels.device == inp["ragged"].tensor.device, tag
    vx.check_equal(got, vx.definition(inp["points"], inp["sizes"], augmentation=inp["aug"], **kw), tag)
    return got


@pytest.mark.parametrize("seed", seeds("voxelize_points"))
def test_voxelize_points_host_sweep(seed):
    for tag, inp, kw in sw.sweep("voxelize_points", seed):
        check_voxelize_points(tag, inp, kw)


# ------------------------------------------------------------------------------------------------------ the lidar chain
def check_lidar_chain(tag, inp, kw):
    """every stage against the chained numpy definitions, bit for bit, in the padded and in the flat forms, and the two
    forms against each other where pillar_features_cases.check_after_voxelize and bev_scatter_cases.check_padded_form do;
    -> the tensors of every stage, for the comparison of device and host"""
    import bev_scatter_cases as bs
    import pillar_features_cases as pf
    import voxelize_cases as vx

    from accvlab.point_cloud import concatenate_voxels, pillar_features, scatter_to_bev

    vkw, flags, dtype, (ny, nx) = kw["voxelize"], kw["flags"], kw["dtype"], kw["grid_hw"]
    grid = dict(voxel_size=vkw["voxel_size"], point_cloud_range=vkw["point_cloud_range"])
    vox = check_voxelize_points(tag + ": voxelize_points", inp, vkw)
    dev = vox.voxels.device
    B, V, T, D = vox.voxels.shape
    counts = vox.voxel_counts.tolist()
    want = vx.definition(inp["points"], inp["sizes"], augmentation=inp["aug"], **vkw)
    # the decoration, on the Voxels tuple and on the concatenated form
    pkw = dict(pf.flag_kw(flags), **grid)
    decorated = pillar_features(vox, **pkw)
    want_dec = pf.definition(want["voxels"], want["num_points"], want["coors"], **pkw)
    pf.assert_bits(decorated, want_dec, tag + ": pillar_features on the tuple")
    fv, fc, fn = concatenate_voxels(vox)
    flat_dec = pillar_features(fv, fn, fc, **pkw)
    pf.assert_bits(flat_dec, pf.definition(fv.cpu().numpy(), fn.cpu().numpy(), fc.cpu().numpy(), **pkw), tag + ": pillar_features, concatenated")
    pf.assert_bits(flat_dec, torch.cat([decorated[b, :n] for b, n in enumerate(counts)]), tag + ": concatenated against padded")
    # the stand-in of the feature net: row 0 of every voxel, cast on the host (one rounding, the same for both devices)
    feats = decorated[:, :, 0, :].cpu().to(dtype).to(dev).contiguous()
    C = feats.shape[-1]
    canvas, index, grad = bs.run_case(dev, dtype, vox.coors.cpu().numpy(), B, ny, nx, C, kw["seed"], tag + ": scatter_to_bev, padded", V=V,
                                      features=feats)
    assert int((index >= 0).sum()) == sum(counts), f"{tag}: a voxel lost its cell"
    keep = torch.arange(V, device=dev).view(1, V) < vox.voxel_counts.view(B, 1)
    assert not bs.bits_of(grad[~keep]).any(), f"{tag}: a padding voxel takes a gradient"
    go = bs.random_values(kw["seed"] + 1, (B, C, ny, nx), dtype, dev)
    canvas_f, index_f, grad_f = bs.run_case(dev, dtype, fc.cpu().numpy(), B, ny, nx, C, kw["seed"], tag + ": scatter_to_bev, flat",
                                            features=feats[keep].contiguous(), grad=go)
    bs.assert_bits(canvas_f, canvas, tag + ": flat canvas against padded")
    assert torch.equal(index_f >= 0, index >= 0), f"{tag}: flat and padded occupy different cells"
    bs.assert_bits(grad_f, grad[keep], tag + ": flat gradient against padded")
    assert scatter_to_bev(feats, vox.coors, grid_hw=(ny, nx)).shape == canvas.shape
    return tuple(vox) + (decorated, flat_dec, canvas, index, grad, canvas_f, index_f, grad_f)


@pytest.mark.parametrize("seed", seeds("lidar_chain"))
def test_lidar_chain_host_sweep(seed):
    for tag, inp, kw in sw.sweep("lidar_chain", seed):
        check_lidar_chain(tag, inp, kw)


# -------------------------------------------------------------------------------------------------- lidar_depth_targets
def check_lidar_depth_targets(tag, inp, kw, device):
    """oracle (a) bit for bit; oracle (b) with its own bar for placed cases without image transforms;
    -> (result, the largest error in units of that bar or None)"""
    import depth_targets_cases as dt

    case, tr = inp["case"], inp["transforms"]
    okw = {k: v for k, v in kw.items() if k != "size_dtype"}
    got = dt.run(case, device, kw["size_dtype"], image_transforms=tr, **okw)
    assert got.depth.device.type == torch.device(device).type, tag
    dt.check_equal(got, dt.definition(case["points"], case["sizes"], case["projection"], image_transforms=tr, **okw), tag)
    share = None
    if inp["placed"] and tr is None:
        share = dt.check_f64(got, case, tag, **okw)
    return got, share


@pytest.mark.parametrize("seed", seeds("lidar_depth_targets"))
def test_lidar_depth_targets_host_sweep(seed):
    for tag, inp, kw in sw.sweep("lidar_depth_targets", seed):
        check_lidar_depth_targets(tag, inp, kw, "cpu")


# ------------------------------------------------------------------------------------------------------ the two decoders
def check_query_decode(which, tag, inp, kw):
    """the module's acceptance split and its 1e-5 bar, unchanged; -> (result, the definition's dict)"""
    import query_decode_cases as qc

    from accvlab.draw_heatmap import query_box_decode_2d, query_box_decode_3d

    op, definition = (query_box_decode_3d, qc.definition_3d) if which == "3d" else (query_box_decode_2d, qc.definition_2d)
    cls, rows, M = inp
    got, want = qc.run(op, definition, cls, rows, M, **kw)
    assert all(x.tensor.device == cls.device for x in got), tag
    qc.check(got, want, tag)
    return got, want


def decoder_sweep(which, seed):
    op = "query_box_decode_" + which
    before, cases = sw.REDRAWS[op], 0
    for tag, inp, kw in sw.sweep(op, seed):
        cases += 1
        check_query_decode(which, tag, inp, kw)
    report_redraws(op, cases, sw.REDRAWS[op] - before)


@pytest.mark.parametrize("seed", seeds("query_box_decode_3d"))
def test_query_box_decode_3d_host_sweep(seed):
    decoder_sweep("3d", seed)


@pytest.mark.parametrize("seed", seeds("query_box_decode_2d"))
def test_query_box_decode_2d_host_sweep(seed):
    decoder_sweep("2d", seed)


def test_the_exact_sweeps_never_redraw():
    """the operators compared bit for bit have no margin rule: their draws hold no redraw loop at all"""
    assert set(sw.REDRAWS) == {"query_box_decode_3d", "query_box_decode_2d"}
    assert set(sw.SWEEPS) - set(sw.REDRAWS) == {"pillar_features", "voxel_mean", "scatter_to_bev", "voxelize_points", "lidar_chain",
                                                 "lidar_depth_targets"}
    assert np.all(np.diff([base for base, _, _ in sw.SWEEPS.values()]) == 10000) and min(b for b, _, _ in sw.SWEEPS.values()) == 910000
