"""The seeded sweeps of tests/camera_sweep_cases.py on the GPU: the HIP kernels of the camera-side and augmentation operators
against their definitions through the check functions of test_camera_sweeps_cpu.py (the operators' own comparisons, no
tolerance added or moved), and bit for bit against their host entries on every output of every draw, over random
combinations of shape, dtype, alignment, ragged sizes and flags that the hand-picked cases cross one at a time (DESIGN.md
§9zb).  ACCV_FUZZ_SCALE=k runs k times as many seeds.  After a complete run the worst error seen per operator and dtype goes
to profiles/camera_sweeps_accuracy.log; a partial run writes nothing."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import camera_sweep_cases as sw  # noqa: E402
import test_camera_sweeps_cpu as host_checks  # noqa: E402
from test_camera_sweeps_cpu import bits, report_redraws, seeds  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = "exact"      # the dtype column of an operator whose outputs are compared bit for bit


@pytest.fixture(scope="module")
def worst():
    """every sweep records its largest errors here; written out once every seed of every sweep of the module is through"""
    seen = sw.Worst()
    seen.done = set()
    yield seen
    if seen.done != {(op, s) for op in sw.SWEEPS for s in seeds(op)}:      # a partial run (-k, -x) leaves no log
        return
    lines = [f"camera sweeps on {torch.cuda.get_device_name(0)} (tests/test_camera_sweeps_gpu.py, ACCV_FUZZ_SCALE "
             f"{os.environ.get('ACCV_FUZZ_SCALE', '1')}): the largest error seen per operator and dtype.  Every output of every case",
             "is bit-equal between the device and the host entry (asserted), except where a 'vs_host' figure is listed.",
             "oracle: prepare_images float32 against the float64 oracle, as a share of image_prep_cases.bar (bound 1; the 16-bit",
             "results are the float32 result rounded once, bit for bit).  map: boxes_to_heatmap's map against the float64 painter,",
             "absolute, in units of max(1, max |k|) (bar 1e-5); map_vs_host: device against host entry, absolute.  oracle_b: the",
             "augmentations against their float64 oracle (b), as a share of its bar n x 2^-24 x largest intermediate (bound 1).",
             "score / score_vs_host: the decoder's sigmoid scores against float64 and against the host entry, absolute (bar 1e-5)."]
    lines += seen.lines()
    try:
        with open(os.path.join(ROOT, "profiles", "camera_sweeps_accuracy.log"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:      # a read-only checkout: the figures were asserted all the same
        pass


def both_devices(op, seed):
    """the cases of one seed drawn on the device and on the host: (tag, device inputs, device kwargs, host inputs, host kwargs)"""
    for (tag, inp, kw), (_, hinp, hkw) in zip(sw.sweep(op, seed, DEV), sw.sweep(op, seed, "cpu")):
        yield tag, inp, kw, hinp, hkw


# ------------------------------------------------------------------------------------------ visible boxes, box heat maps
@pytest.mark.parametrize("seed", seeds("visible_boxes"))
def test_visible_boxes_sweep(seed, worst):
    for tag, inp, kw, hinp, _ in both_devices("visible_boxes", seed):
        assert inp[2][0].tensor.is_cuda
        mask = host_checks.check_visible_boxes(tag + " device", inp, kw)
        assert torch.equal(mask, host_checks.check_visible_boxes(tag + " host", hinp, kw)), f"{tag}: device and host entry differ"
        worst.add("visible_bbox_mask / select_visible_bboxes", EXACT)
    worst.done.add(("visible_boxes", seed))


@pytest.mark.parametrize("seed", seeds("boxes_to_heatmap"))
def test_boxes_to_heatmap_sweep(seed, worst):
    import box_heatmap_cases as bc

    for tag, case, kw in sw.sweep("boxes_to_heatmap", seed):
        got, want = host_checks.check_boxes_to_heatmap(tag + " device", case, kw, DEV)
        assert got.center.tensor.is_cuda
        host, _ = host_checks.check_boxes_to_heatmap(tag + " host", case, kw, "cpu", want)
        bc.check_objects(got, bc.as_numpy(host), tag + " (device against host)")
        vs_host = (got.heatmap.cpu().double() - host.heatmap.double()).abs()
        worst.add("boxes_to_heatmap", torch.float32, map=host_checks.map_error(got, want),
                  map_vs_host=float(vs_host.max()) if vs_host.numel() else 0.0)
    worst.done.add(("boxes_to_heatmap", seed))


# ------------------------------------------------------------------------------------------------ images and NV12 planes
@pytest.mark.parametrize("seed", seeds("prepare_images"))
def test_prepare_images_sweep(seed, worst):
    from accvlab.image_prep import prepare_images

    for tag, inp, kw, hinp, hkw in both_devices("prepare_images", seed):
        refs, got, err, _ = host_checks.check_prepare_images(tag + " device", inp, kw, DEV)
        assert got.is_cuda
        store = kw["store"]
        for layout in ("CHW", "HWC"):
            assert torch.equal(bits(refs[layout]), bits(prepare_images(hinp[1], **hkw["tensors"], layout=layout))), \
                f"{tag}: {layout}: device and host entry differ"
        host = prepare_images(hinp[1], **hkw["tensors"], layout=store["layout"], dtype=store["dtype"])
        assert torch.equal(bits(got), bits(host)), f"{tag}: {store['dtype']}: device and host entry differ"
        worst.add("prepare_images", store["dtype"], oracle=err)
    worst.done.add(("prepare_images", seed))


@pytest.mark.parametrize("seed", seeds("nv12_to_rgb"))
def test_nv12_to_rgb_sweep(seed, worst):
    for tag, planes, fmt, hplanes, _ in both_devices("nv12_to_rgb", seed):
        assert planes[0].is_cuda
        got = host_checks.check_nv12_to_rgb(tag + " device", planes, fmt)
        assert torch.equal(got.cpu(), host_checks.check_nv12_to_rgb(tag + " host", hplanes, fmt)), f"{tag}: device and host entry differ"
        worst.add("nv12_to_rgb", EXACT)
    worst.done.add(("nv12_to_rgb", seed))


@pytest.mark.parametrize("seed", seeds("prepare_images_nv12"))
def test_prepare_images_nv12_sweep(seed, worst):
    for tag, planes, kw, hplanes, hkw in both_devices("prepare_images_nv12", seed):
        fused = host_checks.check_prepare_images_nv12(tag + " device", planes, kw, DEV)
        assert fused.is_cuda
        host = host_checks.check_prepare_images_nv12(tag + " host", hplanes, hkw, "cpu")
        assert torch.equal(bits(fused), bits(host)), f"{tag}: device and host entry differ"
        worst.add("prepare_images_nv12", EXACT)
    worst.done.add(("prepare_images_nv12", seed))


# ------------------------------------------------------------------------------------------------- the two augmentations
def augment_sweep(module, op, label, seed, worst):
    for tag, case, kw in sw.sweep(op, seed):
        got, a, ratio = host_checks.check_augment(module, tag, case, kw, DEV)
        host = module.run(case, "cpu", **kw["how"])
        module.assert_same(got, host, f"{tag}: device against host entry:")
        if kw["ordinary"]:
            worst.add(label, torch.float32, oracle_b=ratio)
        else:
            worst.add(label, EXACT)
    worst.done.add((op, seed))


@pytest.mark.parametrize("seed", seeds("bev_augment_boxes"))
def test_bev_augment_boxes_sweep(seed, worst):
    import bev_augment_cases as ba

    augment_sweep(ba, "bev_augment_boxes", "bev_augment_boxes", seed, worst)


@pytest.mark.parametrize("seed", seeds("camera_augment_boxes"))
def test_camera_augment_boxes_sweep(seed, worst):
    import camera_boxes_cases as cb

    augment_sweep(cb, "camera_augment_boxes", "camera_augment_boxes", seed, worst)


# ------------------------------------------------------------------------------------------------ decoding and the NMS
def score_error(got, want):
    g, a = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(g - a).max()) if g.size else 0.0


@pytest.mark.parametrize("seed", seeds("box_heatmap_decode"))
def test_box_heatmap_decode_sweep(seed, worst):
    import box_decode_cases as bd

    from accvlab.draw_heatmap import box_heatmap_decode

    before, cases = sw.REDRAWS["box_heatmap_decode"], 0
    for tag, case, kw in sw.sweep("box_heatmap_decode", seed):
        cases += 1
        got, want = host_checks.check_decode(tag + " device", case.to(DEV), kw)
        assert all(x.tensor.is_cuda and x.sample_sizes.is_cuda for x in got)
        host = box_heatmap_decode(*case.op_args(), **dict(case.tensors, **kw["options"]))
        bd.check_device_against_host(got, host, want["logits"], tag + " device against host")
        if want["logits"]:
            worst.add("box_heatmap_decode (+ nms_boxes on its result)", case.peaks[0].dtype,
                      score=score_error(got.scores.tensor.cpu(), want["score_approx"]),
                      score_vs_host=score_error(got.scores.tensor.cpu(), host.scores.tensor))
        else:
            worst.add("box_heatmap_decode (+ nms_boxes on its result)", EXACT)
    report_redraws("box_heatmap_decode", cases, sw.REDRAWS["box_heatmap_decode"] - before)
    worst.done.add(("box_heatmap_decode", seed))


@pytest.mark.parametrize("seed", seeds("nms_boxes"))
def test_nms_boxes_sweep(seed, worst):
    import box_decode_cases as bd

    before, cases = sw.REDRAWS["nms_boxes"], 0
    for tag, det, kw in sw.sweep("nms_boxes", seed):
        cases += 1
        got = host_checks.check_nms(tag + " device", det, kw, DEV)
        assert all(x.tensor.is_cuda for x in got)
        bd.check_device_against_host(got, host_checks.check_nms(tag + " host", det, kw, "cpu"), False, tag + " device against host")
        worst.add("nms_boxes", EXACT)
    report_redraws("nms_boxes", cases, sw.REDRAWS["nms_boxes"] - before)
    worst.done.add(("nms_boxes", seed))
