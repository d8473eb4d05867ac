"""The seeded sweeps of tests/camera_sweep_cases.py through the host entries of the camera-side and augmentation operators,
against their definitions — the same draws as test_camera_sweeps_gpu.py, without a GPU: this is what shows that the
references hold over the swept ranges.  Every comparison goes through the operators' own case modules; no
tolerance is added or moved.  The check functions take the inputs on whatever device the draw put them, so the GPU file
runs the same functions on the device.  ACCV_FUZZ_SCALE=k runs k times as many seeds."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import camera_sweep_cases as sw  # noqa: E402
from test_fuzz_gpu import _seeds  # noqa: E402
from test_operator_sweeps_cpu import report_redraws  # noqa: E402


def seeds(op):
    return _seeds(sw.SWEEPS[op][1])


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).cpu()


# ------------------------------------------------------------------------------------------ visible boxes, box heat maps
def check_visible_boxes(tag, inp, kw):
    """visible_bbox_mask against the canvas painter, select_visible_bboxes against mask + batched_bool_indexing; -> mask"""
    import visible_boxes_cases as vb

    from accvlab.batching_helpers import batched_bool_indexing
    from accvlab.draw_heatmap import select_visible_bboxes, visible_bbox_mask

    frames, G, (boxes, depths, hw) = inp
    got = visible_bbox_mask(boxes, depths if kw["check_occlusion"] else None, image_hw=hw, **kw)
    assert got.tensor.dtype == torch.bool and got.tensor.shape == boxes.tensor.shape[:2] and got.sample_sizes is boxes.sample_sizes, tag
    assert got.tensor.device == boxes.tensor.device, tag
    mask = got.tensor.cpu()
    want = vb.oracle(frames, G, **kw)                       # padding slots False
    assert torch.equal(mask, want), f"{tag}: the mask differs from the canvas in {int((mask != want).sum())} slots"
    sel = select_visible_bboxes(boxes, depths, image_hw=hw, **kw)
    assert torch.equal(sel[0].tensor, got.tensor), f"{tag}: select_visible_bboxes' mask"
    for out, src in zip(sel[1:], (boxes, depths)):
        ref = batched_bool_indexing(src, got)
        assert torch.equal(out.tensor, ref.tensor) and torch.equal(out.sample_sizes, ref.sample_sizes), f"{tag}: compaction"
    return mask


@pytest.mark.parametrize("seed", seeds("visible_boxes"))
def test_visible_boxes_host_sweep(seed):
    for tag, inp, kw in sw.sweep("visible_boxes", seed):
        check_visible_boxes(tag, inp, kw)


def check_boxes_to_heatmap(tag, case, kw, device, want=None):
    """the module's exact checks of the per-object outputs and its bar on the map, `out=` full of NaN; -> (result, oracle)"""
    import box_heatmap_cases as bc

    from accvlab.draw_heatmap import boxes_to_heatmap

    want = bc.oracle_of(case) if want is None else want
    bboxes, okw = bc.batch(case, device, size_dtype=kw["size_dtype"])
    out = torch.full(want["heatmap"].shape, float("nan"), device=device)
    got = boxes_to_heatmap(bboxes, **okw, out=out)
    assert got.heatmap is out, tag
    bc.check_objects(got, want, tag)
    bc.check_map(got.heatmap, want, tag)
    for r in got[1:]:
        assert torch.equal(r.sample_sizes.cpu(), torch.tensor([len(f["boxes"]) for f in case.frames])), tag
    return got, want


def map_error(got, want):
    err = np.abs(got.heatmap.detach().cpu().numpy().astype(np.float64) - want["heatmap"])
    return float(err.max() / want["max_k"]) if err.size else 0.0


@pytest.mark.parametrize("seed", seeds("boxes_to_heatmap"))
def test_boxes_to_heatmap_host_sweep(seed):
    for tag, case, kw in sw.sweep("boxes_to_heatmap", seed):
        check_boxes_to_heatmap(tag, case, kw, "cpu")


# ------------------------------------------------------------------------------------------------------ prepare_images
def run_store(op, args, tensors, store, device):
    """the operator with the drawn layout, dtype and `out=`; -> (result, whether the guard bands are intact)"""
    from accvlab.image_prep import padded_hw

    kw = dict(tensors, layout=store["layout"], dtype=store["dtype"])
    if store["out"] is None:
        return op(*args, **kw), True
    B, Hs, Ws = args[0].shape[:3]
    Hp, Wp = padded_hw(tensors["output_hw"] or (Hs, Ws), tensors.get("tile_hw", 1))
    shape = (B, 3, Hp, Wp) if store["layout"] == "CHW" else (B, Hp, Wp, 3)
    buf, out = sw.banded_out(shape, store["dtype"], store["out"], device)
    got = op(*args, **kw, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got, sw.bands_intact(buf, store["out"], out.numel())


def check_prepare_images(tag, inp, kw, device, want=None):
    """float32 within image_prep_cases.bar of the float64 oracle in both layouts, `out=` full of NaN and no element
    excluded; the drawn dtype bit-equal to the float32 result's .to(dtype) through the drawn `out=`, guard bands intact.
    -> (the two float32 results by layout, the drawn-store result, largest error / bar, the oracle)"""
    import image_prep_cases as ic

    from accvlab.image_prep import prepare_images

    case, images = inp
    tensors, store = kw["tensors"], kw["store"]
    want = ic.oracle_of(case) if want is None else want
    limit, worst, refs = ic.bar(case), 0.0, {}
    for layout in ("CHW", "HWC"):
        shape = want.shape if layout == "CHW" else (want.shape[0], want.shape[2], want.shape[3], 3)
        out = torch.full(shape, float("nan"), device=device)
        refs[layout] = prepare_images(images, **tensors, layout=layout, out=out)
        got = ic.as_chw64(refs[layout], layout)
        assert np.isfinite(got).all(), f"{tag}: {layout}: an element is not finite (not written?)"
        err = float(np.abs(got - want).max()) if want.size else 0.0
        assert err <= limit, f"{tag}: {layout}: max abs error {err:.3e} above the bar {limit:.3e}"
        worst = max(worst, err / limit)
    got, intact = run_store(prepare_images, (images,), tensors, store, device)
    assert intact, f"{tag}: wrote outside out"
    assert torch.equal(bits(got), bits(refs[store["layout"]].to(store["dtype"]))), f"{tag}: not the float32 result rounded once"
    return refs, got, worst, want


@pytest.mark.parametrize("seed", seeds("prepare_images"))
def test_prepare_images_host_sweep(seed):
    for tag, inp, kw in sw.sweep("prepare_images", seed):
        check_prepare_images(tag, inp, kw, "cpu")


# ---------------------------------------------------------------------------------------------------------------- NV12
def check_nv12_to_rgb(tag, planes, fmt):
    import nv12_cases as nc

    from accvlab.image_prep import nv12_to_rgb

    y, uv = planes
    got = nv12_to_rgb(y, uv, **fmt)
    want = nc.oracle_image(*nc.numpy_planes(y, uv), **fmt)
    assert got.dtype == torch.uint8 and got.device == y.device and tuple(got.shape) == want.shape, tag
    assert np.array_equal(got.cpu().numpy(), want), f"{tag}: {int((got.cpu().numpy() != want).sum())} bytes differ from the oracle"
    return got


@pytest.mark.parametrize("seed", seeds("nv12_to_rgb"))
def test_nv12_to_rgb_host_sweep(seed):
    for tag, planes, fmt in sw.sweep("nv12_to_rgb", seed):
        check_nv12_to_rgb(tag, planes, fmt)


def check_prepare_images_nv12(tag, planes, kw, device):
    """the fused call, through the drawn `out=`, bit-equal to prepare_images(nv12_to_rgb(...)); -> the fused result"""
    from accvlab.image_prep import nv12_to_rgb, prepare_images, prepare_images_nv12

    y, uv = planes
    fmt, tensors, store = kw["format"], kw["tensors"], kw["store"]
    fused, intact = run_store(lambda y, uv, **k: prepare_images_nv12(y, uv, **fmt, **k), (y, uv), tensors, store, device)
    assert intact, f"{tag}: wrote outside out"
    composed = prepare_images(nv12_to_rgb(y, uv, **fmt), is_bgr=fmt["as_bgr"], **tensors, layout=store["layout"], dtype=store["dtype"])
    assert not bool(torch.isnan(fused).any()), f"{tag}: an element was not written"
    assert torch.equal(bits(fused), bits(composed)), f"{tag}: fused and composed differ"
    return fused


@pytest.mark.parametrize("seed", seeds("prepare_images_nv12"))
def test_prepare_images_nv12_host_sweep(seed):
    for tag, planes, kw in sw.sweep("prepare_images_nv12", seed):
        check_prepare_images_nv12(tag, planes, kw, "cpu")


# ------------------------------------------------------------------------------------------------- the two augmentations
def check_augment(module, tag, case, kw, device, a=None):
    """bev_augment_cases / camera_boxes_cases: equal to oracle (a) on every output, and within the bar of oracle (b) where
    the draw says the numbers are ordinary; -> (outputs, oracle (a), the largest ratio / bar against oracle (b))"""
    a = module.oracle_a(case) if a is None else a
    got = module.run(case, device, **kw["how"])
    module.assert_same(got, a, f"{tag} on {device}:")
    worst = 0.0
    if kw["ordinary"]:
        ratios = module.check_against_b(got, case, a, what=f"{tag} on {device}:")
        worst = max([r / n for r, n in ratios.values()] + [0.0])
    return got, a, worst


@pytest.mark.parametrize("seed", seeds("bev_augment_boxes"))
def test_bev_augment_boxes_host_sweep(seed):
    import bev_augment_cases as ba

    for tag, case, kw in sw.sweep("bev_augment_boxes", seed):
        check_augment(ba, tag, case, kw, "cpu")


@pytest.mark.parametrize("seed", seeds("camera_augment_boxes"))
def test_camera_augment_boxes_host_sweep(seed):
    import camera_boxes_cases as cb

    for tag, case, kw in sw.sweep("camera_augment_boxes", seed):
        check_augment(cb, tag, case, kw, "cpu")


# ------------------------------------------------------------------------------------------------ decoding and the NMS
def check_decode(tag, case, kw):
    """box_heatmap_decode against its definition (box_decode_cases.run / check), its kept ranks against the float64 greedy
    loop, and nms_boxes on its result against nms_definition where the draw asks for it; `case` may be on any device"""
    import box_decode_cases as bd

    from accvlab.draw_heatmap import box_heatmap_decode, nms_boxes

    opt = kw["options"]
    got, want = bd.run(box_heatmap_decode, case, **opt)
    bd.check(got, want, tag)
    ranks = sw.f64_kept_ranks(case, opt)
    if ranks is not None:
        for f, r in enumerate(ranks):
            assert bd.kept_ranks(got, f) == r, f"{tag}: frame {f}: not the float64 greedy loop's boxes"
    if kw["nms"] is not None:
        nkw = dict(kw["nms"])
        thr = nkw.pop("iou_threshold")
        again = nms_boxes(got, thr, **nkw)
        bd.check(again, bd.nms_definition(sw.detection_tensors(got), thr, **nkw), f"{tag}: nms_boxes on the result")
    return got, want


@pytest.mark.parametrize("seed", seeds("box_heatmap_decode"))
def test_box_heatmap_decode_host_sweep(seed):
    before, cases = sw.REDRAWS["box_heatmap_decode"], 0
    for tag, case, kw in sw.sweep("box_heatmap_decode", seed):
        cases += 1
        check_decode(tag, case, kw)
    report_redraws("box_heatmap_decode", cases, sw.REDRAWS["box_heatmap_decode"] - before)


def check_nms(tag, det, kw, device):
    """nms_boxes on a drawn ragged set against nms_definition, and its kept rows against the float64 greedy loop"""
    import box_decode_cases as bd

    from accvlab.draw_heatmap import nms_boxes

    kw = dict(kw)
    thr = kw.pop("iou_threshold")
    d = sw.detections(det, device)
    got = nms_boxes(d, thr, **kw)
    want = bd.nms_definition(det, thr, **kw)
    bd.check(got, want, tag)
    if thr is not None:
        boxes, labels, N = det[0].double().numpy(), det[2].numpy(), det[0].shape[1]
        M = min(v for v in (N, kw.get("pre_max_size"), kw.get("post_max_size")) if v is not None)
        for f in range(boxes.shape[0]):
            n = min(max(int(det[5][f]), 0), N)
            n = n if kw.get("pre_max_size") is None else min(n, kw["pre_max_size"])
            # a row that is not finite is kept and compared with nothing: the float64 loop skips its NaN IoUs, an infinite
            # corner gives inf / inf = NaN or 0 there as well
            keep, gap = bd.greedy_nms_f64(np.where(np.isfinite(boxes[f, :n]).all(1, keepdims=True), boxes[f, :n], np.nan), labels[f, :n].tolist(),
                                          thr, kw["class_agnostic"], limit=M)
            assert gap > sw.IOU_MARGIN, f"{tag}: frame {f}: the draw left an IoU {gap:.2e} from the threshold"
            assert bd.kept_ranks(got, f) == det[3][f, keep].tolist(), f"{tag}: frame {f}: not the float64 greedy loop's rows"
    return got


@pytest.mark.parametrize("seed", seeds("nms_boxes"))
def test_nms_boxes_host_sweep(seed):
    before, cases = sw.REDRAWS["nms_boxes"], 0
    for tag, det, kw in sw.sweep("nms_boxes", seed):
        cases += 1
        check_nms(tag, det, kw, "cpu")
    report_redraws("nms_boxes", cases, sw.REDRAWS["nms_boxes"] - before)


def test_the_exact_sweeps_never_redraw():
    """the operators compared bit for bit have no margin rule: their draws hold no redraw loop at all"""
    assert set(sw.REDRAWS) == {"box_heatmap_decode", "nms_boxes"}
