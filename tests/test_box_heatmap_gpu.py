"""boxes_to_heatmap on the GPU: the kernel against the numpy oracle of box_heatmap_cases.py and against the host entry (the
per-object outputs bit for bit, the map to 1e-5 x max(1, max k), zeros outside every patch) for every case and for the
reference's own test; a misaligned `out=`, guard bands around every output, a non-default stream without host
synchronisation, and the validation of the raw C-ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_heatmap_cases as bc  # noqa: E402

from accvlab import _amd_native as nat  # noqa: E402
from accvlab.batching_helpers import RaggedBatch  # noqa: E402
from accvlab.draw_heatmap import BoxHeatmapTargets, boxes_to_heatmap  # noqa: E402
from accvlab.draw_heatmap.box_heatmap import MAX_BOXES  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
op = boxes_to_heatmap
REFERENCE, GOLDEN = bc.reference_cases()


@pytest.mark.parametrize("name", bc.case_names())
def test_case_against_the_oracle_and_the_host_entry(name):
    """`out=` arrives full of NaN: every element of the map must be written"""
    case = bc.cases()[name]
    want = bc.oracle(case)
    out = torch.full(want["heatmap"].shape, float("nan"), device=DEV)
    got = bc.run(op, case, DEV, out=out)
    assert got.heatmap is out and got.center.tensor.is_cuda
    bc.check(got, case)
    bc.check_objects(got, bc.as_numpy(bc.run(op, case, "cpu")), name + " (device against host)")


@pytest.mark.parametrize("case", REFERENCE, ids=repr)
def test_reference_test_vector(case):
    expected = GOLDEN["expected_is_active"]
    for s in GOLDEN["single_heatmap"]:
        if case.name == "reference_single_" + s["id"]:
            expected = s["expected_is_active"]
    got = bc.run(op, case, DEV)
    assert got.is_active.tensor[0].tolist() == expected
    bc.check(got, case)


@pytest.mark.parametrize("name", ["tile_edges", "shape_17x64_G256_B1_C2", "shape_15x131_G256_B3_C2"])
def test_out_view_with_a_16_byte_misaligned_base(name):
    """a width that is a multiple of 4 behind a base that is not 16-byte aligned takes the 4-byte stores; the floats on
    both sides of the view stay as they are"""
    case = bc.cases()[name]
    shape = bc.oracle(case)["heatmap"].shape
    n = int(np.prod(shape))
    for shift in (1, 3):
        buf = torch.full((shift + n + 5,), -7.0, device=DEV)
        out = buf[shift: shift + n].view(shape)
        assert out.data_ptr() % 16 == 4 * shift
        got = bc.run(op, case, DEV, out=out)
        bc.check(got, case)
        assert bool((buf[:shift] == -7.0).all()) and bool((buf[shift + n:] == -7.0).all())


def _raw_call(case, bufs, param_struct, stream=None, **override):
    """the plain ctypes binding with the case's inputs; bufs: the seven output tensors"""
    bboxes, kw = bc.batch(case, DEV, size_dtype=torch.int32)
    ptr = lambda t: None if t is None else (t.tensor if hasattr(t, "tensor") else t).data_ptr()   # noqa: E731
    hw = kw["image_hw"] if isinstance(kw["image_hw"], torch.Tensor) else None
    cats = kw.get("categories")
    flags = (nat.BH_HW_I64 if hw is not None and hw.dtype == torch.int64 else 0) | \
            (nat.BH_CATEGORIES_I64 if cats is not None and cats.dtype == torch.int64 else 0)
    args = dict(boxes=ptr(bboxes), centers=ptr(kw.get("centers")), categories=ptr(cats), is_valid=ptr(kw.get("is_valid")),
                counts=ptr(bboxes.sample_sizes), image_hw=ptr(hw), flags=flags, B=len(case.frames), G=case.G,
                params=ctypes.addressof(param_struct), **{f"o{i}": ptr(t) for i, t in enumerate(bufs)})
    args.update(override)
    keep = (bboxes, kw)   # noqa: F841 - the inputs outlive the asynchronous launch
    stream = nat.stream_ptr(torch.device(DEV, torch.cuda.current_device())) if stream is None else stream
    status = nat.ctypes_lib().accv_box_heatmap(*args.values(), stream)
    torch.cuda.synchronize()
    return status


def _params(case):
    p = dict(bc.DEFAULTS, **case.kw)
    q = nat.BoxHeatmapParams()
    q.image_h, q.image_w = case.image_hw[0]
    q.map_h, q.map_w = case.heatmap_hw
    for n in ("min_fraction_area_clipping", "min_radius", "max_radius", "radius_scaling_factor", "radius_to_sigma_factor"):
        setattr(q, n, p[n])
    q.num_categories = p["num_categories"] or 0
    q.per_category_heatmap = int(p["use_per_category_heatmap"])
    if p["min_object_size"] is not None:
        q.has_min_object_size, q.min_object_size[0], q.min_object_size[1] = (1,) + tuple(p["min_object_size"])
    if p["per_category_min_object_sizes"] is not None:
        q.has_per_category_min_object_sizes = 1
        for c, (h, w) in enumerate(p["per_category_min_object_sizes"]):
            q.per_category_min_object_sizes[c][0], q.per_category_min_object_sizes[c][1] = h, w
    planes = q.num_categories if q.per_category_heatmap else 1
    for c in range(planes):
        q.k_for_classes[c] = 1.0 if p["k_for_classes"] is None else p["k_for_classes"][c]
    return q, planes


@pytest.mark.parametrize("name", ["shape_17x65_G64_B3_C3", "shape_15x64_G65_B3_CNone", "shape_1x131_G63_B3_C2"])
def test_every_output_between_guard_bands(name):
    """the map and every per-object output live inside larger buffers full of a sentinel: after the call the bands on both
    sides are intact and the inside equals the oracle, padding slots included"""
    case = bc.cases()[name]
    want = bc.oracle(case)
    params, planes = _params(case)
    B, G, (Hm, Wm), pad = len(case.frames), case.G, case.heatmap_hw, 256
    specs = [(torch.float32, 4 * B * planes * Hm * Wm), (torch.uint8, B * G), (torch.int32, 4 * B * G * 2),
             (torch.float32, 4 * B * G * 2), (torch.float32, 4 * B * G * 2), (torch.float32, 4 * B * G * 4), (torch.float32, 4 * B * G)]
    whole = [torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=DEV) for _, nbytes in specs]   # the inside too
    inner = [w[pad: pad + nbytes].view(dt) for w, (dt, nbytes) in zip(whole, specs)]
    assert _raw_call(case, inner, params) == 0, nat.ctypes_lib().accv_last_error()
    for w, (_, nbytes) in zip(whole, specs):
        assert bool((w[:pad] == 0xA5).all()) and bool((w[pad + nbytes:] == 0xA5).all()), "wrote outside its buffer"
    shaped = {"heatmap": inner[0].view(want["heatmap"].shape), "is_active": inner[1].view(B, G).bool(),
              "center": inner[2].view(B, G, 2), "center_offset": inner[3].view(B, G, 2), "height_width": inner[4].view(B, G, 2),
              "bboxes_heatmap": inner[5].view(B, G, 4), "radii": inner[6].view(B, G)}
    assert bool((inner[1] <= 1).all()), "is_active holds something that is neither 0 nor 1"
    sizes = torch.tensor([len(f["boxes"]) for f in case.frames])
    got = BoxHeatmapTargets(shaped["heatmap"], *[RaggedBatch(shaped[n], sample_sizes=sizes) for n in BoxHeatmapTargets._fields[1:]])
    bc.check(got, case)


def test_non_default_stream_and_no_host_synchronisation():
    case = bc.cases()["shape_17x65_G64_B3_C3"]
    bboxes, kw = bc.batch(case, DEV)
    first = op(bboxes, **kw)                                        # warm-up: library load, allocator
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            on_stream = op(bboxes, **kw)
        again = op(bboxes, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for other in (on_stream, again):
        assert torch.equal(other.heatmap.view(torch.int32), first.heatmap.view(torch.int32))
        bc.check_objects(other, bc.as_numpy(first), "a second call")
    bc.check(on_stream, case)


def test_raw_c_abi_validation_never_reaches_a_launch():
    case = bc.cases()["category_range_int32"]
    lib = nat.ctypes_lib()
    B, G, (Hm, Wm) = 1, case.G, case.heatmap_hw
    bufs = [torch.zeros(B * 2 * Hm * Wm, device=DEV), torch.zeros(B * G, dtype=torch.uint8, device=DEV),
            torch.zeros(B * G * 2, dtype=torch.int32, device=DEV), torch.zeros(B * G * 2, device=DEV),
            torch.zeros(B * G * 2, device=DEV), torch.zeros(B * G * 4, device=DEV), torch.zeros(B * G, device=DEV)]

    def refused(text, mutate=None, **override):
        params, _ = _params(case)
        if mutate:
            mutate(params)
        assert _raw_call(case, bufs, params, **override) == -1
        assert text in lib.accv_last_error().decode(), lib.accv_last_error()

    refused("box slots per frame, at most 256", G=MAX_BOXES + 1)
    refused("categories, 0 (not used) to 128", lambda p: setattr(p, "num_categories", 129))
    refused("exclude each other", lambda p: setattr(p, "has_min_object_size", 1))
    refused("null heatmap", o0=None)
    refused("null boxes / per-object output", o4=None)
    refused("categories is null", categories=None)
    refused("null params", params=None)
    refused("unknown flags", flags=64)
    refused("map of 0 x", lambda p: setattr(p, "map_h", 0))
    refused("max_radius", lambda p: setattr(p, "max_radius", 1e9))
    refused("not finite", lambda p: setattr(p, "min_radius", float("nan")))
    refused("radius_to_sigma_factor", lambda p: setattr(p, "radius_to_sigma_factor", -1.0))
    refused("not aligned", o3=bufs[3].data_ptr() + 2)
    refused("grid limit", lambda p: (setattr(p, "map_h", 1 << 24), setattr(p, "map_w", 1 << 24)))
    assert all(not bool(b.any()) for b in bufs), "a refused call wrote something"
    params, _ = _params(case)
    assert _raw_call(case, bufs, params) == 0 and bool(bufs[0].any())


def test_more_slots_than_max_boxes_raises_before_any_launch():
    sizes = torch.tensor([1], device=DEV)
    boxes = RaggedBatch(torch.zeros((1, MAX_BOXES + 1, 4), device=DEV), sample_sizes=sizes)
    with pytest.raises(RuntimeError, match="boxes_to_heatmap.*MAX_BOXES"):
        op(boxes, image_hw=(8, 8), heatmap_hw=(8, 8), use_per_category_heatmap=False)
    with pytest.raises(RuntimeError, match="boxes_to_heatmap: image_hw must be on the boxes' device"):
        op(RaggedBatch(torch.zeros((1, 2, 4), device=DEV), sample_sizes=sizes), image_hw=torch.zeros((1, 2), dtype=torch.int32),
           heatmap_hw=(8, 8), use_per_category_heatmap=False)
