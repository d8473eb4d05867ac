"""nv12_to_rgb and prepare_images_nv12 on the GPU; every comparison is exact equality of bits.  The conversion kernel against
the library's host entry (which test_nv12_cpu.py holds to the numpy oracle): all 2^24 (Y, U, V) triples in both ranges, the
shape grid on pitched views with `out=` between sentinel bands and pitch padding that is never read.  The fused kernel
against the device's own conversion + prepare_images and against the host entry's fused result for every case of
image_prep_cases.py, in every layout and dtype through aligned and misaligned `out=` views; a non-default stream without
host synchronisation; limits and wrong devices refused before any launch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_prep_cases as ic  # noqa: E402
import nv12_cases as nc  # noqa: E402
from test_image_prep_gpu import STORE_CASES  # noqa: E402

from accvlab.image_prep import nv12_to_rgb, prepare_images, prepare_images_nv12  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
def test_every_triple_against_the_host_entry(full_range):
    y, uv = nc.exhaustive_planes()
    want = nv12_to_rgb(y, uv, full_range=full_range).to(DEV)
    out = torch.full((1, 4096, 4096, 3), 77, dtype=torch.uint8, device=DEV)
    got = nv12_to_rgb(y.to(DEV), uv.to(DEV), full_range=full_range, out=out)
    assert got is out and bool(torch.equal(got, want))


@pytest.mark.parametrize("W", nc.GRID_W)
@pytest.mark.parametrize("H", nc.GRID_H)
def test_shape_grid_on_pitched_views_with_offset_out_and_padding(H, W):
    """B = 3, pitched views, both ranges, bit-equal to the host entry; `out=` 0, 1 and 3 bytes off an aligned base between
    sentinel bands that stay intact; surface padding of 0 and of 255 give the same bytes"""
    y, uv = nc.grid_planes(H, W, fill=0)
    yd, uvd = nc.grid_planes(H, W, fill=0, device=DEV)
    y255, uv255 = nc.grid_planes(H, W, fill=255, device=DEV)
    assert not yd.is_contiguous() and torch.equal(yd.cpu(), y) and torch.equal(uvd.cpu(), uv)
    n, band = 3 * H * W * 3, 64
    for fmt in ("limited", "full", "full_bgr_vu"):
        f = nc.FORMATS[fmt]
        want = nv12_to_rgb(y, uv, **f).to(DEV)
        assert torch.equal(nv12_to_rgb(y255, uv255, **f), want), f"{fmt}: the pitch padding was read"
        for shift in (0, 1, 3):
            buf = torch.full((band + shift + n + band,), 77, dtype=torch.uint8, device=DEV)
            out = buf[band + shift: band + shift + n].view(want.shape)
            assert out.data_ptr() % 4 == shift
            got = nv12_to_rgb(yd, uvd, out=out, **f)
            assert got.data_ptr() == out.data_ptr() and torch.equal(got, want), f"{fmt}, shift {shift}"
            assert bool((buf[:band + shift] == 77).all()) and bool((buf[band + shift + n:] == 77).all()), "wrote outside out"


@pytest.mark.parametrize("name", ic.case_names())
def test_fused_equals_conversion_plus_prepare_images_and_the_host_entry(name):
    """`out=` arrives full of NaN: every element must be written"""
    case = ic.cases()[name]
    want = nc.run_composed(case, DEV)
    out = torch.full(want.shape, float("nan"), device=DEV)
    got = nc.run_fused(case, DEV, out=out)
    assert got is out and got.is_cuda and not bool(torch.isnan(got).any())
    assert torch.equal(nc.bits(got), nc.bits(want)), f"{name}: fused and conversion + prepare_images differ on the device"
    assert torch.equal(nc.bits(got), nc.bits(nc.run_fused(case, "cpu"))), f"{name}: device and host entry differ"


@pytest.mark.parametrize("fmt", ["full", "bgr", "vu", "full_bgr_vu"])
@pytest.mark.parametrize("name", nc.FORMAT_CASES + sorted(nc.translation_cases()))
def test_fused_contract_in_the_other_formats(name, fmt):
    case = ic.cases()[name] if name in ic.cases() else nc.translation_cases()[name]
    got = nc.run_fused(case, DEV, fmt)
    assert torch.equal(nc.bits(got), nc.bits(nc.run_composed(case, DEV, fmt)))
    assert torch.equal(nc.bits(got), nc.bits(nc.run_fused(case, "cpu", fmt)))


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", STORE_CASES)
def test_layouts_dtypes_offset_views_and_guard_bands(name, dtype, layout):
    case = ic.cases()[name]
    ref = nc.run_composed(case, DEV, layout=layout, dtype=dtype)
    want, shape = nc.bits(ref), ref.shape
    assert torch.equal(want, nc.bits(nc.run_fused(case, "cpu", layout=layout, dtype=dtype))), "device and host entry differ"
    n, band = ref.numel(), 64
    for shift in (0, 1, 3):
        buf = torch.full((band + shift + n + band,), -7.0, dtype=dtype, device=DEV)
        out = buf[band + shift: band + shift + n].view(shape)
        out.fill_(float("nan"))
        assert out.data_ptr() % 16 == (shift * out.element_size()) % 16
        got = nc.run_fused(case, DEV, layout=layout, dtype=dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(nc.bits(got), want), f"shift {shift}"
        assert bool((buf[:band + shift] == -7.0).all()) and bool((buf[band + shift + n:] == -7.0).all()), "wrote outside out"


def test_non_default_stream_and_no_host_synchronisation():
    case = ic.cases()["batch_7_parameters_per_image"]
    y, uv = nc.case_planes(case, DEV)
    kw = nc.case_kw(case, DEV)
    rgb_first = nv12_to_rgb(y, uv, as_bgr=True)                           # warm-up: library load, allocator
    first = prepare_images_nv12(y, uv, as_bgr=True, **kw)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rgb_on_stream = nv12_to_rgb(y, uv, as_bgr=True)
            on_stream = prepare_images_nv12(y, uv, as_bgr=True, **kw)
        rgb_again = nv12_to_rgb(y, uv, as_bgr=True)
        again = prepare_images_nv12(y, uv, as_bgr=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(rgb_on_stream, rgb_first) and torch.equal(rgb_again, rgb_first)
    assert torch.equal(nc.bits(on_stream), nc.bits(first)) and torch.equal(nc.bits(again), nc.bits(first))
    assert torch.equal(nc.bits(first), nc.bits(prepare_images(rgb_first, is_bgr=True, **kw)))


def test_limits_and_wrong_devices_raise_before_any_launch():
    y = torch.zeros((1, 4, 6), dtype=torch.uint8, device=DEV)
    uv = torch.zeros((1, 2, 3, 2), dtype=torch.uint8, device=DEV)
    wide = torch.zeros((1, 1, 16386), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="nv12_to_rgb: .*every extent must be in"):
        nv12_to_rgb(wide, torch.zeros((1, 1, 8193, 2), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="prepare_images_nv12: .*every extent must be in"):
        prepare_images_nv12(y, uv, transforms=torch.zeros((1, 2, 3), device=DEV), output_hw=(4, 16385))
    for op in (nv12_to_rgb, prepare_images_nv12):
        with pytest.raises(RuntimeError, match=f"{op.__name__}: uv must be on y's device"):
            op(y, uv.cpu())
        with pytest.raises(TypeError, match=f"{op.__name__}: y must be uint8"):
            op(y.float(), uv)
    with pytest.raises(RuntimeError, match="nv12_to_rgb: out must be on the planes' device"):
        nv12_to_rgb(y, uv, out=torch.zeros((1, 4, 6, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="prepare_images_nv12: transforms must be on the planes' device"):
        prepare_images_nv12(y, uv, transforms=torch.zeros((1, 2, 3)))
    with pytest.raises(RuntimeError, match="prepare_images_nv12: out must be on the planes' device"):
        prepare_images_nv12(y, uv, out=torch.zeros((1, 3, 4, 6)))
    assert nv12_to_rgb(y[:0], uv[:0]).shape == (0, 4, 6, 3) and prepare_images_nv12(y[:0], uv[:0]).shape == (0, 3, 4, 6)
