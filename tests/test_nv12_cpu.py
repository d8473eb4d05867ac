"""nv12_to_rgb and prepare_images_nv12 without a GPU, through the library's host entries; every comparison is exact equality
of bits.  The conversion against the numpy oracle of nv12_cases.py: all 2^24 (Y, U, V) triples in both ranges, the shape
grid on pitched plane views, pitch padding that is never read, `out=` views between sentinel bands.  The fused call against
conversion + prepare_images for every case of image_prep_cases.py and for bilinear pairs that straddle UV pairs and chroma
rows.  The argument rules of the Python layer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_prep_cases as ic  # noqa: E402
import nv12_cases as nc  # noqa: E402

import accvlab.image_prep as ip  # noqa: E402
from accvlab.image_prep import nv12_planes, nv12_to_rgb, prepare_images, prepare_images_nv12  # noqa: E402

DEV = "cpu"


def test_exported_and_the_exhaustive_image_holds_every_triple_once():
    assert {"nv12_to_rgb", "prepare_images_nv12", "nv12_planes"} <= set(ip.__all__)
    assert nc.every_triple_occurs_once()
    # two triples by hand: black and white of the limited range, mid-grey chroma
    r, g, b = nc.oracle_rgb(*(np.asarray([v], np.uint8) for v in (16, 128, 128)))
    assert (int(r[0]), int(g[0]), int(b[0])) == (0, 0, 0)
    r, g, b = nc.oracle_rgb(*(np.asarray([v], np.uint8) for v in (235, 128, 128)))
    assert (int(r[0]), int(g[0]), int(b[0])) == (255, 255, 255)


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
def test_every_triple_against_the_oracle(full_range):
    y, uv = nc.exhaustive_planes()
    got = nv12_to_rgb(y, uv, full_range=full_range)
    assert got.shape == (1, 4096, 4096, 3) and got.dtype == torch.uint8
    assert torch.equal(got, nc.exhaustive_oracle(full_range))


@pytest.mark.parametrize("fmt", ["bgr", "vu", "full_bgr_vu"])
def test_bgr_and_vu_on_a_crop_of_the_exhaustive_image(fmt):
    y, uv = nc.exhaustive_planes()
    y, uv = y[:, 1024:1280, 2048:2304], uv[:, 512:640, 1024:1152]          # strided views
    want = nc.oracle_image(*nc.numpy_planes(y, uv), **nc.FORMATS[fmt])
    assert np.array_equal(nv12_to_rgb(y, uv, **nc.FORMATS[fmt]).numpy(), want)
    if fmt == "bgr":
        assert torch.equal(nv12_to_rgb(y, uv, as_bgr=True), nv12_to_rgb(y, uv).flip(-1))


@pytest.mark.parametrize("W", nc.GRID_W)
@pytest.mark.parametrize("H", nc.GRID_H)
def test_shape_grid_on_pitched_views(H, W):
    """B = 3, planes cut from one surface tensor (pitch W + 13 rounded up to even, uv_row = H + 3, batch stride larger than
    the surface); padding of 0 and of 255 give the same bytes: nothing outside [H, W] is read"""
    y, uv = nc.grid_planes(H, W, fill=0)
    assert not y.is_contiguous() and not uv.is_contiguous()
    assert y.stride(0) > y.stride(1) * (H + 3 + (H + 1) // 2)
    y255, uv255 = nc.grid_planes(H, W, fill=255)
    assert torch.equal(y, y255) and torch.equal(uv, uv255) and y.data_ptr() != y255.data_ptr()
    for fmt in ("limited", "full"):
        want = nc.oracle_image(*nc.numpy_planes(y, uv), **nc.FORMATS[fmt])
        got = nv12_to_rgb(y, uv, **nc.FORMATS[fmt])
        assert got.shape == (3, H, W, 3)
        assert np.array_equal(got.numpy(), want), fmt
        assert torch.equal(nv12_to_rgb(y255, uv255, **nc.FORMATS[fmt]), got), f"{fmt}: the pitch padding was read"


@pytest.mark.parametrize("hw", [(5, 7), (17, 131), (16, 64)])
def test_out_views_between_sentinel_bands(hw):
    y, uv = nc.grid_planes(*hw)
    want = nv12_to_rgb(y, uv)
    n, band = want.numel(), 64
    for shift in (0, 1, 3):
        buf = torch.full((band + shift + n + band,), 77, dtype=torch.uint8)
        out = buf[band + shift: band + shift + n].view(want.shape)
        got = nv12_to_rgb(y, uv, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, want), f"shift {shift}"
        assert bool((buf[:band + shift] == 77).all()) and bool((buf[band + shift + n:] == 77).all()), "wrote outside out"


def test_nv12_planes_makes_views():
    s = torch.arange(2 * 12 * 10, dtype=torch.uint8).reshape(2, 12, 10)
    y, uv = nv12_planes(s, (5, 7), uv_row=8)
    assert y.shape == (2, 5, 7) and uv.shape == (2, 3, 4, 2)
    assert y.data_ptr() == s.data_ptr() and uv.data_ptr() == s[0, 8].data_ptr()
    assert y.stride() == (120, 10, 1) and uv.stride() == (120, 10, 2, 1)
    assert torch.equal(uv[1, 2, 3], s[1, 10, 6:8])
    y2, uv2 = nv12_planes(s, (8, 10))                                     # default: the UV plane follows the luma
    assert uv2.data_ptr() == s[0, 8].data_ptr() and uv2.shape == (2, 4, 5, 2)


# ------------------------------------------------------------------------------------------------------ fused contract
@pytest.mark.parametrize("name", ic.case_names())
def test_fused_equals_conversion_plus_prepare_images(name):
    """`out=` arrives full of NaN: every element must be written"""
    case = ic.cases()[name]
    want = nc.run_composed(case, DEV)
    out = torch.full(want.shape, float("nan"))
    got = nc.run_fused(case, DEV, out=out)
    assert got is out and not bool(torch.isnan(got).any())
    assert torch.equal(nc.bits(got), nc.bits(want))


@pytest.mark.parametrize("fmt", ["full", "bgr", "vu", "full_bgr_vu"])
@pytest.mark.parametrize("name", nc.FORMAT_CASES)
def test_fused_contract_in_the_other_formats(name, fmt):
    case = ic.cases()[name]
    assert torch.equal(nc.bits(nc.run_fused(case, DEV, fmt)), nc.bits(nc.run_composed(case, DEV, fmt)))


@pytest.mark.parametrize("fmt", ["limited", "full"])
@pytest.mark.parametrize("name", sorted(nc.translation_cases()))
def test_pairs_that_straddle_uv_pairs_and_chroma_rows(name, fmt):
    case = nc.translation_cases()[name]
    got, want = nc.run_fused(case, DEV, fmt), nc.run_composed(case, DEV, fmt)
    assert torch.equal(nc.bits(got), nc.bits(want))
    if name.endswith("_1.0"):       # an integer translation samples single source pixels: the conversion, shifted
        y, uv = nc.case_planes(case, DEV)
        rgb = nv12_to_rgb(y, uv, **nc.FORMATS[fmt])
        plain = prepare_images(rgb, **nc.case_kw(case, DEV, transforms=None))
        if "_x_" in name:
            assert torch.equal(nc.bits(got[..., 1:]), nc.bits(plain[..., :-1]))
        else:
            assert torch.equal(nc.bits(got[..., 1:, :]), nc.bits(plain[..., :-1, :]))


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_fused_layouts_and_dtypes(dtype, layout):
    for name in ("partition_17x131", "batch_7_parameters_per_image", "colour_all_with_a_warp"):
        case = ic.cases()[name]
        got = nc.run_fused(case, DEV, layout=layout, dtype=dtype)
        assert torch.equal(nc.bits(got), nc.bits(nc.run_composed(case, DEV, layout=layout, dtype=dtype))), name


def test_source_hw_keeps_luma_outside_it_unread():
    """the valid region sits inside larger planes; changing every luma byte outside it changes nothing"""
    case = ic.cases()["batch_7_parameters_per_image"]
    y, uv = nc.case_planes(case, DEV)
    y2 = y.clone()
    for b, (h, w) in enumerate(case.source_hw):
        h, w = min(int(h), y.shape[1]), min(int(w), y.shape[2])
        y2[b, h:] ^= 0xff
        y2[b, :, w:] ^= 0xff
    assert not torch.equal(y, y2)
    kw = nc.case_kw(case, DEV)
    assert torch.equal(nc.bits(prepare_images_nv12(y2, uv, as_bgr=True, **kw)), nc.bits(prepare_images_nv12(y, uv, as_bgr=True, **kw)))


# -------------------------------------------------------------------------------------------------------------- errors
def test_argument_rules():
    y, uv = nc.grid_planes(5, 7)
    for op in (nv12_to_rgb, prepare_images_nv12):
        who = op.__name__
        with pytest.raises(TypeError, match=f"{who}: y must be uint8"):
            op(y.float(), uv)
        with pytest.raises(TypeError, match=f"{who}: uv must be uint8"):
            op(y, uv.float())
        with pytest.raises(RuntimeError, match=f"{who}: uv must have stride"):
            op(y, torch.zeros((3, 3, 4, 4), dtype=torch.uint8)[..., :2])      # stride(-2) == 4
        with pytest.raises(RuntimeError, match=f"{who}: y must have stride"):
            op(torch.zeros((3, 5, 14), dtype=torch.uint8)[..., ::2], uv)       # stride(-1) == 2
        with pytest.raises(RuntimeError, match=f"{who}: uv must be uint8 \\[3, 3, 4, 2\\]"):
            op(y, uv[:, :2])
        with pytest.raises(RuntimeError, match=f"{who}: uv must be uint8 \\[3, 3, 4, 2\\]"):
            op(y, uv[:, :, :3])
        with pytest.raises(RuntimeError, match=f"{who}: uv must be on y's device"):
            op(y, uv.to("meta"))
        with pytest.raises(RuntimeError, match=f"{who}: chroma_order must be"):
            op(y, uv, chroma_order="yuv")
        assert op(y[:0], uv[:0]).shape == ((0, 5, 7, 3) if op is nv12_to_rgb else (0, 3, 5, 7))
    with pytest.raises(TypeError, match="nv12_to_rgb: out must be torch.uint8"):
        nv12_to_rgb(y, uv, out=torch.zeros((3, 5, 7, 3)))
    with pytest.raises(RuntimeError, match="nv12_to_rgb: out must be torch.uint8 \\[3, 5, 7, 3\\]"):
        nv12_to_rgb(y, uv, out=torch.zeros((3, 5, 7, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="nv12_to_rgb: out must be contiguous"):
        nv12_to_rgb(y, uv, out=torch.zeros((3, 5, 3, 7), dtype=torch.uint8).transpose(2, 3))
    with pytest.raises(TypeError, match="prepare_images_nv12: transforms must be float32"):
        prepare_images_nv12(y, uv, transforms=torch.zeros((3, 2, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="prepare_images_nv12: output_hw .* needs transforms"):
        prepare_images_nv12(y, uv, output_hw=(4, 4))
    with pytest.raises(ValueError, match="prepare_images_nv12: std must be positive"):
        prepare_images_nv12(y, uv, std=0.0)
    with pytest.raises(TypeError):
        prepare_images_nv12(y, uv, is_bgr=True)


def test_nv12_planes_rules():
    s = torch.zeros((2, 12, 10), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="nv12_planes: a pitch of 10 bytes is too small"):
        nv12_planes(s, (4, 11))
    with pytest.raises(RuntimeError, match="nv12_planes: 12 rows do not hold"):
        nv12_planes(s, (9, 8))
    with pytest.raises(RuntimeError, match="nv12_planes: 12 rows do not hold"):
        nv12_planes(s, (6, 8), uv_row=10)
    with pytest.raises(RuntimeError, match="nv12_planes: uv_row must be"):
        nv12_planes(s, (6, 8), uv_row=5)
    with pytest.raises(TypeError, match="nv12_planes: surfaces must be uint8"):
        nv12_planes(s.float(), (4, 4))
    with pytest.raises(RuntimeError, match="nv12_planes: surfaces must be uint8 \\[B, rows, pitch\\]"):
        nv12_planes(s.transpose(1, 2), (4, 4))
