"""prepare_images without a GPU: every case of image_prep_cases.py through the library's host entry against the float64
oracle (one derived bar, no element excluded), the sample positions bit for bit against the numpy-float32 restatement the
oracle uses, layouts, dtypes, `out=` views and guard bands, the bit-equalities the operator promises, the host-side helpers,
the argument rules of the Python layer and the validation of the raw C-ABI through both bindings."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_prep_cases as ic  # noqa: E402

import accvlab.image_prep as ip  # noqa: E402
from accvlab import _amd_native as nat  # noqa: E402
from accvlab.image_prep import (output_size_transform, padded_hw, prepare_images, sample_photometric_params,  # noqa: E402
                                sample_positions)

DEV = "cpu"
STORE_CASES = ["partition_17x131", "partition_15x63", "partition_16x64", "batch_7_parameters_per_image",
               "pad_tile_8x32_before_normalize", "colour_all_with_a_warp"]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_exported_and_constants():
    assert {"prepare_images", "sample_photometric_params", "output_size_transform", "padded_hw"} <= set(ip.__all__)
    assert (ic.TW, ic.TH) == (64, 16) == (ip.TILE_W, ip.TILE_H) and ip.MAX_EXTENT == 16384
    assert ip.CHANNEL_PERMUTATIONS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 1, 0), (2, 0, 1), (1, 2, 0))
    assert set(ic.PARTITION_WIDTHS) == {1, 3, 4, 5, 63, 64, 65, 131} and set(ic.PARTITION_HEIGHTS) == {1, 15, 16, 17}
    assert ic.K_ROUNDED_OPS == 23 and abs(ic.bar(ic.cases()["warp_none"]) - 23 * 2.0 ** -24 * 2 * 255) < 1e-12


@pytest.mark.parametrize("name", ic.case_names())
def test_case_against_the_oracle(name):
    """`out=` arrives full of NaN: every element must be written"""
    case = ic.cases()[name]
    out = torch.full(ic.oracle(name).shape, float("nan"))
    got = ic.run(case, DEV, out=out)
    assert got is out
    ic.check(got, case)


@pytest.mark.parametrize("name", [n for n in ic.case_names() if ic.cases()[n].transforms is not None])
def test_sample_positions_equal_the_float32_restatement_bit_for_bit(name):
    """what the oracle samples at is what the library samples at"""
    case = ic.cases()[name]
    t = ic.tensors(case, DEV)
    got = sample_positions(t["images"], output_hw=case.output_hw, transforms=t["transforms"], source_hw=t["source_hw"]).numpy()
    B, Hs, Ws = case.images.shape[:3]
    Ho, Wo = case.output_hw or (Hs, Ws)
    assert got.shape == (B, Ho, Wo, 4)
    for b in range(B):
        Hv, Wv = (Hs, Ws) if case.source_hw is None else np.clip(case.source_hw[b], 0, (Hs, Ws))
        x0, y0, wx, wy, _ = ic.positions_f32(case.transforms[b], Ho, Wo, int(Wv), int(Hv))
        want = np.stack([x0.astype(np.float32), y0.astype(np.float32), wx, wy], -1)
        assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), f"{name}: image {b}"


def test_positions_on_dyadic_matrices_are_exact():
    """scale 0.5, a flip and a half-pixel shift: the positions are the exact rationals"""
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    pos = lambda m, hw: sample_positions(img, output_hw=hw, transforms=torch.tensor([m], dtype=torch.float32))[0]   # noqa: E731
    p = pos([[0.5, 0, 0], [0, 0.5, 0]], (4, 4))      # centre X + 0.5 -> 2X + 1 -> sample 2X + 0.5
    assert p[1, 2].tolist() == [4.0, 2.0, 0.5, 0.5]
    p = pos([[-1, 0, 8], [0, 1, 0]], (8, 8))
    assert p[3, 0].tolist() == [7.0, 3.0, 0.0, 0.0] and p[3, 7].tolist() == [0.0, 3.0, 0.0, 0.0]
    p = pos([[1, 0, 0.5], [0, 1, 0.5]], (8, 8))
    assert p[0, 0].tolist() == [-1.0, -1.0, 0.5, 0.5] and p[7, 7].tolist() == [6.0, 6.0, 0.5, 0.5]
    p = pos([[1, 0, 9], [0, 1, 0]], (8, 8))          # sx = X - 9 <= -2: nothing inside
    assert bool((p == torch.tensor([-2.0, -2.0, 0.0, 0.0])).all())


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", STORE_CASES)
def test_layouts_dtypes_offset_views_and_guard_bands(name, dtype, layout):
    """float32 against the oracle in both layouts; f16 / bf16 bit-equal to the float32 result's .to(dtype); `out=` is a view
    1 and 3 elements into a buffer of sentinels, which stay intact on both sides"""
    case = ic.cases()[name]
    ref = ic.run(case, DEV, layout=layout)
    ic.check(ref, case, layout)
    for shift in (0, 1, 3):
        buf = torch.full((shift + ref.numel() + 7,), -7.0, dtype=dtype)
        out = buf[shift: shift + ref.numel()].view(ref.shape)
        got = ic.run(case, DEV, layout=layout, dtype=dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(bits(got), bits(ref.to(dtype))), f"shift {shift}"
        assert bool((buf[:shift] == -7.0).all()) and bool((buf[shift + ref.numel():] == -7.0).all())


def test_identity_matrix_and_identity_row_give_the_bits_of_none():
    for name in ("warp_none", "colour_none", "pad_tile_8x32_before_normalize"):
        case = ic.cases()[name]
        B = case.images.shape[0]
        plain = ic.run(case, DEV)
        ident = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]] * B)
        row = torch.tensor([ic.IDENTITY_PHOTOMETRIC] * B)
        assert torch.equal(bits(ic.run(case, DEV, transforms=ident)), bits(plain))
        assert torch.equal(bits(ic.run(case, DEV, photometric=row)), bits(plain))
        assert torch.equal(bits(ic.run(case, DEV, transforms=ident, photometric=row)), bits(plain))
    a, b = (ic.run(ic.cases()[n], DEV) for n in ("warp_none", "warp_identity"))
    assert torch.equal(bits(a), bits(b))
    a, b = (ic.run(ic.cases()[n], DEV) for n in ("colour_none", "colour_identity_row"))
    assert torch.equal(bits(a), bits(b))
    # hue 360 is a full turn: continuous, so within the bar of no change
    ic.check(ic.run(ic.cases()["colour_hue_360"], DEV), ic.cases()["colour_none"])


@pytest.mark.parametrize("with_matrix", [False, True])
def test_source_hw_equals_the_cropped_source(with_matrix):
    """the valid region sits inside a larger tensor whose other bytes are 255: they are never sampled"""
    rng = np.random.default_rng(5)
    valid = [(9, 13), (12, 7), (1, 1)]
    Hs, Ws = 12, 13
    padded = np.full((3, Hs, Ws, 3), 255, np.uint8)
    for b, (h, w) in enumerate(valid):
        padded[b, :h, :w] = rng.integers(0, 256, (h, w, 3))
    m = [[1.3, 0.2, -1.0], [-0.1, 0.9, 2.0]]
    out_hw = (14, 17) if with_matrix else None
    for dt in (torch.int32, torch.int64):
        kw = dict(output_hw=out_hw, transforms=torch.tensor([m] * 3) if with_matrix else None, mean=3.0, std=2.0)
        got = prepare_images(torch.from_numpy(padded), source_hw=torch.tensor(valid, dtype=dt), **kw)
        for b, (h, w) in enumerate(valid):
            if with_matrix:
                alone = prepare_images(torch.from_numpy(np.ascontiguousarray(padded[b:b + 1, :h, :w])), output_hw=out_hw,
                                       transforms=torch.tensor([m]), mean=3.0, std=2.0)
                assert torch.equal(bits(got[b:b + 1]), bits(alone))
            else:
                want = torch.full((3, Hs, Ws), -1.5)       # outside: the value 0, normalised
                want[:, :h, :w] = prepare_images(torch.from_numpy(np.ascontiguousarray(padded[b:b + 1, :h, :w])), mean=3.0, std=2.0)[0]
                assert torch.equal(bits(got[b]), bits(want))


@pytest.mark.parametrize("name", ["warp_singular_zero", "warp_singular_rank_1", "warp_nan_entry", "warp_inf_entry",
                                  "warp_det_underflows", "warp_fully_outside", "source_hw_zero"])
def test_an_image_that_is_outside_equals_the_chain_of_value_0(name):
    case = ic.cases()[name]
    got = ic.run(case, DEV)
    black = prepare_images(torch.zeros_like(torch.from_numpy(case.images)),
                           photometric=None if case.photometric is None else torch.from_numpy(case.photometric), **case.kw)
    assert torch.equal(bits(got), bits(black))
    assert len(torch.unique(got[0, 0])) == 1


def test_padding_holds_the_pad_value_of_every_channel():
    for before, want in ((True, (-5.0, -5.0, -3.75)), (False, (0.0, 0.0, 0.0))):
        case = ic.cases()[f"pad_tile_32_multiple_plus_1_{'before' if before else 'after'}_normalize"]
        got = ic.run(case, DEV)
        assert got.shape == (2, 3, 64, 96)
        for c in range(3):
            assert bool((got[:, c, 33:, :] == want[c]).all()) and bool((got[:, c, :, 65:] == want[c]).all())
    exact = ic.run(ic.cases()["pad_tile_32_exact_multiple_before_normalize"], DEV)
    assert exact.shape == (2, 3, 32, 64)


# ------------------------------------------------------------------------------------------------------------ helpers
RANGES = dict(min_max_brightness=(-32.0, 32.0), min_max_hue=(-18.0, 18.0), min_max_contrast=(0.5, 1.5),
              min_max_saturation=(0.6, 1.4))


def test_sample_photometric_params():
    gen = lambda: torch.Generator().manual_seed(7)   # noqa: E731
    a = sample_photometric_params(200, 6, generator=gen(), **RANGES)
    assert a.shape == (1200, 6) and a.dtype == torch.float32 and a.device.type == "cpu"
    assert torch.equal(a, sample_photometric_params(200, 6, generator=gen(), **RANGES))
    assert not torch.equal(a, sample_photometric_params(200, 6, generator=torch.Generator().manual_seed(8), **RANGES))
    g = a.view(200, 6, 6)
    assert bool((g == g[:, :1]).all()), "the views of a group share one draw"
    rows = g[:, 0]
    lo = torch.tensor([-32 / 255, 0.5, 0.6, -18.0, 0.5, 0.0], dtype=torch.float64)
    hi = torch.tensor([32 / 255, 1.5, 1.4, 18.0, 1.5, 5.0], dtype=torch.float64)
    assert bool((rows.double() >= lo).all()) and bool((rows.double() <= hi).all())
    assert not bool(((rows[:, 1] != 1) & (rows[:, 4] != 1)).any()), "both contrast columns are active"
    assert bool((rows[:, 1] != 1).any()) and bool((rows[:, 4] != 1).any())
    assert set(rows[:, 5].tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    for col, ident in enumerate(ic.IDENTITY_PHOTOMETRIC):   # every augmentation is sometimes on and sometimes off
        on = int((rows[:, col] != ident).sum())
        assert 40 <= on <= 160, (col, on)
    never = sample_photometric_params(50, 2, generator=gen(), prob_brightness_aug=0, prob_hue_aug=0, prob_contrast_aug=0,
                                      prob_saturation_aug=0, prob_swap_channels=0, **RANGES)
    assert torch.equal(never, torch.tensor([ic.IDENTITY_PHOTOMETRIC] * 100))
    always = sample_photometric_params(50, 1, generator=gen(), prob_brightness_aug=1, prob_hue_aug=1, prob_contrast_aug=1,
                                       prob_saturation_aug=1, prob_swap_channels=1, **RANGES)
    assert bool(((always[:, 1] != 1) ^ (always[:, 4] != 1)).all())
    assert sample_photometric_params(0, 3, **RANGES).shape == (0, 6)
    with pytest.raises(RuntimeError, match="min_max_hue"):
        sample_photometric_params(1, 1, **dict(RANGES, min_max_hue=(3.0, 1.0)))


def _reference_output_size(input_hw, output_hw, mode, anchor):
    """AffineTransformer._get_transformation_to_output_size, affine_transformer.py:917-956, in plain numbers"""
    if mode == "stretch":
        return [[output_hw[1] / input_hw[1], 0, 0], [0, output_hw[0] / input_hw[0], 0]]
    pick = min if mode == "pad" else max
    scale_output_input = pick(output_hw[0] / input_hw[0], output_hw[1] / input_hw[1])
    if anchor == "top_or_left":
        shift_x = shift_y = 0.0
    else:
        scale = 0.5 if anchor == "center" else 1.0
        shift_x = output_hw[1] * scale - scale_output_input * input_hw[1] * scale
        shift_y = output_hw[0] * scale - scale_output_input * input_hw[0] * scale
    return [[scale_output_input, 0, shift_x], [0, scale_output_input, shift_y]]


@pytest.mark.parametrize("mode", ["stretch", "pad", "crop"])
@pytest.mark.parametrize("anchor", ["top_or_left", "center", "bottom_or_right"])
@pytest.mark.parametrize("hw", [((900, 1600), (256, 704)), ((45, 80), (13, 35)), ((300, 200), (64, 64))])
def test_output_size_transform(mode, anchor, hw):
    got = output_size_transform(*hw, mode, anchor)
    assert np.allclose(got, _reference_output_size(*hw, mode, anchor), rtol=1e-15, atol=0)
    assert all(isinstance(v, float) for r in got for v in r) and len(got) == 2 and len(got[0]) == 3
    assert output_size_transform(*hw, mode.upper(), anchor.upper()) == got


def test_output_size_transform_streampetr_and_errors():
    assert output_size_transform((900, 1600), (256, 704), "crop", "center") == [[0.44, 0.0, 0.0], [0.0, 0.44, -70.0]]
    with pytest.raises(ValueError, match="mode"):
        output_size_transform((4, 4), (2, 2), "squash", "center")
    with pytest.raises(ValueError, match="anchor"):
        output_size_transform((4, 4), (2, 2), "pad", "middle")


def test_padded_hw():
    assert padded_hw((256, 704), 32) == (256, 704) and padded_hw((257, 705), 32) == (288, 736)
    assert padded_hw((17, 40), (8, 32)) == (24, 64) and padded_hw((5, 7), 1) == (5, 7) and padded_hw((3, 5), (20, 72)) == (20, 72)
    with pytest.raises(RuntimeError, match="tile_hw"):
        padded_hw((4, 4), 0)


# ---------------------------------------------------------------------------------------------------------- interface
def _img(B=1, H=4, W=5, **kw):
    return torch.zeros((B, H, W, 3), dtype=torch.uint8, **kw)


@pytest.mark.parametrize("images, kw, exc, match", [
    (_img().float(), {}, TypeError, "images must be uint8"),
    (_img().to(torch.int8), {}, TypeError, "images must be uint8"),
    (_img()[..., :2], {}, RuntimeError, r"images must be uint8 \[B, H, W, 3\]"),
    (_img()[0], {}, RuntimeError, r"images must be uint8 \[B, H, W, 3\]"),
    (_img(W=10)[:, :, ::2], {}, RuntimeError, "images must be contiguous"),
    (_img(), dict(std=0.0), ValueError, "std must be positive"),
    (_img(), dict(std=(1.0, -1.0, 1.0)), ValueError, "std must be positive"),
    (_img(), dict(std=(1.0, 1.0)), RuntimeError, "std must be a finite Python number or three"),
    (_img(), dict(mean=float("nan")), RuntimeError, "mean must be a finite"),
    (_img(), dict(output_hw=(8, 8)), RuntimeError, "needs transforms"),
    (_img(), dict(output_hw=(4.0, 5)), RuntimeError, "output_hw must be"),
    (_img(), dict(transforms=torch.zeros((2, 2, 3))), RuntimeError, r"transforms must be torch.float32 \[1, 2, 3\]"),
    (_img(), dict(transforms=torch.zeros((1, 3, 3))), RuntimeError, "transforms must be"),
    (_img(), dict(transforms=torch.zeros((1, 2, 3), dtype=torch.float64)), TypeError, "transforms must be float32"),
    (_img(), dict(photometric=torch.zeros((1, 5))), RuntimeError, "photometric must be"),
    (_img(), dict(photometric=torch.zeros((1, 6), dtype=torch.float16)), TypeError, "photometric must be float32"),
    (_img(), dict(source_hw=torch.zeros((1, 2))), RuntimeError, "source_hw must be"),
    (_img(), dict(source_hw=torch.zeros((2, 2), dtype=torch.int64)), RuntimeError, "source_hw must be"),
    (_img(), dict(transforms=torch.zeros((1, 2, 6))[..., ::2]), RuntimeError, "transforms must be contiguous"),
    (_img(), dict(tile_hw=0), RuntimeError, "tile_hw"),
    (_img(), dict(tile_hw=(8, 8, 8)), RuntimeError, "tile_hw"),
    (_img(), dict(layout="NCHW"), RuntimeError, "layout"),
    (_img(), dict(dtype=torch.float64), TypeError, "dtype must be"),
    (_img(), dict(out=torch.zeros((1, 3, 4, 5), dtype=torch.float16)), TypeError, "out must be torch.float32"),
    (_img(), dict(out=torch.zeros((1, 4, 5, 3))), RuntimeError, "out must be"),
    (_img(), dict(out=torch.zeros((1, 3, 4, 10))[..., ::2]), RuntimeError, "out must be contiguous"),
    (_img(), dict(transforms=torch.zeros((1, 2, 3)), output_hw=(16385, 4)), RuntimeError, "every extent must be in"),
    (_img(), dict(transforms=torch.zeros((1, 2, 3)), output_hw=(4, 0)), RuntimeError, "every extent must be in"),
    (_img(H=0), {}, RuntimeError, "every extent must be in"),
    (torch.zeros((1, 1, 16385, 3), dtype=torch.uint8), {}, RuntimeError, "every extent must be in"),
])
def test_argument_rules(images, kw, exc, match):
    with pytest.raises(exc, match="prepare_images: .*" + match):
        prepare_images(images, **kw)


def test_empty_batch_and_output_hw_equal_to_the_source():
    got = ic.run(ic.cases()["batch_0"], DEV)
    assert got.shape == (0, 3, 4, 8) and got.dtype == torch.float32
    assert prepare_images(_img(B=0), layout="HWC", dtype=torch.bfloat16).shape == (0, 4, 5, 3)
    assert prepare_images(_img(), output_hw=(4, 5)).shape == (1, 3, 4, 5)


def _params(**kw):
    p = nat.PrepareImagesParams()
    base = dict(batch=1, source_h=4, source_w=5, output_h=4, output_w=5, tile_h=1, tile_w=1, layout=0, dtype=0)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    for c in range(3):
        p.mean[c], p.std[c] = kw.get("mean_all", 0.0), kw.get("std_all", 1.0)
    return p


@pytest.mark.parametrize("path", ["trampoline", "ctypes"])
@pytest.mark.parametrize("entry", ["accv_prepare_images", "accv_prepare_images_host"])
def test_c_abi_validation_without_gpu(path, entry):
    """ACCV_EINVAL before anything is touched, and the empty problem's success, through both host bindings"""
    lib = nat.lib() if path == "trampoline" else nat.ctypes_lib()
    if path == "trampoline":
        assert nat._fastcall is not None
    fn = getattr(lib, entry)
    img = np.zeros((1, 4, 5, 3), np.uint8)
    out = np.full((3, 4, 5), 7.0, np.float32)
    mats = np.zeros((1, 2, 3), np.float32)

    def call(p, images=img.ctypes.data, source_hw=None, transforms=None, photometric=None, out_ptr=out.ctypes.data, last=None):
        return fn(images, source_hw, transforms, photometric, None if p is None else ctypes.addressof(p), out_ptr, last)

    def refused(text, *a, **kw):
        assert call(*a, **kw) == -1
        assert text in nat.ctypes_lib().accv_last_error().decode(), nat.ctypes_lib().accv_last_error()

    refused("null params", None)
    refused("negative batch", _params(batch=-1))
    refused("each must be in [1, 16384]", _params(source_h=0))
    refused("each must be in [1, 16384]", _params(output_w=16385), transforms=mats.ctypes.data)
    refused("each must be in [1, 16384]", _params(tile_h=0))
    refused("needs transforms", _params(output_h=8))
    refused("unknown layout", _params(layout=2))
    refused("unknown output dtype", _params(dtype=3))
    refused("std > 0", _params(std_all=0.0))
    refused("std > 0", _params(mean_all=float("inf")))
    refused("null images / out", _params(), images=None)
    refused("null images / out", _params(), out_ptr=None)
    refused("transforms / photometric are not aligned", _params(), transforms=mats.ctypes.data + 2)
    refused("source_hw is not aligned", _params(source_hw_i64=1), source_hw=mats.ctypes.data + 4)
    refused("out is not aligned", _params(), out_ptr=out.ctypes.data + 2)
    refused("exceed the grid limit", _params(batch=1 << 40))
    assert bool((out == 7.0).all()), "a refused call wrote something"
    assert call(_params(batch=0), images=None, out_ptr=None) == 0        # the empty problem: nothing is touched
    assert call(_params(batch=0, output_h=9)) == -1                      # but its parameters are still checked
    if entry.endswith("_host"):
        assert call(_params()) == 0 and bool((out == 0.0).all())
