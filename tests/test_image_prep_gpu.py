"""prepare_images on the GPU: the kernel against the float64 oracle of image_prep_cases.py (one derived bar, no element
excluded) and bit for bit against the library's host entry for every case; every dtype and layout through aligned and
misaligned `out=` views between guard bands; the bit-equalities the operator promises; a non-default stream without host
synchronisation; limits and wrong devices refused before any launch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_prep_cases as ic  # noqa: E402

from accvlab.image_prep import prepare_images  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
STORE_CASES = ["partition_17x131", "partition_15x63", "partition_16x64", "partition_1x1", "partition_17x5",
               "batch_7_parameters_per_image", "pad_tile_8x32_before_normalize", "colour_all_with_a_warp"]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


@pytest.mark.parametrize("name", ic.case_names())
def test_case_against_the_oracle_and_the_host_entry(name):
    """`out=` arrives full of NaN: every element must be written"""
    case = ic.cases()[name]
    out = torch.full(ic.oracle(name).shape, float("nan"), device=DEV)
    got = ic.run(case, DEV, out=out)
    assert got is out and got.is_cuda
    ic.check(got, case)
    assert torch.equal(bits(got), bits(ic.run(case, "cpu"))), f"{name}: device and host entry differ"


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", STORE_CASES)
def test_layouts_dtypes_offset_views_and_guard_bands(name, dtype, layout):
    """float32 against the oracle in both layouts; f16 / bf16 bit-equal to the float32 result's .to(dtype); `out=` at an
    aligned base and 1 and 3 elements off it (the per-element stores), full of NaN inside a buffer of sentinels that stay
    intact on both sides"""
    case = ic.cases()[name]
    ref = ic.run(case, DEV, layout=layout)
    ic.check(ref, case, layout)
    want = bits(ref.to(dtype))
    assert torch.equal(want, bits(ic.run(case, "cpu", layout=layout, dtype=dtype))), "device and host entry differ"
    n, band = ref.numel(), 64
    for shift in (0, 1, 3):
        buf = torch.full((band + shift + n + band,), -7.0, dtype=dtype, device=DEV)
        out = buf[band + shift: band + shift + n].view(ref.shape)
        out.fill_(float("nan"))
        assert out.data_ptr() % 16 == (shift * out.element_size()) % 16
        got = ic.run(case, DEV, layout=layout, dtype=dtype, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(bits(got), want), f"shift {shift}"
        assert bool((buf[:band + shift] == -7.0).all()) and bool((buf[band + shift + n:] == -7.0).all()), "wrote outside out"


def test_identity_matrix_and_identity_row_give_the_bits_of_none():
    for name in ("warp_none", "colour_none", "pad_tile_8x32_before_normalize"):
        case = ic.cases()[name]
        B = case.images.shape[0]
        plain = ic.run(case, DEV)
        ident = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]] * B, device=DEV)
        row = torch.tensor([ic.IDENTITY_PHOTOMETRIC] * B, device=DEV)
        assert torch.equal(bits(ic.run(case, DEV, transforms=ident)), bits(plain))
        assert torch.equal(bits(ic.run(case, DEV, photometric=row)), bits(plain))
        assert torch.equal(bits(ic.run(case, DEV, transforms=ident, photometric=row)), bits(plain))


def test_source_hw_equals_the_cropped_source():
    """the valid region sits inside a larger tensor whose other bytes are 255: they are never sampled"""
    gen = torch.Generator().manual_seed(5)
    valid = [(9, 13), (12, 7), (1, 1)]
    padded = torch.full((3, 12, 13, 3), 255, dtype=torch.uint8)
    for b, (h, w) in enumerate(valid):
        padded[b, :h, :w] = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8)
    m = [[1.3, 0.2, -1.0], [-0.1, 0.9, 2.0]]
    got = prepare_images(padded.to(DEV), source_hw=torch.tensor(valid, dtype=torch.int32, device=DEV), output_hw=(14, 17),
                         transforms=torch.tensor([m] * 3, device=DEV), mean=3.0, std=2.0)
    for b, (h, w) in enumerate(valid):
        alone = prepare_images(padded[b:b + 1, :h, :w].contiguous().to(DEV), output_hw=(14, 17),
                               transforms=torch.tensor([m], device=DEV), mean=3.0, std=2.0)
        assert torch.equal(bits(got[b:b + 1]), bits(alone))


def test_non_default_stream_and_no_host_synchronisation():
    case = ic.cases()["batch_7_parameters_per_image"]
    t = ic.tensors(case, DEV)
    images = t.pop("images")
    kw = dict(case.kw, output_hw=case.output_hw, **t)
    first = prepare_images(images, **kw)                              # warm-up: library load, allocator
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            on_stream = prepare_images(images, **kw)
        again = prepare_images(images, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(bits(on_stream), bits(first)) and torch.equal(bits(again), bits(first))
    ic.check(on_stream, case)


def test_limits_and_wrong_devices_raise_before_any_launch():
    img = torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="prepare_images: .*every extent must be in"):
        prepare_images(img, transforms=torch.zeros((1, 2, 3), device=DEV), output_hw=(4, 16385))
    with pytest.raises(RuntimeError, match="prepare_images: transforms must be on the images' device"):
        prepare_images(img, transforms=torch.zeros((1, 2, 3)))
    with pytest.raises(RuntimeError, match="prepare_images: out must be on the images' device"):
        prepare_images(img, out=torch.zeros((1, 3, 4, 5)))
    with pytest.raises(TypeError, match="prepare_images: images must be uint8"):
        prepare_images(img.float())
    with pytest.raises(ValueError, match="prepare_images: std must be positive"):
        prepare_images(img, std=0.0)
    assert prepare_images(img[:0]).shape == (0, 3, 4, 5)
