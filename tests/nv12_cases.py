"""Cases and an independent oracle for accvlab.image_prep.nv12_to_rgb and prepare_images_nv12, shared by test_nv12_cpu.py and
test_nv12_gpu.py.

The oracle is a numpy restatement of the operator's docstring, not of the library: the limited range in int64 (so an
overflow of the library's int32 would show), the full range in numpy float32, one operation per step.  Every comparison
made with it is exact equality of bytes; no tolerance exists in these tests.

The fused operator has no oracle of its own: its contract is bit-equality with ``prepare_images(nv12_to_rgb(...))``, and
``prepare_images`` is held to its float64 oracle by test_image_prep_*.py.  The geometry, photometric rows, ``source_hw``,
normalisation and tiles come from ``image_prep_cases.cases()``; the planes are seeded noise of the case's ``[B, Hs, Ws]``, cut
from pitched surfaces.
"""
import functools

import numpy as np
import torch

import image_prep_cases as ic
from accvlab.image_prep import nv12_planes, nv12_to_rgb, prepare_images, prepare_images_nv12

F32 = np.float32
FORMATS = {"limited": {}, "full": dict(full_range=True), "bgr": dict(as_bgr=True), "vu": dict(chroma_order="vu"),
           "full_bgr_vu": dict(full_range=True, as_bgr=True, chroma_order="vu")}
GRID_H = (1, 2, 3, 5, 16, 17)
GRID_W = (1, 2, 3, 4, 5, 7, 63, 64, 65, 131)
# the fused contract in the other formats: partition cases, the batch case, two pad cases, every colour stage with a warp
FORMAT_CASES = ["partition_17x131", "partition_15x63", "partition_16x64", "partition_1x1", "batch_7_parameters_per_image",
                "pad_tile_8x32_before_normalize", "pad_tile_8x32_after_normalize", "colour_all_with_a_warp"]


# ------------------------------------------------------------------------------------------------------------- oracle
def _descale_clamp(t):
    return np.clip((t.astype(np.int64) + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def oracle_rgb(Y, U, V, full_range=False):
    """(R, G, B) uint8 arrays from uint8 arrays of equal shape"""
    if not full_range:
        Y, U, V = (a.astype(np.int64) for a in (Y, U, V))
        yy = np.maximum(0, Y - 16) * 1220542
        uu, vv = U - 128, V - 128
        t = (yy + 1673527 * vv, yy - 852492 * vv - 409993 * uu, yy + 2116026 * uu)
        assert all(-2 ** 31 <= int(x.min()) and int(x.max()) + (1 << 19) < 2 ** 31 for x in t)
        return tuple(_descale_clamp(x) for x in t)
    C0, C1, C2, C3, C4 = (F32(c) for c in (1048230.1882352941, 1470078.6196078432, -748855.7176470588, -360150.7137254902,
                                            1858783.6235294119))
    half = F32(0.5)
    yy = np.maximum(F32(0), Y.astype(F32)) * C0
    uu, vv = U.astype(F32) - F32(127.5), V.astype(F32) - F32(127.5)
    r = (yy + C1 * vv) + half
    g = ((yy + C2 * vv) + C3 * uu) + half
    b = (yy + C4 * uu) + half
    assert r.dtype == g.dtype == b.dtype == F32
    return tuple(_descale_clamp(np.trunc(x).astype(np.int32)) for x in (r, g, b))


def oracle_image(y, uv, full_range=False, as_bgr=False, chroma_order="uv"):
    """uint8 [B, H, W, 3] from numpy planes y [B, H, W] and uv [B, ceil(H/2), ceil(W/2), 2]: chroma sample (y // 2, x // 2)"""
    B, H, W = y.shape
    rows, cols = np.arange(H) // 2, np.arange(W) // 2
    up = uv[:, rows][:, :, cols]
    u, v = (up[..., 1], up[..., 0]) if chroma_order == "vu" else (up[..., 0], up[..., 1])
    r, g, b = oracle_rgb(y, u, v, full_range)
    return np.stack((b, g, r) if as_bgr else (r, g, b), axis=-1)


# -------------------------------------------------------------------------------------------------------------- planes
@functools.lru_cache(maxsize=None)
def exhaustive_planes():
    """y [1, 4096, 4096], uv [1, 2048, 2048, 2] (torch, CPU, shared, never written to) in which every (Y, U, V) triple
    occurs once: chroma sample k = row * 2048 + col holds pair k // 64 as (U, V) = (pair >> 8, pair & 255), and the four
    luma bytes under it are (k % 64) * 4 + 0..3, so the 64 samples of a pair run through 0..255"""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair, slot = k // 64, k % 64
    uv = np.stack([pair >> 8, pair & 255], axis=-1).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[dy::2, dx::2] = slot * 4 + dy * 2 + dx
    return torch.from_numpy(y[None]), torch.from_numpy(uv[None])


@functools.lru_cache(maxsize=None)
def exhaustive_oracle(full_range):
    """uint8 [1, 4096, 4096, 3] (torch), computed once per module run and never written to"""
    y, uv = exhaustive_planes()
    return torch.from_numpy(oracle_image(y.numpy(), uv.numpy(), full_range=full_range))


def every_triple_occurs_once():
    y, uv = (t.numpy()[0].astype(np.int64) for t in exhaustive_planes())
    up = uv[np.arange(4096) // 2][:, np.arange(4096) // 2]
    code = (y << 16) | (up[..., 0] << 8) | up[..., 1]
    return np.array_equal(np.sort(code.ravel()), np.arange(1 << 24))


def surfaces(B, H, W, seed, fill=0, extra_pitch=13, uv_gap=3, device="cpu"):
    """(surfaces, uv_row): uint8 [B, rows, pitch] whole surfaces, a view into a larger tensor (the batch stride exceeds the
    surface), holding `fill` everywhere except in the two planes of images of H x W, which are seeded noise that does not
    depend on `fill`.  pitch = W + extra_pitch rounded up to even; the UV plane starts uv_gap rows below the luma."""
    pitch = W + extra_pitch + ((W + extra_pitch) & 1)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    uv_row = H + uv_gap
    rows = uv_row + Hc + 1
    rng = np.random.default_rng(seed)
    big = np.full((B, rows + 2, pitch), fill, np.uint8)
    big[:, :H, :W] = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    big[:, uv_row:uv_row + Hc, :2 * Wc] = rng.integers(0, 256, (B, Hc, 2 * Wc), dtype=np.uint8)
    return torch.from_numpy(big).to(device)[:, :rows], uv_row


def grid_planes(H, W, seed=7, fill=0, device="cpu"):
    """the pitched plane views of the shape grid: B = 3"""
    s, uv_row = surfaces(3, H, W, seed, fill=fill, device=device)
    return nv12_planes(s, (H, W), uv_row=uv_row)


def numpy_planes(y, uv):
    return y.cpu().contiguous().numpy(), uv.cpu().contiguous().numpy()


# ------------------------------------------------------------------------------------------------------ fused contract
def case_planes(case, device):
    """seeded planes of the case's [B, Hs, Ws], cut from pitched surfaces whose padding is 255"""
    B, Hs, Ws = case.images.shape[:3]
    seed = sum(case.name.encode()) + 1000 * Hs + Ws
    s, uv_row = surfaces(B, Hs, Ws, seed, fill=255, extra_pitch=6, uv_gap=1, device=device)
    return nv12_planes(s, (Hs, Ws), uv_row=uv_row)


def case_kw(case, device, **over):
    t = ic.tensors(case, device)
    t.pop("images")
    kw = {k: v for k, v in case.kw.items() if k != "is_bgr"}
    return {**t, **kw, "output_hw": case.output_hw, **over}


def case_format(case, fmt):
    """the format keywords: in the limited-range run of every case, as_bgr follows the case's is_bgr"""
    f = dict(FORMATS[fmt])
    if fmt == "limited" and case.kw.get("is_bgr", False):
        f["as_bgr"] = True
    return f


def run_fused(case, device, fmt="limited", **over):
    y, uv = case_planes(case, device)
    return prepare_images_nv12(y, uv, **case_format(case, fmt), **case_kw(case, device, **over))


def run_composed(case, device, fmt="limited", **over):
    """conversion + prepare_images: what the fused call must equal bit for bit"""
    y, uv = case_planes(case, device)
    f = case_format(case, fmt)
    return prepare_images(nv12_to_rgb(y, uv, **f), is_bgr=f.get("as_bgr", False), **case_kw(case, device, **over))


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).cpu()


def translation_cases():
    """a 6 x 7 source translated by 0.5, 1.0 and 1.5 pixels in x and in y: bilinear pairs that straddle two UV pairs (odd x0)
    and two chroma rows (odd y0), footprints on the border included"""
    rng = np.random.default_rng(11)
    out = {}
    for axis in "xy":
        for t in (0.5, 1.0, 1.5):
            m = [[1, 0, t if axis == "x" else 0], [0, 1, t if axis == "y" else 0]]
            name = f"translate_{axis}_{t}"
            out[name] = ic.Case(name, rng.integers(0, 256, (1, 6, 7, 3), dtype=np.uint8), transforms=np.asarray([m], F32),
                                kw=dict(mean=(10.0, 20.0, 30.0), std=(2.0, 4.0, 8.0)))
    return out
