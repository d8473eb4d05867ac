"""CPU-only checks of the centre-point regression operators: the C-ABI status codes (through the trampoline table and plain
ctypes), the argument checks the Python layer makes before anything reaches a device, the public exports, and the float64
oracle of center_regression_cases.py against a plain per-object loop."""
import ctypes

import pytest
import torch

import center_regression_cases as cr


class _Args:
    """arguments of the four entries that pass every check, as plain integers (the trampoline takes no ctypes objects)"""

    def __init__(self, nat):
        self.nat = nat
        self.d = 256
        self.maps = (ctypes.c_void_p * 8)(*[256 + 64 * i for i in range(8)])
        self.chans = (ctypes.c_int * 8)(2, 1, 3, 2, 2, 1, 1, 1)
        self.params = nat.CenterRegressionParams(nat.CR_L1, nat.FL_AVG_NUM_POS, 1.0, 0.0)

    def geometry(self, maps="ok", chans="ok", n=5, dtype=0, shape=(2, 40, 50), centers=256, counts=256, N=7):
        maps = ctypes.addressof(self.maps) if maps == "ok" else maps
        chans = ctypes.addressof(self.chans) if chans == "ok" else chans
        return (maps, chans, n, dtype, *shape, centers, counts, N)


@pytest.mark.parametrize("path", ["lib", "ctypes"])
def test_center_regression_cabi_status_codes(path):
    from accvlab import _amd_native as nat

    lib = nat.lib() if path == "lib" else nat.ctypes_lib()
    a = _Args(nat)
    d, p = a.d, ctypes.addressof(a.params)
    entries = {
        "gather": lambda flags=0, out=d, **kw: lib.accv_gather_at_centers(*a.geometry(**kw), flags, out, None),
        "scatter": lambda flags=0, out=d, **kw: lib.accv_scatter_at_centers(*a.geometry(**kw), flags, out, None),
        "loss": lambda flags=0, params=p, t=d, outs=(d, d), ws=d, ws_bytes=1 << 20, avg=None, **kw:
            lib.accv_center_regression_loss(*a.geometry(**kw), flags, t, None, params, avg, *outs, ws, ws_bytes, None),
        "loss_bwd": lambda flags=0, params=p, t=d, scalars=(d, d), gmaps="ok", maps="ok", **kw:
            lib.accv_center_regression_loss_bwd(a.geometry(maps=maps)[0], ctypes.addressof(a.maps) if gmaps == "ok" else gmaps,
                                                *a.geometry(**kw)[1:], flags, t, None, params, *scalars, None),
    }
    for name, call in entries.items():
        # negative sizes, unknown dtype codes and flags, map and channel limits -> ACCV_EINVAL before the device
        for bad in ((-1, 40, 50), (2, -40, 50), (2, 40, -50)):
            assert call(shape=bad) == -1, name
            assert b"negative" in lib.accv_last_error()
        assert call(N=-1) == -1 and b"negative" in lib.accv_last_error()
        for code in (-1, 3, 7):
            assert call(dtype=code) == -1 and b"dtype" in lib.accv_last_error(), name
        assert call(flags=64) == -1 and b"flag" in lib.accv_last_error(), name
        for n in (0, 9, -1):
            assert call(n=n) == -1 and b"1..8 maps" in lib.accv_last_error(), name
        many = (ctypes.c_int * 8)(32, 32, 1, 0, 0, 0, 0, 0)
        assert call(chans=ctypes.addressof(many), n=3) == -1 and b"more than 64 channels" in lib.accv_last_error(), name
        assert call(chans=ctypes.addressof(many), n=2, shape=(0, 40, 50)) == 0, name   # the cap itself is taken (empty batch)
        neg = (ctypes.c_int * 8)(2, -1, 0, 0, 0, 0, 0, 0)
        assert call(chans=ctypes.addressof(neg), n=2) == -1 and b"negative channel" in lib.accv_last_error(), name
        assert call(shape=(1, 65536, 32768)) == -1 and b"2^31" in lib.accv_last_error(), name
        # null arrays, null and misaligned maps, null centres and counts
        assert call(chans=None) == -1 and b"null array" in lib.accv_last_error(), name
        if name != "loss_bwd":
            assert call(maps=None) == -1 and b"null array" in lib.accv_last_error(), name
        holes = (ctypes.c_void_p * 8)(256, None, 256, 256, 256, 256, 256, 256)
        odd = (ctypes.c_void_p * 8)(256, 258, 256, 256, 256, 256, 256, 256)
        key = "gmaps" if name == "loss_bwd" else "maps"
        assert call(**{key: ctypes.addressof(holes)}) == -1 and b"map 1 is null" in lib.accv_last_error(), name
        assert call(**{key: ctypes.addressof(odd)}) == -1 and b"not aligned" in lib.accv_last_error(), name
        assert call(centers=None) == -1 and b"null centers" in lib.accv_last_error(), name
        assert call(counts=None) == -1 and b"null counts" in lib.accv_last_error(), name
        # B == 0 -> ACCV_OK without a launch, even with null pointers
        assert call(shape=(0, 40, 50), centers=None, counts=None) == 0, name
    # the index form needs no counts and is a gather-only flag
    assert entries["gather"](flags=nat.CR_INDEX_FORM, counts=None, out=None) == -1 and b"null output" in lib.accv_last_error()
    assert entries["scatter"](flags=nat.CR_INDEX_FORM, counts=None, out=None) == -1 and b"null gradient rows" in lib.accv_last_error()
    for name in ("loss", "loss_bwd"):
        call = entries[name]
        assert call(flags=nat.CR_INDEX_FORM) == -1 and b"flag" in lib.accv_last_error()
        assert call(maps=None) == -1 and b"null array" in lib.accv_last_error()
        assert call(params=None) == -1 and b"null params" in lib.accv_last_error()
        for kind in (1, 3, -1):
            bad = nat.CenterRegressionParams(kind, 0, 1.0, 0.0)
            assert call(params=ctypes.addressof(bad)) == -1 and b"loss kind" in lib.accv_last_error()
        for beta in (0.0, -1.0, float("nan")):
            bad = nat.CenterRegressionParams(nat.CR_SMOOTH_L1, 0, beta, 0.0)
            assert call(params=ctypes.addressof(bad)) == -1 and b"beta" in lib.accv_last_error()
        assert call(t=None) == -1 and b"null targets" in lib.accv_last_error()
    # empty outputs of the gather launch nothing
    assert entries["gather"](N=0, out=None, centers=None) == 0
    # the forward: avg modes, outputs, workspace
    loss = entries["loss"]
    for mode in (-1, 3):
        bad = nat.CenterRegressionParams(nat.CR_L1, mode, 1.0, 0.0)
        assert loss(params=ctypes.addressof(bad)) == -1 and b"avg_factor mode" in lib.accv_last_error()
    dev_mode = nat.CenterRegressionParams(nat.CR_L1, nat.FL_AVG_DEVICE, 1.0, 0.0)
    assert loss(params=ctypes.addressof(dev_mode)) == -1 and b"null avg_factor" in lib.accv_last_error()
    for outs in ((None, d), (d, None)):
        assert loss(outs=outs) == -1 and b"null output" in lib.accv_last_error()
    need = lib.accv_center_regression_loss_workspace_bytes(2)
    assert need == 32 and lib.accv_center_regression_loss_workspace_bytes(0) == 0
    assert lib.accv_center_regression_loss_workspace_bytes(-3) == 0 and lib.accv_center_regression_loss_workspace_bytes(1001) == 16016
    assert loss(ws_bytes=need - 16) == -3 and b"workspace" in lib.accv_last_error()
    assert loss(ws=None) == -3
    assert loss(ws=264) == -3
    for scalars in ((None, d), (d, None)):
        assert entries["loss_bwd"](scalars=scalars) == -1 and b"null grad_out" in lib.accv_last_error()


def test_center_regression_is_exported():
    import accvlab.draw_heatmap as dh
    from accvlab.draw_heatmap.center_regression import MAX_CHANNELS, MAX_MAPS, center_regression_loss, gather_at_centers

    assert "gather_at_centers" in dh.__all__ and "center_regression_loss" in dh.__all__
    assert dh.gather_at_centers is gather_at_centers and dh.center_regression_loss is center_regression_loss
    assert MAX_MAPS == 8 and MAX_CHANNELS >= 32


def test_center_regression_refuses_cpu_tensors_and_non_tensors():
    from accvlab.draw_heatmap import center_regression_loss, gather_at_centers

    xy = cr.ragged(torch.zeros(2, 3, 2, dtype=torch.int32), [3, 1])
    tg = torch.zeros(2, 3, 4)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        maps = torch.zeros(2, 4, 8, 8, dtype=dtype)
        with pytest.raises(RuntimeError, match="gather_at_centers.*CUDA"):
            gather_at_centers(maps, xy)
        with pytest.raises(RuntimeError, match="gather_at_centers.*CUDA"):
            gather_at_centers([maps, maps], torch.zeros(2, 3, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="center_regression_loss.*CUDA"):
            center_regression_loss(maps, xy, tg)
    for bad in ([[0.0]], None, [], [torch.zeros(1, 1, 2, 2), 3.0]):
        with pytest.raises(RuntimeError, match="tensor"):
            gather_at_centers(bad, xy)
        with pytest.raises(RuntimeError, match="tensor"):
            center_regression_loss(bad, xy, tg)
    with pytest.raises(RuntimeError, match="at most 8 maps"):
        gather_at_centers([torch.zeros(1, 1, 2, 2)] * 9, xy)


@pytest.mark.parametrize("kind", ["l1", "smooth_l1"])
@pytest.mark.parametrize("weights", ["none", "object", "channel"])
@pytest.mark.parametrize("avg", ["default", "number", "tensor"])
def test_oracle_equals_a_per_object_loop(kind, weights, avg):
    B, N, H, W, channels = 3, 6, 5, 7, [2, 1, 3]
    C = sum(channels)
    sizes = torch.tensor([6, 0, 4])
    maps = cr.make_maps(B, channels, H, W, torch.float64, "cpu", seed=3)
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=4, margin=2)
    xy[0, 1] = xy[0, 0] = torch.tensor([3, 2], dtype=torch.int32)   # two objects on one cell
    xy[2, 3] = xy[0, 0]                                              # and the same cell in another frame
    g = torch.Generator().manual_seed(5)
    targets = torch.randn(B, N, C, generator=g, dtype=torch.float64) * 3.0
    targets[0, 0, 0] = maps[0][0, 0, 2, 3] - 0.25                    # inside the quadratic zone of smooth_l1
    w = {"none": None, "object": torch.rand(B, N, generator=g, dtype=torch.float64),
         "channel": torch.rand(B, N, C, generator=g, dtype=torch.float64)}[weights]
    avg_factor = {"default": None, "number": 7.5, "tensor": torch.tensor(3.25)}[avg]
    loss, grads = cr.oracle_loss(maps, xy, sizes, targets, w, kind, 0.8, avg_factor)
    want, want_grads = cr.loop_loss(maps, xy, sizes, targets, w, kind, 0.8, avg_factor)
    valid, _ = cr.valid_and_index(xy, sizes, H, W)
    assert 0 < int(valid.sum()) < int(sizes.sum()), "the case must hold centres inside and outside the map"
    assert abs(float(loss) - want) <= 1e-12 * abs(want)
    for got, ref in zip(grads, want_grads):
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-15)
        assert torch.equal(got == 0, ref == 0)
    # the gather of the oracle: rows of valid slots are the maps' values, every other row is 0
    rows = cr.oracle_gather(maps, xy, sizes)
    f = torch.cat(maps, 1)
    for b in range(B):
        for n in range(N):
            want_row = f[b, :, int(xy[b, n, 1]), int(xy[b, n, 0])] if bool(valid[b, n]) else torch.zeros(C, dtype=torch.float64)
            assert torch.equal(rows[b, n], want_row)
    ind = torch.where(valid, xy[..., 1].long() * W + xy[..., 0].long(), torch.full((B, N), -1))
    assert torch.equal(cr.oracle_gather_indices(maps, ind), rows)


def test_oracle_keeps_nan_of_invalid_slots_out():
    B, N, H, W = 2, 4, 3, 3
    sizes = torch.tensor([2, 1])
    maps = cr.make_maps(B, [2], H, W, torch.float64, "cpu")
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", margin=0)
    valid, _ = cr.valid_and_index(xy, sizes, H, W)
    targets = torch.zeros(B, N, 2, dtype=torch.float64)
    targets[~valid] = float("nan")
    weights = torch.ones(B, N, dtype=torch.float64)
    weights[~valid] = float("nan")
    loss, grads = cr.oracle_loss(maps, xy, sizes, targets, weights)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grads[0]).all())
