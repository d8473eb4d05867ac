"""CPU-only checks of the fused Gaussian focal loss: the C-ABI status codes (through the trampoline table and plain ctypes),
the public export, and the argument checks the Python layer makes before anything reaches a device."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("path", ["lib", "ctypes"])
def test_focal_loss_cabi_status_codes(path):
    from accvlab import _amd_native as nat

    lib = nat.lib() if path == "lib" else nat.ctypes_lib()
    d = ctypes.c_void_p(256)
    p = (2.0, 4.0, 1.0, 1.0, 1e-4)

    def fwd(x, t, n, dtype=0, params=p, mode=nat.FL_AVG_NUM_POS, dev=None, loss=d, den=d, ws=d, ws_bytes=1 << 20):
        return lib.accv_gaussian_focal_loss(x, t, n, dtype, *params, mode, 1.0, dev, loss, den, ws, ws_bytes, None)

    def bwd(x, t, n, dtype=0, params=p, go=d, den=d, g=d):
        return lib.accv_gaussian_focal_loss_bwd(x, t, n, dtype, *params, go, den, g, None)

    assert lib.accv_gaussian_focal_loss_workspace_bytes(0) == 0
    assert lib.accv_gaussian_focal_loss_workspace_bytes(-5) == 0
    need = lib.accv_gaussian_focal_loss_workspace_bytes(64 * 1080 * 1920)
    assert need > 0 and need % 16 == 0
    assert lib.accv_gaussian_focal_loss_workspace_bytes(1) >= 16
    # negative numel, bad dtype codes, null pointers with numel > 0 -> ACCV_EINVAL before touching the device
    assert fwd(d, d, -1) == -1
    assert b"negative" in lib.accv_last_error()
    assert bwd(d, d, -1) == -1
    for code in (-1, 3, 7):
        assert fwd(d, d, 16, dtype=code) == -1
        assert b"dtype" in lib.accv_last_error()
        assert bwd(d, d, 16, dtype=code) == -1
    assert fwd(None, d, 16) == -1 and b"null" in lib.accv_last_error()
    assert fwd(d, None, 16) == -1
    assert fwd(d, d, 16, loss=None) == -1
    assert fwd(d, d, 16, den=None) == -1
    assert fwd(d, d, 16, mode=nat.FL_AVG_DEVICE, dev=None) == -1
    assert fwd(d, d, 16, mode=5) == -1
    assert bwd(None, d, 16) == -1
    assert bwd(d, d, 16, go=None) == -1
    assert bwd(d, d, 16, den=None) == -1
    assert bwd(d, d, 16, g=None) == -1
    # exponent range
    assert fwd(d, d, 16, params=(0.5, 4.0, 1.0, 1.0, 1e-4)) == -1 and b"alpha" in lib.accv_last_error()
    assert fwd(d, d, 16, params=(2.0, -1.0, 1.0, 1.0, 1e-4)) == -1
    assert fwd(d, d, 16, params=(float("nan"), 4.0, 1.0, 1.0, 1e-4)) == -1
    assert bwd(d, d, 16, params=(0.5, 4.0, 1.0, 1.0, 1e-4)) == -1
    assert fwd(d, d, 16, params=(2.0, 4.0, 1.0, 1.0, 0.5)) == -1
    # a short, missing or misaligned workspace -> ACCV_EWORKSPACE
    n = 1 << 20
    short = lib.accv_gaussian_focal_loss_workspace_bytes(n) - 16
    assert fwd(d, d, n, ws_bytes=short) == -3
    assert b"workspace" in lib.accv_last_error()
    assert fwd(d, d, n, ws=None) == -3
    assert fwd(d, d, n, ws=ctypes.c_void_p(264)) == -3
    # numel == 0 -> ACCV_OK without a launch, even with null pointers everywhere
    assert fwd(None, None, 0, loss=None, den=None, ws=None, ws_bytes=0) == 0
    assert bwd(None, None, 0, go=None, den=None, g=None) == 0


def test_focal_loss_is_exported():
    import accvlab.draw_heatmap as dh
    from accvlab.draw_heatmap.focal_loss import gaussian_focal_loss

    assert "gaussian_focal_loss" in dh.__all__
    assert dh.gaussian_focal_loss is gaussian_focal_loss


def test_focal_loss_refuses_cpu_tensors():
    from accvlab.draw_heatmap import gaussian_focal_loss

    x = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        gaussian_focal_loss(x, torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError, match="CUDA"):
        gaussian_focal_loss(x.bfloat16(), torch.zeros(2, 8, 8))


def test_focal_loss_refuses_non_contiguous_tensors():
    from accvlab.draw_heatmap import gaussian_focal_loss

    x = torch.zeros(8, 6).t()
    assert not x.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        gaussian_focal_loss(x, torch.zeros(6, 8))


def test_focal_loss_refuses_non_tensors():
    from accvlab.draw_heatmap import gaussian_focal_loss

    with pytest.raises(RuntimeError):
        gaussian_focal_loss([0.0, 1.0], torch.zeros(2))
