"""CPU-only checks of the heat-map peak extraction: the C-ABI status codes (through the trampoline table and plain ctypes),
the workspace query, the public export, and the argument checks the Python layer makes before anything reaches a device."""
import pytest
import torch


@pytest.mark.parametrize("path", ["lib", "ctypes"])
def test_heatmap_peaks_cabi_status_codes(path):
    from accvlab import _amd_native as nat

    lib = nat.lib() if path == "lib" else nat.ctypes_lib()
    d = 256   # a plain integer: the trampoline would pass a c_void_p object's own host address instead of its value
    shape = (2, 3, 40, 50)

    def call(x=d, dtype=0, shape=shape, kernel=3, k=100, per_class=0, outs=(d, d, d, d, d), ws=d, ws_bytes=1 << 30):
        return lib.accv_heatmap_peaks(x, dtype, *shape, kernel, k, per_class, *outs, ws, ws_bytes, None)

    # negative sizes, bad dtype codes, even or out-of-range kernels, k out of range -> ACCV_EINVAL before the device
    for bad in ((-1, 3, 40, 50), (2, -3, 40, 50), (2, 3, -40, 50), (2, 3, 40, -50)):
        assert call(shape=bad) == -1
        assert b"negative" in lib.accv_last_error()
    for code in (-1, 3, 7):
        assert call(dtype=code) == -1
        assert b"dtype" in lib.accv_last_error()
    for kernel in (0, 2, 4, 8, 9, -3):
        assert call(kernel=kernel) == -1
        assert b"kernel" in lib.accv_last_error()
    for k in (0, -1, 1025):
        assert call(k=k) == -1
        assert b"k must be" in lib.accv_last_error()
    # k above the group: 40 * 50 per plane, 3 * 40 * 50 per frame
    assert call(k=1001, shape=(2, 3, 20, 50), per_class=1) == -1
    assert b"group size" in lib.accv_last_error()
    assert call(k=5, shape=(2, 1, 2, 2)) == -1
    # groups of 2^32 - 1 elements or more do not fit the key's index word
    assert call(shape=(1, 1, 65536, 65536)) == -1
    assert call(shape=(1, 2, 65536, 32768)) == -1
    # null pointers
    assert call(x=None) == -1 and b"null" in lib.accv_last_error()
    for i in range(5):
        outs = [d] * 5
        outs[i] = None
        assert call(outs=tuple(outs)) == -1
        assert b"null" in lib.accv_last_error()
    # a short, missing or misaligned workspace -> ACCV_EWORKSPACE
    need = lib.accv_heatmap_peaks_workspace_bytes(*shape, 100)
    assert call(ws_bytes=need - 16) == -3
    assert b"workspace" in lib.accv_last_error()
    assert call(ws=None) == -3
    assert call(ws=264) == -3
    # B == 0 -> ACCV_OK without a launch, even with null pointers
    assert call(x=None, shape=(0, 3, 40, 50), outs=(None,) * 5, ws=None, ws_bytes=0) == 0


@pytest.mark.parametrize("path", ["lib", "ctypes"])
def test_heatmap_peaks_workspace_query(path):
    from accvlab import _amd_native as nat

    lib = nat.lib() if path == "lib" else nat.ctypes_lib()
    q = lib.accv_heatmap_peaks_workspace_bytes
    for shape, k in (((64, 1, 1080, 1920), 100), ((4, 10, 180, 180), 500), ((32, 80, 128, 128), 100), ((1, 1, 1, 1), 1),
                     ((1, 1, 37, 53), 7), ((2, 1, 7, 2500), 1024)):
        n = q(*shape, k)
        assert n > 0 and n % 16 == 0, (shape, k, n)
        assert n >= shape[0] * shape[1] * k * 8   # at least k slots of 8 bytes per plane
    # refused sizes report 0
    for shape, k in (((0, 1, 8, 8), 1), ((1, 0, 8, 8), 1), ((1, 1, -8, 8), 1), ((1, 1, 8, 8), 0), ((1, 1, 8, 8), 1025),
                     ((1, 1, 65536, 65536), 1)):
        assert q(*shape, k) == 0, (shape, k)


def test_heatmap_peaks_is_exported():
    import accvlab.draw_heatmap as dh
    from accvlab.draw_heatmap.peaks import HeatmapPeaks, heatmap_peaks

    assert "heatmap_peaks" in dh.__all__
    assert dh.heatmap_peaks is heatmap_peaks
    assert HeatmapPeaks._fields == ("scores", "indices", "classes", "ys", "xs")


def test_heatmap_peaks_refuses_cpu_tensors():
    from accvlab.draw_heatmap import heatmap_peaks

    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="CUDA"):
            heatmap_peaks(torch.zeros(2, 8, 8, dtype=dtype), 4)
        with pytest.raises(RuntimeError, match="CUDA"):
            heatmap_peaks(torch.zeros(2, 3, 8, 8, dtype=dtype), 4, per_class=True)


def test_heatmap_peaks_refuses_non_tensors():
    from accvlab.draw_heatmap import heatmap_peaks

    with pytest.raises(RuntimeError, match="tensor"):
        heatmap_peaks([[0.0, 1.0]], 1)
