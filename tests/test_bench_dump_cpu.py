"""bench.py's output dump and argument checks, on the host: the dump stays under 64 MB in float32 / float64, takes the
same seeded positions on every run and holds the values of the maps it was given."""
import sys

import numpy as np
import pytest
import torch

import bench


def _dump(path, hm):
    bench.dump_outputs(str(path), hm)
    return {f.name: np.load(f) for f in path.iterdir()}, sum(f.stat().st_size for f in path.iterdir())


def test_dump_samples_fixed_positions_of_a_large_batch(tmp_path):
    g = torch.Generator().manual_seed(3)
    hm = torch.rand((8, 1080, 1920), generator=g)
    a, size = _dump(tmp_path / "a", hm)
    b, _ = _dump(tmp_path / "b", hm.clone())
    assert size <= 64 << 20 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[n], b[n]) for n in a)
    pos = a["heatmap_sample_positions.npy"].astype(np.int64)
    assert pos.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(pos) >= 0) and 0 <= pos[0] and pos[-1] < hm.numel()
    assert np.array_equal(a["heatmap_sample.npy"], hm.reshape(-1).numpy()[pos])
    assert np.array_equal(a["heatmap_frame0.npy"], hm[0].numpy())
    np.testing.assert_allclose(a["heatmap_frame_sums.npy"], hm.double().sum(dim=(1, 2)).numpy(), rtol=1e-12)


def test_dump_takes_every_position_of_a_small_batch(tmp_path):
    hm = torch.arange(2 * 30 * 40, dtype=torch.float32).reshape(2, 30, 40)
    a, _ = _dump(tmp_path, hm)
    assert np.array_equal(a["heatmap_sample_positions.npy"], np.arange(hm.numel(), dtype=np.float64))
    assert np.array_equal(a["heatmap_sample.npy"], hm.reshape(-1).numpy())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--batch", "0"]])
def test_bench_rejects_step_counts_it_cannot_time(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
