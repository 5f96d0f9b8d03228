"""bench.py --dump-outputs: the .npy writer (float32 / float64 only, a fixed seeded sample of a large array, the same
elements on every run)."""
import numpy as np
import torch

import bench


def test_dump_outputs_dtypes_sample_and_repeatability(tmp_path):
    g = torch.Generator().manual_seed(3)
    big = torch.randn(3, bench.DUMP_SAMPLE, generator=g)
    arrays = {"loss": torch.tensor([1.5]), "preds": torch.arange(5), "half": torch.ones(4, dtype=torch.bfloat16),
              "dbl": torch.ones(2, dtype=torch.float64), "big.weight": big}
    bench.dump_outputs(tmp_path / "a", arrays)
    bench.dump_outputs(tmp_path / "b", arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(arrays)
    assert got["loss"].dtype == np.float32 and got["half"].dtype == np.float32
    assert got["preds"].dtype == np.float64 and got["dbl"].dtype == np.float64
    assert np.array_equal(got["preds"], np.arange(5.0))
    assert got["big.weight"].shape == (bench.DUMP_SAMPLE,)
    flat = big.reshape(-1).numpy()
    assert np.isin(got["big.weight"], flat).all() and not np.array_equal(got["big.weight"], flat[:bench.DUMP_SAMPLE])
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy")), name
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
