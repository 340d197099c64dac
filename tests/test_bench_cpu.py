"""CPU: what `bench.py --dump-outputs` writes — the arrays of a train step by name, within the byte budget, with the same
sample of a large array on every run."""
from types import SimpleNamespace

import numpy as np
import torch

import bench


def test_step_outputs_names_what_the_step_returns():
    lin = torch.nn.Linear(3, 2)
    loss = lin(torch.ones(1, 3)).sum()
    loss.backward()
    out = SimpleNamespace(elbo=torch.zeros(4, dtype=torch.float64), z=[torch.ones(2, 2), torch.zeros(1)], z_sl=torch.ones(2, dtype=torch.int32),
                          _lazy={"reconstructions": None})  # fmt: skip
    metrics = [SimpleNamespace(name="kl (bpt)", value=1.5), SimpleNamespace(name="bpd", value=2.0)]
    a = bench.step_outputs(lin, {"loss": loss, "metrics": metrics, "out": out})
    assert sorted(a) == ["grad.bias", "grad.weight", "loss", "metric.bpd", "metric.kl_bpt", "out.elbo", "out.z.0", "out.z.1",
                         "param.bias", "param.weight"]  # fmt: skip
    assert a["out.elbo"].dtype == np.float64 and a["param.weight"].dtype == np.float32
    np.testing.assert_array_equal(a["grad.weight"], lin.weight.grad.numpy())


def test_dump_outputs_fits_the_budget_and_samples_the_same_elements(tmp_path):
    rng = np.random.default_rng(1)
    big = rng.standard_normal((500, 300)).astype(np.float32)
    arrays = {"small": rng.standard_normal(10), "half": np.ones((3, 4), np.float16), "scalar": np.float64(2.5), "big": big}
    limit = 200_000
    w1 = bench.dump_outputs(tmp_path / "a", arrays, limit=limit)
    w2 = bench.dump_outputs(tmp_path / "b", arrays, limit=limit)
    assert w1 == w2
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= limit
    for name in ("small", "half", "scalar"):  # within their share: written whole, float64 kept, anything else as float32
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == (np.float64 if np.asarray(arrays[name]).dtype == np.float64 else np.float32)
        np.testing.assert_array_equal(got, arrays[name])
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert w1["big"][1] == big.size and 0 < w1["big"][0] == a.size < big.size
    np.testing.assert_array_equal(a, b)
    assert np.isin(a, big).all()
