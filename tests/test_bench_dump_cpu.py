"""bench.dump_outputs on host tensors: per-Gaussian arrays larger than the row budget are cut to one fixed, seeded sample of
rows shared by every array, written next to them; the total stays within 64 MB."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _engine(P, seed):
    g = torch.Generator().manual_seed(seed)
    grads = {k: torch.rand(P, n, generator=g) for k, n in (("means3D", 3), ("scales", 3), ("rotations", 4), ("opacity", 1),
                                                            ("colors", 3))}
    return SimpleNamespace(P_active=P, out_color=torch.rand(3, 48, 64, generator=g), radii=torch.randint(0, 9, (P,), generator=g,
                           dtype=torch.int32), dL_dmean2D=torch.rand(P, 3, generator=g), grads=grads)


def test_large_outputs_are_sampled_by_fixed_rows(tmp_path):
    P, rows = 5000, 1024
    eng = _engine(P, 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "raster", eng, None, None, rows=rows)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert set(a) == {"image", "radii", "dL_dmean2D", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcolors",
                      "gaussian_rows"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["gaussian_rows"].astype(np.int64)
    assert a["gaussian_rows"].dtype == np.float64 and len(idx) == rows and np.all(np.diff(idx) > 0) and idx[-1] < P
    assert np.array_equal(a["image"], eng.out_color.numpy())
    assert np.array_equal(a["dL_drotations"], eng.grads["rotations"].numpy()[idx])
    assert a["radii"].dtype == np.float32 and np.array_equal(a["radii"], eng.radii.numpy()[idx].astype(np.float32))


def test_small_outputs_are_written_whole_with_the_loss(tmp_path):
    P = 300
    eng = _engine(P, 2)
    params = {k: v + 1 for k, v in eng.grads.items()}
    tstep = SimpleNamespace(engine=eng, params=params, P=P)
    bench.dump_outputs(str(tmp_path), "trainer", eng, tstep, torch.tensor(0.25))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"image", "loss", "means3D", "scales", "rotations", "opacity", "colors"}
    assert got["loss"].tolist() == [0.25] and np.array_equal(got["colors"], params["colors"].numpy())
