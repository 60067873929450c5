"""bench.py --dump-outputs: what ``dump_outputs`` writes for one pipeline result (no GPU needed: it takes any tensors)."""
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_types_names_and_sampling(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMENTS", 1000)
    g = torch.Generator().manual_seed(3)
    big = torch.randn(4, 3000, generator=g)
    out = {"score": torch.rand(2, 50, generator=g), "all_feature": big, "center_pc_index": torch.arange(7),
           "final_mask": torch.tensor([True, False, True]), "keep_per_scene": (torch.ones(2), None),
           "valid_crops": 12, "done": object(), "grasp64": torch.zeros(3, dtype=torch.float64)}
    shapes = bench.dump_outputs(out, str(tmp_path / "a"))
    assert shapes == {"score": [2, 50], "all_feature": [4, 3000], "center_pc_index": [7], "final_mask": [3],
                      "keep_per_scene_0": [2], "grasp64": [3]}
    files = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(files) == sorted(n + ".npy" for n in shapes)
    assert files["score.npy"].dtype == np.float32 and files["grasp64.npy"].dtype == np.float64
    assert files["center_pc_index.npy"].dtype == np.float64 and np.array_equal(files["center_pc_index.npy"], np.arange(7))
    assert np.array_equal(files["final_mask.npy"], [1.0, 0.0, 1.0])
    np.testing.assert_array_equal(files["score.npy"], out["score"].numpy())
    # the large output: a flat sample at seeded, sorted indices that depend on its size only
    idx = np.sort(np.random.default_rng(0).integers(0, big.numel(), 1000))
    np.testing.assert_array_equal(files["all_feature.npy"], big.numpy().reshape(-1)[idx])
    bench.dump_outputs({"all_feature": big}, str(tmp_path / "b"))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "all_feature.npy"), files["all_feature.npy"])


def test_dump_outputs_refuses_more_than_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1000)
    try:
        bench.dump_outputs({"a": torch.zeros(200), "b": torch.zeros(200)}, str(tmp_path))
    except SystemExit as exc:
        assert "exceed" in str(exc)
    else:
        raise AssertionError("a dump over the budget must fail")
