"""bench.py's ``--dump-outputs`` writer and its ``--full`` switch (no GPU)."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_every_tensor_as_float(tmp_path):
    out = {"d_losses": torch.arange(5, dtype=torch.float32) * 0.5, "g_loss": torch.tensor(1.25),
           "label_hard": torch.eye(7, dtype=torch.int64)[torch.tensor([0, 3, 6, 3])],
           "wide": torch.arange(4, dtype=torch.float64) / 3, "note": "not a tensor"}
    d = str(tmp_path / "dump")
    written = bench.dump_outputs(d, out)
    assert sorted(os.listdir(d)) == ["d_losses.npy", "g_loss.npy", "label_hard.npy", "wide.npy"]
    assert written["label_hard"] == [[4, 7], "float32"] and written["wide"] == [[4], "float64"]
    for name in ("d_losses", "g_loss", "label_hard", "wide"):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == (np.float64 if name == "wide" else np.float32)
        assert a.shape == tuple(out[name].shape)
        assert np.array_equal(a, out[name].to(torch.float64).numpy().astype(a.dtype))


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 400)  # 400 bytes per array: 100 floats
    big = torch.arange(1000, dtype=torch.float32).reshape(50, 20)
    small = torch.ones(3)
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a_dir, {"big": big, "small": small})
    bench.dump_outputs(b_dir, {"big": big + 0.0, "small": small})
    a, b = np.load(os.path.join(a_dir, "big.npy")), np.load(os.path.join(b_dir, "big.npy"))
    assert a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(range(1000))  # distinct elements, in flat order
    assert np.load(os.path.join(a_dir, "small.npy")).shape == (3,)
    total = sum(os.path.getsize(os.path.join(a_dir, f)) - 128 for f in os.listdir(a_dir))
    assert total <= 2 * 400
