"""Best-of-k selection inside the inference sweep (InferenceSweep.run /
run_stream with ``select=``), end to end on the three forward paths: f32, f16
launched from Python and f16 as one native call.  A store of 11 synthetic
buildings in batches of 4, three temperatures, device RNG with a fixed seed.

* The predictions with ``select`` equal, bit for bit, those of the same call
  without it from the same RNG state: the selection launch changes nothing.
* Each batch's selected labels are the host gather of its predictions at the
  returned ``best``; ``best`` is the first arg-max of the returned f1 (first
  arg-min of |far_gen - far_ref| under "far").
* f1 against metrics.macro_f1 of a host confusion count: 1e-12 (counts exact,
  <= 2K + 1 roundings on values <= 1 in f64).
"""
import numpy as np
import pytest
import torch

from vgan import metrics
from vgan.config import Configuration
from vgan.infer import InferenceSweep, geometric_taus
from vgan.loader import GraphLoader
from vgan.models import VoxelGNNGenerator
from vgan.rng import RNG
from vgan.store import write_store
from vgan.synth import SyntheticDataset

pytestmark = pytest.mark.gpu

K = 7
PATHS = {"f32": ("f32", True), "f16": ("f16", True), "f16-python": ("f16", False)}


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return write_store(str(tmp_path_factory.mktemp("select") / "s"), SyntheticDataset(11, seed=17))


def _setup(cuda, store, path, monkeypatch):
    from vgan import infer

    dtype, native = PATHS[path]
    monkeypatch.setattr(infer, "_NATIVE", native)
    cfg = Configuration()
    cfg.DEVICE = str(cuda)
    torch.manual_seed(5)
    G = VoxelGNNGenerator(cfg, 17, 12).to(cuda)

    def loader():
        return GraphLoader(store, list(range(len(store))), batch_size=4, shuffle=False, device=cuda, prefetch=2,
                           prepare=(K, ()))

    return G, dtype, loader


def _check_batch(pred, sel, ptr, truth, criterion):
    """One batch: pred [k, N] int8 (host), sel the dict of host copies."""
    pred, ptr, truth = pred.numpy(), ptr.numpy(), truth.numpy()
    k, n = pred.shape
    g = len(ptr) - 1
    batch = np.repeat(np.arange(g), np.diff(ptr))
    labels, best, f1 = sel["labels"].numpy(), sel["best"].numpy(), sel["f1"].numpy()
    far_gen, far_ref = sel["far_gen"].numpy(), sel["far_ref"].numpy()
    assert labels.dtype == np.int8 and labels.shape == (n,) and best.shape == (g,)
    assert f1.dtype == np.float64 and f1.shape == (k, g) and far_gen.shape == (k, g) and far_ref.shape == (g,)
    assert np.array_equal(labels, pred[best[batch], np.arange(n)])
    conf = np.stack([np.bincount((batch * K + truth) * K + pred[c], minlength=g * K * K).reshape(g, K, K)
                     for c in range(k)])
    err = np.abs(f1 - metrics.macro_f1(conf)).max()
    print(f"{criterion}: {g} buildings, max |f1 - macro_f1| = {err:.3e}")
    assert err <= 1e-12
    if criterion == "f1":
        assert np.array_equal(best, np.argmax(f1, axis=0))
    else:
        assert np.array_equal(best, np.argmin(np.abs(far_gen - far_ref[None, :]), axis=0))
    assert np.all(np.isfinite(far_gen)) and np.all(far_gen >= 0) and np.all(far_ref > 0)


@pytest.mark.parametrize("path", list(PATHS))
def test_stream_select_f1(cuda, store, path, monkeypatch):
    G, dtype, loader = _setup(cuda, store, path, monkeypatch)
    taus = geometric_taus(1.0, 0.1, 3)
    G.rng = RNG("device", seed=99)
    res = InferenceSweep(G, taus, dtype=dtype).run_stream(loader(), collect=True, select="f1")
    torch.cuda.synchronize()
    G.rng = RNG("device", seed=99)
    ref = InferenceSweep(G, taus, dtype=dtype).run_stream(loader(), collect=True)
    torch.cuda.synchronize()
    assert "selected" not in ref and sorted(ref) == ["batches", "graphs", "predictions", "samples"]
    assert res["batches"] == 3 and res["graphs"] == 11 and res["samples"] == 33
    assert len(res["predictions"]) == len(ref["predictions"]) == len(res["selected"]) == 3
    for a, b in zip(res["predictions"], ref["predictions"]):
        assert a.dtype == torch.int8 and a.shape == b.shape and torch.equal(a, b)
    truths = [(vox.ptr.cpu(), vox.type.cpu()) for _, vox in loader()]
    for pred, sel, (ptr, truth) in zip(res["predictions"], res["selected"], truths):
        assert sorted(sel) == ["best", "f1", "far_gen", "far_ref", "labels"]
        _check_batch(pred, sel, ptr, truth, "f1")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_graphed_run_select_far(cuda, store, dtype, monkeypatch):
    """run(..., select="far") over resident batches replayed from captured
    graphs: the selection is an ordinary launch after each replay."""
    G, dtype, loader = _setup(cuda, store, dtype, monkeypatch)
    taus = geometric_taus(1.0, 0.1, 3)
    batches = list(loader())
    G.rng = RNG("device", seed=7)
    sw = InferenceSweep(G, taus, graphed=True, dtype=dtype)
    sw.run(batches)  # captures
    res = sw.run(batches, collect=True, select="far")  # replays
    torch.cuda.synchronize()
    G.rng = RNG("device", seed=7)
    sw2 = InferenceSweep(G, taus, graphed=True, dtype=dtype)
    sw2.run(batches)
    ref = sw2.run(batches, collect=True)
    torch.cuda.synchronize()
    assert "selected" not in ref and len(res["selected"]) == 3
    for a, b in zip(res["predictions"], ref["predictions"]):
        assert torch.equal(a, b)
    for pred, sel, (_, vox) in zip(res["predictions"], res["selected"], batches):
        _check_batch(pred, sel, vox.ptr.cpu(), vox.type.cpu(), "far")


def test_select_method_on_one_batch(cuda, store, monkeypatch):
    """InferenceSweep.select on a run_batch result: device tensors, the
    candidates untouched, equal to ops.sweep_select on the batch's arrays."""
    from vgan import data as vdata, ops

    G, dtype, loader = _setup(cuda, store, "f32", monkeypatch)
    G.rng = RNG("device", seed=3)
    sw = InferenceSweep(G, geometric_taus(1.0, 0.1, 3), dtype=dtype)
    loc, vox = next(iter(loader()))
    pred = sw.run_batch(loc, vox)
    keep = pred.clone()
    sel = sw.select(pred, loc, vox, "f1")
    assert sel.labels.is_cuda and sel.conf.shape == (3, vox.num_graphs, K, K) and torch.equal(pred, keep)
    want = ops.sweep_select(pred, vox.ptr, vdata.prepared(loc, vox, K).voxel_x, vox.site_area, truth=vox.type)
    for a, b in zip(sel, want):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="select"):
        sw.run([(loc, vox)], select="iou")
