"""Best-of-k by the critic's score on the GPU.

* T1 vg_critic_embed_labels is exact: one f32 add and a max per element.
* T2 vg_sweep_select_score: f64 means within 1e-12 max(1, max|scores|) (an f64
  sum of fewer than 2^11 f32 values; the bound test_select_sweep_gpu.py uses
  for its f64 figures), first arg-max, gather, ties to the lower index, and
  the same bits on a second launch.
* T3 VoxelGNNDiscriminator.score_labels against k separate D(loc, vox, onehot)
  forwards in eval mode: rtol 1e-3, atol 1e-4, the project's stacked-versus-
  separate bound (tests/test_models_gpu.py).
* T4 the per-building means against the f64 CPU oracle: within 4 e0, e0 being
  the error of the separate GPU forwards (the factor covers the other
  summation order of the first layer and of the stacked GraphNorm partials);
  the chosen candidate equals the oracle's wherever the oracle's top-two gap
  exceeds 10 x that bound.
* T5 InferenceSweep(..., critic=D) with select="critic", end to end.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from parity_util import batches_from_items
from vgan import ops
from vgan.config import Configuration
from vgan.infer import InferenceSweep, geometric_taus
from vgan.loader import GraphLoader
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
from vgan.rng import RNG
from vgan.store import write_store
from vgan.synth import SyntheticDataset, make_building

pytestmark = pytest.mark.gpu

K = 7
F = 29  # matched (17) + voxel.x (12) columns in front of the label columns


# ------------------------------------------------------------------ T1
@pytest.mark.parametrize("n,h,classes,k", [(1, 64, 7, 1), (67, 20, 5, 3), (1030, 64, 7, 9), (300, 256, 32, 2),
                                           (67, 21, 5, 3)])  # the last: H % 4 != 0, the scalar form
def test_embed_labels_is_exact(cuda, n, h, classes, k):
    g = torch.Generator().manual_seed(n + h)
    W = torch.randn(h, F + classes, generator=g).to(cuda)
    base_c = torch.randn(n, h, generator=g).to(cuda)
    pred_c = torch.randint(0, classes, (k, n), generator=g).to(torch.int8).to(cuda)

    def want(base, pred):
        p = pred.long()
        add = W[:, F + p.clamp(min=0)].permute(1, 2, 0)  # [k, n, h]
        add = torch.where((p >= 0).unsqueeze(-1), add, torch.zeros_like(add))
        return torch.relu(base.unsqueeze(0) + add).reshape(k * n, h)

    y = ops.critic_embed_labels(base_c, W, F, pred_c)
    assert y.shape == (k * n, h) and torch.equal(y, want(base_c, pred_c))
    assert torch.equal(y, torch.cat([torch.relu(base_c + W[:, F + pred_c[c].long()].T) for c in range(k)]))
    # views: row strides H + 4 and N + 3 (a candidate row then starts at any byte)
    bbuf = torch.zeros(n, h + 4, device=cuda)
    pbuf = torch.zeros(k, n + 3, dtype=torch.int8, device=cuda)
    base_v, pred_v = bbuf[:, :h], pbuf[:, :n]
    base_v.copy_(base_c)
    pred_v.copy_(pred_c)
    assert base_v.stride(0) == h + 4 and pred_v.stride(0) == n + 3
    assert torch.equal(ops.critic_embed_labels(base_v, W, F, pred_v), y)
    # base one float off the 16-byte grid: the scalar form, same values
    base_o = torch.zeros(n, h + 4, device=cuda)[:, 1:h + 1]
    base_o.copy_(base_c)
    assert torch.equal(ops.critic_embed_labels(base_o, W, F, pred_v), y)
    # one label outside [0, K): an all-zero one-hot row
    c, v = k - 1, n // 2
    pred_v[c, v] = -1
    y2 = ops.critic_embed_labels(base_v, W, F, pred_v)
    assert torch.equal(y2[c * n + v], torch.relu(base_c[v]))
    assert torch.equal(y2, want(base_c, pred_v))
    pred_v[c, v] = classes  # one past the last class
    assert torch.equal(ops.critic_embed_labels(base_v, W, F, pred_v), y2)


# ------------------------------------------------------------------ T2
SIZES = [1, 63, 64, 257, 1030]


def _select_inputs(cuda, k, seed=0):
    n = sum(SIZES)
    g = torch.Generator().manual_seed(100 + k + seed)
    sbuf = torch.zeros(k, n + 3, device=cuda)
    pbuf = torch.zeros(k, n + 3, dtype=torch.int8, device=cuda)
    scores, pred = sbuf[:, :n], pbuf[:, :n]
    scores.copy_(torch.randn(k, n, generator=g) * 3)
    pred.copy_(torch.randint(0, K, (k, n), generator=g).to(torch.int8))
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64, device=cuda)
    return scores, pred, ptr


def _host_means(scores, ptr):
    s = scores.detach().cpu().numpy().astype(np.float64)
    p = ptr.cpu().numpy()
    return np.stack([s[:, p[g]:p[g + 1]].mean(axis=1) for g in range(len(p) - 1)], axis=1)  # [k, G]


def _check_selection(sel, scores, pred, ptr):
    k, n = pred.shape
    p = ptr.cpu().numpy()
    batch = np.repeat(np.arange(len(p) - 1), np.diff(p))
    score, best, labels = sel.score.cpu().numpy(), sel.best.cpu().numpy(), sel.labels.cpu().numpy()
    assert score.dtype == np.float64 and score.shape == (k, len(p) - 1)
    assert best.dtype == np.int32 and best.shape == (len(p) - 1,) and labels.dtype == np.int8 and labels.shape == (n,)
    bound = 1e-12 * max(1.0, float(scores.abs().max()))
    err = float(np.abs(score - _host_means(scores, ptr)).max())
    print(f"k = {k}: max |score - host f64 mean| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert np.array_equal(best, np.argmax(score, axis=0))
    assert np.array_equal(labels, pred.cpu().numpy()[best[batch], np.arange(n)])


@pytest.mark.parametrize("k", [1, 3, 9])
def test_select_score(cuda, k):
    scores, pred, ptr = _select_inputs(cuda, k)
    assert scores.stride(0) == sum(SIZES) + 3 and pred.stride(0) == sum(SIZES) + 3
    keep_s, keep_p = scores.clone(), pred.clone()
    a = ops.sweep_select_score(scores, pred, ptr)
    b = ops.sweep_select_score(scores, pred, ptr)
    torch.cuda.synchronize()
    assert torch.equal(scores, keep_s) and torch.equal(pred, keep_p)  # inputs untouched
    _check_selection(a, scores, pred, ptr)
    for x, y in zip(a, b):  # no atomics: the same bits
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)
    # contiguous inputs: the same means (the summation order follows the building, not the addresses)
    c = ops.sweep_select_score(scores.contiguous(), pred.contiguous(), ptr)
    assert torch.equal(c.score, a.score) and torch.equal(c.best, a.best) and torch.equal(c.labels, a.labels)
    if k == 1:
        assert int(a.best.abs().max()) == 0 and torch.equal(a.labels, pred[0])
        return
    # two identical candidate rows ahead of all others: the lower index wins
    lo_i, hi_i = 1, k - 1
    scores[lo_i] += 50.0
    scores[hi_i].copy_(scores[lo_i])
    pred[hi_i].copy_(pred[lo_i])
    d = ops.sweep_select_score(scores, pred, ptr)
    _check_selection(d, scores, pred, ptr)
    assert torch.equal(d.score[lo_i], d.score[hi_i]) and bool((d.best == lo_i).all())
    # a NaN never replaces an earlier candidate
    scores[hi_i, ::7] = float("nan")
    e = ops.sweep_select_score(scores, pred, ptr)
    assert bool((e.best == lo_i).all()) and bool(torch.isnan(e.score[hi_i]).all())


def test_select_score_refuses_bad_tensors(cuda):
    scores, pred, ptr = _select_inputs(cuda, 3)
    with pytest.raises(ValueError):
        ops.sweep_select_score(scores.double(), pred, ptr)
    with pytest.raises(ValueError):
        ops.sweep_select_score(scores[:2], pred, ptr)
    with pytest.raises(ValueError):
        ops.sweep_select_score(scores, pred.to(torch.int32), ptr)
    with pytest.raises(ValueError):
        ops.sweep_select_score(scores, pred, ptr.to(torch.int32))
    with pytest.raises(ValueError):
        ops.critic_embed_labels(torch.zeros(5, 8, device=cuda), torch.zeros(8, 40, device=cuda), 2, pred[:, :5])  # K = 38


# ------------------------------------------------------------ T3 / T4
@pytest.fixture(scope="module")
def case():
    """Four buildings (486 / 320 / 504 / 280 voxels) and k = 4 candidate
    labellings: candidate c is the truth with a mask rand(n) < 0.25 c + 0.1
    redrawn by randint(0, K) -- mask then values, in candidate order."""
    items = [make_building(17, i) for i in range(4)]
    truth = torch.cat([v.type for _, v in items])
    n = truth.numel()
    g = torch.Generator().manual_seed(3)
    cands = []
    for c in range(4):
        mask = torch.rand(n, generator=g) < 0.25 * c + 0.1
        vals = torch.randint(0, K, (n,), generator=g)
        cands.append(torch.where(mask, vals, truth))
    pred = torch.stack(cands).to(torch.int8)
    assert [int(v.type.numel()) for _, v in items] == [486, 320, 504, 280]
    return items, pred


def _critic(cuda, wgangp: bool, conv: str, perturbed: bool = False):
    cfg = Configuration()  # default widths: DISCRIMINATOR_HIDDEN_DIM = 64 (a width-2 decoder is dead at init)
    cfg.DEVICE = str(cuda)
    cfg.USE_WGANGP = wgangp
    cfg.DISCRIMINATOR_CONV_TYPE = conv
    assert cfg.DISCRIMINATOR_HIDDEN_DIM == 64
    torch.manual_seed(5)
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    if perturbed:
        with torch.no_grad():
            for p in D.parameters():
                q = p.detach().cpu()
                p.copy_((q + 0.3 * torch.randn(q.shape) * (q.abs().mean() + 0.05)).to(p.device))
    return cfg, D


def _separate(D, loc, vox, pred):
    """The path without score_labels: one D(loc, vox, onehot) per candidate, eval mode."""
    D.eval()
    with torch.no_grad():
        return torch.stack([D(loc, vox, torch.nn.functional.one_hot(pred[c].long(), K).float()).reshape(-1)
                            for c in range(pred.shape[0])])


@pytest.mark.parametrize("wgangp,conv,perturbed", [(True, "GATCONV", False), (False, "GATCONV", False),
                                                   (True, "GATV2CONV", False), (False, "GATV2CONV", False),
                                                   (True, "GATCONV", True)])
def test_score_labels_equals_separate_forwards(cuda, case, wgangp, conv, perturbed):
    items, pred = case
    _, (loc, vox) = batches_from_items(items, cuda)
    _, D = _critic(cuda, wgangp, conv, perturbed)
    pred = pred.to(cuda)
    D.train()
    got = D.score_labels(loc, vox, pred)
    assert D.training and all(m.training for m in D.modules())  # the flag is restored
    assert got.shape == pred.shape and got.dtype == torch.float32
    D.eval()
    assert torch.equal(D.score_labels(loc, vox, pred), got) and not D.training  # eval semantics: no dropout
    want = _separate(D, loc, vox, pred)
    err = float((got - want).abs().max())
    print(f"USE_WGANGP={wgangp} {conv} perturbed={perturbed}: max |stacked - separate| = {err:.3e}, "
          f"max |score| = {float(want.abs().max()):.3e}, spread over candidates {float(want.std(0).mean()):.3e}")
    assert torch.allclose(got, want, rtol=1e-3, atol=1e-4)
    if not wgangp:
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0  # Sigmoid included
    # one candidate: the plain CSR
    one = D.score_labels(loc, vox, pred[2:3])
    assert one.shape == (1, pred.shape[1]) and torch.allclose(one[0], want[2], rtol=1e-3, atol=1e-4)
    # under a bf16 training scope the scores are still the f32 ones
    from vgan._lib import gemm_precision_scope

    with gemm_precision_scope("bf16"):
        assert torch.equal(D.score_labels(loc, vox, pred), got)
    with pytest.raises(ValueError):
        D.score_labels(loc, vox, pred[:, :-1])


@pytest.mark.parametrize("wgangp", [True, False])
def test_score_labels_against_the_oracle(cuda, case, wgangp):
    """Measured on an MI355X, max over the 4 x 4 per-building
    means: WGAN-GP e0 5.3e-9, score_labels + select 6.0e-9 (bound 2.1e-8);
    BCE e0 4.2e-9, new path 2.8e-9 (bound 1.7e-8).  The oracle's top-two gaps
    are 1.9e-4 .. 1.6e-3 (WGAN-GP) and 4.6e-5 .. 4.0e-4 (BCE): every building
    is checked."""
    from oracle import reference as R

    items, pred = case
    (ol, ov), (loc, vox) = batches_from_items(items, cuda)
    cfg, D = _critic(cuda, wgangp, "GATCONV")
    Do = R.Discriminator(cfg).double()
    Do.load_state_dict({k: v.detach().cpu().double() for k, v in D.state_dict().items()})
    Do.eval()
    ol.x, ov.x = ol.x.double(), ov.x.double()
    with torch.no_grad():
        ref = torch.stack([Do(ol, ov, torch.nn.functional.one_hot(pred[c].long(), K).double()).reshape(-1)
                           for c in range(pred.shape[0])])
    ptr = vox.ptr
    ref_means = _host_means(ref, ptr)
    e0 = float(np.abs(_host_means(_separate(D, loc, vox, pred.to(cuda)), ptr) - ref_means).max())
    scores = D.score_labels(loc, vox, pred.to(cuda))
    sel = ops.sweep_select_score(scores, pred.to(cuda), ptr)
    e1 = float(np.abs(sel.score.cpu().numpy() - ref_means).max())
    bound = 4 * e0
    top = np.sort(ref_means, axis=0)
    gaps = top[-1] - top[-2]
    print(f"USE_WGANGP={wgangp}: separate GPU forwards vs f64 oracle e0 = {e0:.3e}; score_labels + select = {e1:.3e} "
          f"(bound 4 e0 = {bound:.3e}); oracle top-two gaps {[f'{x:.2e}' for x in gaps]}")
    assert e1 <= bound
    checked = gaps > 10 * bound
    assert int((~checked).sum()) <= 1, gaps
    best = sel.best.cpu().numpy()
    assert np.array_equal(best[checked], np.argmax(ref_means, axis=0)[checked])
    _check_selection(sel, scores, pred.to(cuda), ptr)


# ------------------------------------------------------------------ T5
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return write_store(str(tmp_path_factory.mktemp("critic_select") / "s"), SyntheticDataset(11, seed=17))


def _sweep_setup(cuda, store):
    cfg = Configuration()
    cfg.DEVICE = str(cuda)
    torch.manual_seed(5)
    G = VoxelGNNGenerator(cfg, 17, 12).to(cuda)
    D = VoxelGNNDiscriminator(cfg, 17, 12).to(cuda)

    def loader():
        return GraphLoader(store, list(range(len(store))), batch_size=4, shuffle=False, device=cuda, prefetch=2,
                           prepare=(K, ()))

    return G, D, loader


def _check_batch(D, pred, sel, loc, vox):
    """One batch: pred [k, N] int8 (host), sel the dict of host copies."""
    assert sorted(sel) == ["best", "labels", "score"]
    ptr = vox.ptr.cpu().numpy()
    k, n = pred.shape
    g = len(ptr) - 1
    batch = np.repeat(np.arange(g), np.diff(ptr))
    labels, best, score = sel["labels"].numpy(), sel["best"].numpy(), sel["score"].numpy()
    assert labels.dtype == np.int8 and labels.shape == (n,) and best.shape == (g,)
    assert score.dtype == np.float64 and score.shape == (k, g)
    assert np.array_equal(labels, pred.numpy()[best[batch], np.arange(n)])
    assert np.array_equal(best, np.argmax(score, axis=0))
    s = D.score_labels(loc, vox, pred.to(vox.x.device))
    err = float(np.abs(score - _host_means(s, vox.ptr)).max())
    bound = 1e-12 * max(1.0, float(s.abs().max()))
    print(f"{g} buildings: max |score - host mean of score_labels| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_stream_select_critic(cuda, store, dtype):
    G, D, loader = _sweep_setup(cuda, store)
    taus = geometric_taus(1.0, 0.1, 3)
    D.train()
    G.rng = RNG("device", seed=99)
    sw = InferenceSweep(G, taus, dtype=dtype, critic=D)
    res = sw.run_stream(loader(), collect=True, select="critic")
    torch.cuda.synchronize()
    assert D.training
    G.rng = RNG("device", seed=99)
    ref = InferenceSweep(G, taus, dtype=dtype).run_stream(loader(), collect=True)
    torch.cuda.synchronize()
    assert "selected" not in ref and res["batches"] == 3 and res["graphs"] == 11 and res["samples"] == 33
    assert len(res["predictions"]) == len(ref["predictions"]) == len(res["selected"]) == 3
    for a, b in zip(res["predictions"], ref["predictions"]):
        assert a.dtype == torch.int8 and a.shape == b.shape and torch.equal(a, b)
    for pred, sel, (loc, vox) in zip(res["predictions"], res["selected"], list(loader())):
        _check_batch(D, pred, sel, loc, vox)
    # the hand-written criteria on the same sweep keep their five keys
    G.rng = RNG("device", seed=99)
    f1 = sw.run_stream(loader(), collect=True, select="f1")
    for a, b, sel in zip(f1["predictions"], ref["predictions"], f1["selected"]):
        assert torch.equal(a, b) and sorted(sel) == ["best", "f1", "far_gen", "far_ref", "labels"]
    with pytest.raises(ValueError, match="select"):
        sw.run_stream(loader(), select="iou")
    with pytest.raises(ValueError, match="critic"):
        InferenceSweep(G, taus, dtype=dtype).run_stream(loader(), select="critic")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_graphed_run_select_critic(cuda, store, dtype):
    """run(..., select="critic") over resident batches replayed from captured
    graphs, twice: the scoring is launched eagerly after each replay."""
    G, D, loader = _sweep_setup(cuda, store)
    taus = geometric_taus(1.0, 0.1, 3)
    batches = list(loader())
    G.rng = RNG("device", seed=7)
    sw = InferenceSweep(G, taus, graphed=True, dtype=dtype, critic=D)
    sw.run(batches)  # captures
    got = [sw.run(batches, collect=True, select="critic") for _ in range(2)]  # replays
    torch.cuda.synchronize()
    G.rng = RNG("device", seed=7)
    sw2 = InferenceSweep(G, taus, graphed=True, dtype=dtype)
    sw2.run(batches)
    want = [sw2.run(batches, collect=True) for _ in range(2)]
    torch.cuda.synchronize()
    for res, ref in zip(got, want):
        assert "selected" not in ref and len(res["selected"]) == 3
        for a, b in zip(res["predictions"], ref["predictions"]):
            assert torch.equal(a, b)
        for pred, sel, (loc, vox) in zip(res["predictions"], res["selected"], batches):
            _check_batch(D, pred, sel, loc, vox)
    far = sw.run(batches, collect=True, select="far")
    assert all(sorted(s) == ["best", "f1", "far_gen", "far_ref", "labels"] for s in far["selected"])


def test_select_method_returns_device_tensors(cuda, store):
    G, D, loader = _sweep_setup(cuda, store)
    G.rng = RNG("device", seed=3)
    sw = InferenceSweep(G, geometric_taus(1.0, 0.1, 3), critic=D)
    loc, vox = next(iter(loader()))
    pred = sw.run_batch(loc, vox)
    keep = pred.clone()
    ctr = G.rng._iter(vox.x.device).clone()
    sel = sw.select(pred, loc, vox, "critic")
    assert isinstance(sel, ops.CriticSelection) and all(t.is_cuda for t in sel) and torch.equal(pred, keep)
    assert torch.equal(G.rng._iter(vox.x.device), ctr)  # scoring leaves the generator's counter alone
    want = ops.sweep_select_score(D.score_labels(loc, vox, pred), pred, vox.ptr)
    for a, b in zip(sel, want):
        assert torch.equal(a, b)
