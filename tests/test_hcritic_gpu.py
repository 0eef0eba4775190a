"""The f16 critic scorer on the GPU.

* T1 vg_hcritic_embed_labels is exact: an f32 add, a max and ONE rounding to
  f16 per element; zero pad columns.
* T2 vg_hcritic_decode against torch in f32 on the same f16-rounded rows with
  the same f32 parameters (summation order is the only difference): the bound
  of tests/test_chain_gpu.py, 1e-5 max(1, max |y|).  Other widths are refused
  by the kernel entry, and a critic with such a decoder takes the per-layer
  path under T4's bound.
* T3 the native call (vg_hcritic_score) equals the same launches issued from
  Python bit for bit, the select tail included.
* T4 per-building means against the f64 CPU oracle within 4 e_emu, e_emu the
  error of an f16 emulation of the oracle itself (below).
* T5 InferenceSweep(..., critic=D, critic_dtype="f16") end to end.
* T6 refresh().  T7 capture.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from parity_util import batches_from_items
from vgan import ops
from vgan._lib import LIB, VG_EINVAL, ptr, stream_handle
from vgan.config import Configuration
from vgan.half import HalfCritic
from vgan.infer import InferenceSweep, geometric_taus
from vgan.loader import GraphLoader
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
from vgan.nn import MLP, Linear
from vgan.rng import RNG
from vgan.store import write_store
from vgan.synth import SyntheticDataset, make_building

pytestmark = pytest.mark.gpu

K = 7
F = 29  # matched (17) + voxel.x (12) columns in front of the label columns


def _r8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------ T1
def _embed(base, W, col0, pred, h):
    k, n = pred.shape
    ldy = _r8(h)
    y = torch.full((k * n, ldy), float("nan"), dtype=torch.float16, device=base.device)
    rc = LIB.vg_hcritic_embed_labels(ptr(base), base.stride(0) if n > 1 else h, ptr(W), W.stride(0), col0,
                                     W.shape[1] - col0, ptr(pred), pred.stride(0) if k > 1 else n, k, n, h, ptr(y),
                                     ldy, stream_handle(base.device))
    assert rc == 0, rc
    return y


@pytest.mark.parametrize("n,h,classes,k", [(1, 64, 7, 1), (67, 20, 5, 3), (1030, 64, 7, 9), (300, 256, 32, 2)])
def test_embed_labels_is_exact(cuda, n, h, classes, k):
    g = torch.Generator().manual_seed(n + h)
    W = torch.randn(h, F + classes, generator=g).to(cuda)
    base_c = torch.randn(n, h, generator=g).to(cuda)
    pred_c = torch.randint(0, classes, (k, n), generator=g).to(torch.int8).to(cuda)

    def want(pred):
        p = pred.long()
        add = W[:, F + p.clamp(0, classes - 1)].permute(1, 2, 0)  # [k, n, h]
        add = torch.where(((p >= 0) & (p < classes)).unsqueeze(-1), add, torch.zeros_like(add))
        return torch.relu(base_c.unsqueeze(0) + add).reshape(k * n, h).half()

    y = _embed(base_c, W, F, pred_c, h)
    assert torch.equal(y[:, :h], want(pred_c))
    assert torch.equal(y[:, :h], torch.cat([torch.relu(base_c + W[:, F + pred_c[c].long()].T).half() for c in range(k)]))
    assert y.shape[1] == _r8(h) and bool((y[:, h:] == 0).all())  # the pad columns are written, as zeros
    # views: row strides H + 4 and N + 3 (a candidate row then starts at any byte)
    bbuf = torch.zeros(n, h + 4, device=cuda)
    pbuf = torch.zeros(k, n + 3, dtype=torch.int8, device=cuda)
    base_v, pred_v = bbuf[:, :h], pbuf[:, :n]
    base_v.copy_(base_c)
    pred_v.copy_(pred_c)
    assert base_v.stride(0) == h + 4 and pred_v.stride(0) == n + 3
    assert torch.equal(_embed(base_v, W, F, pred_v, h), y)
    # base one float off the 16-byte grid: single-float loads, the same bits
    base_o = torch.zeros(n, h + 4, device=cuda)[:, 1:h + 1]
    base_o.copy_(base_c)
    assert base_o.data_ptr() % 16 == 4
    assert torch.equal(_embed(base_o, W, F, pred_v, h), y)
    # a row stride that is no multiple of 4 floats: the same
    base_s = torch.zeros(n, h + 3, device=cuda)[:, :h]
    base_s.copy_(base_c)
    assert torch.equal(_embed(base_s, W, F, pred_v, h), y)
    # labels -1 and K: an all-zero one-hot row
    c, v = k - 1, n // 2
    pred_v[c, v] = -1
    y2 = _embed(base_v, W, F, pred_v, h)
    assert torch.equal(y2[c * n + v, :h], torch.relu(base_c[v]).half())
    assert torch.equal(y2[:, :h], want(pred_v)) and bool((y2[:, h:] == 0).all())
    pred_v[c, v] = classes
    assert torch.equal(_embed(base_v, W, F, pred_v, h), y2)


# ------------------------------------------------------------------ T2
def _decode(x16, ld, widths, Ws, bs, sigmoid):
    rows = x16.shape[0]
    out = torch.full((rows,), float("nan"), device=x16.device)
    nl = len(Ws)
    wd = (ctypes.c_int32 * (nl + 1))(*widths)
    wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in Ws])
    bp = (ctypes.c_void_p * nl)(*[b.data_ptr() for b in bs])
    rc = LIB.vg_hcritic_decode(ptr(x16), ld, rows, wd, nl, wp, bp, int(sigmoid), ptr(out), stream_handle(x16.device))
    return rc, out


def _decoder_params(cuda, widths, g):
    Ws = [(torch.randn(b, a, device=cuda, generator=g) / a ** 0.5).contiguous() for a, b in zip(widths, widths[1:])]
    bs = [torch.randn(b, device=cuda, generator=g) for b in widths[1:]]
    return Ws, bs


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("h", [16, 64, 128])
@pytest.mark.parametrize("rows", [1, 63, 1030])
def test_decode_matches_torch_f32(cuda, rows, h, sigmoid):
    g = torch.Generator(device=cuda).manual_seed(rows + h)
    widths = [h, h // 2, h // 4, h // 8, 1]
    Ws, bs = _decoder_params(cuda, widths, g)
    ld = h + 8  # rows inside a wider buffer
    buf = torch.randn(rows, ld, device=cuda, generator=g).half()
    rc, out = _decode(buf, ld, widths, Ws, bs, sigmoid)
    assert rc == 0
    y = buf[:, :h].float()
    for i, (W, b) in enumerate(zip(Ws, bs)):
        y = torch.nn.functional.linear(y, W, b)
        if i < 3:
            y = torch.relu(y)
    if sigmoid:
        y = torch.sigmoid(y)
    y = y.reshape(-1)
    err = float((out - y).abs().max())
    bound = 1e-5 * max(1.0, float(y.abs().max()))
    print(f"rows {rows} H {h} sigmoid {sigmoid}: max |decode - torch f32| = {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(out).all() and err <= bound


def test_decode_refuses_other_widths(cuda):
    g = torch.Generator(device=cuda).manual_seed(1)
    for widths in ([24, 12, 6, 3, 1], [64, 32, 16, 8], [64, 24, 12, 6, 1], [256, 128, 64, 32, 1]):
        Ws, bs = _decoder_params(cuda, widths, g)
        x = torch.randn(10, _r8(widths[0]), device=cuda, generator=g).half()
        rc, out = _decode(x, x.shape[1], widths, Ws, bs, False)
        torch.cuda.synchronize()
        assert rc == VG_EINVAL and bool(torch.isnan(out).all())  # refused before any launch


# ------------------------------------------------------------ T3 / T4
@pytest.fixture(scope="module")
def case():
    """tests/test_critic_select_gpu.py's case: four buildings (486 / 320 / 504
    / 280 voxels) and k = 4 candidate labellings: candidate c is the truth
    with a mask rand(n) < 0.25 c + 0.1 redrawn by randint(0, K) -- mask then
    values, in candidate order."""
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


def _critic(device, wgangp: bool, perturbed: bool = False, odd_decoder: bool = False):
    cfg = Configuration()  # default widths: DISCRIMINATOR_HIDDEN_DIM = 64
    cfg.DEVICE = str(device)
    cfg.USE_WGANGP = wgangp
    assert cfg.DISCRIMINATOR_HIDDEN_DIM == 64
    torch.manual_seed(5)
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    if odd_decoder:  # 64 -> 24 -> 12 -> 6 -> 1: no vg_hcritic_decode kernel
        mods = []
        for a, b in ((64, 24), (24, 12), (12, 6)):
            mods += [Linear(a, b), torch.nn.ReLU(True)]
        mods.append(Linear(6, 1))
        if not wgangp:
            mods.append(torch.nn.Sigmoid())
        D.decoder = MLP(*mods).to(device)
    if perturbed:
        with torch.no_grad():
            for p in D.parameters():
                q = p.detach().cpu()
                p.copy_((q + 0.3 * torch.randn(q.shape) * (q.abs().mean() + 0.05)).to(p.device))
    return cfg, D


def _host_means(scores, ptr_):
    s = scores.detach().cpu().numpy().astype(np.float64)
    p = ptr_.cpu().numpy()
    return np.stack([s[:, p[g]:p[g + 1]].mean(axis=1) for g in range(len(p) - 1)], axis=1)  # [k, G]


def _oracle_and_emulation(cfg, D, ol, ov, pred, ptr_):
    """(the f64 oracle's per-building means [k, G], e_emu): e_emu is the
    largest error, against those means, of the f32 oracle critic run on the
    CPU with its weight matrices rounded to f16 and the output of every leaf
    module rounded to f16 -- except the decoder's last Linear and the Sigmoid,
    whose outputs the kernels keep in f32."""
    from oracle import reference as R

    state = {k: v.detach().cpu() for k, v in D.state_dict().items()}

    def build(dtype):
        Do = R.Discriminator(cfg)
        Do.decoder = torch.nn.Sequential(*[
            torch.nn.Linear(m.in_features, m.out_features) if isinstance(m, torch.nn.Linear) else type(m)()
            for m in D.decoder.children()])  # (the odd decoder of T2's critic; the default's is the same)
        Do = Do.to(dtype)
        Do.load_state_dict({k: v.to(dtype) for k, v in state.items()})
        return Do.eval()

    def run(Do, dtype):
        x_l, x_v = ol.x, ov.x
        ol.x, ov.x = x_l.to(dtype), x_v.to(dtype)
        try:
            with torch.no_grad():
                return torch.stack([Do(ol, ov, torch.nn.functional.one_hot(pred[c].long(), K).to(dtype)).reshape(-1)
                                    for c in range(pred.shape[0])])
        finally:
            ol.x, ov.x = x_l, x_v

    ref_means = _host_means(run(build(torch.float64), torch.float64), ptr_)
    De = build(torch.float32)
    with torch.no_grad():
        for p in De.parameters():
            if p.dim() == 2:
                p.copy_(p.half().float())
    dec = list(De.decoder.children())
    keep_f32 = {id(m) for m in dec if isinstance(m, torch.nn.Sigmoid)}
    keep_f32.add(id([m for m in dec if isinstance(m, torch.nn.Linear)][-1]))
    for m in De.modules():
        if not list(m.children()) and id(m) not in keep_f32:
            m.register_forward_hook(lambda mod, inp, out: out.half().float())
    emu = run(De, torch.float32)
    e_emu = float(np.abs(_host_means(emu, ptr_) - ref_means).max())
    return ref_means, e_emu


@pytest.mark.parametrize("wgangp", [True, False])
@pytest.mark.parametrize("k", [1, 4])
def test_native_call_equals_the_python_path(cuda, case, wgangp, k):
    items, pred = case
    _, (loc, vox) = batches_from_items(items, cuda)
    _, D = _critic(cuda, wgangp)
    D.train()
    hc = HalfCritic(D)
    p = pred[:k].to(cuda)
    a = hc.score_labels(loc, vox, p)
    b = hc.score_labels(loc, vox, p, native=False)
    torch.cuda.synchronize()
    assert D.training  # nothing switched, nothing drawn
    assert a.shape == (k, p.shape[1]) and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.equal(hc.score_labels(loc, vox, p), a)  # the arena reused: the same bits
    if not wgangp:
        assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0  # Sigmoid included
    # a strided view of a wider buffer
    pbuf = torch.zeros(k, p.shape[1] + 3, dtype=torch.int8, device=cuda)
    pbuf[:, :p.shape[1]].copy_(p)
    assert torch.equal(hc.score_labels(loc, vox, pbuf[:, :p.shape[1]]), a)
    # the f32 critic's scores, for scale: f16 rounding apart
    f32 = D.score_labels(loc, vox, p)
    print(f"USE_WGANGP={wgangp} k={k}: max |f16 - f32 scores| = {float((a - f32).abs().max()):.3e}, "
          f"max |score| = {float(f32.abs().max()):.3e}")
    # the select tail
    sel = hc.select(loc, vox, p)
    want = ops.sweep_select_score(a, p, vox.ptr)
    for x, y in zip(sel, want):
        assert x.dtype == y.dtype and torch.equal(x, y)
    with pytest.raises(ValueError):
        hc.score_labels(loc, vox, p[:, :-1])


@pytest.mark.parametrize("wgangp", [True, False])
@pytest.mark.parametrize("odd_decoder", [False, True])
def test_scores_against_the_oracle(cuda, case, wgangp, odd_decoder):
    """Per-building means of HalfCritic against the f64 CPU oracle, bound
    4 e_emu (module docstring).  odd_decoder: a 64-24-12-6-1 decoder, which
    vg_hcritic_decode refuses -- the per-layer vg_hgemm path, same bound.
    The perturbed critics are run for the error bound only (their oracle
    top-two gap falls to 3e-6).

    Measured on an MI355X, largest |mean - oracle mean| over
    the 4 x 4 per-building means, (e_emu; bound) behind it:
      WGAN-GP at init 4.45e-5 (2.61e-5; 1.04e-4), perturbed 2.20e-5 (3.37e-5; 1.35e-4)
      BCE     at init 1.10e-5 (6.48e-6; 2.59e-5), perturbed 5.45e-6 (8.37e-6; 3.35e-5)
      64-24-12-6-1 decoder: WGAN-GP 4.05e-5 / 4.68e-5 (bounds 1.61e-4 / 2.10e-4),
                            BCE 9.85e-6 / 1.12e-5 (bounds 3.91e-5 / 4.99e-5)
    At init three of the four buildings have an oracle top-two gap above twice
    the bound under either objective and best equals the oracle's choice on
    them; the fourth (gap 1.9e-4 against 2.1e-4, 4.6e-5 against 5.2e-5) goes
    unchecked."""
    items, pred = case
    (ol, ov), (loc, vox) = batches_from_items(items, cuda)
    for perturbed in (False, True):
        cfg, D = _critic(cuda, wgangp, perturbed, odd_decoder)
        ref_means, e_emu = _oracle_and_emulation(cfg, D, ol, ov, pred, vox.ptr)
        hc = HalfCritic(D)
        p = pred.to(cuda)
        sel = hc.select(loc, vox, p)
        assert torch.equal(hc.score_labels(loc, vox, p), hc.score_labels(loc, vox, p, native=False))
        got = sel.score.cpu().numpy()
        e1 = float(np.abs(got - ref_means).max())
        bound = 4 * e_emu
        top = np.sort(ref_means, axis=0)
        gaps = top[-1] - top[-2]
        print(f"USE_WGANGP={wgangp} odd_decoder={odd_decoder} perturbed={perturbed}: e_emu = {e_emu:.3e}; "
              f"|HalfCritic means - oracle means| = {e1:.3e} (bound 4 e_emu = {bound:.3e}); "
              f"oracle top-two gaps {[f'{x:.2e}' for x in gaps]}")
        assert e1 <= bound
        if perturbed or odd_decoder:  # run for the error bound only
            continue
        checked = gaps > 2 * bound
        assert int((~checked).sum()) <= 1, gaps
        best = sel.best.cpu().numpy()
        assert np.array_equal(best[checked], np.argmax(ref_means, axis=0)[checked])


# ------------------------------------------------------------------ T5
@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return write_store(str(tmp_path_factory.mktemp("hcritic") / "s"), SyntheticDataset(7, seed=17))


def test_stream_select_with_the_f16_critic(cuda, store):
    cfg = Configuration()
    cfg.DEVICE = str(cuda)
    torch.manual_seed(5)
    G = VoxelGNNGenerator(cfg, 17, 12).to(cuda)
    D = VoxelGNNDiscriminator(cfg, 17, 12).to(cuda)

    def loader():
        return GraphLoader(store, list(range(len(store))), batch_size=4, shuffle=False, device=cuda, prefetch=2,
                           prepare=(K, ()))

    taus = geometric_taus(1.0, 0.1, 3)
    D.train()
    G.rng = RNG("device", seed=99)
    sw = InferenceSweep(G, taus, dtype="f16", critic=D, critic_dtype="f16")
    assert isinstance(sw.half_critic, HalfCritic)
    res = sw.run_stream(loader(), collect=True, select="critic")
    torch.cuda.synchronize()
    ctr = G.rng._iter(cuda).clone()
    assert D.training
    G.rng = RNG("device", seed=99)
    ref = InferenceSweep(G, taus, dtype="f16").run_stream(loader(), collect=True)
    torch.cuda.synchronize()
    assert torch.equal(G.rng._iter(cuda), ctr)  # the generator's counter: the same with and without the critic
    assert "selected" not in ref and res["batches"] == 2 and res["graphs"] == 7 and res["samples"] == 21
    assert len(res["predictions"]) == len(ref["predictions"]) == len(res["selected"]) == 2
    for a, b in zip(res["predictions"], ref["predictions"]):
        assert a.dtype == torch.int8 and a.shape == b.shape and torch.equal(a, b)
    hc = HalfCritic(D)
    for pred, sel, (loc, vox) in zip(res["predictions"], res["selected"], list(loader())):
        assert sorted(sel) == ["best", "labels", "score"]
        p = vox.ptr.cpu().numpy()
        k, n = pred.shape
        batch = np.repeat(np.arange(len(p) - 1), np.diff(p))
        labels, best, score = sel["labels"].numpy(), sel["best"].numpy(), sel["score"].numpy()
        assert labels.dtype == np.int8 and labels.shape == (n,) and best.shape == (len(p) - 1,)
        assert score.dtype == np.float64 and score.shape == (k, len(p) - 1)
        assert np.array_equal(labels, pred.numpy()[best[batch], np.arange(n)])  # the gather of best
        assert np.array_equal(best, np.argmax(score, axis=0))
        want = ops.sweep_select_score(hc.score_labels(loc, vox, pred.to(cuda)), pred.to(cuda), vox.ptr)
        assert np.array_equal(score, want.score.cpu().numpy()) and np.array_equal(best, want.best.cpu().numpy())
    # without critic_dtype: the f32 critic, to the bit
    G.rng = RNG("device", seed=99)
    dflt = InferenceSweep(G, taus, dtype="f16", critic=D)
    assert dflt.half_critic is None and dflt.critic_dtype == "f32"
    res32 = dflt.run_stream(loader(), collect=True, select="critic")
    for pred, sel, (loc, vox) in zip(res32["predictions"], res32["selected"], list(loader())):
        want = ops.sweep_select_score(D.score_labels(loc, vox, pred.to(cuda)), pred.to(cuda), vox.ptr)
        for name in ("labels", "best", "score"):
            assert torch.equal(sel[name], getattr(want, name).cpu()), name
    # critic_dtype is independent of dtype
    G.rng = RNG("device", seed=99)
    mixed = InferenceSweep(G, taus, dtype="f32", critic=D, critic_dtype="f16")
    loc, vox = next(iter(loader()))
    pred = mixed.run_batch(loc, vox)
    sel = mixed.select(pred, loc, vox, "critic")
    want = ops.sweep_select_score(hc.score_labels(loc, vox, pred), pred, vox.ptr)
    assert isinstance(sel, ops.CriticSelection) and all(torch.equal(a, b) for a, b in zip(sel, want))
    cfg2 = Configuration()
    cfg2.DEVICE = str(cuda)
    cfg2.DISCRIMINATOR_CONV_TYPE = "GATV2CONV"
    with pytest.raises(ValueError, match="GATCONV"):
        InferenceSweep(G, taus, dtype="f16", critic=VoxelGNNDiscriminator(cfg2, 17, 12), critic_dtype="f16")


# ------------------------------------------------------------------ T6
def test_refresh_follows_the_weights(cuda, case):
    items, pred = case
    _, (loc, vox) = batches_from_items(items, cuda)
    _, D = _critic(cuda, True)
    p = pred.to(cuda)
    hc = HalfCritic(D)
    a = hc.score_labels(loc, vox, p).clone()
    with torch.no_grad():
        for q in D.parameters():
            q.add_(0.05 * torch.randn(q.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1)))
    assert torch.equal(hc.score_labels(loc, vox, p), a)  # a snapshot: unchanged until refresh()
    hc.refresh()
    b = hc.score_labels(loc, vox, p)
    assert not torch.equal(a, b)
    fresh = HalfCritic(D)
    assert torch.equal(fresh.score_labels(loc, vox, p), b)
    assert torch.equal(fresh.score_labels(loc, vox, p, native=False), b)


# ------------------------------------------------------------------ T7
def test_score_labels_can_be_captured(cuda, case):
    """The native call only launches: one chain on the capturing stream."""
    items, pred = case
    _, (loc, vox) = batches_from_items(items, cuda)
    _, D = _critic(cuda, False)
    p = pred.to(cuda)
    hc = HalfCritic(D)
    want = hc.score_labels(loc, vox, p).clone()  # warm-up: the arena, the f16 image of the batch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hc.score_labels(loc, vox, p)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
