"""The BCE objective (USE_WGANGP = False) on the HIP engines.

* vg_bce_critic_head and the generator's BCE loss head against torch's own
  arithmetic (sigmoid, then F.binary_cross_entropy, f32 on the CPU, through
  autograd), saturated rows included;
* BceCriticEngine (vgan/bce.py) against the CPU oracle's discriminator_loss
  backward and against the autograd path on the GPU;
* GeneratorEngine under BCE against the autograd generator iteration;
* the trainer: engine selection, eager steps, step_graphed and step_fresh.

Tolerances are the project's (tests/test_critic_gpu.py): kernels 1e-5 relative
to the output's scale, engine loss 1e-5, gradients grads_close at 1e-3.  They
have margin: for |s| <= 4.5 a 1-ulp change of p = sigmoid(s) moves a BCE term
and its seed by at most 3e-7 relative, so the comparison scores are randn * 1
(s in about 12..18 is 1-ulp sensitive -- 1 - p has few bits left -- and stays
out of the closeness checks); the saturated rows are checked at their exact
or stated values.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import reference as R
from parity_util import batches_from_items, grads_close
from vgan import synth
from vgan._lib import LIB, check, ptr, stream_handle
from vgan.config import Configuration
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
from vgan.synth import SyntheticDataset
from vgan.trainer import Trainer

pytestmark = pytest.mark.gpu

HEAD_ROWS = [1, 63, 64, 65, 1000, 20001]  # one row, the wave edges, several workgroups, a ragged tail


def _close(got, ref, tol=1e-5):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    scale = max(ref.abs().max().item(), 1e-12)
    err = (got - ref).abs().max().item() / scale
    return err <= tol, err


# ------------------------------------------------------------ critic head
def _critic_head(cuda, s):
    """(out [3], seeds [2N]) of vg_bce_critic_head on the stacked scores s [2N]."""
    n = s.numel() // 2
    sd = s.to(cuda).contiguous()
    out, seeds = torch.empty(3, device=cuda), torch.empty(2 * n, device=cuda)
    ws = torch.empty(int(LIB.vg_bce_critic_head_ws_floats(n)), device=cuda)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    check(LIB.vg_bce_critic_head(ptr(sd), n, ptr(out), ptr(seeds), ptr(ws), ptr(cnt), stream_handle(cuda)),
          "vg_bce_critic_head")
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0  # the counter is left at 0
    return out.cpu(), seeds.cpu()


def _critic_head_torch(s):
    """sigmoid then F.binary_cross_entropy in f32 on the CPU, through autograd."""
    n = s.numel() // 2
    leaf = s.clone().requires_grad_(True)
    p = torch.sigmoid(leaf)
    real = F.binary_cross_entropy(p[:n], torch.ones(n))
    fake = F.binary_cross_entropy(p[n:], torch.zeros(n))
    loss = fake + real
    (g,) = torch.autograd.grad(loss, leaf)
    return torch.stack([loss, real, fake]).detach(), g


@pytest.mark.parametrize("n", HEAD_ROWS)
def test_critic_head_matches_torch(cuda, n):
    s = torch.randn(2 * n, generator=torch.Generator().manual_seed(100 + n))
    out, seeds = _critic_head(cuda, s)
    ref, g = _critic_head_torch(s)
    for i, name in enumerate(("loss", "loss_real", "loss_fake")):
        err = abs(out[i].item() - ref[i].item()) / max(abs(ref[i].item()), 1e-12)
        print(f"n {n} {name}: {out[i].item():.7f} vs {ref[i].item():.7f} rel {err:.2e}")
        assert err <= 1e-5, (name, out[i].item(), ref[i].item())
    ok, err = _close(seeds, g)
    print(f"n {n} seeds: max err / scale {err:.2e}")
    assert ok, err
    out2, seeds2 = _critic_head(cuda, s)  # fixed-order fold: bit-identical run to run
    assert torch.equal(out, out2) and torch.equal(seeds, seeds2)


def test_critic_head_saturated_rows(cuda):
    """Rows whose probability is 0 or 1 in f32, and the row where the 1e-12
    clamp of the backward bites: the reference's values, not a softplus's."""
    def one(s_real, s_fake):
        out, seeds = _critic_head(cuda, torch.tensor([s_real, s_fake]))
        return out[1].item(), out[2].item(), seeds[0].item(), seeds[1].item()

    for s in (40.0, 120.0):
        real, fake, g_real, g_fake = one(s, s)
        assert fake == 100.0 and g_fake == 0.0  # p == 1 against target 0: the clamped term, no gradient
        assert real == 0.0 and g_real == 0.0  # p == 1 against target 1
    real, fake, g_real, g_fake = one(-120.0, -120.0)
    assert real == 100.0 and g_real == 0.0  # p == 0 against target 1
    assert fake == 0.0 and g_fake == 0.0
    real, fake, g_real, g_fake = one(-30.0, -40.0)
    assert abs(real - 30.0) <= 1e-5 * 30.0
    # N = 1: (p - 1) / 1e-12 * (1 - p) p = about -0.0936 (the softplus value would be about -1)
    exact = -1e12 / (1.0 + math.exp(30.0))
    assert abs(exact + 0.0936) < 1e-4 and abs(g_real - exact) <= 1e-5 * abs(exact), (g_real, exact)
    # and all of them in one launch against torch itself
    s = torch.tensor([40.0, 120.0, -120.0, -30.0, 0.5, 40.0, 120.0, -120.0, -30.0, -0.5])
    out, seeds = _critic_head(cuda, s)
    ref, g = _critic_head_torch(s)
    assert torch.allclose(out, ref, rtol=1e-5, atol=0.0), (out, ref)
    assert torch.allclose(seeds, g, rtol=1e-5, atol=1e-12), (seeds, g)


# --------------------------------------------------- generator BCE head
LAMBDAS = (1.3, 0.3, 0.7, 0.11, 0.05)  # (adv, label, ratio, ratio_void, far): every one off its default
UPSTREAM = 1.7


def _gen_inputs(n, k, g, seed):
    gen = torch.Generator().manual_seed(seed)
    vtype = torch.randint(0, k, (n,), generator=gen)
    return dict(d_fake=torch.randn(n, 1, generator=gen), hard=torch.rand(n, k, generator=gen),
                logits=torch.randn(n, k, generator=gen), onehot=F.one_hot(vtype, k).float(), vtype=vtype,
                far_gen=torch.rand(g, generator=gen), far_ref=torch.rand(g, generator=gen))


def _gen_loss_torch(inp, lam):
    """trainer.py:334-385 with the BCE adversarial term (:341) restated in
    torch, f32 on the CPU: the loss and its gradients w.r.t. the pre-sigmoid
    scores, hard and logits under an upstream factor."""
    d_fake, hard, logits = (inp[k].clone().requires_grad_(True) for k in ("d_fake", "hard", "logits"))
    onehot, vtype, fg, fr = inp["onehot"], inp["vtype"], inp["far_gen"], inp["far_ref"]
    n = hard.shape[0]
    p = torch.sigmoid(d_fake)
    adv = F.binary_cross_entropy(p, torch.ones_like(p)) * lam[0]
    rg, rr = hard.sum(0) / n, onehot.sum(0) / n
    loss = (adv + F.mse_loss(rg[:-2], rr[:-2]) * lam[2] + F.cross_entropy(logits, vtype) * lam[1]
            + F.mse_loss(rg[-2:], rr[-2:]) * lam[3] + F.mse_loss(fg, fr) * lam[4])
    return loss.detach(), torch.autograd.grad(loss * UPSTREAM, (d_fake, hard, logits))


def _check_gen_head(cuda, n, k, g, lam, seed):
    inp = _gen_inputs(n, k, g, seed)
    dev = {key: v.to(cuda).contiguous() for key, v in inp.items()}
    st = stream_handle(cuda)
    out = torch.empty(k + 3, device=cuda)
    ws = torch.empty(int(LIB.vg_gen_loss_ws_floats(n, k)), device=cuda)
    check(LIB.vg_gen_loss_bce_fwd(ptr(dev["d_fake"]), ptr(dev["hard"]), ptr(dev["logits"]), ptr(dev["onehot"]),
                                  ptr(dev["vtype"]), n, k, ptr(dev["far_gen"]), ptr(dev["far_ref"]), g, *lam, ptr(out),
                                  ptr(ws), st), "vg_gen_loss_bce_fwd")
    up = torch.tensor([UPSTREAM], device=cuda)
    g_d, g_h, g_l = torch.empty(n, 1, device=cuda), torch.empty(n, k, device=cuda), torch.empty(n, k, device=cuda)
    check(LIB.vg_gen_loss_bce_bwd(ptr(up), ptr(out), ptr(dev["d_fake"]), ptr(dev["logits"]), ptr(dev["vtype"]), n, k,
                                  ptr(g_d), ptr(g_h), ptr(g_l), st), "vg_gen_loss_bce_bwd")
    torch.cuda.synchronize()
    loss, grads = _gen_loss_torch(inp, lam)
    err = abs(out[0].item() - loss.item()) / max(abs(loss.item()), 1e-12)
    print(f"gen BCE head n {n} K {k}: loss {out[0].item():.7f} vs {loss.item():.7f} rel {err:.2e}")
    assert err <= 1e-5
    for name, got, ref in (("d d_fake", g_d, grads[0]), ("d hard", g_h, grads[1]), ("d logits", g_l, grads[2])):
        ok, e = _close(got, ref)
        print(f"gen BCE head n {n} K {k} {name}: max err / scale {e:.2e}")
        assert ok, (name, e)


@pytest.mark.parametrize("n", HEAD_ROWS)
def test_gen_bce_head_matches_torch(cuda, n):
    _check_gen_head(cuda, n, 7, 3, (1.0, 1.0, 1.0, 1.0, 1.0), 7 * n + 1)


def test_gen_bce_head_three_classes(cuda):
    _check_gen_head(cuda, 1000, 3, 5, (1.0, 1.0, 1.0, 1.0, 1.0), 41)


def test_gen_bce_head_every_lambda_off_its_default(cuda):
    _check_gen_head(cuda, 1000, 7, 5, LAMBDAS, 43)


def test_gen_bce_head_saturated_scores(cuda):
    """target 1: s = -120 gives the clamped term 100 and no gradient, s = +40 neither."""
    n, k = 2, 7
    inp = _gen_inputs(n, k, 1, 3)
    inp["d_fake"] = torch.tensor([[-120.0], [40.0]])
    dev = {key: v.to(cuda).contiguous() for key, v in inp.items()}
    st = stream_handle(cuda)
    out = torch.empty(k + 3, device=cuda)
    ws = torch.empty(int(LIB.vg_gen_loss_ws_floats(n, k)), device=cuda)
    lam = (1.0, 0.0, 0.0, 0.0, 0.0)
    check(LIB.vg_gen_loss_bce_fwd(ptr(dev["d_fake"]), ptr(dev["hard"]), ptr(dev["logits"]), ptr(dev["onehot"]),
                                  ptr(dev["vtype"]), n, k, ptr(dev["far_gen"]), ptr(dev["far_ref"]), 1, *lam, ptr(out),
                                  ptr(ws), st), "vg_gen_loss_bce_fwd")
    one = torch.ones(1, device=cuda)
    g_d = torch.empty(n, 1, device=cuda)
    check(LIB.vg_gen_loss_bce_bwd(ptr(one), ptr(out), ptr(dev["d_fake"]), None, None, n, k, ptr(g_d), None, None, st),
          "vg_gen_loss_bce_bwd")
    torch.cuda.synchronize()
    assert out[0].item() == 50.0  # mean(100, 0)
    assert g_d.abs().max().item() == 0.0


# ---------------------------------------------------------- critic engine
class _RecRNG:
    """Seeded CPU draws in the engine's (= the autograd path's) order, recorded."""
    mode = "fixed"

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.draws = []

    def keep_mask(self, shape, p, device):
        t = torch.empty(*shape).bernoulli_(1 - p, generator=self.g).div_(1 - p)
        self.draws.append(t)
        return t.to(device)

    def uniform(self, shape, device):
        raise AssertionError("the BCE critic draws no eps")


class _replayed_dropout:
    """Feeds recorded dropout multipliers to the oracle's nn.Dropout modules,
    in call order (D(real)'s blocks, then D(fake)'s)."""

    def __init__(self, masks):
        self.masks = list(masks)

    def __enter__(self):
        self.orig = F.dropout

        def replay(x, p=0.5, training=True, inplace=False):
            # (the oracle's GATConv calls F.dropout on its attention with p = 0: no draw)
            return x * self.masks.pop(0) if training and p > 0.0 else x
        F.dropout = replay
        return self

    def __exit__(self, *exc):
        F.dropout = self.orig


def _bce_cfg(cuda):
    cfg = Configuration()
    cfg.DEVICE = str(cuda)
    cfg.USE_WGANGP = False
    return cfg


def _items(kind):
    if kind == "buildings":
        return [synth.make_building(777, n) for n in (1, 2, 3)]
    # 49 nodes, below the 64-row threshold: the unfused GraphNorm-backward branch
    return [synth.make_stress_building(777, 1, F=1, Y=7, X=7)]


_SETUPS = {}


def _engine_setup(cuda, kind, seed=11, shared=True):
    """(cfg, D, flat, oracle pair, vgan pair, hard, soft, engine), built once
    per batch kind (``shared=False``: a model of the caller's own)."""
    if shared and kind in _SETUPS:
        return _SETUPS[kind]
    from vgan.bce import BceCriticEngine
    from vgan.flat import FlatParams

    cfg = _bce_cfg(cuda)
    torch.manual_seed(seed)
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    flat = FlatParams(D)
    (ol, ov), (loc, vox) = batches_from_items(_items(kind), cuda)
    n = vox.num_nodes
    g = torch.Generator().manual_seed(seed + 1)
    soft = torch.softmax(torch.randn(n, 7, generator=g) * 2, 1)
    hard = F.one_hot(soft.argmax(1), 7).float()
    setup = (cfg, D, flat, (ol, ov), (loc, vox), hard, soft, BceCriticEngine(D, cfg))
    if shared:
        _SETUPS[kind] = setup
    return setup


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("kind", ["buildings", "stress49"])
def test_critic_engine_matches_oracle(cuda, kind, training):
    cfg, D, flat, (ol, ov), (loc, vox), hard, soft, eng = _engine_setup(cuda, kind)
    n = vox.num_nodes
    assert (n == 49) == (kind == "stress49") and (n >= 64) == (kind == "buildings")
    D.train(training)
    rng = _RecRNG(3)
    flat.zero_grad()
    hd, sd = hard.to(cuda).unsqueeze(0), soft.to(cuda).unsqueeze(0)
    pair = torch.full((2,), 7.0, device=cuda)
    loss = eng.loss_and_grad(loc, vox, hd, sd, rng, out=pair)
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in D.named_parameters()}
    assert len(rng.draws) == (2 * len(eng.blocks) if training else 0)
    Do = R.Discriminator(cfg)
    Do.load_state_dict({k: v.detach().cpu() for k, v in D.state_dict().items()})
    Do.train(training)
    with _replayed_dropout(rng.draws) as rep:
        ref = R.discriminator_loss(Do, cfg, ol, ov, hard.unsqueeze(0), soft.unsqueeze(0))
        ref.backward()
        assert not rep.masks
    print(f"{kind} training {training}: d_loss {loss.item():.7f} vs oracle {ref.item():.7f}")
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert pair[0].item() == loss.item() and pair[1].item() == 0.0  # out receives (d_loss, 0.0)
    assert abs(eng.last_loss_real.item() + eng.last_loss_fake.item() - loss.item()) <= 1e-6
    ref_grads = {k: p.grad for k, p in Do.named_parameters()}
    ok, worst, total = grads_close(grads, ref_grads, rtol=1e-3)
    print(f"{kind} training {training}: D gradient relative error {total:.2e}, worst {worst}")
    assert ok, (worst, total)
    # gradients are accumulated: a second call on top of a non-zero .grad adds to it
    if not training:
        eng.loss_and_grad(loc, vox, hd, sd, rng)
        torch.cuda.synchronize()
        twice = {k: p.grad.detach().cpu() for k, p in D.named_parameters()}
        ok, worst, total = grads_close(twice, {k: 2 * v for k, v in ref_grads.items()}, rtol=1e-3)
        assert ok, (worst, total)
    D.train(True)


def test_critic_engine_matches_autograd_path_on_gpu(cuda):
    """Same D, batch and host-RNG draws: the engine consumes the stream exactly
    like Trainer._compute_discriminator_loss (masks of D(real), then D(fake))."""
    from vgan.rng import RNG

    cfg, D, flat, _, (loc, vox), hard, soft, eng = _engine_setup(cuda, "buildings", shared=False)
    cfg_t = _bce_cfg(cuda)
    cfg_t.runtime["rng"] = "host"
    cfg_t.runtime["critic"] = "autograd"
    G = VoxelGNNGenerator(cfg_t, 17, 12)
    tr = Trainer(G, D, None, torch.optim.Adam(G.parameters()), torch.optim.Adam(D.parameters()), None, cfg_t)
    assert tr.critic is None
    D.train(True)
    rng = RNG("host")
    hd, sd = hard.to(cuda).unsqueeze(0), soft.to(cuda).unsqueeze(0)
    torch.manual_seed(123)
    tr.flat_d.zero_grad()
    l_eng = eng.loss_and_grad(loc, vox, hd, sd, rng)
    g_eng = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
    after = torch.get_rng_state()
    torch.manual_seed(123)
    tr.flat_d.zero_grad()
    l_ag = tr._compute_discriminator_loss(loc, vox, hd, sd)
    l_ag.backward()
    assert torch.equal(torch.get_rng_state(), after)
    g_ag = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
    print(f"d_loss engine {l_eng.item():.7f} autograd {l_ag.item():.7f}")
    assert abs(l_eng.item() - l_ag.item()) <= 1e-5 * max(1.0, abs(l_ag.item()))
    ok, worst, total = grads_close(g_eng, g_ag, rtol=1e-3)
    print(f"engine vs autograd D gradient relative error {total:.2e}, worst {worst}")
    assert ok, (worst, total)


# ------------------------------------------------------- generator engine
def _trainer(cfg, seed=777):
    torch.manual_seed(seed)
    G, D = VoxelGNNGenerator(cfg, 17, 12), VoxelGNNDiscriminator(cfg, 17, 12)
    og = torch.optim.Adam(G.parameters(), lr=cfg.LEARNING_RATE_GENERATOR, betas=cfg.BETAS)
    od = torch.optim.Adam(D.parameters(), lr=cfg.LEARNING_RATE_DISCRIMINATOR, betas=cfg.BETAS)
    return Trainer(G, D, None, og, od, None, cfg)


def _dev_cfg(cuda, wgangp=False, **runtime):
    cfg = Configuration()
    cfg.DEVICE = str(cuda)
    cfg.USE_WGANGP = wgangp
    cfg.runtime["rng"] = "device"
    cfg.runtime.update(runtime)
    return cfg


def _g_grads(tr):
    flat = tr.flat_g
    return {k: flat.grad[flat._offset(p):flat._offset(p) + p.numel()].clone()
            for k, p in tr.generator.named_parameters()}


def test_generator_engine_matches_autograd_iteration(cuda):
    """From identical parameters and device-RNG state both paths draw the same
    numbers and run the same forward kernels up to D's last Linear: the labels
    are bit-identical; the loss to 1e-6 (the head's sigmoid / log and its
    reduction order against torch's elementwise kernels and mean)."""
    loc, vox = SyntheticDataset(4, seed=31).batch(range(4))
    loc, vox = loc.to(cuda), vox.to(cuda)
    a, b = _trainer(_dev_cfg(cuda, gen="engine")), _trainer(_dev_cfg(cuda, gen="autograd"))
    assert a.gen_engine is not None and a.gen_engine.bce and b.gen_engine is None
    for it in range(2):  # the second draws from the advanced device counter
        outs = []
        for tr in (a, b):
            g_loss, hard = tr._gen_iteration(loc, vox)
            outs.append((g_loss.detach().clone(), hard.detach().clone(), _g_grads(tr)))
        torch.cuda.synchronize()
        (la, ha, ga), (lb, hb, gb) = outs
        assert torch.equal(ha, hb), it
        print(f"iteration {it}: g_loss engine {float(la):.7f} autograd {float(lb):.7f}")
        assert abs(float(la) - float(lb)) <= 1e-6 * max(1.0, abs(float(lb))), (it, float(la), float(lb))
        ok, worst, total = grads_close(ga, gb, rtol=1e-3)
        print(f"iteration {it}: engine vs autograd G gradient relative error {total:.2e}, worst {worst}")
        assert ok, (it, worst, total)
    assert a.gen_engine.__dict__.get("native_calls", 0) == 0  # the native C++ engine is WGAN-GP only


# ---------------------------------------------------------------- trainer
def test_trainer_selects_the_engines(cuda):
    from vgan.bce import BceCriticEngine
    from vgan.critic import CriticEngine

    tr = _trainer(_dev_cfg(cuda))
    assert isinstance(tr.critic, BceCriticEngine) and tr.gen_engine is not None
    tr = _trainer(_dev_cfg(cuda, critic="autograd", gen="autograd"))
    assert tr.critic is None and tr.gen_engine is None
    tr = _trainer(_dev_cfg(cuda, wgangp=True))
    assert type(tr.critic) is CriticEngine


def _batch(cuda, k=0):
    loc, vox = SyntheticDataset(16, seed=4).batch(range(4 * k, 4 * k + 4))
    return loc.to(cuda), vox.to(cuda)


def test_trainer_eager_steps(cuda):
    tr = _trainer(_dev_cfg(cuda))
    loc, vox = _batch(cuda)
    g0, d0 = tr.flat_g.param.clone(), tr.flat_d.param.clone()
    for _ in range(2):
        out = tr.step(loc, vox)
        torch.cuda.synchronize()
        assert torch.isfinite(out["d_losses"]).all() and torch.isfinite(out["g_loss"]).all()
        assert not torch.equal(tr.flat_g.param, g0) and not torch.equal(tr.flat_d.param, d0)
        g0, d0 = tr.flat_g.param.clone(), tr.flat_d.param.clone()
    # a BCE critic loss is a sum of two non-negative means, near 2 log 2 at initialisation
    assert float(out["d_losses"].min()) > 0.0


def _check_step_pair(a, b, oa, ob, k, n_critic):
    """The comparison standard of tests/test_trainer_gpu.py::test_step_fresh_matches_eager_step."""
    da, db = oa["d_losses"].cpu(), ob["d_losses"].cpu()
    print(f"step {k}: d_losses eager {da.tolist()} other {db.tolist()}; "
          f"max |param diff| G {float((a.flat_g.param - b.flat_g.param).abs().max()):.2e} "
          f"D {float((a.flat_d.param - b.flat_d.param).abs().max()):.2e}")
    assert torch.allclose(da, db, rtol=1e-4, atol=1e-5)
    assert abs(float(oa["g_loss"]) - float(ob["g_loss"])) <= 1e-4 * max(1.0, abs(float(oa["g_loss"])))
    for x, y in ((a.flat_g.param, b.flat_g.param), (a.flat_d.param, b.flat_d.param)):
        d = (x - y).abs()
        assert float(d.max()) <= 5e-4 and float((d > 1e-6).float().mean()) < 2e-3
    assert int(a.adam_d.step_t.item()) == int(b.adam_d.step_t.item()) == (k + 1) * n_critic


def test_step_graphed_matches_eager_steps(cuda):
    """step_graphed captured once and replayed against two eager steps from the
    same snapshot and device-RNG stream."""
    cfg = _dev_cfg(cuda)
    a, b = _trainer(cfg), _trainer(cfg)
    loc, vox = _batch(cuda)
    for k in range(2):
        oa = a.step(loc, vox)
        ob = b.step_graphed(loc, vox)
        torch.cuda.synchronize()
        _check_step_pair(a, b, oa, ob, k, cfg.N_CRITIC)
        with torch.no_grad():  # continue from identical state
            for x, y in zip(a._state_tensors(), b._state_tensors()):
                y.copy_(x)


def test_step_fresh_matches_eager_steps(cuda):
    cfg = _dev_cfg(cuda)
    a, b = _trainer(cfg), _trainer(cfg)
    for k in range(2):
        loc, vox = _batch(cuda, k)
        oa = a.step(loc, vox)
        ob = b.step_fresh(loc, vox)
        torch.cuda.synchronize()
        _check_step_pair(a, b, oa, ob, k, cfg.N_CRITIC)
        with torch.no_grad():
            for x, y in zip(a._state_tensors(), b._state_tensors()):
                y.copy_(x)
