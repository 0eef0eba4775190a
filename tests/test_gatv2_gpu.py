"""GATv2Conv on the HIP core against the f64 CPU restatement (tests/gatv2_ref.py),
from the kernels up to the models, the trainer and the inference sweep.

Tolerances are the project's own (tests/test_ops_gpu.py): forward 1e-5 relative,
gradients 1e-4, double backward 1e-4 against an f64 CPU reference; the model and
trainer bounds are those of parity_util.run_smoke / step_iterations_vs_oracle.
"""
from __future__ import annotations

import functools

import pytest
import torch

import gatv2_ref as V2
from oracle import reference as R
from parity_util import _FixedUniform, batches_from_items, grads_close, rel_err, tiny_config
from vgan import ops, synth
from vgan._lib import LIB, check, ptr
from vgan.config import Configuration
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
from vgan.trainer import Trainer

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 8, 9, 16, 24, 32, 64, 100, 128, 130, 256)


def _star_graph(n=300):
    """Lattice-free star (tests/test_ops_gpu.py): node 0 receives from every
    node (degree n - 1 > 4 * 64) plus a ring -- every long-row path."""
    src = list(range(1, n)) + list(range(n)) + [(i + 1) % n for i in range(n)]
    dst = [0] * (n - 1) + [(i + 1) % n for i in range(n)] + list(range(n))
    return torch.unique(torch.tensor([src, dst], dtype=torch.long), dim=1), n


@functools.lru_cache(maxsize=None)
def _items():
    return tuple(synth.make_building(777, n) for n in (1, 2))


@functools.lru_cache(maxsize=None)
def _graph(kind: str):
    """(edge_index on the CPU, num_nodes, CSR on the GPU)."""
    if kind == "star":
        ei, n = _star_graph()
    elif kind == "small":
        ei, n = V2.small_graph(40), 40
    else:
        from vgan.graph import GraphBatch

        vox = GraphBatch.from_data_list([v for _, v in _items()])
        ei, n = vox.edge_index, vox.num_nodes
    return ei, n, ops.CSR(ei.cuda(), n)


def _inputs(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)  # noqa: E731
    return [r(n, C), r(n, C), r(C) / C ** 0.5, r(C)]  # x_l, x_r, att, bias


def _to_gpu(ts, grad=True):
    return [t.detach().float().cuda().requires_grad_(grad) for t in ts]


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("graph", ["lattice", "star", "small"])
def test_gatv2_conv_forward_backward(cuda, C, graph):
    ei, n, csr = _graph(graph)
    base = [t.requires_grad_(True) for t in _inputs(n, C, 100 + C)]
    ref = V2.gatv2_propagate(*base, ei)
    g_out = torch.randn(n, C, dtype=torch.float64, generator=torch.Generator().manual_seed(C))
    ref_grads = torch.autograd.grad(ref, base, g_out)
    gt = _to_gpu(base)
    out = ops.gatv2_conv(csr, *gt)
    err = rel_err(out, ref)
    print(f"forward rel err {err:.2e}")
    assert err < 1e-5
    grads = torch.autograd.grad(out, gt, g_out.float().cuda())
    for name, got, want in zip(("x_l", "x_r", "att", "bias"), grads, ref_grads):
        err = rel_err(got, want)
        print(f"grad {name} rel err {err:.2e}")
        assert err < 1e-4, name
    comp = ops.gatv2_conv_composed(csr, *gt)
    assert rel_err(comp, out) < 1e-5


def _raw_forward(csr, x_l, x_r, att, bias):
    n, c = x_l.shape
    out = torch.empty(n, c, device=x_l.device)
    alpha = torch.empty(csr.num_edges, device=x_l.device)
    check(LIB.vg_gatv2_fwd(ptr(csr.row_ptr), ptr(csr.col), n, c, ptr(x_l), x_l.stride(0), ptr(x_r), x_r.stride(0),
                           ptr(att), ptr(bias), 0.2, ptr(out), ptr(alpha), csr.stream()), "vg_gatv2_fwd")
    return out, alpha


def _raw_backward(csr, x_l, x_r, att, alpha, g_out, g_xl, g_xr, g_att, g_bias, accumulate=0):
    n, c = x_l.shape
    ws = torch.empty(int(LIB.vg_gatv2_bwd_ws_floats(n, csr.num_edges, c)), device=x_l.device)
    check(LIB.vg_gatv2_bwd(ptr(csr.row_ptr), ptr(csr.col), ptr(csr.csc_ptr), ptr(csr.csc_slot), ptr(csr.csc_dst), n,
                           csr.num_edges, c, ptr(x_l), x_l.stride(0), ptr(x_r), x_r.stride(0), ptr(att), ptr(alpha),
                           ptr(g_out), 0.2, ptr(g_xl), g_xl.stride(0), ptr(g_xr), g_xr.stride(0), ptr(g_att),
                           ptr(g_bias), accumulate, ptr(ws), csr.stream()), "vg_gatv2_bwd")


def _raw_all(csr, x_l, x_r, att, bias, g_out, g_xl, g_xr):
    c = x_l.shape[1]
    out, alpha = _raw_forward(csr, x_l, x_r, att, bias)
    g_att, g_bias = torch.empty(c, device=out.device), torch.empty(c, device=out.device)
    _raw_backward(csr, x_l, x_r, att, alpha, g_out, g_xl, g_xr, g_att, g_bias)
    return out, alpha, g_xl, g_xr, g_att, g_bias


@pytest.mark.parametrize("C", [3, 9, 16, 100])
@pytest.mark.parametrize("graph", ["lattice", "star"])
def test_gatv2_strided_operands_equal_contiguous(cuda, C, graph):
    """x_l / x_r the two halves of one [N, 2C] buffer, the gradients written
    into the halves of another: bit for bit the contiguous call's results."""
    _, n, csr = _graph(graph)
    x_l, x_r, att, bias = _to_gpu(_inputs(n, C, 7 + C), grad=False)
    g_out = torch.randn(n, C, device=cuda)
    want = _raw_all(csr, x_l, x_r, att, bias, g_out, torch.empty(n, C, device=cuda), torch.empty(n, C, device=cuda))
    y = torch.cat([x_l, x_r], dim=1).contiguous()
    g_y = torch.full((n, 2 * C), float("nan"), device=cuda)
    got = _raw_all(csr, y[:, :C], y[:, C:], att, bias, g_out, g_y[:, :C], g_y[:, C:])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.isnan(g_y).any()


@pytest.mark.parametrize("C", [16, 32, 64])
def test_gatv2_misaligned_views_take_the_scalar_path(cuda, C):
    """Widths whose shape allows vector loads, read from views that start one
    float off the boundary: the path is picked from the addresses, and the
    results are those of the aligned call."""
    _, n, csr = _graph("lattice")
    x_l, x_r, att, bias = _to_gpu(_inputs(n, C, 31 + C), grad=False)
    g_out = torch.randn(n, C, device=cuda)
    want = _raw_all(csr, x_l, x_r, att, bias, g_out, torch.empty(n, C, device=cuda), torch.empty(n, C, device=cuda))
    wide = torch.zeros(n, 2 * C + 4, device=cuda)
    wide[:, 1:1 + C], wide[:, C + 2:2 * C + 2] = x_l, x_r
    g_w = torch.zeros(n, 2 * C + 4, device=cuda)
    got = _raw_all(csr, wide[:, 1:1 + C], wide[:, C + 2:2 * C + 2], att, bias, g_out, g_w[:, 1:1 + C],
                   g_w[:, C + 2:2 * C + 2])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(g_w[:, 0].abs().max()) == 0 and float(g_w[:, 2 * C + 2:].abs().max()) == 0  # nothing beside the views


@pytest.mark.parametrize("C", [3, 16, 64, 130])
@pytest.mark.parametrize("graph", ["lattice", "star"])
def test_gatv2_fused_backward_matches_composed(cuda, C, graph):
    _, n, csr = _graph(graph)
    gt = _to_gpu(_inputs(n, C, 50 + C))
    g_out = torch.randn(n, C, device=cuda)
    out = ops.gatv2_conv(csr, *gt)
    fused = torch.autograd.grad(out, gt, g_out, retain_graph=True)  # grad mode off in backward: vg_gatv2_bwd
    composed = torch.autograd.grad(out, gt, g_out, create_graph=True)  # grad mode on: the composed formulas
    for name, a, b in zip(("x_l", "x_r", "att", "bias"), fused, composed):
        assert b.requires_grad or name == "bias"
        assert rel_err(a, b) < 1e-5, name


@pytest.mark.parametrize("C", [3, 16, 64])
def test_gatv2_conv_double_backward(cuda, C):
    """The WGAN-GP pattern (tests/test_ops_gpu.py): the input gradient with
    create_graph, a penalty on it, its gradient w.r.t. x and every parameter."""
    ei, n, csr = _graph("lattice")
    g = torch.Generator().manual_seed(3 + C)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)  # noqa: E731
    cin = max(2, C // 2)
    base = [r(n, cin), r(C, cin) / cin ** 0.5, r(C) * 0.1, r(C, cin) / cin ** 0.5, r(C) * 0.1, r(C) / C ** 0.5, r(C)]
    w1 = r(n, C)

    def run(ts, fn, w1):
        x, wl, bl, wr, br, att, b = ts
        out = fn(x @ wl.t() + bl, x @ wr.t() + br, att, b)
        gx, = torch.autograd.grad((out * w1).sum(), x, create_graph=True)
        pen = (gx.norm(dim=1) - 1).pow(2).mean()
        res = torch.autograd.grad(pen, ts, allow_unused=True)
        return [torch.zeros_like(t) if q is None else q for q, t in zip(res, ts)]

    ref = run([t.clone().requires_grad_(True) for t in base], lambda a, b, c, d: V2.gatv2_propagate(a, b, c, d, ei), w1)
    got = run(_to_gpu(base), lambda a, b, c, d: ops.gatv2_conv(csr, a, b, c, d), w1.float().cuda())
    scale = max(float(q.norm()) for q in ref)
    for name, a, b in zip(("x", "W_l", "b_l", "W_r", "b_r", "att", "bias"), got, ref):
        d = float((a.double().cpu() - b).norm())
        print(f"{name}: |diff| {d:.3e}, |ref| {float(b.norm()):.3e}")
        assert d <= 1e-4 * float(b.norm()) + 1e-7 * scale, name


def test_gatv2_deterministic_on_the_star(cuda):
    _, n, csr = _graph("star")
    C = 64
    x_l, x_r, att, bias = _to_gpu(_inputs(n, C, 9), grad=False)
    g_out = torch.randn(n, C, device=cuda)
    runs = [_raw_all(csr, x_l, x_r, att, bias, g_out, torch.empty(n, C, device=cuda), torch.empty(n, C, device=cuda))
            for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C", [5, 64])
def test_gatv2_backward_accumulates_parameter_gradients(cuda, C):
    _, n, csr = _graph("lattice")
    x_l, x_r, att, bias = _to_gpu(_inputs(n, C, 13 + C), grad=False)
    g_out = torch.randn(n, C, device=cuda)
    _, alpha, _, _, g_att, g_bias = _raw_all(csr, x_l, x_r, att, bias, g_out, torch.empty(n, C, device=cuda),
                                             torch.empty(n, C, device=cuda))
    prior_a, prior_b = torch.randn(C, device=cuda), torch.randn(C, device=cuda)
    acc_a, acc_b = prior_a.clone(), prior_b.clone()
    _raw_backward(csr, x_l, x_r, att, alpha, g_out, torch.empty(n, C, device=cuda), torch.empty(n, C, device=cuda),
                  acc_a, acc_b, accumulate=1)
    assert rel_err(acc_a, prior_a.double() + g_att.double()) <= 1e-6
    assert rel_err(acc_b, prior_b.double() + g_bias.double()) <= 1e-6
    # no parameter gradients wanted: the input gradients alone
    g1, g2 = torch.empty(n, C, device=cuda), torch.empty(n, C, device=cuda)
    _raw_backward(csr, x_l, x_r, att, alpha, g_out, g1, g2, None, None)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()


# ------------------------------------------------------------------ models
EVAL_SEED = 4321


def _cfg(tiny: bool, g_kind="GATV2CONV", d_kind="GATV2CONV", device="cuda", rng="device"):
    cfg = Configuration()
    cfg.DEVICE = device
    if tiny:
        tiny_config(cfg)
    cfg.GENERATOR_CONV_TYPE, cfg.DISCRIMINATOR_CONV_TYPE = g_kind, d_kind
    cfg.runtime["rng"] = rng
    return cfg


def _fill_zeros_(model, gen):
    """Zero-initialised parameters (biases) get values, so their paths count."""
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().max()) == 0:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)


@functools.lru_cache(maxsize=None)
def _eval_case(tiny: bool):
    """Everything the eval-mode comparison needs, computed once on the CPU: the
    swapped oracle's f32 results from seeded weights and draws, and the check
    that the f32 oracle stays within a quarter of each bound of its f64 run."""
    cfg = _cfg(tiny, device="cpu")
    (ol, ov), _ = batches_from_items(list(_items()), device="cpu")
    gen = torch.Generator().manual_seed(EVAL_SEED)
    torch.manual_seed(EVAL_SEED)
    Go, Do = V2.build_v2(R.Generator, cfg).eval(), V2.build_v2(R.Discriminator, cfg).eval()
    _fill_zeros_(Go, gen)
    _fill_zeros_(Do, gen)
    n = ov.num_nodes
    z = torch.randn(1, n, cfg.Z_DIM, generator=gen)
    noise = torch.empty(n, cfg.NUM_CLASSES).exponential_(generator=gen)
    eps = torch.rand(n, 1, generator=gen)

    def cast_batch(b, dt):
        return type(b)(**{k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b._d.items()})

    logits, hard, soft = Go(ol, ov, z, noise=noise)
    logits, hard, soft = logits.detach(), hard.detach(), soft.detach()
    with torch.no_grad():
        score = Do(ol, ov, hard.unsqueeze(0))

    def d_loss_and_grads(D, ol_, ov_, hard_, soft_, eps_):
        D.zero_grad()
        d_real = D(ol_, ov_, ov_.types_onehot.unsqueeze(0))
        d_fake = D(ol_, ov_, hard_.unsqueeze(0))
        loss = d_fake.mean() - d_real.mean() + R.gradient_penalty(D, cfg, ol_, ov_, soft_.unsqueeze(0), eps=eps_)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in D.named_parameters()}

    d_loss, d_grads = d_loss_and_grads(Do, ol, ov, hard, soft, eps)
    # the same in f64
    G64, D64 = V2.swap_convs(R.Generator(cfg)).double().eval(), V2.swap_convs(R.Discriminator(cfg)).double().eval()
    G64.load_state_dict({k: v.double() for k, v in Go.state_dict().items()})
    D64.load_state_dict({k: v.double() for k, v in Do.state_dict().items()})
    ol64, ov64 = cast_batch(ol, torch.float64), cast_batch(ov, torch.float64)
    with torch.no_grad():
        logits64, _, _ = G64(ol64, ov64, z.double(), noise=noise.double())
        score64 = D64(ol64, ov64, hard.double().unsqueeze(0))
    d_loss64, d_grads64 = d_loss_and_grads(D64, ol64, ov64, hard.double(), soft.double(), eps.double())
    own = {"logits": float((logits.double() - logits64).abs().max()),
           "score": float((score.double() - score64).abs().max()),
           "d_loss": abs(float(d_loss) - float(d_loss64)) / max(1.0, abs(float(d_loss64)))}
    ok, worst, total = grads_close(d_grads, d_grads64, rtol=0.25e-3, floor=0.25e-6)
    print(f"f32 oracle vs its f64 run: {own}, D gradient {total:.2e} (worst {worst})")
    assert own["logits"] <= 0.25e-3 and own["score"] <= 0.25e-3 and own["d_loss"] <= 0.25e-3, own
    assert ok, (worst, total)
    return dict(cfg=cfg, g0=Go.state_dict(), d0=Do.state_dict(), z=z, noise=noise, eps=eps, logits=logits, hard=hard,
                soft=soft, score=score, d_loss=float(d_loss), d_grads=d_grads)


@pytest.mark.parametrize("tiny", [True, False])
def test_gatv2_models_eval_match_swapped_oracle(cuda, tiny):
    """run_smoke's comparison with GATV2CONV in both models: G logits, D scores,
    the WGAN-GP d_loss and D's gradients through the composed second order."""
    case = _eval_case(tiny)
    cfg = _cfg(tiny)
    G, D = VoxelGNNGenerator(cfg, 17, 12), VoxelGNNDiscriminator(cfg, 17, 12)
    G.load_state_dict(case["g0"])
    D.load_state_dict(case["d0"])
    G.eval()
    D.eval()
    _, (loc, vox) = batches_from_items(list(_items()))
    with torch.no_grad():
        logits, _, _ = G(loc, vox, case["z"].cuda(), noise=case["noise"].cuda())
        score = D(loc, vox, case["hard"].cuda().unsqueeze(0))
    err = float((logits.cpu() - case["logits"]).abs().max())
    s_err = float((score.cpu() - case["score"]).abs().max())
    print(f"logits max|err| {err:.2e}, scores max|err| {s_err:.2e}")
    assert err <= 1e-3 and s_err <= 1e-3
    tr = Trainer(G, D, None, None, None, None, cfg)
    assert tr.critic is None and tr.gen_engine is None
    tr.rng = _FixedUniform(case["eps"].cuda())
    d_loss = tr._compute_discriminator_loss(loc, vox, case["hard"].cuda().unsqueeze(0), case["soft"].cuda().unsqueeze(0))
    tr.adam_d.zero_grad()
    d_loss.backward()
    ok, worst, total = grads_close({k: p.grad for k, p in D.named_parameters()}, case["d_grads"])
    print(f"d_loss {d_loss.item():.6f} vs {case['d_loss']:.6f}, D gradient rel err {total:.2e} (worst {worst})")
    assert abs(d_loss.item() - case["d_loss"]) <= 1e-3 * max(1.0, abs(case["d_loss"]))
    assert ok, (worst, total)


# ----------------------------------------------------------------- trainer
def _trainer(cfg, g0=None, d0=None, seed=777):
    torch.manual_seed(seed)
    G, D = VoxelGNNGenerator(cfg, 17, 12), VoxelGNNDiscriminator(cfg, 17, 12)
    if g0 is not None:
        G.load_state_dict(g0)
        D.load_state_dict(d0)
    og = torch.optim.Adam(G.parameters(), lr=cfg.LEARNING_RATE_GENERATOR, betas=cfg.BETAS)
    od = torch.optim.Adam(D.parameters(), lr=cfg.LEARNING_RATE_DISCRIMINATOR, betas=cfg.BETAS)
    return Trainer(G, D, None, og, od, None, cfg)


def test_gatv2_trainer_iterations_match_swapped_oracle(cuda):
    """parity_util.step_iterations_vs_oracle with both models GATV2CONV and
    the oracle's convs swapped: one critic iteration and the generator
    iteration from the same parameters and replayed CPU draws (rng 'host')."""
    cfg = _cfg(True, rng="host")
    (ol, ov), (loc, vox) = batches_from_items(list(_items()))
    torch.manual_seed(2024)
    Go, Do = V2.build_v2(R.Generator, cfg), V2.build_v2(R.Discriminator, cfg)
    g0, d0 = Go.state_dict(), Do.state_dict()
    tr = _trainer(cfg, g0, d0)
    G, D = tr.generator, tr.discriminator
    assert tr.critic is None and tr.gen_engine is None and tr._train_mode() == "eager"
    with pytest.raises(ValueError, match="GATV2CONV"):
        tr.capture(loc, vox)
    torch.manual_seed(99)
    # ---- one critic iteration
    state = torch.get_rng_state()
    with torch.no_grad():
        _, hard, soft = tr._generate(loc, vox)
    mid = torch.get_rng_state()
    torch.set_rng_state(state)
    with torch.no_grad():
        _, ho, so = Go(ol, ov, torch.randn(1, ov.num_nodes, cfg.Z_DIM))
    assert torch.equal(torch.get_rng_state(), mid)  # identical RNG consumption
    assert (soft.squeeze(0).cpu() - so).abs().max().item() < 1e-4
    assert (hard.squeeze(0).cpu().argmax(1) != ho.argmax(1)).float().mean().item() < 0.01
    tr.adam_d.zero_grad()
    d_loss = tr._compute_discriminator_loss(loc, vox, ho.unsqueeze(0).to(cuda), so.unsqueeze(0).to(cuda))
    d_loss.backward()
    after = torch.get_rng_state()
    torch.set_rng_state(mid)
    Do.zero_grad()
    d_ref = R.discriminator_loss(Do, cfg, ol, ov, ho.unsqueeze(0), so.unsqueeze(0))
    d_ref.backward()
    assert torch.equal(torch.get_rng_state(), after)
    print(f"d_loss {d_loss.item():.6f} vs {d_ref.item():.6f}")
    assert abs(d_loss.item() - d_ref.item()) <= 1e-4 * abs(d_ref.item())
    ok, worst, total = grads_close({k: p.grad for k, p in D.named_parameters()},
                                   {k: p.grad for k, p in Do.named_parameters()}, rtol=1e-2, total_rtol=5e-3)
    print(f"critic iteration: D gradient relative error {total:.2e}, worst parameter {worst}")
    assert ok, (worst, total)
    # ---- the generator iteration (autograd: no engine for GATV2CONV)
    state = torch.get_rng_state()
    Go.zero_grad()
    lo, ho, _ = Go(ol, ov, torch.randn(1, ov.num_nodes, cfg.Z_DIM))
    g_ref = R.generator_loss(Do, cfg, ol, ov, lo, ho.unsqueeze(0))
    g_ref.backward()
    torch.set_rng_state(state)
    tr.adam_g.zero_grad()
    g_loss, _ = tr._gen_iteration(loc, vox)
    assert abs(g_loss.item() - g_ref.item()) <= 1e-4 * max(1.0, abs(g_ref.item())), (g_loss.item(), g_ref.item())
    ok, worst, total = grads_close({k: p.grad for k, p in G.named_parameters()},
                                   {k: p.grad for k, p in Go.named_parameters()}, rtol=5e-3, total_rtol=1e-2)
    print(f"generator iteration: G gradient relative error {total:.2e}, worst parameter {worst}")
    assert ok, (worst, total)


def test_gatv2_trainer_steps_and_checkpoints(cuda):
    cfg = _cfg(True)
    cfg.N_CRITIC = 2
    _, (loc, vox) = batches_from_items(list(_items()))
    # seed 2024 (the parity test's weights): the tiny critic's 2-wide last ReLU
    # layer is dead from seed 777's draws -- a constant D, exactly zero gradients
    tr = _trainer(cfg, seed=2024)
    assert tr.critic is None and tr.gen_engine is None and tr._train_mode() == "eager"
    before = [tr.flat_g.param.clone(), tr.flat_d.param.clone()]
    for _ in range(2):
        out = tr.step(loc, vox)
        assert torch.isfinite(out["d_losses"]).all() and torch.isfinite(out["g_loss"]).all()
    assert not torch.equal(before[0], tr.flat_g.param) and not torch.equal(before[1], tr.flat_d.param)
    assert torch.isfinite(tr.flat_g.param).all() and torch.isfinite(tr.flat_d.param).all()
    for call in (tr.capture, tr.step_graphed, tr.step_fresh):
        with pytest.raises(ValueError, match="GATV2CONV"):
            call(loc, vox)
    states = tr.checkpoint_states(3, 0.5)
    tr2 = _trainer(cfg, seed=1)
    tr2.load_states(states)
    for name in ("generator", "discriminator"):
        a, b = getattr(tr, name).state_dict(), getattr(tr2, name).state_dict()
        assert list(a) == list(b) == list(states[name])
        assert any(k.endswith("lin_r.bias") for k in a) and any(k.endswith(".att") for k in a)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(tr.adam_d.exp_avg, tr2.adam_d.exp_avg) and torch.equal(tr.adam_g.exp_avg_sq, tr2.adam_g.exp_avg_sq)
    cfg16 = _cfg(True)
    cfg16.runtime["precision"] = "bf16"
    with pytest.raises(ValueError, match="GATV2CONV"):
        _trainer(cfg16)


def test_mixed_conv_types_step(cuda):
    """G = GATV2CONV on autograd, D = GATCONV on the critic engine."""
    from vgan.critic import CriticEngine

    cfg = _cfg(True, d_kind="GATCONV")
    cfg.N_CRITIC = 2
    _, (loc, vox) = batches_from_items(list(_items()))
    tr = _trainer(cfg)
    assert isinstance(tr.critic, CriticEngine) and tr.gen_engine is None and tr._train_mode() == "eager"
    out = tr.step(loc, vox)
    assert torch.isfinite(out["d_losses"]).all() and torch.isfinite(out["g_loss"]).all()


def test_gatv2_inference_sweep(cuda):
    from vgan.infer import InferenceSweep, geometric_taus
    from vgan.rng import RNG

    cfg = _cfg(True)
    torch.manual_seed(5)
    G = VoxelGNNGenerator(cfg, 17, 12)
    G.rng = RNG("device", seed=3)
    _, (loc, vox) = batches_from_items(list(_items()))
    taus = geometric_taus(1.0, 0.1, 3)
    sw = InferenceSweep(G, taus, dtype="f32")
    pred = sw.run_batch(loc, vox)
    assert tuple(pred.shape) == (3, vox.num_nodes) and pred.dtype == torch.int8
    assert int(pred.min()) >= 0 and int(pred.max()) < cfg.NUM_CLASSES
    res = sw.run([(loc, vox)], collect=True, select="f1")
    assert tuple(res["predictions"][0].shape) == (3, vox.num_nodes)
    sel = res["selected"][0]
    assert tuple(sel["labels"].shape) == (vox.num_nodes,) and sel["best"].numel() == vox.num_graphs
    with pytest.raises(ValueError, match="GATV2CONV"):
        InferenceSweep(G, taus, dtype="f16")
