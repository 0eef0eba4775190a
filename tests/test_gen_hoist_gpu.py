"""The generator iteration's forward run as the last copy of the stacked
critic-label forward (vg_gen_forward_stacked + vg_gen_loss_and_grad_from,
DESIGN.md 4.52) against the step that runs the two forwards separately
(genstep._HOIST = False): labels of every copy, the generator loss, its labels
and every gradient, and whole steps' losses and parameters are BIT-IDENTICAL;
the hand-over is single-use and dropped by anything but exactly N_CRITIC
critic iterations on the same batch."""
import pytest
import torch

from test_gen_engine_gpu import _trainer
from vgan import genstep
from vgan.synth import SyntheticDataset

pytestmark = pytest.mark.gpu

BATCHES = [(4, 41), (8, 9)]  # (buildings, seed); the second has an odd node count


def _batch(cuda, batch, seed):
    loc, vox = SyntheticDataset(batch, seed=seed).batch(range(batch))
    return loc.to(cuda), vox.to(cuda)


def _with(monkeypatch, hoist: bool, fn):
    monkeypatch.setattr(genstep, "_HOIST", hoist)
    return fn()


def _count(tr, name):
    return tr.gen_engine.__dict__.get(name, 0)


def test_some_batch_has_odd_rows():
    assert any(SyntheticDataset(b, seed=s).batch(range(b))[1].num_nodes % 2 for b, s in BATCHES)


@pytest.mark.parametrize("batch,seed", BATCHES)
def test_label_forward_and_iteration_bit_identical(cuda, monkeypatch, batch, seed):
    loc, vox = _batch(cuda, batch, seed)
    a, b = _trainer(cuda), _trainer(cuda)
    k = a.configuration.N_CRITIC
    for it in range(2):  # the second from the advanced counter, gradients accumulating
        outs = []
        for tr, hoist in ((a, True), (b, False)):
            def one():
                hard, soft = tr._critic_labels(loc, vox)
                for _ in range(k):  # the critic iterations' counter advances (their work does not touch G)
                    tr._iter_begin(tr.adam_d)
                g_loss, label = tr._gen_iteration(loc, vox)
                return hard.clone(), soft.clone(), g_loss.detach().clone(), label.detach().clone(), \
                    tr.flat_g.grad.clone()
            outs.append(_with(monkeypatch, hoist, one))
        torch.cuda.synchronize()
        names = ("label copies hard", "label copies soft", "g_loss", "label_hard", "flat_g.grad")
        for name, x, y in zip(names, *outs):
            print(f"batch {batch} n {vox.num_nodes} iteration {it} {name}: max |diff| "
                  f"{float((x.float() - y.float()).abs().max()):.3e}")
        for name, x, y in zip(names, *outs):
            assert x.shape == y.shape and torch.equal(x, y), (it, name)
        assert outs[0][0].shape[0] == k
    assert _count(a, "hoisted_forwards") == 2 and _count(a, "hoisted_calls") == 2 and _count(a, "native_calls") == 2
    assert _count(b, "hoisted_forwards") == 0 and _count(b, "hoisted_calls") == 0 and _count(b, "native_calls") == 2


@pytest.mark.parametrize("mode", ["step", "step_fresh", "step_graphed"])
def test_whole_steps_bit_identical(cuda, monkeypatch, mode):
    loc, vox = _batch(cuda, 8, 9)
    a, b = _trainer(cuda), _trainer(cuda)
    if mode == "step_graphed":  # the arenas sized outside any capture
        _with(monkeypatch, True, lambda: a.step(loc, vox))
        _with(monkeypatch, False, lambda: b.step(loc, vox))
    before = _count(a, "hoisted_calls")
    for i in range(3):
        oa = _with(monkeypatch, True, lambda: getattr(a, mode)(loc, vox))
        ob = _with(monkeypatch, False, lambda: getattr(b, mode)(loc, vox))
        torch.cuda.synchronize()
        for key in ("d_losses", "g_loss", "label_hard"):
            assert torch.equal(oa[key], ob[key]), (mode, i, key)
        assert torch.equal(a.flat_g.param, b.flat_g.param), (mode, i)
        assert torch.equal(a.flat_d.param, b.flat_d.param), (mode, i)
    assert _count(a, "hoisted_calls") > before  # (step_graphed: recorded inside the capture)
    assert _count(b, "hoisted_calls") == 0
    if mode != "step_graphed":
        assert _count(a, "hoisted_calls") - before == 3


def _reference_iteration(cuda, monkeypatch, loc, vox, extra_begins=0, warm=None):
    """(g_loss, label_hard, grad) of the unhoisted trainer after the same calls."""
    b = _trainer(cuda)

    def one():
        if warm is not None:
            b._critic_labels(*warm)
        else:
            b._critic_labels(loc, vox)
        for _ in range(b.configuration.N_CRITIC + extra_begins):
            b._iter_begin(b.adam_d)
        g_loss, label = b._gen_iteration(loc, vox)
        return g_loss.detach().clone(), label.detach().clone(), b.flat_g.grad.clone()
    return _with(monkeypatch, False, one)


def test_direct_iteration_takes_the_whole_path(cuda, monkeypatch):
    loc, vox = _batch(cuda, 4, 41)
    a, b = _trainer(cuda), _trainer(cuda)
    ga, ha = _with(monkeypatch, True, lambda: a._gen_iteration(loc, vox))
    gb, hb = _with(monkeypatch, False, lambda: b._gen_iteration(loc, vox))
    torch.cuda.synchronize()
    assert torch.equal(ga, gb) and torch.equal(ha, hb) and torch.equal(a.flat_g.grad, b.flat_g.grad)
    assert _count(a, "native_calls") == 1 and _count(a, "hoisted_calls") == 0


def test_extra_iteration_drops_the_state(cuda, monkeypatch):
    loc, vox = _batch(cuda, 4, 41)
    a = _trainer(cuda)

    def one():
        a._critic_labels(loc, vox)
        for _ in range(a.configuration.N_CRITIC + 1):  # one more than the hoisted draws assumed
            a._iter_begin(a.adam_d)
        g_loss, label = a._gen_iteration(loc, vox)
        return g_loss.detach().clone(), label.detach().clone(), a.flat_g.grad.clone()
    got = _with(monkeypatch, True, one)
    ref = _reference_iteration(cuda, monkeypatch, loc, vox, extra_begins=1)
    torch.cuda.synchronize()
    assert _count(a, "hoisted_forwards") == 1 and _count(a, "hoisted_calls") == 0 and _count(a, "native_calls") == 1
    assert all(torch.equal(x, y) for x, y in zip(got, ref))


def test_other_batch_drops_the_state(cuda, monkeypatch):
    loc, vox = _batch(cuda, 4, 41)
    loc2, vox2 = _batch(cuda, 4, 6)
    a = _trainer(cuda)

    def one():
        a._critic_labels(loc2, vox2)
        for _ in range(a.configuration.N_CRITIC):
            a._iter_begin(a.adam_d)
        g_loss, label = a._gen_iteration(loc, vox)
        return g_loss.detach().clone(), label.detach().clone(), a.flat_g.grad.clone()
    got = _with(monkeypatch, True, one)
    ref = _reference_iteration(cuda, monkeypatch, loc, vox, warm=(loc2, vox2))
    torch.cuda.synchronize()
    assert _count(a, "hoisted_forwards") == 1 and _count(a, "hoisted_calls") == 0 and _count(a, "native_calls") == 1
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    assert a.__dict__.get("_hoist") is None and a.gen_engine.__dict__.get("_hoist") is None


def test_gating_forced_false_runs_the_old_path(cuda, monkeypatch):
    """An aggregation whose kernel form would differ between n and the
    stacked row counts (here: a row threshold patched below them) keeps the
    label forward and the generator iteration separate."""
    from vgan import _lib

    loc, vox = _batch(cuda, 4, 41)
    a, b = _trainer(cuda), _trainer(cuda)
    n = vox.num_nodes
    real = _lib.LIB.vg_gat_gnp_rows

    class Patched:
        def __getattr__(self, name):
            if name == "vg_gat_gnp_rows":  # another partial-block size above n rows, as past the slice threshold
                return lambda rows, c: int(real(rows, c)) * (2 if rows > n else 1)
            return getattr(_lib.LIB, name)
    monkeypatch.setattr(genstep, "LIB", Patched())
    oa = _with(monkeypatch, True, lambda: a.step(loc, vox))
    monkeypatch.setattr(genstep, "LIB", _lib.LIB)
    ob = _with(monkeypatch, False, lambda: b.step(loc, vox))
    torch.cuda.synchronize()
    assert _count(a, "hoisted_forwards") == 0 and _count(a, "hoisted_calls") == 0 and _count(a, "native_calls") == 1
    for key in ("d_losses", "g_loss", "label_hard"):
        assert torch.equal(oa[key], ob[key]), key
    assert torch.equal(a.flat_g.param, b.flat_g.param)
