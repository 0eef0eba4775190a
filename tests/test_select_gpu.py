"""vg_sweep_select through ops.sweep_select on hand-made inputs (no model):
one launch scores k candidate labellings of every building, picks one per
building and gathers its labels.

One batch of buildings with 257, 0, 1, 63, 64, 700 and 40 rows (several block
strides, an empty building, a single row, a wave boundary minus one and on it,
256 + 1, and a building where no candidate hits a true label), copies in
{1, 3, 16} x classes in {3, 7}, plus copies = 16 at 32 classes: the largest
shape the ABI admits (exactly 64 KB of LDS counters).  Some candidates are
exact duplicates of others (ties), a few truth values are -1 and K, a few
predictions -1.

Bounds (derived, not measured):
* conf, far_ref, best, labels: exact.
* f1 against metrics.scores: 1e-12.  The counts are exact in f64; each label
  costs one rounded division and the mean at most K + 1 more roundings on
  values <= 1: below 1e-14 for K <= 32.
* far_gen against a float64 evaluation of the same formula on the stored f32
  values: relative (rows + 8) 2^-24 -- three roundings per term (two scalings
  and the product), at most `rows` more for a sum of non-negative terms in any
  order, one for the division; contraction only lowers it.
"""
import functools

import numpy as np
import pytest
import torch

from vgan import metrics, ops

pytestmark = pytest.mark.gpu

SIZES = (257, 0, 1, 63, 64, 700, 40)
EMPTY, ZERO = 1, 6  # the empty building; the building whose every F1 is 0
CASES = [(1, 3), (3, 3), (16, 3), (1, 7), (3, 7), (16, 7), (16, 32)]


@functools.lru_cache(maxsize=None)
def _case(copies, K):
    """Seeded inputs and their host reference (numpy; built once per shape, never modified)."""
    rng = np.random.default_rng(1000 * copies + K)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n, g = int(ptr[-1]), len(SIZES)
    batch = np.repeat(np.arange(g), SIZES)
    truth = rng.integers(0, K, n).astype(np.int64)
    pred = np.where(rng.random((copies, n)) < 0.5, truth[None, :], rng.integers(0, K, (copies, n))).astype(np.int8)
    lo, hi = ptr[ZERO], ptr[ZERO + 1]
    truth[lo:hi] = 0
    pred[:, lo:hi] = rng.integers(1, K, (copies, hi - lo))
    for b in (0, 5):  # rows out of range, in the 257- and the 700-row building
        rows = ptr[b] + rng.choice(SIZES[b], 9, replace=False)
        truth[rows[:3]] = -1
        truth[rows[3:6]] = K
        pred[rng.integers(0, copies, 3), rows[6:]] = -1
        pred[0, rows[0]] = -1  # both out of range in one row
    if copies >= 3:
        pred[2] = pred[0]
    if copies >= 16:
        pred[5] = pred[1]
        pred[9] = pred[1]
        pred[0] = pred[12]  # the duplicate of LOWER index must win
        pred[2] = pred[0]
    x = rng.uniform(-1.0, 1.0, (n, 12)).astype(np.float32)
    x[:, 3:6] = rng.uniform(0.2, 0.6, (n, 3)).astype(np.float32)
    x[:, 9] = np.repeat(rng.uniform(0.5, 4.0, g), SIZES).astype(np.float32)
    site = np.repeat(np.array([400.0, 537.37, 1024.0, 333.3, 900.0, 1211.125, 625.0], dtype=np.float32), SIZES)
    void = K - 1

    t_ok = (truth >= 0) & (truth < K)
    conf = np.zeros((copies, g, K, K), dtype=np.int64)
    far = np.zeros((copies, g), dtype=np.float64)
    area = (x[:, 4].astype(np.float64) * 11.0) * (x[:, 5].astype(np.float64) * 11.0)
    for c in range(copies):
        p = pred[c].astype(np.int64)
        p_ok = (p >= 0) & (p < K)
        m = t_ok & p_ok
        conf[c] = np.bincount((batch[m] * K + truth[m]) * K + p[m], minlength=g * K * K).reshape(g, K, K)
        solid = p_ok & (p != void)
        far[c] = np.bincount(batch[solid], weights=area[solid], minlength=g)
    f1 = np.array([[metrics.scores(conf[c, b])[0] for b in range(g)] for c in range(copies)])
    far_ref = np.zeros(g, dtype=np.float32)
    for b in range(g):
        if SIZES[b]:
            far[:, b] /= np.float64(site[ptr[b]])
            far_ref[b] = x[ptr[b], 9]
    return dict(copies=copies, K=K, n=n, g=g, ptr=ptr, batch=batch, truth=truth, pred=pred, x=x, site=site,
                void=void, conf=conf, f1=f1, far=far, far_ref=far_ref)


def _dev(case, cuda):
    return {k: torch.from_numpy(case[k]).to(cuda) for k in ("ptr", "truth", "pred", "x", "site")}


def _select(case, d, criterion, truth=True, pred=None):
    return ops.sweep_select(d["pred"] if pred is None else pred, d["ptr"], d["x"], d["site"],
                            truth=d["truth"] if truth else None, criterion=criterion, void_class=case["void"],
                            classes=case["K"])


def _check(case, sel, criterion, truth=True):
    copies, K, g, ptr = case["copies"], case["K"], case["g"], case["ptr"]
    labels, best = sel.labels.cpu().numpy(), sel.best.cpu().numpy()
    far_gen, far_ref = sel.far_gen.cpu().numpy(), sel.far_ref.cpu().numpy()
    assert labels.dtype == np.int8 and best.dtype == np.int32 and far_gen.dtype == np.float32
    assert far_gen.shape == (copies, g) and far_ref.shape == (g,) and best.shape == (g,)
    if truth:
        conf, f1 = sel.conf.cpu().numpy(), sel.f1.cpu().numpy()
        assert conf.dtype == np.int32 and f1.dtype == np.float64 and f1.shape == (copies, g)
        assert np.array_equal(conf, case["conf"])
        err = np.abs(f1 - case["f1"]).max()
        print(f"copies {copies} K {K} {criterion}: max |f1 - scores| = {err:.3e}")
        assert err <= 1e-12
        assert np.all(f1[:, ZERO] == 0.0) and np.all(f1[:, EMPTY] == 0.0)
    else:
        assert sel.conf is None and sel.f1 is None
    assert far_ref.tobytes() == case["far_ref"].tobytes()
    for b in range(g):
        bound = (SIZES[b] + 8) * 2.0 ** -24
        rel = np.abs(far_gen[:, b].astype(np.float64) - case["far"][:, b]) / np.maximum(case["far"][:, b], 1e-300)
        rel = np.where(case["far"][:, b] == 0, np.where(far_gen[:, b] == 0, 0.0, np.inf), rel)
        print(f"  building {b} ({SIZES[b]} rows): far_gen rel err {rel.max():.3e} (bound {bound:.3e})")
        assert rel.max() <= bound, (b, rel.max(), bound)
    assert np.all(far_gen[:, EMPTY] == 0.0) and far_ref[EMPTY] == 0.0
    if criterion == "f1":
        assert np.array_equal(best, np.argmax(f1, axis=0))  # first arg-max of the device's own scores
        host_best = case["f1"].max(axis=0)
        chosen = case["f1"][best, np.arange(g)]
        assert np.all(host_best - chosen <= 1e-12), (host_best - chosen).max()
        assert best[ZERO] == 0 and best[EMPTY] == 0
    else:
        diff = np.abs(far_gen - far_ref[None, :])  # f32, as on the device
        assert diff.dtype == np.float32
        assert np.array_equal(best, np.argmin(diff, axis=0))
        assert best[EMPTY] == 0
    assert np.array_equal(labels, case["pred"][best[case["batch"]], np.arange(case["n"])])
    if copies >= 3:  # candidate 2 duplicates candidate 0: never chosen
        assert not np.any(best == 2)
    if copies >= 16:
        assert not np.any(np.isin(best, (5, 9, 12)))


def _same(a, b):
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert u.dtype == v.dtype and torch.equal(u, v)


@pytest.mark.parametrize("copies,K", CASES)
def test_select_f1(cuda, copies, K):
    case = _case(copies, K)
    d = _dev(case, cuda)
    sel = _select(case, d, "f1")
    _check(case, sel, "f1")
    _same(sel, _select(case, d, "f1"))  # deterministic: bit-identical on a second call


@pytest.mark.parametrize("copies,K", CASES)
def test_select_far_with_and_without_truth(cuda, copies, K):
    case = _case(copies, K)
    d = _dev(case, cuda)
    with_t = _select(case, d, "far")
    _check(case, with_t, "far")
    without = _select(case, d, "far", truth=False)
    _check(case, without, "far", truth=False)
    for k in ("labels", "best", "far_gen", "far_ref"):
        assert torch.equal(getattr(with_t, k), getattr(without, k)), k
    _same(without, _select(case, d, "far", truth=False))


@pytest.mark.parametrize("copies,K", [(3, 7), (16, 3)])
@pytest.mark.parametrize("pad,offset", [(13, 3), (16, 0), (6, 1)])
def test_select_strided_candidates_equal_contiguous(cuda, copies, K, pad, offset):
    """pred as a view of a wider buffer (copy_stride > N; rows that start at
    every alignment, strides that are and are not a multiple of 4)."""
    case = _case(copies, K)
    d = _dev(case, cuda)
    n = case["n"]
    buf = torch.full((copies, n + pad), 1, dtype=torch.int8, device=cuda)
    view = buf[:, offset:offset + n]
    view.copy_(d["pred"])
    assert view.stride(0) == n + pad > n
    for criterion in ("f1", "far"):
        _same(_select(case, d, criterion, pred=view), _select(case, d, criterion))


@pytest.mark.parametrize("copies,K", CASES)
def test_conf_equals_ops_confusion_for_in_range_predictions(cuda, copies, K):
    """With every prediction in [0, K) the counts are those of vg_confusion
    on the one-hot of each candidate (truth outside [0, K) left out by both)."""
    case = _case(copies, K)
    d = _dev(case, cuda)
    pred = d["pred"].clamp(min=0)
    sel = _select(case, d, "f1", pred=pred)
    for c in range(copies):
        onehot = torch.nn.functional.one_hot(pred[c].long(), K).float()
        assert torch.equal(sel.conf[c], ops.confusion(d["truth"], onehot, d["ptr"])[0]), c


def test_select_refuses_what_the_abi_refuses(cuda):
    case = _case(3, 7)
    d = _dev(case, cuda)
    with pytest.raises(ValueError, match="true types"):
        _select(case, d, "f1", truth=False)
    with pytest.raises(ValueError, match="int8"):
        _select(case, d, "f1", pred=d["pred"].int())
    wide = torch.zeros(65, case["n"], dtype=torch.int8, device=cuda)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _select(case, d, "f1", pred=wide)
