"""Device-mode draws (vg_rng_fill, counter-based Philox): distribution moments,
fresh draws when the device counter advances, identical draws for the same
(seed, counter, salt), distinct streams per seed; and the exact values: the
uniform draws and the in-kernel dropout masks bit for bit against the host
Philox4x32-10 of tests/philox_ref.py (pinned to the published known-answer
vectors in tests/test_philox_ref_cpu.py), the exponential and normal draws
against float64 transforms of the same words."""
import numpy as np
import pytest
import torch

import philox_ref
from vgan.rng import RNG, DropSpec

pytestmark = pytest.mark.gpu


def test_moments(cuda):
    r = RNG("device", seed=1234)
    r.reset()
    z = r.normal((1 << 20,), cuda)
    u = r.uniform((1 << 20,), cuda)
    e = r.exponential((1 << 20,), cuda)
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1) < 5e-3
    assert float(u.min()) >= 0 and float(u.max()) < 1 and abs(float(u.mean()) - 0.5) < 2e-3
    assert float(e.min()) > 0 and abs(float(e.mean()) - 1) < 5e-3 and torch.isfinite(e).all()
    # odd sizes: every element written
    odd = r.normal((7, 3), cuda)
    assert torch.isfinite(odd).all() and odd.shape == (7, 3)


def test_exponential_strictly_positive(cuda):
    """The Gumbel noise g = -log(E) of the label head (models.py:150) is +inf
    at E = 0, and the label softmax NaN.  The device Exp(1) draw uses 23-bit
    midpoints u' = (x + 0.5) / 2^23: E in [2^-24, 16.7) for every draw.
    2^25 draws cover each 23-bit value ~4 times (the former -log(1 - u) with
    u = 0 returned 0 once per 2^24 draws: a NaN step every ~130 steps at 16
    buildings, tools/nan_probe.py)."""
    r = RNG("device", seed=77)
    lo, hi = float("inf"), 0.0
    for _ in range(4):
        r.reset()
        e = r.exponential((1 << 23,), cuda)
        lo, hi = min(lo, float(e.min())), max(hi, float(e.max()))
        assert torch.isfinite(e).all()
    assert lo >= 2.0 ** -24 * 0.99 and hi < 16.7, (lo, hi)


def test_counter_and_seed(cuda):
    a, b = RNG("device", seed=5), RNG("device", seed=5)
    a.reset()
    b.reset()
    x1, y1 = a.normal((1000,), cuda), b.normal((1000,), cuda)
    assert torch.equal(x1, y1)  # same seed, counter and salt
    a.reset()
    assert not torch.equal(a.normal((1000,), cuda), x1)  # counter advanced
    c = RNG("device", seed=6)
    c.reset()
    assert not torch.equal(c.normal((1000,), cuda), x1)  # another seed


@pytest.mark.parametrize("C", [1, 6, 64])
def test_inkernel_dropout_without_store(cuda, C):
    """GraphNorm + ReLU + in-kernel dropout (DropSpec) in a no-grad forward
    applies the same mask without storing it (vg_graphnorm_fwd_drop with
    keep_out NULL): y is bitwise the grad-mode y, whose stored mask has the
    Bernoulli(0.8) / 0.8 values."""
    from vgan import ops

    torch.manual_seed(C)
    n = 300
    x = torch.randn(n, C, device=cuda)
    w, b, ms = torch.rand(C, device=cuda) + 0.5, torch.randn(C, device=cuda), torch.rand(C, device=cuda)
    r = RNG("device", seed=9)
    r.reset()
    spec = r.keep_mask((n, C), 0.2, cuda)
    xg = x.clone().requires_grad_(True)
    y_grad = ops.graphnorm_relu_dropout(xg, w, b, ms, spec, 1e-5)
    with torch.no_grad():
        y_nograd = ops.graphnorm_relu_dropout(x, w, b, ms, spec, 1e-5)
    assert torch.equal(y_grad.detach(), y_nograd)
    keep = y_grad.grad_fn.saved_tensors[4]
    vals = set(torch.unique(keep).tolist())
    assert vals <= {0.0, 1.25} and 0.0 in vals and abs(float((keep > 0).float().mean()) - 0.8) < 0.08


SEED = 0x123456789ABCDEF0


def _fill(cuda, n, kind, seed, it, salt):
    from vgan._lib import LIB, check, ptr, stream_handle

    out = torch.full((n + 8,), -7.0, device=cuda)  # 8 guard elements behind the draw
    itt = torch.tensor([it], dtype=torch.int64, device=cuda)
    check(LIB.vg_rng_fill(ptr(out), n, kind, seed, ptr(itt), salt, stream_handle(cuda)), "vg_rng_fill")
    res = out.cpu().numpy()
    assert (res[n:] == -7.0).all(), "vg_rng_fill wrote past n"
    return res[:n]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025, 4 * 256 * 2048 + 5])
def test_uniform_is_philox4x32_10_bit_for_bit(cuda, n):
    """kind 1 = (w >> 8) * 2^-24 of the Philox words at counter (group, salt,
    iteration), key = seed; the last size is past the 2048-block grid, so the
    stride loop and the tail both run."""
    for it, salt in ((0, 0x40000001), (7, 3)):
        got = _fill(cuda, n, 1, SEED, it, salt)
        want = philox_ref.uniform(n, salt, it, SEED)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (n, it, salt, bad[:8], got[bad[:8]], want[bad[:8]])


def test_uniform_follows_every_counter_and_key_word(cuda):
    n, it, salt = 1025, 7, 3
    base = _fill(cuda, n, 1, SEED, it, salt)
    for seed2, it2, salt2 in ((SEED ^ 1, it, salt), (SEED ^ (1 << 32), it, salt), (SEED, it, salt + 1),
                              (SEED, it + 1, salt), (SEED, salt, it)):
        got = _fill(cuda, n, 1, seed2, it2, salt2)
        assert not np.array_equal(got, base), (hex(seed2), it2, salt2)
        assert np.array_equal(got, philox_ref.uniform(n, salt2, it2, seed2)), (hex(seed2), it2, salt2)


# max |got - ref| / max(1, |ref|) of the two transformed draws against their
# float64 restatement from the same Philox words: only the device's logf,
# sqrtf and sincosf and the float32 products differ.  Measured on the MI355X at
# n = 4099 (both counters / salts below): exponential 1.695e-7 and 1.673e-7,
# normal 1.560e-7 and 1.870e-7 (about 3 x 2^-24); the bounds are 4x the larger
# figure, rounded up, and must stay under 2^-20 = 9.54e-7.
EXP_BOUND = 7.0e-7
NRM_BOUND = 7.5e-7


def _rel(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize("it,salt", [(0, 0x40000001), (7, 3)])
def test_exponential_matches_f64_transform(cuda, it, salt):
    """kind 2 = -log(1 - ue), ue = ((w >> 9) + 0.5) * 2^-23 (1 - ue is exact in
    float32, so only logf differs from the float64 reference)."""
    n = 4099
    got = _fill(cuda, n, 2, SEED, it, salt)
    w = philox_ref.words(n, salt, it, SEED)
    ue = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    ref = -np.log(1.0 - ue)
    err = _rel(got, ref)
    print(f"exponential it {it} salt {salt:#x}: max rel err {err:.3e} ({err * 2 ** 24:.2f} x 2^-24)")
    assert EXP_BOUND <= 2.0 ** -20 and err <= EXP_BOUND


@pytest.mark.parametrize("it,salt", [(0, 0x40000001), (7, 3)])
def test_normal_matches_f64_box_muller(cuda, it, salt):
    """kind 0: per word pair (w0, w1) of a block, u1 = ((w0 >> 8) + 1) * 2^-24,
    angle = the float32 product 6.2831855f * ((w1 >> 8) * 2^-24); elements
    [r cos, r sin], r = sqrt(-2 log u1)."""
    n = 4099
    got = _fill(cuda, n, 0, SEED, it, salt)
    w = philox_ref.words(4 * ((n + 3) // 4), salt, it, SEED).reshape(-1, 2)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    ang = (np.float32(6.283185307179586) * u2).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    ref = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)[:n]
    err = _rel(got, ref)
    print(f"normal it {it} salt {salt:#x}: max rel err {err:.3e} ({err * 2 ** 24:.2f} x 2^-24)")
    assert NRM_BOUND <= 2.0 ** -20 and err <= NRM_BOUND


@pytest.mark.parametrize("shape", [(300, 1), (257, 3), (300, 6), (300, 64), (1000, 128)])
def test_inkernel_dropout_mask_is_philox_keep_mask(cuda, shape):
    """The mask vg_graphnorm_fwd_drop draws and stores (scalar and quad
    kernels, rows that straddle a 4-element Philox group) is the host
    reference's, element for element."""
    from vgan import ops

    n, C = shape
    torch.manual_seed(C)
    x = torch.randn(n, C, device=cuda, requires_grad=True)
    w, b, ms = torch.rand(C, device=cuda) + 0.5, torch.randn(C, device=cuda), torch.rand(C, device=cuda)
    seed, it, salt = SEED, 5, 11
    spec = DropSpec(0.2, seed, torch.tensor([it], dtype=torch.int64, device=cuda), salt, (n, C))
    y = ops.graphnorm_relu_dropout(x, w, b, ms, spec, 1e-5)
    keep = y.grad_fn.saved_tensors[4]
    want = torch.from_numpy(philox_ref.keep_mask((n, C), 0.2, salt, it, seed))
    assert keep.shape == want.shape
    assert torch.equal(keep.cpu(), want), int((keep.cpu() != want).sum())
