"""Kernel-level pieces of the hoisted generator forward.

A tail segment of a stacked launch draws its dropout under a second key --
(seed, counter + delta, tail salt) at the element index relative to the first
tail row -- and stores its multipliers (and, in vg_gat_lin_att_gn, its
GraphNorm output) to buffers of its own: exactly what a launch over the tail
rows alone would draw and store once the counter has advanced by delta.  The
rows before the tail are those of the plain call.  Likewise vg_rng_fill_at
(the fill a later iteration will make) and vg_gemm_ln_act_from (the backward
state of the rows from a first row on).

Everything is compared with torch.equal: the claim is bit identity.  Shapes:
3 segments of 97 rows, the tail the last one (odd rows; odd first-tail-row x C
products at C = 1), widths that take the scalar (C = 1, 2), quad and
one-launch-fold GraphNorm forms."""
from __future__ import annotations

import ctypes

import pytest
import torch

from vgan import ops
from vgan._lib import LIB, VgDrawTail, VgGnApply, check, ptr

pytestmark = pytest.mark.gpu

EPS = 1e-5
SEG, S = 97, 3
ROW0 = SEG * (S - 1)
V, DELTA = 11, 6  # the device counter, and the advance before the tail's own iteration
SEED, SALT, TSALT, P = 1234, 77, 91, 0.2
PAD = 8  # rows past the tail buffers' end that must stay untouched

_NAN = float("nan")


def _nan(*shape, dev):
    return torch.full(shape, _NAN, dtype=torch.float32, device=dev)


def _same(a, b):
    return torch.equal(a, b)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _counters(dev):
    return (torch.tensor([V], dtype=torch.int64, device=dev),
            torch.tensor([V + DELTA], dtype=torch.int64, device=dev))


def _gn_params(C, dev):
    return (1 + 0.2 * torch.randn(C, device=dev), 0.2 * torch.randn(C, device=dev),
            1 + 0.2 * torch.randn(C, device=dev))


def _tail(keep, y=None):
    return VgDrawTail(row0=ROW0, salt=TSALT, iter_delta=DELTA, keep=keep.data_ptr(),
                      y=y.data_ptr() if y is not None else None)


def _check_tail_call(C, y, keep_out, tkeep, stats, full, tail_ref):
    """y / keep_out / tkeep of the call with a tail against the plain call over
    all rows (``full``: y, keep, stats) and the plain call over the tail rows
    with the tail's key (``tail_ref``: y, keep, stats)."""
    y_f, k_f, st_f = full
    y_t, k_t, st_t = tail_ref
    assert _same(y[:ROW0], y_f[:ROW0]) and _same(keep_out[:ROW0], k_f[:ROW0])
    assert _same(y[ROW0:], y_t) and _same(tkeep[:SEG], k_t)
    assert _all_nan(keep_out[ROW0:]) and _all_nan(tkeep[SEG:])
    assert _same(stats, st_f) and _same(stats[2 * C * (S - 1):], st_t)
    assert not _same(k_t, k_f[ROW0:])  # the tail really draws under another key
    assert 0.05 < (k_t == 0).float().mean().item() < 0.4 or C * SEG < 200


@pytest.mark.parametrize("C", [1, 2, 4, 16, 64])
def test_graphnorm_drop_tail(cuda, C):
    torch.manual_seed(C)
    dev, st = cuda, ops.stream_handle(cuda)
    x = torch.randn(S * SEG, C, device=dev)
    w, b, ms = _gn_params(C, dev)
    it, it_d = _counters(dev)
    ws = torch.empty(int(LIB.vg_graphnorm_seg_ws_floats(S, SEG, C)), device=dev)

    def plain(xx, segs, counter, salt):
        y, k, s_ = torch.empty_like(xx), torch.empty_like(xx), torch.empty(segs * 2 * C, device=dev)
        check(LIB.vg_graphnorm_fwd_drop(ptr(xx), segs, SEG, C, ptr(w), ptr(b), ptr(ms), P, SEED, ptr(counter), salt,
                                        EPS, ptr(y), ptr(k), ptr(s_), ptr(ws), None, st), "vg_graphnorm_fwd_drop")
        return y, k, s_

    full = plain(x, S, it, SALT)
    tail_ref = plain(x[ROW0:].clone(), 1, it_d, TSALT)
    y, keep_out, tkeep = torch.empty_like(x), _nan(S * SEG, C, dev=dev), _nan(SEG + PAD, C, dev=dev)
    stats = torch.empty(S * 2 * C, device=dev)
    tail = _tail(tkeep)
    check(LIB.vg_graphnorm_fwd_drop_tail(ptr(x), S, SEG, C, ptr(w), ptr(b), ptr(ms), P, SEED, ptr(it), SALT, EPS,
                                         ptr(y), ptr(keep_out), ptr(stats), ptr(ws), ctypes.byref(tail), st),
          "vg_graphnorm_fwd_drop_tail")
    torch.cuda.synchronize()
    _check_tail_call(C, y, keep_out, tkeep, stats, full, tail_ref)
    # no tail (NULL, or row0 = 0): the plain call
    for t in (None, ctypes.byref(VgDrawTail())):
        y0, k0 = torch.empty_like(x), torch.empty_like(x)
        check(LIB.vg_graphnorm_fwd_drop_tail(ptr(x), S, SEG, C, ptr(w), ptr(b), ptr(ms), P, SEED, ptr(it), SALT, EPS,
                                             ptr(y0), ptr(k0), ptr(stats), ptr(ws), t, st), "vg_graphnorm_fwd_drop_tail")
        assert _same(y0, full[0]) and _same(k0, full[1])


def _ring_graph(dev):
    """97 nodes, each with a few random neighbours (both directions)."""
    g = torch.Generator().manual_seed(5)
    src = torch.arange(SEG).repeat(3)
    dst = (src + torch.randint(1, SEG, (3 * SEG,), generator=g)) % SEG
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    csr = ops.CSR(ei.to(dev), SEG)
    csr.ell()
    return csr


@pytest.mark.parametrize("C", [1, 2, 4, 16, 64])
def test_graphnorm_gnp_tail(cuda, C):
    """The same through the aggregation's partials (vg_graphnorm_fwd_gnp): the
    stacked launch's last segment against an aggregation + GraphNorm over that
    copy alone -- the hand-over the hoisted forward relies on."""
    torch.manual_seed(100 + C)
    dev, st = cuda, ops.stream_handle(cuda)
    csr1 = _ring_graph(dev)
    csr = csr1.stacked(S)
    h = torch.randn(S * SEG, C, device=dev)
    a_s, a_d = 0.5 * torch.randn(S * SEG, device=dev), 0.5 * torch.randn(S * SEG, device=dev)
    bias = torch.randn(C, device=dev)
    w, b, ms = _gn_params(C, dev)
    it, it_d = _counters(dev)

    def aggregate(c_, hh, s1, s2):
        gnp, g = ops.gnp_buffer(c_, C, dev)
        assert gnp is not None
        out, alpha = torch.empty_like(hh), torch.empty(c_.num_edges, device=dev)
        ops.aggregate_fwd_raw(c_, C, ptr(hh), ptr(s1), ptr(s2), ptr(bias), 0.2, ptr(out), ptr(alpha), st, gnp)
        return out, alpha, gnp, g

    out, alpha, gnp, g = aggregate(csr, h, a_s, a_d)
    out1, alpha1, gnp1, g1 = aggregate(csr1, h[ROW0:].clone(), a_s[ROW0:].clone(), a_d[ROW0:].clone())
    assert g == g1 and _same(out[ROW0:], out1) and _same(alpha[csr1.num_edges * (S - 1):], alpha1)

    def plain(xx, segs, counter, salt, parts):
        y, k, s_ = torch.empty_like(xx), torch.empty_like(xx), torch.empty(segs * 2 * C, device=dev)
        check(LIB.vg_graphnorm_fwd_gnp(ptr(xx), segs, SEG, C, ptr(w), ptr(b), ptr(ms), None, P, SEED, ptr(counter),
                                       salt, EPS, ptr(y), ptr(k), ptr(s_), ptr(parts), g, st), "vg_graphnorm_fwd_gnp")
        return y, k, s_

    full = plain(out, S, it, SALT, gnp)
    tail_ref = plain(out1, 1, it_d, TSALT, gnp1)
    y, keep_out, tkeep = torch.empty_like(out), _nan(S * SEG, C, dev=dev), _nan(SEG + PAD, C, dev=dev)
    stats = torch.empty(S * 2 * C, device=dev)
    tail = _tail(tkeep)
    check(LIB.vg_graphnorm_fwd_gnp_tail(ptr(out), S, SEG, C, ptr(w), ptr(b), ptr(ms), P, SEED, ptr(it), SALT, EPS,
                                        ptr(y), ptr(keep_out), ptr(stats), ptr(gnp), g, ctypes.byref(tail), st),
          "vg_graphnorm_fwd_gnp_tail")
    torch.cuda.synchronize()
    _check_tail_call(C, y, keep_out, tkeep, stats, full, tail_ref)


@pytest.mark.parametrize("cin,C", [(8, 16), (16, 32)])
def test_lin_att_gn_tail(cuda, cin, C):
    """vg_gat_lin_att_gn with a tail: H / a_src / a_dst of every row, y and
    keep of the tail rows only, in the tail's buffers."""
    torch.manual_seed(cin)
    dev, st = cuda, ops.stream_handle(cuda)
    n = S * SEG
    x = torch.randn(n, cin, device=dev)
    W = torch.randn(C, cin, device=dev) / cin ** 0.5
    att_s, att_d = torch.randn(C, device=dev), torch.randn(C, device=dev)
    w, b, ms = _gn_params(cin, dev)
    it, it_d = _counters(dev)
    ws = torch.empty(int(LIB.vg_graphnorm_seg_ws_floats(S, SEG, cin)), device=dev)
    stats = torch.empty(S * 2 * cin, device=dev)
    check(LIB.vg_graphnorm_stats(ptr(x), S, SEG, cin, ptr(ms), EPS, ptr(stats), ptr(ws), st), "vg_graphnorm_stats")

    def call(xx, rows, stats_, counter, salt, y, keep_out, tail=None):
        H = torch.empty(rows, C, device=dev)
        a1, a2 = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        d = VgGnApply(stats=stats_.data_ptr(), weight=w.data_ptr(), bias=b.data_ptr(), mean_scale=ms.data_ptr(),
                      keep=None, eps=EPS, p_drop=P, seg_rows=SEG, salt=salt, seed=SEED, iter=counter.data_ptr(),
                      y=y.data_ptr(), keep_out=keep_out.data_ptr())
        if tail is not None:
            d.tail = tail
        check(LIB.vg_gat_lin_att_gn(ptr(xx), ptr(W), rows, cin, C, ptr(att_s), ptr(att_d), ptr(H), ptr(a1), ptr(a2),
                                    ctypes.byref(d), st), "vg_gat_lin_att_gn")
        return H, a1, a2

    y_f, k_f = torch.empty_like(x), torch.empty_like(x)
    H_f, as_f, ad_f = call(x, n, stats, it, SALT, y_f, k_f)
    xt = x[ROW0:].clone()
    y_t, k_t = torch.empty_like(xt), torch.empty_like(xt)
    H_t, as_t, ad_t = call(xt, SEG, stats[2 * cin * (S - 1):].clone(), it_d, TSALT, y_t, k_t)

    y, keep_out = _nan(n, cin, dev=dev), _nan(n, cin, dev=dev)
    ty, tkeep = _nan(SEG + PAD, cin, dev=dev), _nan(SEG + PAD, cin, dev=dev)
    H, a1, a2 = call(x, n, stats, it, SALT, y, keep_out, _tail(tkeep, ty))
    torch.cuda.synchronize()
    assert _same(H[:ROW0], H_f[:ROW0]) and _same(a1[:ROW0], as_f[:ROW0]) and _same(a2[:ROW0], ad_f[:ROW0])
    assert _same(H[ROW0:], H_t) and _same(a1[ROW0:], as_t) and _same(a2[ROW0:], ad_t)
    assert _same(y[:ROW0], y_f[:ROW0]) and _same(keep_out[:ROW0], k_f[:ROW0])
    assert _all_nan(y[ROW0:]) and _all_nan(keep_out[ROW0:])
    assert _same(ty[:SEG], y_t) and _same(tkeep[:SEG], k_t)
    assert _all_nan(ty[SEG:]) and _all_nan(tkeep[SEG:])
    assert not _same(k_t, k_f[ROW0:])


@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("n", [1, 5, 4 * 97 + 3])
def test_rng_fill_at(cuda, kind, n):
    """Delta d at counter v draws what delta 0 draws at counter v + d."""
    dev, st = cuda, ops.stream_handle(cuda)
    it, it_d = _counters(dev)
    a, b, c = _nan(n + PAD, dev=dev), _nan(n, dev=dev), _nan(n, dev=dev)
    check(LIB.vg_rng_fill_at(ptr(a), n, kind, SEED, ptr(it), DELTA, 0x40000003, st), "vg_rng_fill_at")
    check(LIB.vg_rng_fill_at(ptr(b), n, kind, SEED, ptr(it_d), 0, 0x40000003, st), "vg_rng_fill_at")
    check(LIB.vg_rng_fill(ptr(c), n, kind, SEED, ptr(it_d), 0x40000003, st), "vg_rng_fill")
    torch.cuda.synchronize()
    assert _same(a[:n], b) and _same(b, c) and _all_nan(a[n:]) and bool(torch.isfinite(b).all())
    d = _nan(n, dev=dev)
    check(LIB.vg_rng_fill(ptr(d), n, kind, SEED, ptr(it), 0x40000003, st), "vg_rng_fill")
    assert not _same(d, c)


@pytest.mark.parametrize("K,M", [(128, 128), (128, 32)])
def test_gemm_ln_act_from(cuda, K, M):
    """Y of every row; H / mean / rstd of the rows from the first state row on,
    in buffers of that many rows."""
    torch.manual_seed(M)
    dev, st = cuda, ops.stream_handle(cuda)
    n = S * SEG
    x = torch.randn(n, K, device=dev)
    W, bias = torch.randn(M, K, device=dev) / K ** 0.5, 0.1 * torch.randn(M, device=dev)
    gamma, beta = 1 + 0.1 * torch.randn(M, device=dev), 0.1 * torch.randn(M, device=dev)

    def plain(xx, rows):
        H, Y = torch.empty(rows, M, device=dev), torch.empty(rows, M, device=dev)
        mu, rs = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        check(LIB.vg_gemm_ln_act(ptr(xx), K, ptr(W), rows, M, K, ptr(bias), ptr(gamma), ptr(beta), EPS, 0.2, ptr(H),
                                 ptr(Y), ptr(mu), ptr(rs), st), "vg_gemm_ln_act")
        return H, Y, mu, rs

    H_f, Y_f, mu_f, rs_f = plain(x, n)
    H_t, Y_t, mu_t, rs_t = plain(x[ROW0:].clone(), SEG)
    # one buffer each, NaN before the state's first element and after its last: neither is written
    Hb, mub, rsb = _nan(PAD + SEG + PAD, M, dev=dev), _nan(PAD + SEG + PAD, dev=dev), _nan(PAD + SEG + PAD, dev=dev)
    Y = torch.empty(n, M, device=dev)
    check(LIB.vg_gemm_ln_act_from(ptr(x), K, ptr(W), n, M, K, ptr(bias), ptr(gamma), ptr(beta), EPS, 0.2, ROW0,
                                  ptr(Hb[PAD:]), ptr(Y), ptr(mub[PAD:]), ptr(rsb[PAD:]), st), "vg_gemm_ln_act_from")
    torch.cuda.synchronize()
    assert _same(Y, Y_f) and _same(Y[ROW0:], Y_t)
    for got, full, tail in ((Hb, H_f, H_t), (mub, mu_f, mu_t), (rsb, rs_f, rs_t)):
        assert _same(got[PAD:PAD + SEG], tail) and _same(got[PAD:PAD + SEG], full[ROW0:])
        assert _all_nan(got[:PAD]) and _all_nan(got[PAD + SEG:])
