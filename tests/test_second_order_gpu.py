"""The critic's second-order GAT and GraphNorm kernels, and the sparse
primitives of the autograd fallback, off the default widths and graphs.

Every kernel is compared with torch autograd on the oracle's ops in float64
on the CPU (tests/critic_ref.py units), at the widths that select every
instantiation of VG_DISPATCH_JVP / VG_DISPATCH, on a hub graph whose row 0 and
CSC column 0 hold 302 entries (302 is no multiple of 4, 8, 16 or 32: every
strided edge loop and every 4-edge batch ends on a remainder), on degenerate
graphs, at the leaky-ReLU kink, and past the 4096-workgroup grid cap.

Inputs are drawn in float64 and rounded to float32 before either side sees
them, so the figures below are the kernels' own error.  GraphNorm inputs are
nudged so that no pre-activation z lies within 1e-4 of 0: the ReLU mask is
discontinuous there, and at 4 * 10^6 elements a float32 z would otherwise
land on the other side of it in some run.

Bounds (max |got - ref| / max |ref|, test_critic_gpu._close):
  * kernels against float64: 2e-5, the bound test_critic_gpu.py uses for the
    same kernels.  No case came near it, C = 256 on the 302-entry row
    included, so no case takes a bound of its own.
  * sparse primitives: rel_err < 1e-5 (test_ops_gpu.py's forward tolerance);
    seg_max and gather exactly.
  * the autograd fallback's double backward: 1e-4 |ref| + 1e-7 scale
    (test_ops_gpu.test_gat_conv_double_backward's criterion).

Worst errors observed on an MI355X, per family (every test prints its own):
  vg_gat_jvp2, hub graph                 1.0e-6 (g_att_src, C = 18); bound 2e-5
  vg_gat_jvp2, degenerate graphs         0 exactly
  vg_gat_jvp2 at the kink                1.0e-6 (h_inj, C = 12, slope 0.2)
  vg_gat_jvp2 past the grid cap          5.1e-7 (g_att_dst, C = 64)
  vg_gat_bwd_ex past the grid cap / hub  8.6e-7 (g_att_dst, C = 8) / 5.2e-7
  vg_graphnorm_jvp2                      1.5e-6 (x_inj, C = 68, n = 2)
  ... dead column / unaligned operands   4.0e-7 / 6.6e-7
  GraphNorm sums of the GAT row pass     2.0e-7; vg_graphnorm_jvp2_part 3.8e-7
  spmm / spmm_t / sddmm                  2.3e-7; bound 1e-5
  seg_sum / scatter_src                  2.8e-7; bound 1e-5
  double backward on the hub graph       below 1 % of its bound (W, C = 100:
                                         4.4e-5 against 6.2e-3)
"""
import ctypes
import functools

import pytest
import torch

import critic_ref as CR
from oracle import pyg
from parity_util import rel_err
from test_critic_gpu import _close, _gn_inputs, _graph
from test_ops_gpu import _oracle_gat
from vgan import ops
from vgan._lib import LIB, VgFold, VgGnJvp, VgJvpSrc, check, ptr, stream_handle

pytestmark = pytest.mark.gpu

TOL = 2e-5
MAX_BLOCKS = 4096  # VG_BWD_MAX_BLOCKS: the grid cap of the tangent and backward row passes
W_GAT = [9, 12, 18, 24, 50, 64, 128, 130, 136, 256]
W_SP = [1, 8, 9, 33, 64, 100, 101, 128, 130, 132, 256]
D = torch.float64


# ------------------------------------------------------------------ graphs
@functools.lru_cache(maxsize=None)
def _hub(n=302):
    """i -> 0 and 0 -> i for every i, plus a ring: with GATConv's self loops row
    0 and CSC column 0 hold n entries each, every other row 2-3."""
    i = torch.arange(1, n)
    z = torch.zeros_like(i)
    r = torch.arange(n)
    ei = torch.cat([torch.stack([i, z]), torch.stack([z, i]), torch.stack([r, (r + 1) % n])], 1)
    return torch.unique(ei, dim=1), n


@functools.lru_cache(maxsize=None)
def _stress():
    _, vox = _graph(stress=True)
    return vox.edge_index, vox.num_nodes


def _named_graph(name):
    if name == "hub":
        return _hub()
    if name == "stress":
        return _stress()
    if name == "one_node":
        return torch.zeros(2, 0, dtype=torch.long), 1
    assert name == "edgeless"
    return torch.zeros(2, 0, dtype=torch.long), 50


_CSR = {}


def _csr(cuda, name):
    if name not in _CSR:
        ei, n = _named_graph(name)
        _CSR[name] = ops.CSR(ei.to(cuda), n)
    return _CSR[name]


def _r32(t):
    """float64 values that float32 holds exactly."""
    return t.float().double()


def _gat_fn(ei, n, slope):
    if slope == 0.2:
        return CR.gat_fn(ei, n)

    def f(h, att_s, att_d, bias):
        a_s = (h * att_s.view(1, -1)).sum(-1)
        a_d = (h * att_d.view(1, -1)).sum(-1)
        return pyg.gat_propagate(h, a_s, a_d, ei, slope) + bias
    return f


def _report(family, pairs, tol=TOL):
    """pairs [(name, got, ref)]: every figure printed, then asserted."""
    figs = [(name, _close(got, ref, tol)[1]) for name, got, ref in pairs]
    print(family, " ".join(f"{k}={e:.3e}" for k, e in figs))
    bad = [(k, e) for k, e in figs if not e <= tol]
    assert not bad, (family, bad)


# --------------------------------------------------------------------- GAT
def _gat_draw(n, C, seed, zero_even=False):
    g = torch.Generator().manual_seed(seed)
    h, u, go = (_r32(torch.randn(n, C, generator=g, dtype=D)) for _ in range(3))
    if zero_even:
        h[::2] = 0.0
    P = {"as": _r32(torch.randn(C, generator=g, dtype=D) / C ** 0.5).view(1, 1, C),
         "ad": _r32(torch.randn(C, generator=g, dtype=D) / C ** 0.5).view(1, 1, C),
         "bias": _r32(torch.randn(C, generator=g, dtype=D))}
    base = [_r32(torch.randn(C, generator=g, dtype=D)) for _ in range(3)]  # non-zero initial parameter gradients
    return h, u, go, P, base


@functools.lru_cache(maxsize=None)
def _gat_ref(graph, C, seed, slope=0.2, zero_even=False):
    """(inputs, Unit.jvp2, Unit.vjp) in float64 on the CPU, computed once."""
    ei, n = _named_graph(graph)
    h, u, go, P, base = _gat_draw(n, C, seed, zero_even)
    unit = CR.Unit("gat", _gat_fn(ei, n, slope), ["as", "ad", "bias"])
    return (h, u, go, P, base), unit.jvp2(h, u, go, P), unit.vjp(h, go, P)


class _Layer:
    """One GATConv on the device: inputs (tiled ``copies`` times over a stacked
    CSR) and the forward's saved tensors."""

    def __init__(self, cuda, csr, h, u, go, P, slope=0.2, copies=1):
        self.csr, self.slope = csr, slope
        self.n, self.C, self.e = csr.num_nodes, h.shape[1], csr.num_edges
        assert self.n == h.shape[0] * copies
        self.h, self.u, self.go = (t.float().to(cuda).repeat(copies, 1).contiguous() for t in (h, u, go))
        self.vs, self.vd, self.b = (P[k].float().to(cuda).reshape(-1).contiguous() for k in ("as", "ad", "bias"))
        self.out = torch.empty(self.n, self.C, device=cuda)
        self.alpha = torch.empty(self.e, device=cuda)
        self.a_s, self.a_d = torch.empty(self.n, device=cuda), torch.empty(self.n, device=cuda)
        self.st = stream_handle(cuda)
        self.cuda = cuda
        check(LIB.vg_gat_fwd(ptr(csr.row_ptr), ptr(csr.col), self.n, self.C, ptr(self.h), ptr(self.vs), ptr(self.vd),
                             ptr(self.b), slope, ptr(self.out), ptr(self.alpha), ptr(self.a_s), ptr(self.a_d),
                             self.st), "vg_gat_fwd")

    def graph_args(self):
        c = self.csr
        return (ptr(c.row_ptr), ptr(c.col), ptr(c.csc_ptr), ptr(c.csc_slot), ptr(c.csc_dst), self.n, self.e, self.C)

    def jvp_ws(self, fill=float("nan")):
        return torch.full((int(LIB.vg_gat_jvp2_ws_floats(self.n, self.e, self.C)),), fill, device=self.cuda)

    def outputs(self, base):
        """u_out, h_inj (NaN: an unwritten row fails every comparison), g_att_src, g_att_dst."""
        nan = float("nan")
        return (torch.full((self.n, self.C), nan, device=self.cuda), torch.full((self.n, self.C), nan, device=self.cuda),
                base[0].float().to(self.cuda), base[1].float().to(self.cuda))

    def jvp_args(self, outs):
        return self.graph_args() + (ptr(self.h), ptr(self.u), ptr(self.go), ptr(self.vs), ptr(self.vd), ptr(self.a_s),
                                    ptr(self.a_d), ptr(self.alpha), self.slope) + tuple(ptr(t) for t in outs)

    def jvp2(self, base):
        outs, ws = self.outputs(base), self.jvp_ws()
        check(LIB.vg_gat_jvp2(*self.jvp_args(outs), ptr(ws), self.st), "vg_gat_jvp2")
        return outs, ws

    def part_blocks(self, ws):
        """The att_dst (row pass) and att_src (source pass) partial blocks of a workspace."""
        blocks = int(LIB.vg_gat_jvp2_blocks(self.n, self.C))
        o = 5 * self.e + 3 * self.n
        return ws[o:o + blocks * self.C].clone(), ws[o + MAX_BLOCKS * self.C:o + (MAX_BLOCKS + blocks) * self.C].clone()


def _jvp_pairs(outs, base, ref, scale=1.0):
    ju, hinj, pg = ref
    u_out, h_inj, g_as, g_ad = outs
    return [("u_out", u_out, ju), ("h_inj", h_inj, hinj),
            ("g_att_src", g_as.double().cpu() - base[0], scale * pg["as"].reshape(-1)),
            ("g_att_dst", g_ad.double().cpu() - base[1], scale * pg["ad"].reshape(-1))]


@pytest.mark.parametrize("graph,C", [("hub", c) for c in W_GAT] +
                         [(g, c) for g in ("one_node", "edgeless") for c in (1, 12, 130)])
def test_gat_jvp2_hub_and_degenerate(cuda, graph, C):
    """vg_gat_jvp2 at every VG_DISPATCH_JVP form over rows and CSC columns of
    302 entries (strided loops taken many times, 4-edge batches ending on 2),
    and on graphs whose rows hold the self loop only."""
    (h, u, go, P, base), ref, _ = _gat_ref(graph, C, 100 + C)
    lay = _Layer(cuda, _csr(cuda, graph), h, u, go, P)
    if graph == "hub":
        deg = (lay.csr.row_ptr[1:] - lay.csr.row_ptr[:-1]).cpu()
        cdeg = (lay.csr.csc_ptr[1:] - lay.csr.csc_ptr[:-1]).cpu()
        assert int(deg[0]) == 302 and int(cdeg[0]) == 302 and int(deg[1:].max()) <= 3
    outs, _ = lay.jvp2(base)
    _report(f"gat_jvp2[{graph},C={C}]", _jvp_pairs(outs, base, ref))
    assert ref[2]["bias"].abs().max().item() == 0.0


@pytest.mark.parametrize("slope", [0.2, 0.01])
@pytest.mark.parametrize("C", [12, 64])
def test_gat_jvp2_at_the_leaky_relu_kink(cuda, C, slope):
    """h = 0 on every even node: every edge between two even nodes (the hub row
    included) has pre == 0 exactly, in float32 and float64.  torch's leaky_relu
    derivative there is ``slope``: the kernels' ``pre > 0 ? 1 : slope``."""
    ei, n = _hub()
    (h, u, go, P, base), ref, _ = _gat_ref("hub", C, 200 + C, slope, True)
    full = pyg.add_self_loops(pyg.remove_self_loops(ei), n)
    a_s, a_d = h @ P["as"].view(-1), h @ P["ad"].view(-1)
    assert int(((a_s[full[0]] + a_d[full[1]]) == 0).sum()) >= 300
    lay = _Layer(cuda, _csr(cuda, "hub"), h, u, go, P, slope)
    outs, _ = lay.jvp2(base)
    _report(f"gat_jvp2_kink[C={C},slope={slope}]", _jvp_pairs(outs, base, ref))


@pytest.mark.parametrize("C", [12, 130])
def test_gat_jvp2_ex_supplied_projections_bitwise(cuda, C):
    """vg_gat_jvp2_ex with the tangent projections vg_gat_jvp2 left in its
    workspace (offsets 5E and 5E + N): every output bit-identical."""
    (h, u, go, P, base), _, _ = _gat_ref("hub", C, 100 + C)
    lay = _Layer(cuda, _csr(cuda, "hub"), h, u, go, P)
    outs, ws = lay.jvp2(base)
    up_s = ws[5 * lay.e:5 * lay.e + lay.n].clone()
    up_d = ws[5 * lay.e + lay.n:5 * lay.e + 2 * lay.n].clone()
    assert torch.isfinite(up_s).all() and torch.isfinite(up_d).all()
    outs2, ws2 = lay.outputs(base), lay.jvp_ws()
    check(LIB.vg_gat_jvp2_ex(*lay.jvp_args(outs2), ptr(up_s), ptr(up_d), ptr(ws2), lay.st), "vg_gat_jvp2_ex")
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    assert torch.isnan(ws2[5 * lay.e:5 * lay.e + 2 * lay.n]).all()  # its own projections were not formed
    outs3 = lay.outputs(base)
    assert LIB.vg_gat_jvp2_ex(*lay.jvp_args(outs3), ptr(up_s), None, ptr(ws2), lay.st) != 0
    assert LIB.vg_gat_jvp2_ex(*lay.jvp_args(outs3), None, ptr(up_d), ptr(ws2), lay.st) != 0


def _stacked(cuda, C, L, seed):
    """The stress lattice stacked until its rows pass the grid cap of a width
    with lane groups of L: (single-graph inputs and references, layer, copies)."""
    G = 256 // L
    ei, n = _stress()
    k = MAX_BLOCKS * G // n + 1
    inputs, ref, vref = _gat_ref("stress", C, seed)
    h, u, go, P, _ = inputs
    lay = _Layer(cuda, _csr(cuda, "stress").stacked(k), h, u, go, P, copies=k)
    assert lay.n == k * n > MAX_BLOCKS * G >= (k - 1) * n
    assert int(LIB.vg_gat_jvp2_blocks(lay.n, C)) * G < lay.n  # fails if the cap ever moves
    return inputs, ref, vref, lay, k, n


def _copies_identical(t, k, n, upto=None):
    v = t.view(k, n, -1)[:upto]
    return torch.equal(v[1:], v[:1].expand_as(v[1:]))


@pytest.mark.parametrize("C,L", [(8, 8), (64, 16), (136, 32)])
def test_gat_jvp2_past_the_grid_cap(cuda, C, L):
    """More rows than 4096 workgroups hold: the grid-stride loops of k_jvp_rows
    and jvp_src_body.  Copy 0 against float64; every other copy bit-identical to
    it (the row math is local and its order fixed, so a dropped or doubled
    grid-stride row shows); the att increments k x the single-graph reference."""
    (h, u, go, P, base), ref, _, lay, k, n = _stacked(cuda, C, L, 300 + C)
    outs, _ = lay.jvp2(base)
    assert _copies_identical(outs[0], k, n) and _copies_identical(outs[1], k, n)
    pairs = _jvp_pairs((outs[0][:n], outs[1][:n], outs[2], outs[3]), base, ref, scale=float(k))
    _report(f"gat_jvp2_stacked[C={C},k={k}]", pairs)


def _bwd_ex(lay, base, inj, inj_row0):
    nan = float("nan")
    g_h = torch.full((lay.n, lay.C), nan, device=lay.cuda)
    gs = [b.float().to(lay.cuda) for b in base]
    ws = torch.full((int(LIB.vg_gat_bwd_ws_floats(lay.n, lay.e, lay.C)),), nan, device=lay.cuda)
    injd = inj.float().to(lay.cuda)
    check(LIB.vg_gat_bwd_ex(*lay.graph_args(), ptr(lay.h), ptr(lay.vs), ptr(lay.vd), ptr(lay.a_s), ptr(lay.a_d),
                            ptr(lay.alpha), ptr(lay.go), lay.slope, ptr(g_h), ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), 1,
                            ptr(injd), inj_row0, ptr(ws), lay.st), "vg_gat_bwd_ex")
    return g_h, gs


@pytest.mark.parametrize("C,L", [(8, 8), (64, 16), (136, 32)])
def test_gat_bwd_ex_past_the_grid_cap(cuda, C, L):
    """vg_gat_bwd_ex over the same stacked inputs, an injection on the last copy
    and accumulate = 1: the grid-stride loops of the backward row and source
    passes."""
    (h, u, go, P, base), _, (dx, pg), lay, k, n = _stacked(cuda, C, L, 300 + C)
    inj = _r32(torch.randn(n, C, generator=torch.Generator().manual_seed(7), dtype=D))
    g_h, gs = _bwd_ex(lay, base, inj, (k - 1) * n)
    assert _copies_identical(g_h, k, n, upto=k - 1)
    pairs = [("g_h", g_h[:n], dx), ("g_h+inj", g_h[(k - 1) * n:], dx + inj)] + \
            [(f"g_{key}", got.double().cpu() - b0, float(k) * pg[key].reshape(-1))
             for got, b0, key in zip(gs, base, ("as", "ad", "bias"))]
    _report(f"gat_bwd_ex_stacked[C={C},k={k}]", pairs)


@pytest.mark.parametrize("C", [9, 50, 130, 136])
def test_gat_bwd_ex_hub(cuda, C):
    """The backward's scalar and vector forms over the 302-entry row and column,
    with an injection on the rows from n / 3 and accumulate = 1."""
    (h, u, go, P, base), _, (dx, pg) = _gat_ref("hub", C, 100 + C)
    n = h.shape[0]
    lay = _Layer(cuda, _csr(cuda, "hub"), h, u, go, P)
    row0 = n // 3
    inj = torch.zeros(n, C, dtype=D)
    inj[row0:] = _r32(torch.randn(n - row0, C, generator=torch.Generator().manual_seed(8), dtype=D))
    g_h, gs = _bwd_ex(lay, base, inj[row0:], row0)
    pairs = [("g_h", g_h, dx + inj)] + [(f"g_{key}", got.double().cpu() - b0, pg[key].reshape(-1))
                                         for got, b0, key in zip(gs, base, ("as", "ad", "bias"))]
    _report(f"gat_bwd_ex[hub,C={C}]", pairs)


# ------------------------------------------------ GraphNorm inputs, reference
def _gn_draw(n, C, seed, with_keep=True, dead=None):
    """test_critic_gpu._gn_inputs rounded to float32, with x nudged so that no
    pre-activation z lies within 1e-4 of 0 (the weight is positive: z grows
    with x), and optionally one column driven dead (bias -10: z < 0 on every row)."""
    x, P, keep = _gn_inputs(n, C, seed)
    x, keep = _r32(x), _r32(keep)
    P = {k: _r32(v) for k, v in P.items()}
    if dead is not None:
        P["b"][dead] = -10.0
    g = torch.Generator().manual_seed(seed + 1000)
    u, gy = (_r32(torch.randn(n, C, generator=g, dtype=D)) for _ in range(2))
    base = [_r32(torch.randn(C, generator=g, dtype=D)) for _ in range(2)]
    for _ in range(8):
        z = _gn_z(x, x.mean(0), None, P)
        near = z.abs() < 1e-4
        if not near.any():
            break
        x = _r32(torch.where(near, x + torch.where(z >= 0, 0.01, -0.01), x))
    assert not (z.abs() < 1e-4).any()
    return x, P, (keep if with_keep else None), u, gy, base


def _gn_z(x, mu, d, P, eps=1e-5):
    """The pre-activation from column statistics [mu | d] (d = None: from x)."""
    c = x - mu * P["s"]
    if d is None:
        d = (c.pow(2).mean(0) + eps).sqrt()
    return P["w"] * c / d + P["b"]


def _gn_unit(keep):
    return CR.Unit("gn", CR.gnrd_fn(keep), ["w", "b", "s"])


class _Norm:
    """One GraphNorm(+ReLU+Dropout) on the device after its forward."""

    def __init__(self, cuda, x, P, keep, u, gy, offset=0):
        self.n, self.C = x.shape
        self.cuda, self.st = cuda, stream_handle(cuda)

        def dev(t):  # offset: a view that starts ``offset`` floats into a larger buffer
            if t is None:
                return None
            buf = torch.empty(t.numel() + offset, device=cuda)
            v = buf[offset:].view(t.shape)
            v.copy_(t.float())
            return v
        self.x, self.keep, self.u, self.gy = dev(x), dev(keep), dev(u), dev(gy)
        self.w, self.b, self.s = (P[k].float().to(cuda).contiguous() for k in ("w", "b", "s"))
        self.stats = torch.empty(2 * self.C, device=cuda)
        self.ws = self.new_ws()
        y = torch.empty(self.n, self.C, device=cuda)
        xa = x.float().to(cuda)  # the forward from aligned operands either way: the same statistics
        ka = None if keep is None else keep.float().to(cuda)
        check(LIB.vg_graphnorm_fwd_seg(ptr(xa), 1, self.n, self.C, ptr(self.w), ptr(self.b), ptr(self.s), ptr(ka), 1e-5,
                                       ptr(y), ptr(self.stats), ptr(self.ws), None, self.st), "vg_graphnorm_fwd_seg")
        torch.cuda.synchronize()

    def new_ws(self):
        return torch.full((int(LIB.vg_graphnorm_seg_ws_floats(1, self.n, self.C)),), float("nan"), device=self.cuda)

    def head(self):
        return (ptr(self.x), self.n, self.C, ptr(self.w), ptr(self.b), ptr(self.s), ptr(self.keep), 1e-5,
                ptr(self.stats), ptr(self.u), ptr(self.gy))

    def outputs(self, base):
        nan = float("nan")
        return (torch.full((self.n, self.C), nan, device=self.cuda), torch.full((self.n, self.C), nan, device=self.cuda),
                base[0].float().to(self.cuda), base[1].float().to(self.cuda))

    def jvp2(self, base):
        outs, ws = self.outputs(base), self.new_ws()
        check(LIB.vg_graphnorm_jvp2(*self.head(), *(ptr(t) for t in outs), ptr(ws), None, self.st),
              "vg_graphnorm_jvp2")
        return outs

    def jvp2_split(self, base):
        """_sums / _fold_src without a source pass / _apply."""
        outs, ws = self.outputs(base), self.new_ws()
        check(LIB.vg_graphnorm_jvp2_sums(*self.head(), ptr(ws), self.st), "vg_graphnorm_jvp2_sums")
        check(LIB.vg_graphnorm_jvp2_fold_src(self.n, self.C, ptr(self.w), ptr(self.s), ptr(self.stats), ptr(ws),
                                             ptr(outs[2]), ptr(outs[3]), None, self.st), "vg_graphnorm_jvp2_fold_src")
        check(LIB.vg_graphnorm_jvp2_apply(*self.head(), ptr(outs[0]), ptr(outs[1]), ptr(ws), self.st),
              "vg_graphnorm_jvp2_apply")
        return outs


def _gn_pairs(outs, base, ref):
    ju, xinj, pg = ref
    return [("u_out", outs[0], ju), ("x_inj", outs[1], xinj), ("g_w", outs[2].double().cpu() - base[0], pg["w"]),
            ("g_ms", outs[3].double().cpu() - base[1], pg["s"])]


def _gn_ref(n, C, with_keep, dead=None):
    x, P, keep, u, gy, base = _gn_draw(n, C, 400 + C + n, with_keep, dead)
    return (x, P, keep, u, gy, base), _gn_unit(keep).jvp2(x, u, gy, P)


@pytest.mark.parametrize("n,with_keep", [(2, True), (33, True), (900, True), (900, False), (16389, True)])
@pytest.mark.parametrize("C", [3, 6, 68, 100, 130, 200, 256])
def test_graphnorm_jvp2_widths_and_rows(cuda, C, n, with_keep):
    """vg_graphnorm_jvp2 over a second column slab (C > 64), scalar-path widths,
    more rows than 256 chunks of 32 (n = 16389: 65-row chunks, the last short),
    two rows, and keep == NULL."""
    (x, P, keep, u, gy, base), ref = _gn_ref(n, C, with_keep)
    outs = _Norm(cuda, x, P, keep, u, gy).jvp2(base)
    _report(f"gn_jvp2[C={C},n={n},keep={with_keep}]", _gn_pairs(outs, base, ref))


@pytest.mark.parametrize("C,dead", [(6, 5), (68, 64), (130, 129)])
def test_graphnorm_jvp2_dead_column(cuda, C, dead):
    """A column whose z < 0 on every row carries no second-order term: its
    x_inj, u_out and its g_w / g_ms increments are exactly 0."""
    (x, P, keep, u, gy, base), ref = _gn_ref(900, C, True, dead)
    assert (_gn_z(x, x.mean(0), None, P)[:, dead] < -1.0).all()
    outs = _Norm(cuda, x, P, keep, u, gy).jvp2(base)
    assert outs[0][:, dead].abs().max().item() == 0.0 and outs[1][:, dead].abs().max().item() == 0.0
    assert outs[2][dead].item() == base[0][dead].item() and outs[3][dead].item() == base[1][dead].item()
    _report(f"gn_jvp2_dead[C={C}]", _gn_pairs(outs, base, ref))


@pytest.mark.parametrize("n", [33, 16389])
@pytest.mark.parametrize("C", [68, 130, 256])
def test_graphnorm_jvp2_three_launch_split_bitwise(cuda, C, n):
    x, P, keep, u, gy, base = _gn_draw(n, C, 400 + C + n)
    norm = _Norm(cuda, x, P, keep, u, gy)
    for a, b in zip(norm.jvp2(base), norm.jvp2_split(base)):
        assert torch.equal(a, b)


def test_graphnorm_jvp2_unaligned_operands(cuda):
    """x, u, g_y and keep as views 4 bytes into larger buffers: quad_ok sends
    the column sums to the scalar kernel (which indexes scalars), and the
    results meet the bound of the aligned call."""
    n, C = 900, 64
    x, P, keep, u, gy, base = _gn_draw(n, C, 500)
    ref = _gn_unit(keep).jvp2(x, u, gy, P)
    for offset in (0, 1):
        norm = _Norm(cuda, x, P, keep, u, gy, offset)
        assert all(t.data_ptr() % 16 == 4 * offset for t in (norm.x, norm.keep, norm.u, norm.gy))
        _report(f"gn_jvp2_align[offset={offset}]", _gn_pairs(norm.jvp2(base), base, ref))


# --------------------------------- the GraphNorm sums from the GAT row pass
def _fold_fields(f):
    return (f.width, f.k, f.ldo, f.accumulate, f.nsrc, f.src[0].rows, f.src[0].ld)


def _fold_rows(ws, f):
    off = (f.src[0].part - ws.data_ptr()) // 4
    assert 0 <= off and off + f.src[0].rows * f.src[0].ld <= ws.numel()
    return ws[off:off + f.src[0].rows * f.src[0].ld].clone()


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("C", [12, 50, 64, 130, 136])
def test_gat_jvp2_gn_deferred(cuda, C, with_keep):
    """The GNJ form of k_jvp_rows: u_out, h_inj and the described folds
    bit-identical to vg_gat_jvp2_deferred; its five GraphNorm column sums
    against float64 sums over the same u_out and statistics; and
    vg_graphnorm_jvp2_part from those partials against the float64 unit."""
    (h, u, go, P, base), _, _ = _gat_ref("stress", C, 600 + C)
    n = h.shape[0]
    lay = _Layer(cuda, _csr(cuda, "stress"), h, u, go, P)
    x, GP, keep, _, gy, gbase = _gn_draw(n, C, 700 + C, with_keep)
    norm = _Norm(cuda, x, GP, keep, u, gy)  # its tangent operand is replaced by the GAT's below
    blocks = int(LIB.vg_gat_jvp2_blocks(n, C))
    assert 0 < blocks <= MAX_BLOCKS
    part = torch.full((blocks, 5, C), float("nan"), device=cuda)
    gn = VgGnJvp(ptr(norm.x), ptr(norm.keep), ptr(norm.gy), ptr(norm.stats), ptr(norm.w), ptr(norm.b), ptr(norm.s), 1e-5,
                 ptr(part))
    res = {}
    for fused in (False, True):
        outs, ws = lay.outputs(base), lay.jvp_ws()
        folds, nf = (VgFold * 2)(), ctypes.c_int32(0)
        if fused:
            check(LIB.vg_gat_jvp2_gn_deferred(*lay.jvp_args(outs), None, None, ptr(ws), ctypes.byref(gn), folds,
                                              ctypes.byref(nf), lay.st), "vg_gat_jvp2_gn_deferred")
        else:
            check(LIB.vg_gat_jvp2_deferred(*lay.jvp_args(outs), None, None, ptr(ws), folds, ctypes.byref(nf), lay.st),
                  "vg_gat_jvp2_deferred")
        torch.cuda.synchronize()
        assert nf.value == 2 and folds[0].out == outs[3].data_ptr() and folds[1].out == outs[2].data_ptr()
        res[fused] = (outs[0], outs[1], [_fold_fields(f) for f in folds], _fold_rows(ws, folds[0]),
                      _fold_rows(ws, folds[1]))
        # deferred: the parameter gradients are left to the described folds
        assert torch.equal(outs[2].cpu().double(), base[0]) and torch.equal(outs[3].cpu().double(), base[1])
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert not torch.isnan(res[True][3]).any() and not torch.isnan(res[True][4]).any()
    # the five column sums, in float64 over the kernel's own u_out and statistics
    uo = res[True][0].double().cpu()
    st = norm.stats.double().cpu()
    mu, d = st[:C], st[C:]
    z = _gn_z(x, mu, d, GP)
    assert not (z.abs() < 5e-5).any()
    p = gy * (z > 0).to(D) * (keep if keep is not None else 1.0)
    xt = x - mu
    want = torch.stack([uo.sum(0), (xt * uo).sum(0), p.sum(0), (p * uo).sum(0), (p * xt).sum(0)])
    got = part.double().cpu().sum(0)
    names = ("sum_u", "sum_xt_u", "sum_p", "sum_p_u", "sum_p_xt")
    _report(f"gnj_sums[C={C},keep={with_keep}]", [(k, got[i], want[i]) for i, k in enumerate(names)])
    # the GraphNorm second order from those partials
    norm.u = res[True][0]
    gouts, gws = norm.outputs(gbase), norm.new_ws()
    check(LIB.vg_graphnorm_jvp2_part(*norm.head(), *(ptr(t) for t in gouts), ptr(part), blocks, ptr(gws), norm.st),
          "vg_graphnorm_jvp2_part")
    ref = _gn_unit(keep).jvp2(x, uo, gy, GP)
    _report(f"gn_jvp2_part[C={C},keep={with_keep}]", _gn_pairs(gouts, gbase, ref))


def test_gat_jvp_src_group_two_shapes_bitwise(cuda):
    """Two layers of different shape ids (C = 12: L8 x 2, id 1; C = 136: L32 x 8,
    id 5) planned with vg_gat_jvp2_plan and run by ONE vg_gat_jvp_src_group launch:
    h_inj and the att_src partial blocks bit-identical to each layer's own
    vg_gat_jvp2_deferred."""
    lays, own, planned = [], [], []
    srcs = (VgJvpSrc * 2)()
    for i, (C, shape) in enumerate(((12, 1), (136, 5))):
        (h, u, go, P, base), _, _ = _gat_ref("hub", C, 100 + C)
        lay = _Layer(cuda, _csr(cuda, "hub"), h, u, go, P)
        outs, ws = lay.outputs(base), lay.jvp_ws()
        folds, nf = (VgFold * 2)(), ctypes.c_int32(0)
        check(LIB.vg_gat_jvp2_deferred(*lay.jvp_args(outs), None, None, ptr(ws), folds, ctypes.byref(nf), lay.st),
              "vg_gat_jvp2_deferred")
        own.append((outs, ws))
        outs2, ws2 = lay.outputs(base), lay.jvp_ws()
        src = VgJvpSrc()
        check(LIB.vg_gat_jvp2_plan(*lay.jvp_args(outs2), None, None, ptr(ws2), folds, ctypes.byref(nf),
                                   ctypes.byref(src), lay.st), "vg_gat_jvp2_plan")
        assert src.shape == shape and src.blocks == int(LIB.vg_gat_jvp2_blocks(lay.n, C))
        srcs[i] = src
        planned.append((outs2, ws2))
        lays.append(lay)
    torch.cuda.synchronize()
    for outs2, _ in planned:  # the source pass has not run yet
        assert torch.isnan(outs2[1]).all()
    check(LIB.vg_gat_jvp_src_group(srcs, 2, lays[0].st), "vg_gat_jvp_src_group")
    torch.cuda.synchronize()
    for lay, (outs, ws), (outs2, ws2) in zip(lays, own, planned):
        assert torch.equal(outs[0], outs2[0]) and torch.equal(outs[1], outs2[1])
        assert not torch.isnan(outs2[1]).any()
        for a, b in zip(lay.part_blocks(ws), lay.part_blocks(ws2)):
            assert torch.equal(a, b) and not torch.isnan(a).any()


# ------------------------------- sparse primitives and the autograd fallback
def _edges(cuda, graph):
    csr = _csr(cuda, graph)
    src, dst = (t.cpu() for t in csr.edge_lists())
    return csr, src, dst


@pytest.mark.parametrize("C", W_SP)
@pytest.mark.parametrize("graph", ["hub", "stress"])
def test_sparse_width_primitives_match_f64(cuda, graph, C):
    """ops.spmm / spmm_t / sddmm at every VG_DISPATCH form (both CPL 2 and both
    CPL 4 variants), over rows and CSC columns longer than a lane group
    (k_aggregate's ``deg > L`` branch) on the hub graph."""
    csr, src, dst = _edges(cuda, graph)
    n, E = csr.num_nodes, csr.num_edges
    g = torch.Generator().manual_seed(800 + C)
    w = _r32(torch.randn(E, generator=g, dtype=D))
    x, y = (_r32(torch.randn(n, C, generator=g, dtype=D)) for _ in range(2))
    wd, xd, yd = (t.float().to(cuda) for t in (w, x, y))
    want = {"spmm": torch.zeros(n, C, dtype=D).index_add_(0, dst, w[:, None] * x.index_select(0, src)),
            "spmm_t": torch.zeros(n, C, dtype=D).index_add_(0, src, w[:, None] * y.index_select(0, dst)),
            "sddmm": (y.index_select(0, dst) * x.index_select(0, src)).sum(1)}
    got = {"spmm": ops.spmm(csr, wd, xd), "spmm_t": ops.spmm_t(csr, wd, yd), "sddmm": ops.sddmm(csr, yd, xd)}
    errs = {k: rel_err(got[k], want[k]) for k in want}
    print(f"sparse[{graph},C={C}]", " ".join(f"{k}={e:.3e}" for k, e in errs.items()))
    assert all(e < 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("graph", ["hub", "stress"])
def test_sparse_edge_primitives_match_f64(cuda, graph):
    """gather (both directions), seg_sum, seg_max and scatter_src (they take
    no width): gather and seg_max exactly."""
    csr, src, dst = _edges(cuda, graph)
    n, E = csr.num_nodes, csr.num_edges
    g = torch.Generator().manual_seed(900)
    v, e = _r32(torch.randn(n, generator=g, dtype=D)), _r32(torch.randn(E, generator=g, dtype=D))
    vd, ed = v.float().to(cuda), e.float().to(cuda)
    assert torch.equal(ops.gather(csr, vd, True).cpu().double(), v.index_select(0, src))
    assert torch.equal(ops.gather(csr, vd, False).cpu().double(), v.index_select(0, dst))
    smax = torch.full((n,), float("-inf"), dtype=D).scatter_reduce(0, dst, e, "amax")
    assert torch.equal(ops.seg_max(csr, ed).cpu().double(), smax)
    errs = {"seg_sum": rel_err(ops.seg_sum(csr, ed), torch.zeros(n, dtype=D).index_add_(0, dst, e)),
            "scatter_src": rel_err(ops.scatter_src(csr, ed), torch.zeros(n, dtype=D).index_add_(0, src, e))}
    print(f"sparse_edges[{graph}]", " ".join(f"{k}={e:.3e}" for k, e in errs.items()))
    assert all(e < 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("C", [9, 100, 101, 130])
def test_gat_conv_double_backward_hub(cuda, C):
    """test_ops_gpu.test_gat_conv_double_backward on the hub graph at widths
    whose sparse primitives run the scalar CPL 2 / CPL 4 forms: a penalty on the
    input gradient, then its gradient with respect to x, W, att and bias."""
    ei, n = _hub()
    csr = _csr(cuda, "hub")
    g = torch.Generator().manual_seed(1000 + C)
    cin = max(2, C // 2)
    base = [torch.randn(n, cin, generator=g, dtype=D), torch.randn(C, cin, generator=g, dtype=D) / cin ** 0.5,
            torch.randn(C, generator=g, dtype=D) / C ** 0.5, torch.randn(C, generator=g, dtype=D) / C ** 0.5,
            torch.randn(C, generator=g, dtype=D)]
    base = [_r32(t) for t in base]
    w1 = _r32(torch.randn(n, C, generator=g, dtype=D))

    def run(x, W, a_s, a_d, b, fn, w1):
        out = fn(x, W, a_s, a_d, b)
        gx, = torch.autograd.grad((out * w1).sum(), x, create_graph=True)
        pen = (gx.norm(dim=1) - 1).pow(2).mean()
        res = torch.autograd.grad(pen, (x, W, a_s, a_d, b), allow_unused=True)
        return [torch.zeros_like(t) if r is None else r for r, t in zip(res, (x, W, a_s, a_d, b))]

    ref = run(*[t.clone().requires_grad_(True) for t in base],
              lambda x, W, a_s, a_d, b: _oracle_gat(x @ W.t(), a_s, a_d, b, ei), w1)
    got = run(*[t.float().to(cuda).requires_grad_(True) for t in base],
              lambda x, W, a_s, a_d, b: ops.gat_conv(csr, x @ W.t(), a_s, a_d, b), w1.float().to(cuda))
    scale = max(float(r.norm()) for r in ref)
    figs = [(float((g_.double().cpu() - r).norm()), 1e-4 * float(r.norm()) + 1e-7 * scale) for g_, r in zip(got, ref)]
    print(f"gat_double_backward_hub[C={C}]",
          " ".join(f"{k}={e:.3e}/{b:.3e}" for k, (e, b) in zip(("x", "W", "att_src", "att_dst", "bias"), figs)))
    assert all(e <= b for e, b in figs), figs
