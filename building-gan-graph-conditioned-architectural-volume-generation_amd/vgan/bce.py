"""Explicit BCE critic (USE_WGANGP = False): loss and discriminator gradient
without autograd.

Replaces ``_compute_discriminator_loss(...)`` followed by ``d_loss.backward()``
for the plain GAN objective (``trainer.py:318-330``, ``:476-479``): D ends in a
``Sigmoid`` and the loss is ``BCE(D(fake), 0) + BCE(D(real), 1)``.  First order
only, so the schedule is passes A and D of the WGAN-GP engine
(``vgan/critic.py``) on TWO stacked copies, with the same kernels:

  A     one stacked forward of the real / fake copies ([2N, C] tensors, a
        block-diagonal CSR, per-copy GraphNorm statistics) up to the decoder's
        last ``Linear``: its [2N, 1] output is the pre-sigmoid score s;
  head  vg_bce_critic_head: sigmoid, both BCE means and the adjoint seeds
        dL/ds in one launch (torch's arithmetic on the probability, in f32);
  D     one stacked VJP from those seeds, parameter gradients accumulated,
        every weight-gradient product and fold deferred to one flush.

Gradients are ACCUMULATED into the discriminator's ``.grad`` like
``backward()``; the caller zeroes them first.  Randomness follows the autograd
path's order (the dropout masks of D(real), then of D(fake)) in host / fixed
RNG modes; device mode draws each layer's stacked mask in one call; eval mode
draws nothing.  The native C++ critic (vg_critic_loss_and_grad) is WGAN-GP
only: this schedule is always issued from Python, and a captured step graph
replays its launches.
"""
from __future__ import annotations

import ctypes
from typing import List

import torch
import torch.nn as nn

from . import critic as _critic
from . import data as vdata
from . import ops
from ._lib import LIB, FoldCollector, VgGnBwdIn, check, dense, linear_chain, ptr, stream_handle, sync_counter
from .critic import ACT_MASK, ACT_NONE, ACT_RELU, CriticEngine, _f, _off


def bce_decoder_ok(D: nn.Module) -> bool:
    """D's decoder is the Linear/ReLU chain ending in Linear(., 1) followed by
    exactly one trailing Sigmoid (models.py:176-185 with USE_WGANGP = False)."""
    mods = list(D.decoder.children())
    if len(mods) < 2 or not isinstance(mods[-1], nn.Sigmoid):
        return False
    mods = mods[:-1]
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    return (len(mods) == 2 * len(lins) - 1 and all(isinstance(m, nn.Linear) for m in mods[0::2])
            and all(isinstance(m, nn.ReLU) for m in mods[1::2]) and lins[-1].out_features == 1)


class BceCriticEngine:
    """``CriticEngine``'s interface for the BCE objective.  The dropout rate is
    read once at construction, as there."""

    def __init__(self, discriminator: nn.Module, configuration):
        D = discriminator
        if getattr(configuration, "USE_WGANGP", True):
            raise ValueError("the BCE critic engine implements the plain GAN loss (USE_WGANGP=False)")
        if not bce_decoder_ok(D):
            raise ValueError("the BCE critic engine needs a Linear/ReLU decoder ending in Linear(., 1) and a Sigmoid")
        self.D = D
        self.n_classes = int(configuration.NUM_CLASSES)
        self.mlp: List[nn.Linear] = [m for m in D.mlp_encoder if isinstance(m, nn.Linear)]
        self.dec: List[nn.Linear] = [m for m in D.decoder if isinstance(m, nn.Linear)]
        enc = D.encoder
        self.blocks = [(getattr(enc, f"module_{4 * b}"), getattr(enc, f"module_{4 * b + 1}"))
                       for b in range(enc.num_blocks)]
        self.dropout = float(enc.dropout)
        self._consts = {}

    def _counter(self, dev) -> torch.Tensor:
        """The head's last-block counter (0 between launches)."""
        t = self._consts.get(("bce_counter", dev))
        if t is None:
            t = self._consts[("bce_counter", dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
        return t

    def _loss_mask(self, dev) -> torch.Tensor:
        """[1, 0]: (loss, loss_real) * this = the (d_loss, 0.0) pair of ``out``."""
        t = self._consts.get(("loss_mask", dev))
        if t is None:
            t = self._consts[("loss_mask", dev)] = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)
        return t

    def prepare_batch(self, prep) -> None:
        """Build the stacked graph and the head's constants now, outside any capture."""
        prep.csr.stacked(2).ell()
        self._counter(prep.matched_voxel_x.device)
        self._loss_mask(prep.matched_voxel_x.device)

    def _keeps(self, rng, n: int, dev, training: bool):
        """Dropout multipliers [2N, C_b] per block, drawn in the autograd
        path's order (D(real) masks, then D(fake) masks)."""
        widths = [conv.out_channels for conv, _ in self.blocks]
        if not training:
            return [None] * len(widths)
        if rng.mode == "device":  # DropSpecs: drawn inside the GraphNorm kernel
            return [rng.keep_mask((2 * n, c), self.dropout, dev) for c in widths]
        real = [rng.keep_mask((n, c), self.dropout, dev) for c in widths]
        fake = [rng.keep_mask((n, c), self.dropout, dev) for c in widths]
        return [torch.cat([a, b]) for a, b in zip(real, fake)]

    _gemm = staticmethod(CriticEngine._gemm)
    _gemm_tn = staticmethod(CriticEngine._gemm_tn)

    # ------------------------------------------------------------ engine
    def loss_and_grad(self, local_graph, voxel_graph, label_hard, label_soft, rng, out=None) -> torch.Tensor:
        """d_loss (device scalar) of trainer.py:329-330; D's parameter gradients
        are added to their .grad.  ``label_soft`` is not read.  ``out``: two
        contiguous device floats that receive (d_loss, 0.0)."""
        D = self.D
        prep = vdata.prepared(local_graph, voxel_graph, self.n_classes)
        mvx, real = prep.matched_voxel_x, prep.onehot_f
        n, F = mvx.shape
        K = self.n_classes
        hard = label_hard.reshape(n, K)
        if hard.dtype != torch.float32:
            hard = hard.float()
        hard = hard.contiguous()
        dev = mvx.device
        st = stream_handle(dev)
        sy = sync_counter(dev)
        S = 2
        R, W0 = S * n, F + K
        csr = prep.csr
        csr2 = csr.stacked(S)
        E = csr.num_edges
        params = self.__dict__.get("_params")
        if params is None:
            params = self._params = list(D.parameters())
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        keeps = self._keeps(rng, n, dev, D.training)
        nb, nd, nm = len(self.blocks), len(self.dec), len(self.mlp)
        folds = FoldCollector()
        # a tile straddles at most two stacked copies: n >= 64 rows per copy
        fuse_gn = _critic._GN_FUSE and n >= 64

        # ---------------------------------------------------------- pass A
        X0 = _f(R, W0, dev=dev)
        check(LIB.vg_critic_input(ptr(mvx), n, F, ptr(real), ptr(hard), None, None, K, S, ptr(X0), st),
              "vg_critic_input")
        mlp_out = []
        x, xw = X0, W0
        for lin in self.mlp:
            o = lin.out_features
            y = _f(R, o, dev=dev)
            self._gemm(st, ptr(x), xw, ptr(lin.weight), xw, 1, ptr(y), o, R, o, xw, ptr(lin.bias), ACT_RELU)
            mlp_out.append(y)
            x, xw = y, o
        blk = []
        for (conv, norm), keep in zip(self.blocks, keeps):
            c = conv.out_channels
            H, a_s, a_d = _f(R, c, dev=dev), _f(R, dev=dev), _f(R, dev=dev)
            check(dense("vg_gat_lin_att")(ptr(x), xw, ptr(conv.lin.weight), R, xw, c, ptr(conv.att_src),
                                          ptr(conv.att_dst), ptr(H), ptr(a_s), ptr(a_d), st), "vg_gat_lin_att")
            O, alpha = _f(R, c, dev=dev), _f(S * E, dev=dev)
            gnp, g = ops.gnp_buffer(csr2, c, dev)  # the GraphNorm's column partials from the aggregation
            ops.aggregate_fwd_raw(csr2, c, ptr(H), ptr(a_s), ptr(a_d), ptr(conv.bias), float(conv.negative_slope),
                                  ptr(O), ptr(alpha), st, gnp)
            Y, stats = _f(R, c, dev=dev), _f(S * 2 * c, dev=dev)
            spec = keep if keep is not None and not isinstance(keep, torch.Tensor) else None
            if spec is not None:  # DropSpec: drawn in-kernel, stored for the backward
                keep = _f(R, c, dev=dev)
            w, b, ms, eps = ptr(norm.weight), ptr(norm.bias), ptr(norm.mean_scale), float(norm.eps)
            if gnp is not None:
                args = ((None, float(spec.p), int(spec.seed), ptr(spec.iter), int(spec.salt) & 0xFFFFFFFF)
                        if spec is not None else (ptr(keep), 0.0, 0, None, 0))
                check(LIB.vg_graphnorm_fwd_gnp(ptr(O), S, n, c, w, b, ms, *args, eps, ptr(Y),
                                               ptr(keep) if spec is not None else None, ptr(stats), ptr(gnp), g, st),
                      "vg_graphnorm_fwd_gnp")
            else:
                ws = _f(int(LIB.vg_graphnorm_seg_ws_floats(S, n, c)), dev=dev)
                if spec is not None:
                    check(LIB.vg_graphnorm_fwd_drop(ptr(O), S, n, c, w, b, ms, float(spec.p), int(spec.seed),
                                                    ptr(spec.iter), int(spec.salt) & 0xFFFFFFFF, eps, ptr(Y),
                                                    ptr(keep), ptr(stats), ptr(ws), sy, st), "vg_graphnorm_fwd_drop")
                else:
                    check(LIB.vg_graphnorm_fwd_seg(ptr(O), S, n, c, w, b, ms, ptr(keep), eps, ptr(Y), ptr(stats),
                                                   ptr(ws), sy, st), "vg_graphnorm_fwd_seg")
            blk.append(dict(X=x, xw=xw, H=H, O=O, alpha=alpha, a_s=a_s, a_d=a_d, Y=Y, stats=stats, keep=keep, c=c))
            x, xw = Y, c
        dec_out = [_f(R, lin.out_features, dev=dev) for lin in self.dec]
        dec_w = [xw] + [lin.out_features for lin in self.dec]
        if not linear_chain(ptr(x), xw, R, dec_w,
                            [dict(weight=lin.weight.data_ptr(), bias=lin.bias.data_ptr(), out=z.data_ptr(),
                                  ld_out=lin.out_features, act=ACT_NONE if i == nd - 1 else ACT_RELU)
                             for i, (lin, z) in enumerate(zip(self.dec, dec_out))], st):
            for i, lin in enumerate(self.dec):
                o = lin.out_features
                self._gemm(st, ptr(x), xw, ptr(lin.weight), xw, 1, ptr(dec_out[i]), o, R, o, xw, ptr(lin.bias),
                           ACT_NONE if i == nd - 1 else ACT_RELU)
                x, xw = dec_out[i], o
        scores = dec_out[-1]  # pre-sigmoid: the decoder's trailing Sigmoid is the head's

        # ------------------------------------------------------------ head
        if out is not None and (out.numel() != 2 or not out.is_contiguous() or out.dtype != torch.float32
                                or out.device != dev):
            out = None
        triple, seeds = _f(3, dev=dev), _f(R, 1, dev=dev)
        hws = _f(int(LIB.vg_bce_critic_head_ws_floats(n)), dev=dev)
        check(LIB.vg_bce_critic_head(ptr(scores), n, ptr(triple), ptr(seeds), ptr(hws), ptr(self._counter(dev)), st),
              "vg_bce_critic_head")

        # ---------------------------------------------------------- pass D
        def gn_bwd(b: int, tp, g_y):
            """block b's GraphNorm(+ReLU+Dropout) backward: the column sums and
            parameter gradients; returns g_x, or with _GN_ROWS the descriptor
            with which vg_gat_bwd_gn forms it in its destination-row pass."""
            norm, B = self.blocks[b][1], blk[b]
            c = B["c"]
            ws = _f(int(LIB.vg_graphnorm_seg_ws_floats(S, n, c)), dev=dev)
            pg = (ptr(norm.weight.grad), ptr(norm.bias.grad), ptr(norm.mean_scale.grad))
            g_x = None if _critic._GN_ROWS else _f(R, c, dev=dev)
            gn_in = (ptr(B["O"]), S, n, c, ptr(norm.weight), ptr(norm.bias), ptr(norm.mean_scale), ptr(B["keep"]),
                     float(norm.eps), ptr(B["stats"]), ptr(g_y))
            if tp is not None:
                check(LIB.vg_graphnorm_bwd_seg_tiles(*gn_in, ptr(tp), ptr(g_x), *pg, 1, None, 0, ptr(ws), st),
                      "vg_graphnorm_bwd_seg_tiles")
            else:
                check(LIB.vg_graphnorm_bwd_seg(*gn_in, ptr(g_x), *pg, 1, None, 0, ptr(ws), sy, st),
                      "vg_graphnorm_bwd_seg")
            if g_x is not None:
                return g_x, None, ws
            gn = VgGnBwdIn(x=ptr(B["O"]), keep=ptr(B["keep"]), g_y=ptr(g_y), inj=None, weight=ptr(norm.weight),
                           bias=ptr(norm.bias), mean_scale=ptr(norm.mean_scale), stats=ptr(B["stats"]),
                           sums=_off(ws, int(LIB.vg_graphnorm_bwd_sums_offset(S, c))), eps=float(norm.eps),
                           segments=S, seg_rows=n, inj_offset=0)
            return None, gn, ws

        def gemm_dy(A, lda, Wt, ldw, dY, m: int, k: int, b: int):
            """dY [R, m] = A Wt, the output gradient of block b's GraphNorm; with
            fuse_gn that backward's column partials come from this GEMM's
            epilogue (returned), else None (the separate partial pass)."""
            if not fuse_gn:
                self._gemm(st, A, lda, Wt, ldw, 0, ptr(dY), m, R, m, k)
                return None
            norm, B = self.blocks[b][1], blk[b]
            tp = _f(int(LIB.vg_gemm_gn_tpart_floats(R, m)), dev=dev)
            check(dense("vg_gemm_gn_bwd")(A, lda, Wt, ldw, R, m, k, ptr(dY), m, ptr(B["O"]), ptr(B["keep"]), n,
                                          ptr(norm.weight), ptr(norm.bias), ptr(norm.mean_scale), float(norm.eps),
                                          ptr(B["stats"]), ptr(tp), st), "vg_gemm_gn_bwd")
            return tp

        adj_dec = [_f(R, l.out_features, dev=dev) for l in self.dec[:-1]] + [seeds]
        adj_H = [_f(R, B["c"], dev=dev) for B in blk]
        adj_mlp = [_f(R, l.out_features, dev=dev) for l in self.mlp]
        dec_in = [blk[-1]["Y"] if blk else mlp_out[-1]] + dec_out[:-1]
        ws_ = [self.dec[i].weight.shape[0] for i in range(nd - 1, 0, -1)] + [self.dec[0].weight.shape[0]]
        chained = linear_chain(ptr(adj_dec[nd - 1]), ws_[0], R, ws_,
                               [dict(weight=self.dec[i].weight.data_ptr(), w_trans=1, act=ACT_MASK,
                                     aux=dec_out[i - 1].data_ptr(), ld_aux=self.dec[i].weight.shape[1],
                                     out=adj_dec[i - 1].data_ptr(), ld_out=self.dec[i].weight.shape[1])
                                for i in range(nd - 1, 0, -1)], st)
        dY = tp = None
        for i in range(nd - 1, -1, -1):
            lin = self.dec[i]
            aw, m = lin.weight.shape
            self._gemm_tn(folds, st, dev, ptr(adj_dec[i]), aw, ptr(dec_in[i]), m, R, aw, m, ptr(lin.weight.grad), m,
                          ptr(lin.bias.grad), R)
            if i > 0:
                if not chained:
                    self._gemm(st, ptr(adj_dec[i]), aw, ptr(lin.weight), m, 0, ptr(adj_dec[i - 1]), m, R, m, aw, None,
                               ACT_MASK, ptr(dec_out[i - 1]), m)
            else:
                dY = _f(R, m, dev=dev)
                tp = gemm_dy(ptr(adj_dec[0]), aw, ptr(lin.weight), m, dY, m, aw, nb - 1)
        for b in range(nb - 1, -1, -1):
            (conv, norm), B = self.blocks[b], blk[b]
            c, cin = B["c"], B["xw"]
            ws = _f(int(LIB.vg_gat_bwd_ws_floats(R, S * E, c)), dev=dev)
            gat_args = (ptr(csr2.row_ptr), ptr(csr2.col), ptr(csr2.csc_ptr), ptr(csr2.csc_slot), ptr(csr2.csc_dst), R,
                        S * E, c, ptr(B["H"]), ptr(conv.att_src), ptr(conv.att_dst), ptr(B["a_s"]), ptr(B["a_d"]),
                        ptr(B["alpha"]))
            gat_tail = (float(conv.negative_slope), ptr(adj_H[b]), ptr(conv.att_src.grad), ptr(conv.att_dst.grad),
                        ptr(conv.bias.grad), 1, None, 0, ptr(ws))
            dO, gn, gws = gn_bwd(b, tp, dY)
            if gn is not None:
                dO = _f(R, c, dev=dev)
                folds.call(LIB.vg_gat_bwd_gn, gat_args + (ctypes.byref(gn), ptr(dO)) + gat_tail, st,
                           keep=(ws, gws, dO, dY), name="vg_gat_bwd_gn")
            else:
                folds.call(LIB.vg_gat_bwd_deferred, gat_args + (ptr(dO),) + gat_tail, st, keep=(ws, dO),
                           name="vg_gat_bwd_deferred")
            self._gemm_tn(folds, st, dev, ptr(adj_H[b]), c, ptr(B["X"]), cin, R, c, cin, ptr(conv.lin.weight.grad),
                          cin)
            if b > 0:
                dY = _f(R, cin, dev=dev)
                tp = gemm_dy(ptr(adj_H[b]), c, ptr(conv.lin.weight), cin, dY, cin, c, b - 1)
            else:
                self._gemm(st, ptr(adj_H[b]), c, ptr(conv.lin.weight), cin, 0, ptr(adj_mlp[-1]), cin, R, cin, c,
                           None, ACT_MASK, ptr(mlp_out[-1]), cin)
        for i in range(nm - 1, -1, -1):
            lin = self.mlp[i]
            o, m = lin.weight.shape
            xin = X0 if i == 0 else mlp_out[i - 1]
            self._gemm_tn(folds, st, dev, ptr(adj_mlp[i]), o, ptr(xin), m, R, o, m, ptr(lin.weight.grad), m,
                          ptr(lin.bias.grad), R)
            if i > 0:
                self._gemm(st, ptr(adj_mlp[i]), o, ptr(lin.weight), m, 0, ptr(adj_mlp[i - 1]), m, R, m, o, None,
                           ACT_MASK, ptr(mlp_out[i - 1]), m)
        folds.flush(st)
        self.last_loss_real, self.last_loss_fake = triple[1], triple[2]
        if out is None:
            return triple[0]
        torch.mul(triple[:2], self._loss_mask(dev), out=out)  # (d_loss, 0.0): no penalty term (the means are <= 100)
        return out[0]
