"""f16 generator forward for inference (BASELINE.json configs[4]: "Generator-only
inference sweep ... fp16").

``HalfGenerator(G)`` snapshots a ``VoxelGNNGenerator``'s parameters into the f16
layout of ``include/vgan.h``'s f16 section and runs the eval-mode forward of
``models.py:119-155`` on the f16 kernels:

* every [Linear, LayerNorm, LeakyReLU] block is one ``vg_hgemm_ln_act`` (f16
  MFMA, LayerNorm in the epilogue), the decoder head one ``vg_hgemm`` with f32
  logits;
* every GATConv is ``vg_hgat_lin_att`` (projection + attention projections) and
  ``vg_hgat_fwd`` (edge softmax + gather-sum on f16 rows, half the bytes of the
  f32 scatter kernel), every GraphNorm + ReLU ``vg_graphnorm_fwd_h``;
* the two concatenations of the reference (``models.py:131`` and ``:145``) are
  ONE row buffer ``[enc | x | em | voxel.x | z | 0-pad]``: the encoders write
  their outputs straight into its column slices and the MLP encoder reads its
  input ``[em | voxel.x | z]`` from the same rows, so no concatenation runs;
* the type head stays f32 (``ops.gumbel_head``).

Rows are padded to multiples of 8 halves (16-byte fragments for the MFMA);
pad columns are zero.  Accumulation is f32 everywhere.  Results differ from the
f32 forward by f16 rounding only (``tests/test_half_gpu.py`` states the bounds).
Call ``refresh()`` after the generator's weights change.

``HalfCritic(D)`` is the same for a ``VoxelGNNDiscriminator``: the f16 scorer
of the sweep's best-of-k (``score_labels`` / ``select``).
"""
from __future__ import annotations

import os
import weakref
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import data as vdata
from . import ops
from ._lib import LIB, check, ptr, stream_handle

# sweep_labels as ONE hipGraph launch per batch (vg_hgen_sweep_graphed: the
# native call captured, an executable graph updated in place); 0: the native
# call launches its kernels directly (vg_hgen_sweep)
_GRAPH = os.environ.get("VGAN_HGEN_GRAPH", "1") == "1"



def _r8(c: int) -> int:
    return (c + 7) // 8 * 8


def _w16(weight: torch.Tensor) -> torch.Tensor:
    """[M, K] f32 -> [M, K rounded up to 8] f16, zero pad columns."""
    m, k = weight.shape
    w = torch.zeros(m, _r8(k), dtype=torch.float16, device=weight.device)
    w[:, :k] = weight.detach()
    return w


def _gat_encoder(m, x: torch.Tensor, ldx: int, rows: int, kk: int, n: int, csr, last_out=None, last_ld: int = 0):
    """The GAT encoder of ``m`` (a HalfGenerator / HalfCritic: its ``gat``
    blocks, ``device`` and ``trace``) over ``rows`` = kk * n stacked f16 rows
    of ``x`` (stride ldx) on ``csr``; returns (output, its stride).  A
    block's GraphNorm + ReLU is applied by the next block's projection as it
    loads its operand (vg_hgat_lin_att_gn) when the statistics come from the
    aggregation's partials; the last block's is stored, into ``last_out``
    (stride last_ld) when given.  csrc/hengine.h run_gat_blocks makes the
    same choices, launch for launch."""
    dev = m.device
    s = stream_handle(dev)
    nb = len(m.gat)
    pend = None  # (agg, gw, gb, gms, stats, channels) of a GraphNorm the next projection applies
    for b, (w, att_s, att_d, bias, cin, cout, slope, gw, gb, gms, eps) in enumerate(m.gat):
        ldh = _r8(cout)
        h = torch.empty(rows, ldh, dtype=torch.float16, device=dev)
        a_s = torch.empty(rows, dtype=torch.float32, device=dev)
        a_d = torch.empty(rows, dtype=torch.float32, device=dev)
        if pend is not None:
            p_agg, p_w, p_b, p_ms, p_st, p_c = pend
            check(LIB.vg_hgat_lin_att_gn(ptr(p_agg), p_agg.shape[1], ptr(w), w.shape[1], rows, _r8(cin), cout,
                                         ptr(att_s), ptr(att_d), ptr(h), ldh, ptr(a_s), ptr(a_d), ptr(p_w),
                                         ptr(p_b), ptr(p_ms), ptr(p_st), kk, n, p_c, s), "vg_hgat_lin_att_gn")
            pend = None
        else:
            check(LIB.vg_hgat_lin_att(ptr(x), ldx, ptr(w), w.shape[1], rows, _r8(cin), cout, ptr(att_s),
                                      ptr(att_d), ptr(h), ldh, ptr(a_s), ptr(a_d), s), "vg_hgat_lin_att")
        agg = torch.empty_like(h)
        # the GraphNorm's column partials from the aggregation's epilogue
        # when one copy spans a partial block (always, at sweep sizes)
        g = int(LIB.vg_hgat_gnp_rows(rows, ldh))
        gnp = torch.empty(int(LIB.vg_hgat_gnp_floats(rows, ldh)), dtype=torch.float32, device=dev) \
            if 0 < g <= n else None
        if gnp is not None:
            check(LIB.vg_hgat_fwd_gnp(ptr(csr.row_ptr), ptr(csr.col), rows, cout, ldh, ptr(h), ptr(a_s), ptr(a_d),
                                      ptr(bias), slope, ptr(agg), ldh, n, ptr(gnp), s), "vg_hgat_fwd_gnp")
        else:
            check(LIB.vg_hgat_fwd(ptr(csr.row_ptr), ptr(csr.col), rows, cout, ldh, ptr(h), ptr(a_s), ptr(a_d),
                                  ptr(bias), slope, ptr(agg), ldh, s), "vg_hgat_fwd")
        stats = torch.empty(kk * 2 * cout, dtype=torch.float32, device=dev)
        if gnp is not None and b < nb - 1 and kk <= int(LIB.vg_hgat_gna_max_segments()) and m.trace is None:
            check(LIB.vg_graphnorm_stats_gnp(kk, n, cout, ptr(gnp), g, ptr(gms), eps, ptr(stats), s),
                  "vg_graphnorm_stats_gnp")
            pend = (agg, gw, gb, gms, stats, cout)
            continue
        if b == nb - 1 and last_out is not None:
            y, ldy = last_out, last_ld
        else:
            y, ldy = torch.empty_like(h), ldh
        if gnp is not None:
            check(LIB.vg_graphnorm_fwd_h_gnp(ptr(agg), ldh, kk, n, cout, ptr(gw), ptr(gb), ptr(gms), eps, ptr(y),
                                             ldy, ptr(stats), ptr(gnp), g, s), "vg_graphnorm_fwd_h_gnp")
        else:
            ws = torch.empty(int(LIB.vg_graphnorm_seg_ws_floats(kk, n, cout)), dtype=torch.float32, device=dev)
            check(LIB.vg_graphnorm_fwd_h(ptr(agg), ldh, kk, n, cout, ptr(gw), ptr(gb), ptr(gms), eps, ptr(y), ldy,
                                         ptr(stats), ptr(ws), s), "vg_graphnorm_fwd_h")
        x, ldx = y, ldy
        m._t(f"gat{b}", y, cout)
    return x, ldx


class HalfGenerator:
    def __init__(self, generator):
        from .models import conv_kind

        if conv_kind(generator) != "GATCONV":
            raise ValueError(f"the f16 kernels are built for GATCONV generators only, not {conv_kind(generator)}")
        self.G = generator
        self.trace = None  # a list: the forward appends (name, f32 copy) of every stage (debugging)
        self.refresh()

    def _t(self, name, t, c):
        if self.trace is not None:
            self.trace.append((name, t[:, :c].float().clone()))

    @torch.no_grad()
    def refresh(self) -> None:
        G = self.G
        self._md = None  # the native model descriptor points at the images below
        dev = next(G.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("vgan HIP ops require tensors on a ROCm device (no CPU fallback)")
        self.device = dev
        self.matched = self._mlp_blocks(G.matched_features_encoder)
        self.mlp = self._mlp_blocks(G.mlp_encoder)
        dec = list(G.decoder.children())
        self.decoder = self._mlp_blocks(nn.Sequential(*dec[:-1]))
        head: nn.Linear = dec[-1]
        self.head = (_w16(head.weight), head.bias.detach().float().contiguous(), head.out_features,
                     head.in_features)
        self.gat: List[tuple] = []
        enc = G.encoder
        for b in range(enc.num_blocks):
            conv = getattr(enc, f"module_{4 * b}")
            norm = getattr(enc, f"module_{4 * b + 1}")
            self.gat.append((_w16(conv.lin.weight), conv.att_src.detach().reshape(-1).float().contiguous(),
                             conv.att_dst.detach().reshape(-1).float().contiguous(),
                             conv.bias.detach().float().contiguous(), conv.in_channels, conv.out_channels,
                             float(conv.negative_slope), norm.weight.detach().float().contiguous(),
                             norm.bias.detach().float().contiguous(),
                             norm.mean_scale.detach().float().contiguous(), float(norm.eps)))

    @staticmethod
    def _mlp_blocks(mlp: nn.Module) -> List[tuple]:
        mods = list(mlp.children())
        out = []
        for i in range(0, len(mods), 3):
            lin, ln, act = mods[i:i + 3]
            if not (isinstance(lin, nn.Linear) and isinstance(ln, nn.LayerNorm) and isinstance(act, nn.LeakyReLU)):
                raise TypeError("expected [Linear, LayerNorm, LeakyReLU] blocks")
            out.append((_w16(lin.weight), lin.bias.detach().float().contiguous(),
                        ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(),
                        float(ln.eps), float(act.negative_slope), lin.out_features, lin.in_features))
        return out

    # ----------------------------------------------------------------- layers
    def _run_mlp(self, blocks, a: torch.Tensor, lda: int, k_in: int, rows: int, last_out=None, last_ld=0):
        """The MLP's blocks over ``rows`` rows of ``a`` (stride lda, k_in
        columns); the last block writes into ``last_out`` (stride last_ld) when
        given.  Returns (output, its stride)."""
        s = stream_handle(self.device)
        k = k_in
        for j, (w, b, g, be, eps, slope, m, kin) in enumerate(blocks):
            if _r8(kin) != _r8(k):
                raise ValueError("MLP input width mismatch")
            if j == len(blocks) - 1 and last_out is not None:
                out, ldo = last_out, last_ld
            else:
                out, ldo = torch.empty(rows, _r8(m), dtype=torch.float16, device=self.device), _r8(m)
            check(LIB.vg_hgemm_ln_act(ptr(a), lda, ptr(w), w.shape[1], rows, m, _r8(kin), ptr(b), ptr(g),
                                      ptr(be), eps, slope, ptr(out), ldo, s), "vg_hgemm_ln_act")
            a, lda, k = out, ldo, m
        return a, lda

    @torch.no_grad()
    def logits(self, local_graph, voxel_graph, z: torch.Tensor) -> torch.Tensor:
        """[k * N, 7] f32 logits of the eval forward for z [k, N, Z] (or [1, N, Z])."""
        cfg = self.G.configuration
        prep = vdata.prepared(local_graph, voxel_graph, cfg.NUM_CLASSES)
        dev = self.device
        s = stream_handle(dev)
        n = prep.voxel_x.shape[0]
        kk = z.shape[0] if z.dim() == 3 else 1
        rows = kk * n
        hl = self.matched[-1][6]
        hg = self.mlp[-1][6]
        enc_c = self.gat[-1][5]
        vd = prep.voxel_x.shape[1]
        zd = z.shape[-1]
        # row buffer [enc | x | em | voxel.x | z | pad]  (models.py:145 order)
        o_x, o_em = enc_c, enc_c + hg
        o_vx = o_em + hl
        o_z = o_vx + vd
        width = o_z + zd
        ld = _r8(width)
        buf = torch.empty(rows, ld, dtype=torch.float16, device=dev)
        view = buf.view(kk, n, ld)
        view[:, :, o_vx:o_z] = prep.voxel_x.to(torch.float16)
        view[:, :, o_z:width] = z.reshape(kk, n, zd).to(torch.float16)
        if ld > width:
            buf[:, width:].zero_()
        # program-feature encoder once on N rows, broadcast into every copy
        mx = prep.matched_x
        a0 = torch.zeros(n, _r8(mx.shape[1]), dtype=torch.float16, device=dev)
        a0[:, :mx.shape[1]] = mx
        em, _ = self._run_mlp(self.matched, a0, a0.shape[1], mx.shape[1], n)
        self._t("em", em, hl)
        view[:, :, o_em:o_em + hl] = em[:, :hl]
        # MLP encoder: reads [em | voxel.x | z] in place, writes x into its slice
        self._run_mlp(self.mlp, buf[:, o_em:], ld, width - o_em, rows, last_out=buf[:, o_x:], last_ld=ld)
        self._t("x", buf[:, o_x:], hg)
        # GAT encoder over the stacked block-diagonal graph
        csr = prep.csr if kk == 1 else prep.csr.stacked(kk)
        # (the last block writes enc into columns [0, enc_c) of the row buffer)
        _gat_encoder(self, buf[:, o_x:], ld, rows, kk, n, csr, last_out=buf, last_ld=ld)
        # decoder over the whole row buffer, f32 logits
        d, ldd = self._run_mlp(self.decoder, buf, ld, width, rows)
        w, bias, m, kin = self.head
        logits = torch.empty(rows, m, dtype=torch.float32, device=dev)
        check(LIB.vg_hgemm(ptr(d), ldd, ptr(w), w.shape[1], rows, m, _r8(kin), ptr(bias), 0, 0.0, ptr(logits), m, 1,
                           s), "vg_hgemm")
        return logits

    # ------------------------------------------------- one native call per batch
    def _native_model(self):
        """The vg_hgen_model of the current weight images (rebuilt by refresh)."""
        from ._lib import VG_HGEN_MAX_BLOCKS, VG_HGEN_MAX_LAYERS, VgHgenModel

        md = self.__dict__.get("_md")
        if md is not None:
            return md
        if max(len(self.matched), len(self.mlp), len(self.decoder)) > VG_HGEN_MAX_LAYERS or \
                len(self.gat) > VG_HGEN_MAX_BLOCKS:
            raise ValueError("generator too deep for vg_hgen_sweep")
        md = VgHgenModel()
        md.n_matched, md.n_mlp, md.n_blocks, md.n_dec = len(self.matched), len(self.mlp), len(self.gat), \
            len(self.decoder)

        def lin(dst, blk):
            w, b, g, be, eps, slope, m, kin = blk
            dst.weight, dst.ldw, dst.bias, dst.gamma, dst.beta = w.data_ptr(), w.shape[1], b.data_ptr(), \
                g.data_ptr(), be.data_ptr()
            dst.eps, dst.slope, dst.in_, dst.out = eps, slope, kin, m

        for dst, src in ((md.matched, self.matched), (md.mlp, self.mlp), (md.dec, self.decoder)):
            for i, blk in enumerate(src):
                lin(dst[i], blk)
        w, bias, m, kin = self.head
        md.head.weight, md.head.ldw, md.head.bias, md.head.in_, md.head.out = w.data_ptr(), w.shape[1], \
            bias.data_ptr(), kin, m
        for i, (w, att_s, att_d, bias, cin, cout, slope, gw, gb, gms, eps) in enumerate(self.gat):
            d = md.block[i]
            d.lin_weight, d.ldw, d.att_src, d.att_dst, d.bias, d.slope = w.data_ptr(), w.shape[1], att_s.data_ptr(), \
                att_d.data_ptr(), bias.data_ptr(), slope
            d.gn_weight, d.gn_bias, d.gn_mean_scale, d.gn_eps, d.in_, d.out = gw.data_ptr(), gb.data_ptr(), \
                gms.data_ptr(), eps, cin, cout
        self._md = md
        return md

    @torch.no_grad()
    def sweep_labels(self, local_graph, voxel_graph, copies: int, taus: torch.Tensor,
                     logits: Optional[torch.Tensor] = None, graph: Optional[bool] = None) -> torch.Tensor:
        """InferenceSweep._forward on this f16 generator as ONE native call
        (vg_hgen_sweep): RNG.reset(), z for ``copies`` stacked copies, the
        forward, Exp(1) noise, the Gumbel head at ``taus`` [copies] and the
        argmax -- the same kernels in the same order as ``__call__`` preceded
        by the reset and z draw, so the [copies, N] int8 labels are
        bit-identical to that path's.  ``logits`` [copies * N, classes] f32
        receives the logits when given.  ``graph`` (default VGAN_HGEN_GRAPH):
        the call captured into a hipGraph and launched as one
        (vg_hgen_sweep_graphed), unless the stream is already capturing."""
        import ctypes

        from ._lib import LIB, VgHgenBatch

        G = self.G
        cfg = G.configuration
        prep = vdata.prepared(local_graph, voxel_graph, cfg.NUM_CLASSES)
        dev = self.device
        rng = G.rng
        if rng.mode != "device":
            raise ValueError("vg_hgen_sweep draws z and the noise on the device (RNG mode 'device')")
        had = dict(rng._iters)
        ctrs = rng.reset(defer=True)
        for t in ctrs:  # counters of other devices advance as RNG.reset would
            if t.device != dev:
                t.add_(1)
        it = rng._iter(dev)
        advance = 1 if any(t.device == dev for t in had.values()) else 0
        salt0 = rng._salt
        rng._salt = salt0 + 2  # z (RNG.normal) and the Gumbel noise (RNG.exponential)
        vx, mx = prep.voxel_x.contiguous(), prep.matched_x.contiguous()
        csr = prep.csr
        n = int(vx.shape[0])
        for name, t in (("taus", taus), ("voxel_x", vx), ("matched_x", mx), ("csr.row_ptr", csr.row_ptr),
                        ("csr.col", csr.col)):
            if t.device != dev:  # raw pointers go to device kernels: a host or other-device tensor is refused
                raise ValueError(f"sweep_labels: {name} is on {t.device}, the generator on {dev}")
        tt = taus.reshape(-1).to(torch.float32).contiguous()
        if tt.numel() != copies:
            raise ValueError("one temperature per stacked copy")
        bt = VgHgenBatch()
        bt.n, bt.copies, bt.voxel_dim, bt.matched_dim, bt.z_dim, bt.num_edges = n, int(copies), vx.shape[1], \
            mx.shape[1], int(cfg.Z_DIM), csr.num_edges
        bt.voxel_x, bt.matched_x, bt.row_ptr, bt.col, bt.taus = vx.data_ptr(), mx.data_ptr(), \
            csr.row_ptr.data_ptr(), csr.col.data_ptr(), tt.data_ptr()
        bt.seed, bt.iter, bt.advance_iter = int(rng.seed) & ((1 << 64) - 1), it.data_ptr(), advance
        bt.z_salt, bt.noise_salt = 0x40000000 | (salt0 + 1), 0x40000000 | (salt0 + 2)
        md = self._native_model()
        need = int(LIB.vg_hgen_arena_bytes(ctypes.byref(md), ctypes.byref(bt)))
        if need < 0:
            raise ValueError(f"vg_hgen_arena_bytes: {need}")
        arena = self.__dict__.get("_arena")
        if arena is None or arena.numel() < need:
            # earlier arenas stay alive: a captured sweep graph may still replay on them
            if arena is not None:
                self.__dict__.setdefault("_old_arenas", []).append(arena)
            arena = self._arena = torch.empty(need + need // 4, dtype=torch.uint8, device=dev)
        labels = torch.empty(copies, n, dtype=torch.int8, device=dev)
        if logits is not None and (logits.dtype != torch.float32 or not logits.is_contiguous() or
                                   logits.numel() != copies * n * self.head[2]):
            raise ValueError("logits must be a contiguous f32 [copies * N, classes] tensor")
        lg = None if logits is None else logits.data_ptr()
        # the generator's device is current for the native calls: the graph
        # handle's capture stream belongs to the device current at its creation
        with torch.cuda.device(dev):
            if (_GRAPH if graph is None else graph) and not torch.cuda.is_current_stream_capturing():
                check(LIB.vg_hgen_sweep_graphed(self._graph_handle(), ctypes.byref(md), ctypes.byref(bt),
                                                arena.data_ptr(), arena.numel(), labels.data_ptr(), lg,
                                                stream_handle(dev)), "vg_hgen_sweep_graphed")
            else:
                check(LIB.vg_hgen_sweep(ctypes.byref(md), ctypes.byref(bt), arena.data_ptr(), arena.numel(),
                                        labels.data_ptr(), lg, stream_handle(dev)), "vg_hgen_sweep")
        return labels

    def _graph_handle(self) -> int:
        """The two executable graphs of vg_hgen_sweep_graphed, destroyed with
        this object (after their last launches complete)."""
        h = self.__dict__.get("_hgraph")
        if h is None:
            with torch.cuda.device(self.device):  # the capture stream is made on the current device
                h = LIB.vg_hgen_graph_create()
            if not h:
                raise RuntimeError("vg_hgen_graph_create failed")
            self._hgraph = h
            weakref.finalize(self, LIB.vg_hgen_graph_destroy, h)
        return h

    def graph_stats(self) -> Tuple[int, int]:
        """(instantiations, in-place updates) of the graphed sweep so far."""
        import ctypes

        h = self.__dict__.get("_hgraph")
        if h is None:
            return 0, 0
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        check(LIB.vg_hgen_graph_stats(h, ctypes.byref(a), ctypes.byref(b)), "vg_hgen_graph_stats")
        return a.value, b.value

    @torch.no_grad()
    def __call__(self, local_graph, voxel_graph, z: torch.Tensor, noise: Optional[torch.Tensor] = None,
                 tau=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(logits, label_hard, label_soft) like ``VoxelGNNGenerator.forward`` in
        eval mode; [k, N, 7] for a stacked z [k, N, Z]."""
        logits = self.logits(local_graph, voxel_graph, z)
        if noise is None:
            noise = self.G.rng.exponential(logits.shape, logits.device)
        tau = self.G.tau if tau is None else tau
        hard, soft = ops.gumbel_head(logits, noise.reshape(logits.shape), tau)
        if z.dim() == 3 and z.shape[0] > 1:
            k = z.shape[0]
            return logits.view(k, -1, logits.shape[1]), hard.view(k, -1, hard.shape[1]), soft.view(k, -1, soft.shape[1])
        return logits, hard, soft


class HalfCritic:
    """f16 scorer of a ``VoxelGNNDiscriminator`` for the sweep's best-of-k
    (``InferenceSweep(..., critic=D, critic_dtype="f16")``):
    a snapshot of D's parameters in the f16 layout of ``include/vgan.h`` and
    ``VoxelGNNDiscriminator.score_labels`` on the f16 kernels --

    * the copy-invariant columns [matched | voxel.x] of the first Linear once
      on N rows (``vg_hgemm``, f32 out, bias included), the label columns added
      per candidate from the int8 labels (``vg_hcritic_embed_labels``);
    * the other [Linear, ReLU] layers of the MLP encoder one ``vg_hgemm`` each;
    * the GAT encoder as ``HalfGenerator.logits`` runs it, each copy normalised
      on its own;
    * the decoder, Sigmoid included, in one launch (``vg_hcritic_decode``: f32
      parameters, f32 activations) for the reference's halving widths, else one
      ``vg_hgemm`` per layer.

    Eval semantics, no draw from any RNG.  Scores differ from the f32
    ``score_labels`` by f16 rounding (``tests/test_hcritic_gpu.py`` states the
    bound).  Call ``refresh()`` after the critic's weights change."""

    def __init__(self, critic):
        from .models import conv_kind

        if conv_kind(critic) != "GATCONV":
            raise ValueError(f"the f16 kernels are built for GATCONV critics only, not {conv_kind(critic)}")
        self.D = critic
        self.trace = None  # a list: score_labels(native=False) appends (name, f32 copy) of every stage (debugging)
        self.refresh()

    def _t(self, name, t, c):
        if self.trace is not None:
            self.trace.append((name, t[:, :c].float().clone()))

    @torch.no_grad()
    def refresh(self) -> None:
        D = self.D
        self._md = None  # the native model descriptor points at the images below
        dev = next(D.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("vgan HIP ops require tensors on a ROCm device (no CPU fallback)")
        self.device = dev
        self.classes = int(D.configuration.NUM_CLASSES)

        def f32(t):
            return t.detach().float().contiguous().clone()

        def linears(seq, what, sigmoid_ok):
            """[Linear, ReLU] ... of ``seq`` (the decoder: a bare last Linear, then maybe a Sigmoid)."""
            mods = list(seq.children())
            has_sigmoid = bool(mods) and isinstance(mods[-1], nn.Sigmoid)
            if has_sigmoid:
                if not sigmoid_ok:
                    raise TypeError(f"{what}: unexpected Sigmoid")
                mods = mods[:-1]
            lins = []
            i = 0
            while i < len(mods):
                lin = mods[i]
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                if not isinstance(lin, nn.Linear) or (not relu and (not sigmoid_ok or i != len(mods) - 1)):
                    raise TypeError(f"{what}: expected [Linear, ReLU] layers")
                lins.append(lin)
                i += 2 if relu else 1
            return lins, has_sigmoid

        mlp, _ = linears(D.mlp_encoder, "mlp_encoder", False)
        dec, self.has_sigmoid = linears(D.decoder, "decoder", True)
        if not mlp or not dec or dec[-1].out_features != 1:
            raise TypeError("expected an MLP encoder and a decoder ending in Linear(., 1)")
        self.feat = mlp[0].in_features - self.classes
        if self.feat < 1:
            raise ValueError("the first Linear reads [matched | voxel.x | one-hot label]")

        def lin(l, cols=None):
            """(f16 image, f32 matrix, bias, out, in)"""
            w = l.weight if cols is None else l.weight[:, :cols]
            b = f32(l.bias) if l.bias is not None else torch.zeros(l.out_features, dtype=torch.float32, device=dev)
            return (_w16(w), f32(l.weight), b, l.out_features, l.in_features)

        self.mlp = [lin(mlp[0], self.feat)] + [lin(l) for l in mlp[1:]]
        self.dec = [lin(l) for l in dec]
        self.gat: List[tuple] = []
        enc = D.encoder
        for b in range(enc.num_blocks):
            conv = getattr(enc, f"module_{4 * b}")
            norm = getattr(enc, f"module_{4 * b + 1}")
            self.gat.append((_w16(conv.lin.weight), f32(conv.att_src.reshape(-1)), f32(conv.att_dst.reshape(-1)),
                             f32(conv.bias), conv.in_channels, conv.out_channels, float(conv.negative_slope),
                             f32(norm.weight), f32(norm.bias), f32(norm.mean_scale), float(norm.eps)))

    # ------------------------------------------------------------ batch inputs
    def _inputs(self, local_graph, voxel_graph, pred):
        """(prep, the f16 image of matched_voxel_x -- cached on the prepared
        batch --, k, n, pred's row stride)"""
        prep = vdata.prepared(local_graph, voxel_graph, self.classes)
        mvx = prep.matched_voxel_x
        n, f = mvx.shape
        if f != self.feat:
            raise ValueError(f"score_labels: the batch has {f} [matched | voxel.x] columns, the critic reads {self.feat}")
        if mvx.device != self.device or pred.device != self.device:
            raise ValueError(f"score_labels: the batch and pred must be on {self.device}")
        if pred.dim() != 2 or pred.shape[1] != n:
            raise ValueError(f"score_labels: pred must be int8 [k, {n}]")
        k, _, stride = ops._candidates(pred, "score_labels")
        m16 = prep.consts.get("hcritic_mvx16")
        if m16 is None:
            m16 = torch.zeros(n, _r8(f), dtype=torch.float16, device=self.device)
            m16[:, :f] = mvx
            prep.consts["hcritic_mvx16"] = m16
        return prep, m16, k, n, stride

    # --------------------------------------------- the launches issued from Python
    def _decode(self, x, ldx, rows, scores):
        """vg_hcritic_decode; VG_EINVAL (no kernel for these widths): one
        vg_hgemm per layer and the Sigmoid -- hcritic_engine.hip's choice."""
        import ctypes

        from ._lib import VG_EINVAL

        s = stream_handle(self.device)
        nd = len(self.dec)
        widths = (ctypes.c_int32 * (nd + 1))(self.dec[0][4], *[d[3] for d in self.dec])
        ws = (ctypes.c_void_p * nd)(*[d[1].data_ptr() for d in self.dec])
        bs = (ctypes.c_void_p * nd)(*[d[2].data_ptr() for d in self.dec])
        rc = LIB.vg_hcritic_decode(ptr(x), ldx, rows, widths, nd, ws, bs, int(self.has_sigmoid), ptr(scores), s)
        if rc != VG_EINVAL:
            check(rc, "vg_hcritic_decode")
            return
        for w16, _, b, m, kin in self.dec[:-1]:
            out = torch.empty(rows, _r8(m), dtype=torch.float16, device=self.device)
            check(LIB.vg_hgemm(ptr(x), ldx, ptr(w16), w16.shape[1], rows, m, _r8(kin), ptr(b), 1, 0.0, ptr(out), _r8(m),
                               0, s), "vg_hgemm")
            x, ldx = out, _r8(m)
            self._t("dec", x, m)
        w16, _, b, m, kin = self.dec[-1]
        check(LIB.vg_hgemm(ptr(x), ldx, ptr(w16), w16.shape[1], rows, 1, _r8(kin), ptr(b), 0, 0.0, ptr(scores), 1, 1, s),
              "vg_hgemm")
        if self.has_sigmoid:
            check(LIB.vg_hcritic_sigmoid(ptr(scores), rows, s), "vg_hcritic_sigmoid")

    def _score_python(self, prep, m16, pred, kk, n, stride) -> torch.Tensor:
        dev = self.device
        s = stream_handle(dev)
        rows = kk * n
        w16, w32, b0, hh, ktot = self.mlp[0]
        f, ldb = self.feat, _r8(hh)
        base = torch.empty(n, ldb, dtype=torch.float32, device=dev)
        check(LIB.vg_hgemm(ptr(m16), m16.shape[1], ptr(w16), w16.shape[1], n, hh, _r8(f), ptr(b0), 0, 0.0, ptr(base),
                           ldb, 1, s), "vg_hgemm")
        x = torch.empty(rows, ldb, dtype=torch.float16, device=dev)
        check(LIB.vg_hcritic_embed_labels(ptr(base), ldb, ptr(w32), ktot, f, self.classes, ptr(pred), stride, kk, n,
                                          hh, ptr(x), ldb, s), "vg_hcritic_embed_labels")
        ldx = ldb
        self._t("embed", x, hh)
        for w16, _, b, m, kin in self.mlp[1:]:
            out = torch.empty(rows, _r8(m), dtype=torch.float16, device=dev)
            check(LIB.vg_hgemm(ptr(x), ldx, ptr(w16), w16.shape[1], rows, m, _r8(kin), ptr(b), 1, 0.0, ptr(out), _r8(m),
                               0, s), "vg_hgemm")
            x, ldx = out, _r8(m)
            self._t("mlp", x, m)
        csr = prep.csr if kk == 1 else prep.csr.stacked(kk)
        x, ldx = _gat_encoder(self, x, ldx, rows, kk, n, csr)
        scores = torch.empty(kk, n, dtype=torch.float32, device=dev)
        self._decode(x, ldx, rows, scores)
        return scores

    # ------------------------------------------------------- one native call
    def _native_model(self):
        """The vg_hcritic_model of the current weight images (rebuilt by refresh)."""
        from ._lib import VG_HGEN_MAX_BLOCKS, VG_HGEN_MAX_LAYERS, VgHcriticModel

        md = self.__dict__.get("_md")
        if md is not None:
            return md
        if max(len(self.mlp), len(self.dec)) > VG_HGEN_MAX_LAYERS or len(self.gat) > VG_HGEN_MAX_BLOCKS:
            raise ValueError("critic too deep for vg_hcritic_score")
        md = VgHcriticModel()
        md.n_mlp, md.n_blocks, md.n_dec = len(self.mlp), len(self.gat), len(self.dec)
        md.has_sigmoid, md.classes = int(self.has_sigmoid), self.classes
        for dst, src in ((md.mlp, self.mlp), (md.dec, self.dec)):
            for i, (w16, w32, b, m, kin) in enumerate(src):
                d = dst[i]
                d.weight, d.ldw, d.weight_f32, d.bias, d.in_, d.out = w16.data_ptr(), w16.shape[1], w32.data_ptr(), \
                    b.data_ptr(), kin, m
        for i, (w, att_s, att_d, bias, cin, cout, slope, gw, gb, gms, eps) in enumerate(self.gat):
            d = md.block[i]
            d.lin_weight, d.ldw, d.att_src, d.att_dst, d.bias, d.slope = w.data_ptr(), w.shape[1], att_s.data_ptr(), \
                att_d.data_ptr(), bias.data_ptr(), slope
            d.gn_weight, d.gn_bias, d.gn_mean_scale, d.gn_eps, d.in_, d.out = gw.data_ptr(), gb.data_ptr(), \
                gms.data_ptr(), eps, cin, cout
        self._md = md
        return md

    def _score_native(self, prep, m16, pred, kk, n, stride, graph_ptr=None):
        """(scores [k, N], CriticSelection or None) from one vg_hcritic_score call."""
        import ctypes

        from ._lib import VgHcriticBatch

        dev = self.device
        csr = prep.csr
        for name, t in (("csr.row_ptr", csr.row_ptr), ("csr.col", csr.col)):
            if t.device != dev:  # raw pointers go to device kernels
                raise ValueError(f"score_labels: {name} is on {t.device}, the critic on {dev}")
        bt = VgHcriticBatch()
        bt.n, bt.copies, bt.feat, bt.num_edges, bt.ld_mvx = n, kk, self.feat, csr.num_edges, m16.shape[1]
        bt.row_ptr, bt.col, bt.mvx, bt.pred, bt.copy_stride = csr.row_ptr.data_ptr(), csr.col.data_ptr(), \
            m16.data_ptr(), pred.data_ptr(), stride
        sel = None
        out = (None, None, None)
        if graph_ptr is not None:
            if graph_ptr.device != dev or graph_ptr.dtype != torch.int64 or graph_ptr.dim() != 1 or \
                    graph_ptr.numel() < 2 or not graph_ptr.is_contiguous():
                raise ValueError(f"select: ptr must be a contiguous int64 [G + 1] tensor on {dev}")
            g = graph_ptr.numel() - 1
            bt.ptr, bt.num_graphs = graph_ptr.data_ptr(), g
            sel = ops.CriticSelection(torch.empty(n, dtype=torch.int8, device=dev),
                                      torch.empty(g, dtype=torch.int32, device=dev),
                                      torch.empty(kk, g, dtype=torch.float64, device=dev))
            out = (sel.score.data_ptr(), sel.best.data_ptr(), sel.labels.data_ptr())
        md = self._native_model()
        need = int(LIB.vg_hcritic_arena_bytes(ctypes.byref(md), ctypes.byref(bt)))
        if need < 0:
            raise ValueError(f"vg_hcritic_arena_bytes: {need}")
        arena = self.__dict__.get("_arena")
        if arena is None or arena.numel() < need:
            # earlier arenas stay alive: a captured graph may still replay on them
            if arena is not None:
                self.__dict__.setdefault("_old_arenas", []).append(arena)
            arena = self._arena = torch.empty(need + need // 4, dtype=torch.uint8, device=dev)
        scores = torch.empty(kk, n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(LIB.vg_hcritic_score(ctypes.byref(md), ctypes.byref(bt), arena.data_ptr(), arena.numel(),
                                       scores.data_ptr(), *out, stream_handle(dev)), "vg_hcritic_score")
        return scores, sel

    @torch.no_grad()
    def score_labels(self, local_graph, voxel_graph, pred: torch.Tensor, native: bool = True) -> torch.Tensor:
        """Per-voxel scores [k, N] f32 of the k candidate labellings ``pred``
        (int8 [k, N] on the device; a row-strided view is fine): what
        ``VoxelGNNDiscriminator.score_labels`` gives, on the f16 kernels.
        ``native``: one ``vg_hcritic_score`` call; False: the same launches
        issued from Python in the same order -- the same bits."""
        prep, m16, k, n, stride = self._inputs(local_graph, voxel_graph, pred)
        if native:
            return self._score_native(prep, m16, pred, k, n, stride)[0]
        return self._score_python(prep, m16, pred, k, n, stride)

    @torch.no_grad()
    def select(self, local_graph, voxel_graph, pred: torch.Tensor) -> "ops.CriticSelection":
        """The best candidate per building by mean score: scoring, mean,
        arg-max and gather (``vg_sweep_select_score``) in the ONE native call."""
        prep, m16, k, n, stride = self._inputs(local_graph, voxel_graph, pred)
        return self._score_native(prep, m16, pred, k, n, stride, graph_ptr=voxel_graph.ptr)[1]
