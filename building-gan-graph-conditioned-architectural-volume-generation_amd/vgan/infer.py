"""Generator-only inference sweep (BASELINE.json configs[4]): many buildings,
a Gumbel temperature schedule, hipGraph replay.

The reference samples layouts in ``Trainer.test`` (``trainer.py:749-806``): per
test batch one ``generator(local_graph, voxel_graph, z)`` forward in eval mode
(``models.py:119-155``; ``F.gumbel_softmax`` at tau = 1) and argmax labels.
``InferenceSweep`` runs that forward for a whole schedule of temperatures at
once: one STACKED forward per batch over ``len(taus)`` copies (z [k, N, Z], each
copy normalised on its own -- GraphNorm segments -- exactly as k separate
forwards), and the Gumbel head reads copy c's temperature from a device
vector (``vg_gumbel_fwd_dev``), so a captured hipGraph follows a new schedule
without re-capture.  Per batch the result is the predicted type of every voxel
for every temperature, [k, N] int8.

``graphed=True`` captures the stacked forward of a batch on first use and
replays it afterwards (the batch object caches its graph, as the training
step does); a one-pass sweep over batches seen once runs eagerly.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Union

import torch

from . import data as vdata
from . import graphs as vgraphs
from . import ops
from ._lib import LIB, check, stream_handle
from .gcscope import gc_frozen


# run_stream launches each batch's forward eagerly; VGAN_SWEEP_STREAM=record
# records it and updates an executable graph instead (run_fresh).  Eager
# measured faster: recording costs the host what launching does, and the
# update, the graph launch and its event come on top -- f16 147-204k vs
# 129-167k samples/s, alternated (profiles/r04_sweep_eager_ab.txt)
_STREAM = os.environ.get("VGAN_SWEEP_STREAM", "eager")
# the f16 sweep's forward of a batch as one native call (vg_hgen_sweep, csrc/
# hgen_engine.hip) instead of ~70 launches issued from Python; 0: the Python path
_NATIVE = os.environ.get("VGAN_HGEN_NATIVE", "1") == "1"


def geometric_taus(t0: float = 1.0, t1: float = 0.1, steps: int = 10) -> List[float]:
    """Annealing schedule tau_i = t0 (t1/t0)^(i/(steps-1)) (cfg #5)."""
    if steps <= 1:
        return [float(t0)]
    r = math.log(t1 / t0) / (steps - 1)
    return [float(t0 * math.exp(r * i)) for i in range(steps)]


class InferenceSweep:
    """``dtype="f16"`` runs the forward on the f16 kernels (``vgan.half``,
    configs[4]'s precision); "f32" on the training path's kernels.
    ``critic``: a ``VoxelGNNDiscriminator`` trained next to the generator, for
    ``select="critic"``.  It scores in f32 whatever ``dtype``, unless
    ``critic_dtype="f16"``: then scoring and selection are one native call on
    the f16 kernels (``vgan.half.HalfCritic``; GATCONV critics only), again
    whatever ``dtype``.  Call ``half_critic.refresh()`` after the critic's
    weights change."""

    def __init__(self, generator, taus: Sequence[float], graphed: bool = False, dtype: str = "f32", critic=None,
                 critic_dtype: str = "f32"):
        if dtype not in ("f32", "f16"):
            raise ValueError(f"dtype {dtype!r}: f32 or f16")
        if critic_dtype not in ("f32", "f16"):
            raise ValueError(f"critic_dtype {critic_dtype!r}: f32 or f16")
        self.G = generator
        self.D = critic
        self.taus = [float(t) for t in taus]
        self.graphed = graphed
        self.dtype = dtype
        self.half = None
        if dtype == "f16":
            from .half import HalfGenerator

            self.half = HalfGenerator(generator)  # ValueError for a GATV2CONV generator (f32 only)
        self.critic_dtype = critic_dtype
        self.half_critic = None
        if critic_dtype == "f16" and critic is not None:
            from .half import HalfCritic

            self.half_critic = HalfCritic(critic)  # ValueError for a GATV2CONV critic (f32 only)
        dev = next(generator.parameters()).device
        self.tau_t = torch.tensor(self.taus, dtype=torch.float32, device=dev)
        # one memory pool for every batch's graph: replays are sequential and
        # only each graph's output stays referenced, so intermediates are shared
        self._pool = torch.cuda.graph_pool_handle() if graphed else None
        # run_fresh: its recorder (made on first use, sharing the pool), the
        # executable graphs of the stacked forward and the result's buffer
        self._recorder = None
        self._execs = vgraphs.ExecPair(64)
        self._fresh_out = None

    def set_taus(self, taus: Sequence[float]) -> None:
        """New schedule of the same length: captured graphs keep working."""
        if len(taus) != len(self.taus):
            raise ValueError("a captured sweep keeps its number of temperatures")
        self.taus = [float(t) for t in taus]
        self.tau_t.copy_(torch.tensor(self.taus, dtype=torch.float32))

    @contextlib.contextmanager
    def _eval(self):
        """The generator in eval mode for the body, its mode restored after.
        Module.train() / eval() walk the whole module tree (~0.45 ms of host
        time each for the generator): a generator already in eval mode -- the
        sweeps below set it once for the whole loop -- is left alone.  The
        sweep's critic likewise: ``score_labels`` then finds it in eval mode
        and switches nothing per batch."""
        was = [m for m in (self.G, self.D) if m is not None and m.training]
        for m in was:
            m.eval()
        try:
            yield
        finally:
            for m in was:
                m.train()

    def _forward(self, local_graph, voxel_graph) -> torch.Tensor:
        G = self.G
        k = len(self.taus)
        if self.half is not None and _NATIVE and getattr(G.rng, "mode", None) == "device":
            # the whole batch in one native call (vg_hgen_sweep): bit-identical labels
            return self.half.sweep_labels(local_graph, voxel_graph, k, self.tau_t)
        n = voxel_graph.num_nodes
        G.rng.reset()  # advance the device counter: every (replayed) batch draws fresh z and noise
        z = G.rng.normal((k, n, G.configuration.Z_DIM), voxel_graph.x.device)
        if self.half is not None:
            _, hard, _ = self.half(local_graph, voxel_graph, z, tau=self.tau_t)
            return hard.reshape(k, n, -1).argmax(-1).to(torch.int8)
        saved = G.tau
        G.tau = self.tau_t
        try:
            _, hard, _ = G(local_graph, voxel_graph, z)
        finally:
            G.tau = saved
        return hard.reshape(k, n, -1).argmax(-1).to(torch.int8)

    @torch.no_grad()
    def generate(self, local_graph, voxel_graph):
        """(logits [N, K], label_hard [N, K]) of one sample per voxel at the
        schedule's single temperature: the evaluation forward of
        ``Trainer._validate_each_epoch`` / ``test`` (``trainer.py:545-548,
        769-772``), on the sweep's no-grad path (multi-source first layers, no
        concatenation).  Eval mode is the caller's."""
        if len(self.taus) != 1 or self.half is not None:
            raise ValueError("generate() is the one-temperature f32 forward")
        G = self.G
        G.rng.reset()
        z = G.rng.normal((1, voxel_graph.num_nodes, G.configuration.Z_DIM), voxel_graph.x.device)
        saved = G.tau
        G.tau = self.taus[0]
        try:
            logits, hard, _ = G(local_graph, voxel_graph, z, stacked=True)
        finally:
            G.tau = saved
        return logits.reshape(-1, logits.shape[-1]), hard.reshape(-1, hard.shape[-1])

    @torch.no_grad()
    def run_batch(self, local_graph, voxel_graph) -> torch.Tensor:
        """[len(taus), N] int8 predicted voxel types (device tensor)."""
        with self._eval():
            vdata.prepared(local_graph, voxel_graph, self.G.configuration.NUM_CLASSES)
            if not self.graphed:
                return self._forward(local_graph, voxel_graph)
            cached = voxel_graph.derived("sweep_graph")
            if cached is None or cached[0] is not self:
                forward = lambda: self._forward(local_graph, voxel_graph)  # noqa: E731
                vgraphs.warm_up(voxel_graph.x.device, forward)  # lazy allocations outside the capture
                cached = (self, *vgraphs.capture(self._pool, forward))
                voxel_graph.set_derived("sweep_graph", cached)
            cached[1].replay()
            return cached[2]

    @torch.no_grad()
    def run_fresh(self, local_graph, voxel_graph) -> torch.Tensor:
        """``run_batch`` for a batch seen once (a stream of distinct
        buildings): the stacked forward is RECORDED as a hipGraph and one of
        two executable graphs updated in place from it (vgan.graphs.ExecPair)
        -- no instantiation per batch; a recording of another launch shape
        (the f16 kernels pick their shapes from the sizes) instantiates a new
        one.  Returns [len(taus), N] int8, valid until the next call (clone
        to keep)."""
        with self._eval():
            prep = vdata.prepared(local_graph, voxel_graph, self.G.configuration.NUM_CLASSES)
            k = len(self.taus)
            if k > 1:  # the stacked graph (and its padded columns) before the recording
                prep.csr.stacked(k).ell()
            dev = voxel_graph.x.device
            cur = torch.cuda.current_stream(dev)
            if self._recorder is None:  # lazy initialisation outside any recording; its draws undone
                ctr = self.G.rng._iter(dev) if callable(getattr(self.G.rng, "_iter", None)) else None
                keep = ctr.clone() if ctr is not None else None
                self._forward(local_graph, voxel_graph)
                if ctr is not None:
                    ctr.copy_(keep)
                self._recorder = vgraphs.Recorder(dev, pool=self._pool)
            g, out = self._recorder.record(lambda: self._forward(local_graph, voxel_graph))
            check(LIB.vg_graph_launch(self._execs.adopt(g), stream_handle(dev)), "vg_graph_launch")
            if self._fresh_out is None or self._fresh_out.shape != out.shape:
                self._fresh_out = torch.empty_like(out)
            res = self._fresh_out
            res.copy_(out)  # out lives in the recording's pool, reused by the next batch
            self._execs.launched(cur)
            self._execs.release_if_due(dev)
            return res

    def _check_select(self, select: Optional[str]) -> None:
        if select is not None and select != "critic" and select not in ops.SELECT_CRITERIA:
            raise ValueError(f"select {select!r}: None or one of {sorted([*ops.SELECT_CRITERIA, 'critic'])}")
        if select == "critic" and self.D is None:
            raise ValueError("select 'critic' needs InferenceSweep(..., critic=<the trained discriminator>)")

    @torch.no_grad()
    def select(self, pred: torch.Tensor, local_graph, voxel_graph,
               criterion: str = "f1") -> Union[ops.SweepSelection, ops.CriticSelection]:
        """Best of the k candidates ``pred`` [k, N] (a ``run_batch`` /
        ``run_fresh`` result) per building -- ``criterion`` "f1": the macro-F1
        against the batch's true types (the reference's ``_visualize_one``,
        ``trainer.py:65-84``), "far": the FAR closest to the target -- scored,
        chosen and gathered on the device in one launch (``vg_sweep_select``)
        on the current stream, after and outside the captured or recorded
        forward.  "critic": the largest mean score of the sweep's critic --
        one stacked critic forward over the k candidates
        (``VoxelGNNDiscriminator.score_labels``), then mean, arg-max and
        gather in one launch (``vg_sweep_select_score``); a
        ``CriticSelection``.  With ``critic_dtype="f16"`` both steps are one
        native call on the f16 kernels (``HalfCritic.select``).  The critic
        runs in eval mode and draws nothing, so the generator's random stream
        is the same with and without it.  Device tensors; no host
        synchronisation."""
        if criterion == "critic":
            self._check_select(criterion)
            if self.half_critic is not None:
                return self.half_critic.select(local_graph, voxel_graph, pred)
            scores = self.D.score_labels(local_graph, voxel_graph, pred)
            return ops.sweep_select_score(scores, pred, voxel_graph.ptr)
        cfg = self.G.configuration
        prep = vdata.prepared(local_graph, voxel_graph, cfg.NUM_CLASSES)
        sa = voxel_graph.site_area
        if sa.dtype != torch.float32:
            sa = sa.float()
        return ops.sweep_select(pred, voxel_graph.ptr, prep.voxel_x, sa.contiguous(), truth=voxel_graph.type,
                                criterion=criterion, far_col=9, dy_col=4, dx_col=5,
                                dim_scale=float(cfg.NORMALIZATION_FACTOR_DIMENSION), void_class=cfg.VOID,
                                classes=cfg.NUM_CLASSES)

    @staticmethod
    def _selected_to_host(sels: List[Union[ops.SweepSelection, ops.CriticSelection]]) -> List[Dict[str, torch.Tensor]]:
        return [{k: getattr(s, k).cpu() for k in (("labels", "best", "score") if isinstance(s, ops.CriticSelection)
                                                  else ("labels", "best", "f1", "far_gen", "far_ref"))} for s in sels]

    def run_stream(self, batches: Iterable, collect: bool = False, select: Optional[str] = None) -> Dict[str, object]:
        """Sweep a stream of batches each seen once (each batch's forward
        launched eagerly, or recorded with ``run_fresh`` under
        VGAN_SWEEP_STREAM=record): counts and, with ``collect``, every
        batch's [k, N] predictions.  ``select`` "f1" / "far" / "critic": each
        batch's best candidate per building (``select``) right after its
        predictions -- before the next batch reuses their buffer; with
        ``collect``, ``res["selected"]`` holds per batch the host copies of
        labels, best, f1, far_gen and far_ref ("critic": labels, best and
        score)."""
        self._check_select(select)
        outs: List[torch.Tensor] = []
        sels: List[ops.SweepSelection] = []
        graphs = samples = nb = 0
        eager = _STREAM == "eager" and not self.graphed
        with self._eval(), gc_frozen():  # vgan/gcscope.py
            for local_graph, voxel_graph in batches:
                pred = self.run_batch(local_graph, voxel_graph) if eager else self.run_fresh(local_graph, voxel_graph)
                graphs += voxel_graph.num_graphs
                samples += voxel_graph.num_graphs * len(self.taus)
                nb += 1
                if select is not None:
                    sel = self.select(pred, local_graph, voxel_graph, select)
                    if collect:
                        sels.append(sel)
                if collect:
                    outs.append(pred.clone())
        res: Dict[str, object] = {"graphs": graphs, "samples": samples, "batches": nb}
        if collect:
            res["predictions"] = [o.cpu() for o in outs]
            if select is not None:
                res["selected"] = self._selected_to_host(sels)
        return res

    def run(self, batches: Iterable, collect: bool = False, select: Optional[str] = None) -> Dict[str, object]:
        """Sweep every (local_graph, voxel_graph) batch; returns counts and,
        with ``collect``, the per-batch [k, N] predictions (copied to the host
        once at the end).  ``select``: as in ``run_stream``."""
        self._check_select(select)
        outs: List[torch.Tensor] = []
        sels: List[ops.SweepSelection] = []
        graphs = samples = 0
        with self._eval(), gc_frozen():  # vgan/gcscope.py
            for local_graph, voxel_graph in batches:
                pred = self.run_batch(local_graph, voxel_graph)
                graphs += voxel_graph.num_graphs
                samples += voxel_graph.num_graphs * len(self.taus)
                if select is not None:
                    sel = self.select(pred, local_graph, voxel_graph, select)
                    if collect:
                        sels.append(sel)
                if collect:
                    outs.append(pred.clone() if self.graphed else pred)
        res: Dict[str, object] = {"graphs": graphs, "samples": samples}
        if collect:
            res["predictions"] = [o.cpu() for o in outs]
            if select is not None:
                res["selected"] = self._selected_to_host(sels)
        return res


def sweep(generator, batches, taus: Optional[Sequence[float]] = None, graphed: bool = False,
          collect: bool = False, dtype: str = "f32") -> Dict[str, object]:
    return InferenceSweep(generator, taus or geometric_taus(), graphed, dtype).run(batches, collect)
