"""hipGraph lifecycle of the host code.

``warm_up`` / ``capture``: a static batch (``Trainer.capture``, the evaluation
graphs, ``InferenceSweep.run_batch``) -- the body runs once on a side stream,
then is captured into a pool; undoing the warm-up's draws is the caller's.
``Recorder`` / ``ExecPair``: a batch seen once (``Trainer.step_fresh``,
``InferenceSweep.run_fresh``) -- its launches are recorded, not run, and one of
two executable graphs is updated in place from the recording.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import LIB

# what ExecPair calls, by module-level names (tests/test_graphs_cpu.py patches them)
_exec_update = LIB.vg_graph_exec_update  # (executable graph, recorded graph) handles -> 0 when updated
_device_synchronize = torch.cuda.synchronize
_new_event = torch.cuda.Event


def warm_up(device, fn) -> None:
    """fn() once on a fresh side stream, outside any capture (lazy
    initialisation, constant buffers, allocations)."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)


def capture(pool, fn):
    """(graph, fn's result): fn captured into ``pool``.  Thread-local capture
    mode: the loader's thread keeps collating into pinned buffers and
    uploading meanwhile."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
        out = fn()
    return g, out


class Recorder:
    """The side stream and memory pool (``pool``, else its own) that fresh
    batches are recorded on."""

    def __init__(self, device, pool=None):
        self.stream = torch.cuda.Stream(device)
        self.pool = torch.cuda.graph_pool_handle() if pool is None else pool

    def record(self, fn):
        """(recorded graph, fn's result): fn's launches recorded -- not run.
        torch.cuda.graph() would synchronise the device, collect garbage and
        empty the allocator cache on every capture: the low-level calls
        record without any of that (thread-local mode, as ``capture``)."""
        # No stream waits around the recording: it enqueues no device work,
        # so neither side.wait_stream(cur) nor cur.wait_stream(side) would
        # order anything -- and each costs the device a drain of its queue
        # (a cross-queue barrier): 8.30-8.46 vs 7.71-7.72 ms per fresh step
        # with them (profiles/r04_record_waits_ab.txt).
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.stream(self.stream):
            g.capture_begin(pool=self.pool, capture_error_mode="thread_local")
            try:
                out = fn()
            finally:
                g.capture_end()
        return g, out


class ExecPair:
    """The executable graphs that replay the recordings of one launch sequence.

    Two of them, used by alternate batches, are updated in place from each
    new recording (vg_graph_exec_update) -- instantiating a graph per batch
    and destroying the previous one cost ~3 ms of host time per step.  An
    update rewrites an executable graph's kernel arguments, and HIP does not
    promise that launches of it already queued keep the old ones, so an
    executable graph is updated only after its last launches -- two batches
    back -- have finished: a host wait on the event ``launched`` recorded
    behind them (the device is normally less than one batch behind the host,
    so the wait rarely stalls).

    Recorded graphs are released in batches: destroying one while the device
    is busy blocks the runtime (every thread's launches) for ~8 ms
    (tools/graph_destroy_probe.py; ~0.3 ms on an idle device), so they are
    kept until ``keep`` have gathered and destroyed after one device
    synchronisation.  ``force_instantiate``: no updates."""

    def __init__(self, keep: int, force_instantiate: bool = False):
        self.owners = [None, None]  # the recording each executable graph was instantiated from
        self.events = [None, None]  # behind each one's last launches
        self.parity = 1
        self.dead = []
        self.keep = keep
        self.force_instantiate = force_instantiate

    def adopt(self, g) -> ctypes.c_void_p:
        """The executable graph that replays recording ``g``."""
        j = self.parity = (self.parity + 1) % 2
        owner = self.owners[j]
        if self.events[j] is not None:
            self.events[j].synchronize()
        if owner is None or self.force_instantiate or \
                _exec_update(owner.raw_cuda_graph_exec(), g.raw_cuda_graph()) != 0:
            g.instantiate()  # first batches, or a launch sequence of another shape
            if owner is not None:
                self.dead.append(owner)
            owner = self.owners[j] = g
        else:
            self.dead.append(g)
        return ctypes.c_void_p(owner.raw_cuda_graph_exec())

    def launched(self, stream) -> None:
        """Record the event behind the last launch of ``adopt``'s executable graph."""
        ev = self.events[self.parity] = _new_event()
        ev.record(stream)

    def release_if_due(self, device) -> None:
        if len(self.dead) >= self.keep:
            _device_synchronize(device)
            self.dead.clear()
