"""vgan.graphs.ExecPair, driven with stand-in recordings and events (no
device): which slot adopts a recording, that a slot's executable graph is
touched only after the event behind its last launches has been waited on,
what joins the dead list, and when the list is released."""
import pytest

from vgan import graphs


class Recording:
    """Stands in for a torch.cuda.CUDAGraph(keep_graph=True) after capture_end."""

    def __init__(self, log, n):
        self.log, self.n, self.instantiated = log, n, False

    def instantiate(self):
        self.log.append(("instantiate", self.n))
        self.instantiated = True

    def raw_cuda_graph(self):
        return 1000 + self.n

    def raw_cuda_graph_exec(self):
        assert self.instantiated, "executable handle of a recording never instantiated"
        return 2000 + self.n


class Event:
    def __init__(self, log, n):
        self.log, self.n, self.stream = log, n, None

    def record(self, stream):
        self.log.append(("record", self.n))
        self.stream = stream

    def synchronize(self):
        assert self.stream is not None, "wait on an event never recorded"
        self.log.append(("wait", self.n))


@pytest.fixture
def rig(monkeypatch):
    """log: every call in order; rc: what the update call returns."""
    class Rig:
        def __init__(self):
            self.log, self.rc, self.events = [], 0, []

        def recording(self):
            r = Recording(self.log, sum(1 for e in self.log if e[0] == "new"))
            self.log.append(("new", r.n))
            return r

    rig = Rig()

    def update(graph_exec, graph):
        rig.log.append(("update", graph_exec - 2000, graph - 1000))
        return rig.rc

    def new_event():
        rig.events.append(Event(rig.log, len(rig.events)))
        return rig.events[-1]

    monkeypatch.setattr(graphs, "_exec_update", update)
    monkeypatch.setattr(graphs, "_new_event", new_event)
    monkeypatch.setattr(graphs, "_device_synchronize", lambda device: rig.log.append(("sync", device)))
    return rig


def step(rig, pair):
    """One batch: adopt a new recording, 'launch', mark launched."""
    r = rig.recording()
    handle = pair.adopt(r)
    pair.launched("stream")
    return r, handle.value


def calls(rig, *kinds):
    return [e for e in rig.log if e[0] in kinds]


def test_first_two_adoptions_instantiate_one_per_slot_third_reuses_the_first(rig):
    pair = graphs.ExecPair(keep=100)
    (r0, h0), (r1, h1) = step(rig, pair), step(rig, pair)
    assert calls(rig, "instantiate", "update", "wait") == [("instantiate", 0), ("instantiate", 1)]
    assert (h0, h1) == (r0.raw_cuda_graph_exec(), r1.raw_cuda_graph_exec())
    assert pair.owners == [r0, r1] and pair.dead == []
    r2, h2 = step(rig, pair)
    assert calls(rig, "update") == [("update", 0, 2)]  # slot 0's executable graph, from the new recording
    assert h2 == h0 and pair.owners == [r0, r1]
    r3, h3 = step(rig, pair)
    assert calls(rig, "update")[-1] == ("update", 1, 3) and h3 == h1


@pytest.mark.parametrize("rc,force", [(0, False), (7, False), (0, True)])
def test_slot_event_is_waited_on_before_its_graph_is_touched(rig, rc, force):
    """Slot j's update / re-instantiation in batch b comes after the wait on
    the event recorded by batch b-2's ``launched``; the first two batches
    (no event yet) wait on nothing."""
    rig.rc = rc
    pair = graphs.ExecPair(keep=100, force_instantiate=force)
    for _ in range(6):
        step(rig, pair)
    assert len(rig.events) == 6 and calls(rig, "record") == [("record", b) for b in range(6)]
    assert calls(rig, "wait") == [("wait", b - 2) for b in range(2, 6)]
    for b in range(6):
        lo = rig.log.index(("new", b))
        hi = rig.log.index(("record", b))
        touched = [i for i in range(lo, hi) if rig.log[i][0] in ("update", "instantiate")]
        assert touched, f"batch {b} neither updated nor instantiated"
        if b < 2:
            assert not [e for e in rig.log[lo:hi] if e[0] == "wait"]
        else:
            assert lo < rig.log.index(("wait", b - 2)) < touched[0]


def test_update_succeeds_owner_kept_recording_dead(rig):
    pair = graphs.ExecPair(keep=100)
    r0, h0 = step(rig, pair)
    step(rig, pair)
    r2, h2 = step(rig, pair)
    assert pair.owners[0] is r0 and h2 == r0.raw_cuda_graph_exec()
    assert not r2.instantiated
    assert pair.dead == [r2]


def test_update_fails_recording_becomes_owner_old_owner_dead(rig):
    pair = graphs.ExecPair(keep=100)
    r0, _ = step(rig, pair)
    r1, _ = step(rig, pair)
    rig.rc = 7
    r2, h2 = step(rig, pair)
    assert calls(rig, "update") == [("update", 0, 2)]
    assert r2.instantiated and pair.owners == [r2, r1] and h2 == r2.raw_cuda_graph_exec()
    assert pair.dead == [r0]
    assert r2 not in pair.dead


def test_force_instantiate_never_calls_update(rig):
    pair = graphs.ExecPair(keep=100, force_instantiate=True)
    rs = [step(rig, pair) for _ in range(5)]
    assert calls(rig, "update") == []
    assert calls(rig, "instantiate") == [("instantiate", b) for b in range(5)]
    assert [h for _, h in rs] == [r.raw_cuda_graph_exec() for r, _ in rs]
    assert pair.owners == [rs[4][0], rs[3][0]]
    assert pair.dead == [r for r, _ in rs[:3]]


def test_release_if_due_synchronises_once_at_the_threshold(rig):
    pair = graphs.ExecPair(keep=3)
    for _ in range(4):  # two owners, two dead
        step(rig, pair)
        pair.release_if_due("dev")
    assert len(pair.dead) == 2 and calls(rig, "sync") == []
    step(rig, pair)
    assert len(pair.dead) == 3
    pair.release_if_due("dev")
    assert calls(rig, "sync") == [("sync", "dev")] and pair.dead == []
    pair.release_if_due("dev")
    assert calls(rig, "sync") == [("sync", "dev")]
