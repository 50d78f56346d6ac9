"""The learner step's drivers without a GPU or a kernel library: in which order, on which stream and
with which arguments every form of issue (eager, one graph, DP segment graphs, the one-graph DP step,
the hoisted step and its variants, the chunk graph) runs the step's phases, forks and joins its side
streams, captures and replays its graphs and does its host bookkeeping.  ``torch.cuda``'s streams,
events and graphs and the engine's phases are recorders; every case asserts the whole recorded
sequence.  The GPU tests prove the step's bits, not its issue order, and the order is measured
performance (``_hoist_td_side``: the BPTT started 11 us late when the side branch was captured
first).  Written against the engine whose drivers lived in ``learner_engine.py``, where it passed;
only ``_bare`` and the module alias ``drv`` were ported when they moved."""
import contextlib
import types

import pytest
import torch

from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine import step_driver as drv
from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
from pytorch_r2d2_amd.parallel import graph_rollout

PHASES = ("_sample", "_guard", "_forward_loss", "_backward_core", "_backward_torso", "_update",
          "_priorities", "_gather_dp")
TORSO_OFF, PADDED = 40, 100
VARIANTS = [(p, i, d) for p in (0, 1) for i in ("H", "P") for d in (False, True)]


class World:
    """The recorders that stand in for ``torch.cuda`` and one log (``rec``) for all of them."""

    def __init__(self, monkeypatch):
        w = self
        w.rec, w.n = [], dict(s=0, e=0, g=0, pool=0)
        w.raise_at = 0          # the n-th graph capture from now raises (0: none)
        w.fused_td = True       # the TD launch records the early fork (learner.td_fuse_head_bwd)
        w.eng = None            # with an engine: every phase also logs (_cur, _hoist_due)

        def name(kind):
            w.n[kind] += 1
            return "%s%d" % (kind, w.n[kind])

        class Stream:
            def __init__(self, device=None, name_=None):
                self.name = name_ or name("s")

            def wait_event(self, ev):
                w.rec.append(("wait_event", self.name, ev.name))

            def wait_stream(self, other):
                w.rec.append(("wait_stream", self.name, other.name))

        class Event:
            def __init__(self):
                self.name = name("e")

            def record(self, stream=None):
                w.rec.append(("record", self.name, (stream or w.cur[-1]).name))

        class Graph:
            def __init__(self):
                self.name, self.body, self.mode, self.pool_in = name("g"), None, None, None

            def pool(self):     # (a graph captured into pool X reports X)
                if self.pool_in is None:
                    self.pool_in_own = getattr(self, "pool_in_own", None) or name("pool")
                    return self.pool_in_own
                return self.pool_in

            def replay(self):
                w.rec.append(("replay", self))

        @contextlib.contextmanager
        def stream(s):
            w.rec.append(("enter", s.name))
            w.cur.append(s)
            try:
                yield
            finally:
                w.cur.pop()
                w.rec.append(("exit", s.name))

        @contextlib.contextmanager
        def graph(g, pool=None, capture_error_mode="global"):
            g.pool_in, g.mode = pool, capture_error_mode
            w.rec.append(("capture", g))
            if w.raise_at:
                w.raise_at -= 1
                if not w.raise_at:
                    raise RuntimeError("capture refused\nsecond line")
            outer, w.rec = w.rec, []
            try:
                yield
            finally:
                g.body, w.rec = w.rec, outer

        w.main = Stream(name_="main")
        w.cur = [w.main]
        cuda = drv.torch.cuda
        monkeypatch.setattr(cuda, "Stream", Stream)
        monkeypatch.setattr(cuda, "Event", Event)
        monkeypatch.setattr(cuda, "CUDAGraph", Graph)
        monkeypatch.setattr(cuda, "stream", stream)
        monkeypatch.setattr(cuda, "graph", graph)
        monkeypatch.setattr(cuda, "current_stream", lambda device=None: w.cur[-1])
        monkeypatch.setattr(cuda, "synchronize", lambda device=None: w.rec.append(("synchronize",)))
        monkeypatch.setattr(drv, "_graph_upload", lambda g: w.rec.append(("upload", g)))
        monkeypatch.setattr(drv, "_dispatch_serialized", lambda: False)
        monkeypatch.setattr(graph_rollout, "GraphRollout", lambda *a, **kw: Rollout(w, a, kw))

    def take(self):
        out, self.rec[:] = list(self.rec), []
        return out

    def phase(self, name, after=None):
        def fn(*a, **kw):
            a = tuple(getattr(v, "name", v) for v in a)
            kw = tuple(sorted((k, getattr(v, "name", v)) for k, v in kw.items()))
            st = ((self.eng._cur, self.eng._hoist_due),) if self.eng is not None else ()
            self.rec.append((name, a, kw, self.cur[-1].name) + st)
            return after(*a, **dict(kw)) if after is not None else None
        return fn


class Rollout:
    """``parallel.graph_rollout.GraphRollout`` as far as the drivers use it."""

    def __init__(self, w, a=(), kw=None):
        self.w, self.a, self.kw = w, a, kw or {}
        self.mode, self.is_validating, self.verdict, self.promote = "segments", False, None, False

    def _log(self, *v):
        self.w.rec.append(("ro",) + v)

    def validating(self):
        self._log("validating")
        return self.is_validating

    def record(self, checksum, err, step):
        self._log("record", checksum, err, step)
        return self.verdict

    def want_promote(self, steps_done):
        self._log("want_promote", steps_done)
        return self.promote and self.mode == "segments"

    def agree(self, ok):
        self._log("agree", ok)
        return ok

    def promoted(self):
        self._log("promoted")
        self.mode = "one"

    def refused(self, reason):
        self._log("refused", reason)

    def label(self):
        return "label"


class GSync:
    def __init__(self, w):
        self.w = w

    def start(self, a, b):
        self.w.rec.append(("gsync.start", a, b, self.w.cur[-1].name))

    def finish(self):
        self.w.rec.append(("gsync.finish", self.w.cur[-1].name))


class Timer:
    def __init__(self, w):
        self.w = w

    @contextlib.contextmanager
    def phase(self, name):
        self.w.rec.append(("ph+", name))
        yield
        self.w.rec.append(("ph-", name))


def _bare():
    """A ``LearnerEngine`` that never ran its constructor: the caller sets what the drivers read."""
    e = object.__new__(LearnerEngine)
    # (the state block of LearnerEngine.__init__)
    e._hoist_ready = e._hoist_due = e._early_refused = e._one_dp_graph = e._torso_deferred = False
    e._hoist_gen = e._hoist_unc = e._hoist_t = e._dev_step_off = e._side = e._gather_stream = None
    e._early_fork = e._early_post = e._cgraph = e._one_graph = e._pack_deferred = None
    e._hgraphs, e._hsegs, e._one_graphs = {}, {}, {}
    return e


def _engine(w, hoist=False, dp=False, dp_global=False, early=False, interval=1000, chunk=1, fold=None):
    cfg = get_config("atari57", **{"learner.hoist_early_fork": early, "learner.graph_chunk": chunk,
                                   "learner.target_update_interval": interval})
    e = _bare()
    e.cfg, e.device, e.pg, e.rank = cfg, torch.device("cpu"), None, 0
    e.hoist, e.dp, e.dp_global, e.graph, e.world = hoist, dp, dp_global, None, 1
    e.layout = types.SimpleNamespace(torso_offset=TORSO_OFF, padded=PADDED, H=256)
    e.replay = types.SimpleNamespace(total_written=0, covered_written=0,
                                     step=torch.zeros(1, dtype=torch.int64),
                                     step_end=lambda: w.rec.append(("step_end", w.cur[-1].name)))
    e._sets = [{k: "%s%d" % (k, i) for k in ("starts", "probs", "rows", "h0", "c0", "dp_send")}
               for i in (0, 1)]
    e._cur, e._cover, e._fold_tq, e.tq = 0, None, fold, types.SimpleNamespace(name="tq")
    e.td_done = object() if early else None
    e.steps_done = e.hoisted_steps = e.chunks_run = 0
    e.writes_covered, e.graphs = False, []
    e._hoist_due = False
    e._gsync, e._rollout = GSync(w), Rollout(w)
    e._pg_backend = lambda: "nccl"
    e._dp_checksum, e.err = (lambda: "checksum"), "err"
    e._dp_repair = lambda: w.rec.append(("_dp_repair",))

    def fork(*a, **kw):
        """What the fused TD launch does for the hoisted step's early fork (``_forward_tail``)."""
        ef = e._early_fork if early else None
        if ef is not None and w.fused_td:
            ef.record(w.cur[-1])
            e._early_post = drv.torch.cuda.Event()
            e._early_post.record(w.cur[-1])

    def side(torso, after_td, td_wait=False):
        s = e._side_stream()
        s.wait_event(types.SimpleNamespace(name=after_td))
        return s

    for n in PHASES:
        setattr(e, n, w.phase(n))
    e._forward_rest = w.phase("_forward_rest", lambda tail=True: fork() if tail else None)
    e._forward_tail = w.phase("_forward_tail", fork)
    e._hoist_side = w.phase("_hoist_side", side)
    return e


def P(name, *a, s="main", st=None, **kw):
    return (name, a, tuple(sorted(kw.items())), s) + ((st,) if st is not None else ())


def G(*v, s="main"):
    return ("gsync." + v[0],) + v[1:] + (s,)


def torso(fold=None, **kw):
    return P("_backward_torso", defer_reduce=fold is not None, **kw)


def single_body(presampled=False, s="main"):
    return [P("_forward_loss", presampled, s=s), P("_backward_core", s=s), torso(s=s),
            P("_update", s=s), P("_priorities", s=s)]


def names(rec, *maps):
    """The log with every replayed / captured graph replaced by its key in ``maps``."""
    key = {id(g): k for m in maps for k, g in (m.items() if isinstance(m, dict) else enumerate(m))}
    return [(r[0], key[id(r[1])]) if r[0] in ("replay", "capture", "upload") else r for r in rec]


def one_pool(graphs):
    """Every graph of one capture() shares the first one's pool."""
    graphs = list(graphs)
    assert graphs[0].pool_in is None
    assert [g.pool_in for g in graphs[1:]] == [graphs[0].pool()] * (len(graphs) - 1)


WARM0 = [("wait_stream", "s1", "main"), ("enter", "s1"), ("exit", "s1"), ("wait_stream", "main", "s1"),
         ("synchronize",)]


# ---------------------------------------------------------------- plain single rank
@pytest.mark.parametrize("presampled", [False, True])
def test_single_eager(monkeypatch, presampled):
    w = World(monkeypatch)
    e = _engine(w)
    e.step_eager(_presampled=presampled)
    assert w.take() == single_body(presampled) and e.steps_done == 1
    e.step_eager(timer=Timer(w), _presampled=presampled)
    body = single_body(presampled)
    want = []
    for n, op in zip(("forward+td", "backward_core", "backward_torso", "update", "priorities"), body):
        want += [("ph+", n), op, ("ph-", n)]
    assert w.take() == want and e.steps_done == 2
    e.step()            # (no graph: the eager step)
    assert w.take() == single_body() and e.steps_done == 3


def test_single_fold_defers_the_torso_reduce(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, fold=10)
    e.step_eager()
    assert w.take()[2] == torso(fold=10)


def test_single_capture_and_step(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w)
    e.capture()
    (g,) = e.graphs
    assert names(w.take(), e.graphs) == (
        [("wait_stream", "s1", "main"), ("enter", "s1")] + single_body(s="s1") * 2
        + [("exit", "s1"), ("wait_stream", "main", "s1"), ("synchronize",), ("capture", 0),
           ("synchronize",)])
    assert g.body == single_body() and g.mode == "global" and g.pool_in is None
    assert e.graph and e.steps_done == 2
    e.step()
    e.step()
    assert names(w.take(), e.graphs) == [("replay", 0)] * 2 and e.steps_done == 4


# ---------------------------------------------------------------- serial DP
def gather(gs):
    return [("wait_stream", gs, "main"), ("enter", gs), P("_gather_dp", s=gs), ("exit", gs)]


def dp_eager():
    return [P("_forward_loss"), P("_backward_core"), G("start", 0, TORSO_OFF), torso(),
            G("start", TORSO_OFF, PADDED), P("_priorities", end=False), G("finish"), P("_update"),
            ("step_end", "main")]


def dp_segments(dp_global):
    head = ([[P("_sample")], [P("_forward_rest", tail=False)], [P("_forward_tail"), P("_backward_core")]]
            if dp_global else [[P("_forward_loss"), P("_backward_core")]])
    return head + [[torso()], [P("_priorities", end=False)], [P("_update"), ("step_end", "main")]]


def dp_body(dp_global, gs=None):
    sg = dp_segments(dp_global)
    head = sg[0] + gather(gs) + sg[1] + [("wait_stream", "main", gs)] + sg[2] if dp_global else sg[0]
    return (head + [G("start", 0, TORSO_OFF)] + sg[-3] + [G("start", TORSO_OFF, PADDED)] + sg[-2]
            + [G("finish")] + sg[-1])


@pytest.mark.parametrize("dp_global", [False, True])
def test_dp_eager(monkeypatch, dp_global):
    w = World(monkeypatch)
    e = _engine(w, dp=True, dp_global=dp_global)
    e.step_eager()
    assert w.take() == dp_eager() and e.steps_done == 1
    e.step_eager(timer=Timer(w))
    t = lambda n, *ops: [("ph+", n), *ops, ("ph-", n)]      # noqa: E731
    b = dp_eager()
    assert w.take() == (t("forward+td", b[0]) + t("backward_core", b[1]) + [b[2]] + t("backward_torso", b[3])
                        + [b[4]] + t("priorities", b[5]) + t("allreduce_wait", b[6]) + t("update", b[7], b[8]))
    assert e.dp_graph_label() == "label"


@pytest.mark.parametrize("dp_global", [False, True])
def test_dp_capture_and_segment_step(monkeypatch, dp_global):
    w = World(monkeypatch)
    e = _engine(w, dp=True, dp_global=dp_global)
    e.capture(warmup=0)
    n = 6 if dp_global else 4
    assert names(w.take(), e.graphs) == WARM0 + [("capture", i) for i in range(n)] + [("synchronize",)]
    assert [g.body for g in e.graphs] == dp_segments(dp_global)
    assert {g.mode for g in e.graphs} == {"thread_local"} and e.graph
    one_pool(e.graphs)
    ro = e._rollout
    assert isinstance(ro, Rollout) and ro.kw["enabled"] and (ro.kw["warm"], ro.kw["validate"]) == (3, 50)
    e.step()
    R = lambda i: [("replay", i)]       # noqa: E731
    if dp_global:
        gs = e._gather_stream.name
        head = R(0) + gather(gs) + R(1) + [("wait_stream", "main", gs)] + R(2)
    else:
        head = R(0)
    assert names(w.take(), e.graphs) == (
        head + [G("start", 0, TORSO_OFF)] + R(n - 3) + [G("start", TORSO_OFF, PADDED)] + R(n - 2)
        + [G("finish")] + R(n - 1) + [("ro", "validating"), ("ro", "want_promote", 1)])
    assert e.steps_done == 1


@pytest.mark.parametrize("dp_global", [False, True])
def test_dp_step_body_and_one_graph(monkeypatch, dp_global):
    w = World(monkeypatch)
    e = _engine(w, dp=True, dp_global=dp_global)
    e._dp_step_body()
    gs = e._gather_stream.name if dp_global else None
    assert w.take() == dp_body(dp_global, gs)
    # promoted after a step: the body captured as one graph in the segment graphs' pool
    e.capture(warmup=0)
    w.take()
    e._rollout.promote = True
    e.steps_done = 3
    e._dp_rollout_after_step()
    one = e._one_graph
    assert names(w.take(), {"one": one}) == [
        ("ro", "validating"), ("ro", "want_promote", 3), ("synchronize",), ("capture", "one"),
        ("synchronize",), ("ro", "agree", True), ("ro", "promoted")]
    assert one.body == dp_body(dp_global, gs) and one.mode == "thread_local"
    assert one.pool_in == e.graphs[0].pool() and e._one_dp_graph
    e.step()        # mode "one": one replay, the count, then the rollout hook
    assert names(w.take(), {"one": one}) == [("replay", "one"), ("ro", "validating"), ("ro", "want_promote", 4)]
    assert e.steps_done == 4


# ---------------------------------------------------------------- hoisted single rank
class Ev:
    """The event names a sequence of bodies creates, in creation order."""

    def __init__(self, first=1):
        self.n = first - 1

    def __call__(self):
        self.n += 1
        return "e%d" % self.n


def td_side(ev, due, fwd, early, side, before_join=(), st=None, fused_td=True):
    """``_hoist_td_side``: forward to the TD launch, the event on main, the BPTT BEFORE the side
    branch, the join."""
    kw = {} if st is None else dict(st=st)
    if early:
        fork, post = ev(), (ev() if fused_td else None)
        ops = [P(fwd, **kw)] + ([("record", fork, "main"), ("record", post, "main")] if fused_td else [])
        if not fused_td:       # the fork was never recorded: fork after TD as without the knob
            fork, early = ev(), False
            ops.append(("record", fork, "main"))
    else:
        fork = ev()
        ops = [P(fwd, **kw), ("record", fork, "main")]
    return ops + [P("_backward_core", **kw),
                  P("_hoist_side", torso=not due, after_td=fork, td_wait=early, **kw),
                  ("wait_event", side, fork), *before_join, ("wait_stream", "main", side)]


def hoist_body(ev, p, inm, due, early=False, side="s1", fold=None, fused_td=True):
    ops = [P("_guard", inm == "H")] + ([P("_sample", qreset="tq")] if inm == "P" else [])
    return ops + td_side(ev, due, "_forward_rest", early, side, fused_td=fused_td) + [torso(fold), P("_update")]


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("inm", ["P", "H"])
@pytest.mark.parametrize("due", [False, True])
def test_hoist_body(monkeypatch, inm, due, early):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, early=early, fold=8)
    e._hoist_body(1, inm, due)
    assert w.take() == hoist_body(Ev(), 1, inm, due, early, fold=8)
    assert (e._cur, e._hoist_due, e.starts, e.dp_send) == (1, due, "starts1", "dp_send1")
    assert e._early_fork is None


def test_hoist_body_early_fork_not_recorded(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, early=True)
    w.fused_td = False
    e._hoist_body(0, "H", False)
    assert w.take() == hoist_body(Ev(), 0, "H", False, early=True, fused_td=False)


def _captured_hoist(monkeypatch, chunk=4, interval=1000, early=False):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, chunk=chunk, interval=interval, early=early)
    e.capture(warmup=0)
    return w, e


def test_hoist_capture(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, chunk=4, early=True)
    e._use_set(1)
    e._hoist_due = True
    e.capture(warmup=0)
    hg = e._hgraphs
    assert list(hg) == VARIANTS
    assert names(w.take(), hg, {"chunk": e._cgraph}) == (
        WARM0 + [("capture", k) for k in VARIANTS] + [("capture", "chunk"), ("upload", "chunk"), ("synchronize",)])
    ev = Ev()
    for k in VARIANTS:
        assert hg[k].body == hoist_body(ev, *k, early=True, side="s2"), k
    assert e._cgraph.body == sum((hoist_body(ev, j & 1, "H", False, early=True, side="s2") for j in range(4)), [])
    one_pool(list(hg.values()) + [e._cgraph])
    assert {g.mode for g in hg.values()} | {e._cgraph.mode} == {"global"}
    assert (e._cur, e._hoist_due, e.starts, e.graph) == (1, True, "starts1", True)


def test_hoist_capture_without_chunk(monkeypatch):
    w, e = _captured_hoist(monkeypatch, chunk=1)
    assert e._cgraph is None and e._chunk_len() == 1
    assert names(w.take(), e._hgraphs) == WARM0 + [("capture", k) for k in VARIANTS] + [("synchronize",)]


def test_hoist_steps_pick_their_variant(monkeypatch):
    w, e = _captured_hoist(monkeypatch, chunk=1, interval=3)
    w.take()
    rp = e.replay
    e.step()                        # k 0: nothing pre-sampled
    e.step()                        # k 1
    rp.total_written += 5           # a replay write: the pre-sampled batch is stale
    e.step()                        # k 2, due
    assert e._hoist_gen == 5
    e.step()                        # k 3
    e.invalidate_hoist()
    e.step()                        # k 4
    e.step()                        # k 5, due
    assert names(w.take(), e._hgraphs) == [("replay", k) for k in (
        (0, "P", False), (1, "H", False), (0, "P", True), (1, "H", False), (0, "P", False), (1, "H", True))]
    assert (e.steps_done, e.hoisted_steps, e._dev_step_off, e._cur) == (6, 3, 0, 1)
    e.writes_covered = True         # a driver vouches for its writes
    rp.total_written += 1
    e.step()
    assert names(w.take(), e._hgraphs) == [("replay", (0, "H", False))]
    assert e._hoist_gen == 6


def test_hoist_steps_start_from_the_device_counter(monkeypatch):
    w, e = _captured_hoist(monkeypatch, chunk=1, interval=3)
    w.take()
    e.replay.step[0] = 7            # a resumed run: device step 7 is host step 0; due at 8, 11
    for _ in range(3):
        e.step()
    assert e._dev_step_off == 7
    assert names(w.take(), e._hgraphs) == [("replay", k) for k in ((0, "P", False), (1, "H", True), (0, "H", False))]


def test_hoist_steps_under_cover_writes(monkeypatch):
    w, e = _captured_hoist(monkeypatch, chunk=1)
    w.take()
    rp, actor = e.replay, types.SimpleNamespace(t=7)
    e._cover = dict(actor=actor, A=2)
    write = lambda rows, covered, steps: (setattr(rp, "total_written", rp.total_written + rows),     # noqa: E731
                                          setattr(rp, "covered_written", rp.covered_written + covered),
                                          setattr(actor, "t", actor.t + steps))
    e.step()
    assert (e._hoist_gen, e._hoist_unc, e._hoist_t) == (0, 0, 7)
    write(4, 4, 2)                  # two steps of the covered actor: the batch stays
    e.step()
    assert (e._hoist_gen, e._hoist_unc, e._hoist_t) == (4, 0, 9)
    write(6, 6, 3)                  # three: more than clear_ahead
    e.step()
    write(2, 0, 0)                  # an uncovered write
    e.step()
    write(2, 2, 1)
    e.step()
    assert names(w.take(), e._hgraphs) == [("replay", k) for k in (
        (0, "P", False), (1, "H", False), (0, "P", False), (1, "P", False), (0, "H", False))]
    assert e.hoisted_steps == 2 and (e._hoist_gen, e._hoist_unc, e._hoist_t) == (14, 2, 13)


def test_hoist_eager_step_ignores_the_graphs(monkeypatch):
    w, e = _captured_hoist(monkeypatch, chunk=1)
    w.take()
    e.step_eager()
    e.step_eager()
    ev = Ev(w.n["e"] - 1)
    assert w.take() == hoist_body(ev, 0, "P", False, side="s2") + hoist_body(ev, 1, "H", False, side="s2")
    assert e.graph is True and (e.steps_done, e.hoisted_steps, e._hoist_gen) == (2, 1, 0)
    with pytest.raises(ValueError):
        e.step_eager(_presampled=True)


def _chunk_ready(monkeypatch, interval=1000):
    """Captured with graph_chunk 4, two steps done: even step, fresh batch, counter offset known."""
    w, e = _captured_hoist(monkeypatch, chunk=4, interval=interval)
    e.run_steps(2)
    assert names(w.take()[-2:], e._hgraphs) == [("replay", (0, "P", False)), ("replay", (1, "H", False))]
    return w, e


def _replays(w, e):
    return [k for _, k in names(w.take(), e._hgraphs, {"chunk": e._cgraph})]


def test_run_steps_takes_the_chunk(monkeypatch):
    w, e = _chunk_ready(monkeypatch)
    e._hoist_due = True
    e.run_steps(4)
    assert _replays(w, e) == ["chunk"]
    assert (e.chunks_run, e.steps_done, e.hoisted_steps, e._cur, e._hoist_due) == (1, 6, 5, 1, False)
    assert e.starts == "starts1" and e._hoist_gen == 0
    e.run_steps(9)
    assert _replays(w, e) == ["chunk", "chunk", (0, "H", False)]
    assert (e.chunks_run, e.steps_done, e.hoisted_steps) == (3, 15, 14)


H0, H1 = (0, "H", False), (1, "H", False)


def test_run_steps_odd_start(monkeypatch):
    w, e = _chunk_ready(monkeypatch)
    e.step()
    e.run_steps(4)
    assert _replays(w, e) == [H0, H1, H0, H1, H0] and e.chunks_run == 0
    e.run_steps(5)          # (odd again: one step, then the chunk)
    assert _replays(w, e) == [H1, "chunk"] and e.chunks_run == 1


def test_run_steps_due_inside(monkeypatch):
    w, e = _chunk_ready(monkeypatch, interval=5)       # step 4 syncs the target
    e.run_steps(4)
    assert _replays(w, e) == [H0, H1, (0, "H", True), H1] and e.chunks_run == 0


def test_run_steps_stale_batch(monkeypatch):
    w, e = _chunk_ready(monkeypatch)
    e.replay.total_written += 1
    e.run_steps(4)
    assert _replays(w, e) == [(0, "P", False), H1, H0, H1] and e.chunks_run == 0


def test_run_steps_fewer_than_a_chunk(monkeypatch):
    w, e = _chunk_ready(monkeypatch)
    e.run_steps(3)
    assert _replays(w, e) == [H0, H1, H0] and e.chunks_run == 0


def test_run_steps_counter_offset_unset(monkeypatch):
    w, e = _chunk_ready(monkeypatch)
    e._dev_step_off = None          # (load_full_state)
    e.replay.step[0] = 2
    e.run_steps(4)
    assert _replays(w, e) == [H0, H1, H0, H1] and e.chunks_run == 0 and e._dev_step_off == 0


def test_run_steps_without_graphs_or_hoist(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, chunk=4)
    assert e._chunk_len() == 1
    e.run_steps(2)
    assert w.take() == single_body() * 2 and e.steps_done == 2


# ---------------------------------------------------------------- hoisted DP
def hoist_dp_body(ev, p, inm, due, dp_global, gs, side):
    ops = [P("_guard", False), P("_sample", qreset="tq")] if inm == "P" else []
    ops += gather(gs) if dp_global else []
    ops += ([P("_guard", True)] if inm == "H" else []) + [P("_forward_rest", tail=False)]
    ops += [("wait_stream", "main", gs)] if dp_global else []
    return (ops + td_side(ev, due, "_forward_tail", False, side, [G("start", 0, TORSO_OFF)])
            + [torso(), G("start", TORSO_OFF, PADDED), G("finish"), P("_update")])


@pytest.mark.parametrize("dp_global", [False, True])
@pytest.mark.parametrize("inm", ["P", "H"])
def test_hoist_dp_body(monkeypatch, inm, dp_global):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, dp=True, dp_global=dp_global)
    gs, side = ("s1", "s2") if dp_global else (None, "s1")
    e._hoist_dp_body(1, inm, True)
    assert w.take() == hoist_dp_body(Ev(), 1, inm, True, dp_global, gs, side)
    assert (e._cur, e._hoist_due) == (1, True)


HSEG_KEYS = ([("sample", p) for p in (0, 1)] + [("fwd_head", p, i) for p in (0, 1) for i in "PH"]
             + [("core_side", p, d) for p in (0, 1) for d in (False, True)]
             + [("torso", p) for p in (0, 1)] + [("update", d) for d in (False, True)])


def test_capture_hoist_dp(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, dp=True, dp_global=True)
    e._use_set(1)
    e._hoist_due = True
    w.eng = e
    e._capture_hoist_dp()
    hs = e._hsegs
    assert list(hs) == HSEG_KEYS and len(hs) == 14 and e.graphs == list(hs.values())
    assert names(w.take(), hs) == [("capture", k) for k in HSEG_KEYS]
    ev = Ev()
    for k, g in hs.items():
        st = (k[1], False) if k[0] != "update" else (1, k[1])
        if k[0] == "sample":
            want = [P("_guard", False, st=st), P("_sample", qreset="tq", st=st)]
        elif k[0] == "fwd_head":
            want = ([P("_guard", True, st=st)] if k[2] == "H" else []) + [P("_forward_rest", tail=False, st=st)]
        elif k[0] == "core_side":
            st = (k[1], k[2])
            want = td_side(ev, k[2], "_forward_tail", False, "s1", st=st)
        elif k[0] == "torso":
            want = [torso(st=st)]
        else:
            want = [P("_update", st=st)]
        assert g.body == want, k
    assert {g.mode for g in hs.values()} == {"thread_local"}
    one_pool(hs.values())
    assert (e._cur, e._hoist_due, e.starts) == (1, True, "starts1")


@pytest.mark.parametrize("dp_global", [False, True])
@pytest.mark.parametrize("inm", ["P", "H"])
def test_hoist_dp_segments_follow_the_plan(monkeypatch, inm, dp_global):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, dp=True, dp_global=dp_global)
    e._capture_hoist_dp()
    w.take()
    p, due = 1, True
    e._hoist_dp_segments(p, inm, due)
    gs = e._gather_stream.name if dp_global else None
    key = {"sample": ("sample", p), "fwd_head": ("fwd_head", p, inm), "core_side": ("core_side", p, due),
           "torso": ("torso", p), "update": ("update", due)}
    coll = {"all_gather": gather(gs), "all_reduce_core": [G("start", 0, TORSO_OFF)],
            "all_reduce_torso": [G("start", TORSO_OFF, PADDED), G("finish")]}
    want = []
    for kind, name in drv.dp_hoist_plan(dp_global, inm):
        if name == "core_side" and dp_global:
            want.append(("wait_stream", "main", gs))
        want += coll[name] if kind == "collective" else [("replay", key[name])]
    assert names(w.take(), e._hsegs) == want
    assert (e._cur, e._hoist_due) == (p, due)


def test_hoist_dp_capture_and_steps(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, dp=True, interval=2)
    e.capture(warmup=0)
    assert names(w.take(), e._hsegs) == WARM0 + [("capture", k) for k in HSEG_KEYS] + [("synchronize",)]
    assert e.graph and e._cgraph is None and isinstance(e._rollout, Rollout) and e._chunk_len() == 1
    e.step()            # segments, k 0: 'P', not due
    R = lambda *k: ("replay", k)        # noqa: E731
    assert names(w.take(), e._hsegs) == [
        R("sample", 0), R("fwd_head", 0, "P"), R("core_side", 0, False), G("start", 0, TORSO_OFF),
        R("torso", 0), G("start", TORSO_OFF, PADDED), G("finish"), R("update", False),
        ("ro", "validating"), ("ro", "want_promote", 1)]
    e._rollout.promote = True
    e.run_steps(1)      # k 1: 'H', due; then the one graphs are captured
    og = e._one_graphs
    assert list(og) == VARIANTS
    assert names(w.take(), e._hsegs, og) == [
        R("fwd_head", 1, "H"), R("core_side", 1, True), G("start", 0, TORSO_OFF), R("torso", 1),
        G("start", TORSO_OFF, PADDED), G("finish"), R("update", True),
        ("ro", "validating"), ("ro", "want_promote", 2), ("synchronize",)] + [
        ("capture", k) for k in VARIANTS] + [("synchronize",), ("ro", "agree", True), ("ro", "promoted")]
    ev = Ev(w.n["e"] - 8 + 1)
    for k in VARIANTS:
        assert og[k].body == hoist_dp_body(ev, *k, False, None, "s2"), k
        assert og[k].mode == "thread_local" and og[k].pool_in == e.graphs[0].pool()
    assert (e._cur, e._hoist_due, e._one_dp_graph) == (1, True, True)
    e._rollout.promote = False
    e.step()            # mode "one", k 2
    assert names(w.take(), og) == [R(0, "H", False), ("ro", "validating"), ("ro", "want_promote", 3)]
    assert (e._cur, e._hoist_due, e.steps_done, e.hoisted_steps) == (0, False, 3, 2)
    e.step_eager()      # k 3, due: the eager body, counted; the rollout hook belongs to the graph steps
    assert w.take() == hoist_dp_body(Ev(w.n["e"]), 1, "H", True, False, None, "s2")
    assert (e.steps_done, e.hoisted_steps, e.graph) == (4, 3, True)


def test_capture_one_dp_restores_the_set_when_a_capture_raises(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, hoist=True, dp=True)
    e._capture_hoist_dp()
    w.take()
    e._use_set(1)
    e._hoist_due = True
    w.raise_at = 3      # the third variant's capture raises: (0, 'P', False) after two set-0 bodies
    with pytest.raises(RuntimeError):
        e._capture_one_dp()
    assert [r[0] for r in w.take()] == ["synchronize", "capture", "capture", "capture"]
    assert (e._cur, e._hoist_due, e.starts) == (1, True, "starts1")
    assert not getattr(e, "_one_graphs", None) and not getattr(e, "_one_dp_graph", False)


# ---------------------------------------------------------------- the rollout hook
def test_rollout_refused_capture_clears_host_state(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, dp=True)
    e.capture(warmup=0)
    w.take()
    e._rollout.promote = True
    e._pack_deferred = (1, True)
    w.raise_at = 1
    e.steps_done = 3
    e._dp_rollout_after_step()
    rec = w.take()
    assert [r[:2] for r in rec[:2]] == [("ro", "validating"), ("ro", "want_promote")]
    assert [r[0] for r in rec[2:5]] == ["synchronize", "capture", "synchronize"]
    assert rec[5:] == [("ro", "agree", False), ("ro", "refused", "RuntimeError: capture refused")]
    assert e._pack_deferred is None and e._gsync is None
    assert e._one_graph is None and e._one_dp_graph is False


def test_rollout_validation_mismatch_repairs(monkeypatch):
    w = World(monkeypatch)
    e = _engine(w, dp=True)
    e._rollout.is_validating, e._rollout.verdict, e.steps_done = True, False, 9
    e._dp_rollout_after_step()
    assert w.take() == [("ro", "validating"), ("ro", "record", "checksum", "err", 9), ("_dp_repair",)]
    e._rollout.verdict = None       # inside the window: no verdict yet
    e._dp_rollout_after_step()
    assert w.take() == [("ro", "validating"), ("ro", "record", "checksum", "err", 9)]
    e._rollout = None
    e._dp_rollout_after_step()
    assert w.take() == [] and e.dp_graph_label() == "eager"
