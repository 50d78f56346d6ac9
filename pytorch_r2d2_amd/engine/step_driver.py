"""How the learner step is issued.  ``LearnerEngine`` (what a step computes: the kernel sequence
``_sample`` ... ``_priorities``) inherits ``StepDrivers``, which strings those phases together:

    eager        ``step_eager``: ``_single_body``; DP: with the bucket all-reduces between the phases
    one graph    world 1: ``_single_body`` captured once, replayed by ``step``
    segments     DP: 4 graphs (6 with global sampling), the collectives between them (``_dp_step_body``)
    one DP graph the same body, the collectives captured on their side streams (GraphRollout)
    hoisted      learner.hoist: ``_hoist_body`` (dist.hoist_dp: ``_hoist_dp_body`` / ``_hoist_dp_segments``),
                 one graph per (sample set, sampled by the previous step or not, sync due) variant
    chunk        ``run_steps``: learner.graph_chunk hoisted steps as one graph

and the host bookkeeping that picks between them (``_hoist_step``, ``_hoist_fresh``, ``cover_writes``).
Their host-side state is declared in one block of ``LearnerEngine.__init__``.  The order of every
body's stream operations is measured performance; tests/test_step_driver_cpu.py pins it.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional

import torch

from ..ops._lib import check, kernels, ptr, stream_handle

# the hoisted step's graph variants (sample set, sampled by the previous step 'H' or at the step's
# start 'P', target sync due) in capture order, which decides the pool's layout
_HOIST_VARIANTS = tuple((p, i, d) for p in (0, 1) for i in ("H", "P") for d in (False, True))


def _graph_upload(g) -> None:
    """Upload an instantiated graph's executable to the device (hipGraphUpload on the current
    stream), so its first replay -- possibly inside a timed loop -- does not pay for it.  Best
    effort: without the runtime entry point the first replay uploads as before."""
    try:
        exec_h = int(g.raw_cuda_graph_exec())
        lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        lib.hipGraphUpload.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.hipGraphUpload(ctypes.c_void_p(exec_h), ctypes.c_void_p(stream_handle()))
    except (AttributeError, OSError, RuntimeError):
        pass


def _dispatch_serialized() -> bool:
    """True when kernel dispatches run one at a time (rocprofv3 counter collection / thread trace,
    AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING).  The hoisted step's early fork has a kernel on the
    side queue wait on the device for the TD kernel of the main queue, which a serialised
    dispatcher never runs beside it (a bounded stall and an error word), so it forks after TD there."""
    env = os.environ
    on = lambda k: env.get(k, "0").strip().lower() not in ("", "0", "false", "no", "off")  # noqa: E731
    return (on("ROCPROF_COUNTER_COLLECTION") or on("ROCPROF_ADVANCED_THREAD_TRACE")
            or on("HIP_LAUNCH_BLOCKING") or env.get("AMD_SERIALIZE_KERNEL", "0") not in ("", "0"))


def dp_hoist_plan(dp_global: bool, inm: str):
    """The hoisted data-parallel step (dist.hoist_dp) as ("segment" | "collective", name) pairs in
    issue order.  ``inm``: 'P' = the step samples at its start, 'H' = the previous step's side
    branch sampled.  The collective subsequence depends on neither ``inm`` nor on whether the side
    branch runs target frames (that is inside "core_side"): ranks decide 'P' / 'H' on their own
    replay and must still meet at every collective.  The side branch (priority tail, counter, next
    sample + shard stats, target frames) forks and joins inside "core_side" and holds no collective;
    there is no priority segment."""
    if inm not in ("P", "H"):
        raise ValueError("inm must be 'P' or 'H'")
    plan = [("segment", "sample")] if inm == "P" else []
    if dp_global:
        plan.append(("collective", "all_gather"))        # beside fwd_head, joined before core_side
    plan += [("segment", "fwd_head"), ("segment", "core_side"), ("collective", "all_reduce_core"),
             ("segment", "torso"), ("collective", "all_reduce_torso"), ("segment", "update")]
    return plan


def _phase(timer):
    """``timer.phase`` (utils.profiling.PhaseTimer), or without a timer a context that does nothing."""
    return timer.phase if timer is not None else (lambda name: contextlib.nullcontext())


class StepDrivers:
    # ------------------------------------------------------------------ hoisted step
    # Split-precision step software-pipelined over two steps: single rank, and (opt-in,
    # dist.hoist_dp: "the hoisted step on data-parallel ranks" below) DP ranks (round-6 verdict item
    # 1; reference: the serial /root/reference/learner.py:68-110).  Step k's priority tail needs
    # only its TD errors and step k+1's sample only the repaired tree, so right after the TD
    # launch a side stream runs [priority tail(k) + step counter, sample(k+1) into the other
    # sample set, target-net torso(k+1) frames from a queue] while the main stream runs the
    # BPTT and the rest of step k.  The side torso runs on the CUs the BPTT leaves free and stops
    # taking frames when the BPTT raises its stop word; step k+1's torso launch takes the rest of
    # the queue.  Every frame is computed by the same kernel code from the same operands, the
    # sample uses the same device step counter, and the target packs are only used when no
    # target sync happened in between (the host knows the sync steps: the update is captured with
    # the due decision baked in), so the step is bit-identical to the plain one -- as long as the
    # replay does not change between the hoisted sample and the step that trains on it.  A batch
    # sampled before a replay write is dropped (_hoist_fresh: HBMReplay.total_written moved), and
    # that step samples at its start like the plain one; only a driver that keeps its writes away
    # from pending batches (engine/concurrent.py) sets ``writes_covered``.  ``cover_writes`` keeps
    # the batch across the steps of a serial actor that clears its starts ahead of its write head.
    # Every optimizer setting hoists: the side branch's tail advances the device step counter
    # before the update runs (the join precedes it), so Adam's step count is the counter itself
    # there and counter + 1 in the plain step (``_step_off``, the same reason as
    # ``_baked_interval``); the clip norm (r2_grad_sumsq) is a fixed-order sum, the same bits in
    # both step shapes.
    # Data-parallel ranks hoist only with dist.hoist_dp (default off: the serial DP step, the same
    # graphs, kernels and bits as before the knob existed); no N > 1 RCCL run has exercised it.
    def _hoist_ok(self) -> bool:
        lc = self.cfg.learner
        return bool(lc.hoist and self.sp and self.fused_torso and not self.sp_lib
                    and self.device.type == "cuda"
                    and (not self.dp or self.cfg.dist.hoist_dp)
                    and self.row_dst4 is not None and self.cfg.replay.fused_prio_tail
                    and not lc.zero_stored_state)

    def _use_set(self, i: int) -> None:
        self._cur = i
        S = self._sets[i]
        self.starts, self.probs, self.rows = S["starts"], S["probs"], S["rows"]
        self.h0, self.c0 = S["h0"], S["c0"]
        self.dp_send = S["dp_send"]

    def invalidate_hoist(self) -> None:
        """Drop the batch the previous step sampled (and the target frames it computed) for the
        next one: call after changing the weights between steps, or the replay through a path
        that does not count its rows in ``HBMReplay.total_written`` (the counted writers -- actor
        steps, ingests -- are noticed by ``_hoist_fresh``).  The next step samples at its start,
        as the plain step does."""
        self._hoist_ready = False

    def cover_writes(self, actor) -> None:
        """Keep the pre-sampled batch across the steps of ``actor``, a serial ``BatchedActor`` on
        this engine's replay that clears its starts ``clear_ahead`` rows ahead of its write head
        (actor.hip, ahead > 0): up to ``clear_ahead`` of its steps between two learner steps
        overwrite no window of a batch sampled before them (``_hoist_fresh``).  From now on every
        hoisted step body begins with the device guard (replay.hip hoist_guard_kernel), which
        recounts that claim from the actor's device step counter and write head and reports torn
        pre-sampled windows in bit 29 of ``error_word``.  Call before ``capture``."""
        if self.graph:
            raise RuntimeError("cover_writes() must be called before capture(): the guard is a node "
                               "of every captured step")
        if actor.replay is not self.replay:
            raise ValueError("cover_writes: the actor writes another replay")
        if int(getattr(actor, "clear_ahead", 0)) <= 0:
            raise ValueError("cover_writes: the actor does not clear ahead (actor.clear_ahead > 0)")
        if actor.defer:
            raise ValueError("cover_writes: a deferred actor is covered by the concurrent driver")
        if not self.hoist:
            raise ValueError("cover_writes: this engine does not hoist (learner.hoist and its "
                             "conditions, _hoist_ok)")
        d = self.device
        self._cover = dict(actor=actor, head=actor.head_d, t=actor.t_d, A=int(actor.clear_ahead),
                           t_seen=actor.t_d.clone(),
                           err=torch.zeros(2, dtype=torch.int32, device=d))
        self.invalidate_hoist()

    def _guard(self, presampled: bool) -> None:
        """First operation of a hoisted step body once ``cover_writes`` was called: count the
        slots of the batch in use whose windows the covered actor's steps since the previous
        learner step overwrote (only when the batch was ``presampled``), refresh the snapshot."""
        c = self._cover
        if c is None:
            return
        rp = self.replay
        check(kernels().r2_hoist_guard(ptr(self.starts), self.B, ptr(c["head"]), ptr(c["t"]),
                                       ptr(c["t_seen"]), rp.cap_e, rp.n_sub, self.T, self.n,
                                       ptr(rp.done), int(presampled), ptr(c["err"]), stream_handle()),
              "hoist_guard")

    def guard_count(self) -> int:
        """Pre-sampled slots the guard found torn or in bootstrap violation so far (one D2H read;
        0 without ``cover_writes``)."""
        return int(self._cover["err"][1].item()) if self._cover is not None else 0

    def _note_presample(self) -> None:
        """Host state of the moment the next step's batch was sampled (``_hoist_fresh``)."""
        rp = self.replay
        self._hoist_gen = rp.total_written
        if self._cover is not None:
            self._hoist_unc = rp.total_written - rp.covered_written
            self._hoist_t = self._cover["actor"].t

    def _hoist_fresh(self) -> bool:
        """The previous step sampled this step's batch AND the replay has not been written since
        (every host-side writer bumps ``HBMReplay.total_written``): a batch sampled before a write
        may hold windows the write overwrote, and came from a tree the plain step would not have
        used.  ``writes_covered``: a driver whose writes stay clear of every batch that may
        still be pending (engine/concurrent.py: lookahead >= 2 rounds) vouches for them.
        ``cover_writes``: no uncovered write (``total_written - covered_written`` has not moved)
        and at most ``clear_ahead`` steps of the covered actor."""
        if not self._hoist_ready:
            return False
        rp = self.replay
        if self.writes_covered or self._hoist_gen == rp.total_written:
            return True
        c = self._cover
        return bool(c is not None
                    and self._hoist_unc == rp.total_written - rp.covered_written
                    and 0 <= c["actor"].t - self._hoist_t <= c["A"])

    def _due(self, k: int) -> bool:
        iv = int(self.cfg.learner.target_update_interval)
        return iv <= 1 or (k + 1) % iv == 0

    def _baked_interval(self) -> int:
        """The target-sync interval handed to the update / pack kernels: the hoisted step's graph
        variants bake the due decision (1 = due, 2^62 = never), so the device step counter --
        already advanced by the side stream's priority tail -- is not read for it."""
        if not self.hoist:
            return int(self.cfg.learner.target_update_interval)
        return 1 if self._hoist_due else 1 << 62

    def _step_off(self) -> int:
        """Adam's step count is the device step counter + this: 1 in the plain and DP steps (the
        update runs before the counter advances), 0 in the hoisted step (the side branch's priority
        tail, joined before the update, already advanced it)."""
        return 0 if self.hoist else 1

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def _hoist_body(self, p: int, inm: str, due: bool):
        """The hoisted step as stream operations (eager or captured): sample set ``p``; ``inm``
        'P' = sample at the start (no previous hoisted step), 'H' = the previous step sampled;
        ``due``: this step's update syncs the target (no target frames hoisted for the next
        step: they would use the old target weights)."""
        self._use_set(p)
        self._hoist_due = due
        self._guard(inm == "H")
        if inm == "P":
            self._sample(qreset=self.tq)
        self._hoist_td_side(due, self._forward_rest)
        self._seg_torso()
        self._update()

    def _hoist_chunk(self, m: int):
        """``m`` hoisted steps back to back: from an even step, none due, every batch pre-sampled."""
        for j in range(m):
            self._hoist_body(j & 1, "H", False)

    def _hoist_td_side(self, due: bool, fwd, before_join=None):
        """The middle of a hoisted step: ``fwd`` (the forward up to and including the TD launch),
        the BPTT + post-BPTT group, the side branch forked at the TD launch, and the join.
        ``before_join`` (the DP step): issued on the main stream after the side branch and before
        the join -- the core gradient bucket's all-reduce start."""
        early = (bool(self.cfg.learner.hoist_early_fork) and self.td_done is not None
                 and not self._early_refused and not _dispatch_serialized())
        if early:
            # fork before the TD launch (the side queue's start latency, ~13 us after its fork
            # event, then overlaps TD); the priority tail waits for TD's done flag on the device
            self._early_fork = torch.cuda.Event()
            self._early_post = None
        try:
            fwd()
        finally:
            after_td, self._early_fork = self._early_fork, None
        # (the fork is recorded only by the fused TD + head launch, td_fuse_head_bwd; without it
        # the side branch forks after TD as before)
        early = early and self._early_post is not None
        main = torch.cuda.current_stream(self.device)
        if not early:
            after_td = torch.cuda.Event()
            after_td.record(main)
        # the BPTT and the weight-gradient group are issued (captured) BEFORE the side branch:
        # the graph keeps the first dependent of the TD node on the TD's queue, so the critical
        # path does not pay a cross-queue hand-off (measured: the BPTT started 11 us after the TD
        # when the side branch was captured first)
        self._backward_core()
        side = self._hoist_side(torso=not due, after_td=after_td, td_wait=early)
        # join before the conv backward: the side branch ends with the BPTT (joining at the end of
        # the step instead let the side torso slow the conv backward: measured slower)
        if before_join is not None:
            before_join()
        main.wait_stream(side)

    # ---- the hoisted step on data-parallel ranks (dist.hoist_dp).  The serial DP step runs the
    # priority tail beside the torso bucket's all-reduce and the counter after the update; here the
    # tail, the counter, the next sample and its shard stats (replay.hip r2_prio_tail_sample_dp) are
    # the side branch, so the shard stats become part of the sample set: an 'H' step's all-gather
    # reads what the previous step's side branch wrote, a 'P' step's what its own sample wrote.
    # The all-gather stays at the step start beside the forward and no collective runs on the side
    # branch: whichever variant a rank replays (ranks decide _hoist_fresh on their own replay), it
    # issues the collectives of ``dp_hoist_plan`` in the same order and meets its peers at each.
    def _gather_fork(self):
        """The shard-stats all-gather of the set in use on its own stream, forked from the main
        stream here beside the torso / LSTM part of the forward (joined by ``_gather_join`` before
        the heads / TD): the only fork and join of it, for every DP form of the step."""
        main = torch.cuda.current_stream(self.device)
        if self._gather_stream is None:
            self._gather_stream = torch.cuda.Stream(device=self.device)
        gs = self._gather_stream
        gs.wait_stream(main)
        with torch.cuda.stream(gs):
            self._gather_dp()

    def _gather_join(self):
        torch.cuda.current_stream(self.device).wait_stream(self._gather_stream)

    def _hseg_sample(self):            # 'P' only: guard (no pre-sampled batch to check) + sample
        self._guard(False)
        self._sample(qreset=self.tq)   # (+ the local shard stats into the set, dp_global)

    def _hseg_fwd_head(self, presampled: bool):
        if presampled:
            self._guard(True)
        self._forward_rest(tail=False)

    def _hseg_core_side(self, due: bool, before_join=None):
        self._hoist_td_side(due, self._forward_tail, before_join)

    def _hoist_dp_body(self, p: int, inm: str, due: bool):
        """The hoisted DP step as stream operations (eager, or captured as the one graph with the
        collectives on their streams).  The segments and collectives of ``dp_hoist_plan`` in its
        order, except that the core bucket's all-reduce starts before the side branch is joined
        (inside one capture that is an edge; between segment graphs it cannot be)."""
        L = self.layout
        self._use_set(p)
        self._hoist_due = due
        if inm == "P":
            self._hseg_sample()
        if self.dp_global:
            self._gather_fork()
        self._hseg_fwd_head(inm == "H")
        if self.dp_global:
            self._gather_join()
        self._hseg_core_side(due, lambda: self._sync().start(0, L.torso_offset))
        self._seg_torso()
        self._sync().start(L.torso_offset, L.padded)
        self._sync().finish()
        self._update()                  # (the side branch's tail already advanced the counter)

    def _hoist_dp_segments(self, p: int, inm: str, due: bool):
        """The hoisted DP step as segment graphs with the collectives issued by the host between
        them (gloo; the dist.one_graph_warm steps; after a rollout fallback), driven by
        ``dp_hoist_plan``."""
        L = self.layout
        self._use_set(p)
        self._hoist_due = due
        key = {"sample": (p,), "fwd_head": (p, inm), "core_side": (p, due), "torso": (p,),
               "update": (due,)}
        coll = {"all_gather": self._gather_fork,
                "all_reduce_core": lambda: self._sync().start(0, L.torso_offset),
                "all_reduce_torso": lambda: (self._sync().start(L.torso_offset, L.padded),
                                             self._sync().finish())}
        for kind, name in dp_hoist_plan(self.dp_global, inm):
            if kind == "collective":
                coll[name]()
                continue
            if name == "core_side" and self.dp_global:
                self._gather_join()
            self._hsegs[(name,) + key[name]].replay()

    def _hseg_as(self, p: Optional[int], due: bool, seg, *args):
        """Segment ``seg`` of the hoisted DP step as its graph is captured: on sample set ``p``
        (None: whichever is in use, the update reads none) with the due decision ``due`` baked in."""
        if p is not None:
            self._use_set(p)
        self._hoist_due = due
        seg(*args)

    def _capture_hoist_dp(self):
        """Every segment graph ``_hoist_dp_segments`` can ask for: sample (set), forward up to the
        heads (set x 'P' / 'H': the guard checks a pre-sampled batch), heads + TD + BPTT + side
        branch + join (set x due), torso backward (set), update (due)."""
        S, sets, dues = self._hseg_as, (0, 1), (False, True)
        jobs = [(("sample", p), S, (p, False, self._hseg_sample)) for p in sets]
        jobs += [(("fwd_head", p, i), S, (p, False, self._hseg_fwd_head, i == "H")) for p in sets for i in "PH"]
        jobs += [(("core_side", p, d), S, (p, d, self._hseg_core_side, d)) for p in sets for d in dues]
        jobs += [(("torso", p), S, (p, False, self._seg_torso)) for p in sets]
        jobs += [(("update", d), S, (None, d, self._update)) for d in dues]
        with self._keep_set():
            self._hsegs = self._capture_graphs(jobs)
        self.graphs += self._hsegs.values()

    def _hoist_step(self, graph: bool):
        """One hoisted step: replayed from the captured variants (``graph``) or issued eagerly."""
        k = self.steps_done
        if self._dev_step_off is None:
            self._dev_step_off = int(self.replay.step.item()) - k
        due = self._due(k + self._dev_step_off)
        p = k & 1
        inm = "H" if self._hoist_fresh() else "P"
        if self.dp:
            if not graph:
                self._hoist_dp_body(p, inm, due)
            elif self._rollout.mode == "one":
                self._use_set(p)
                self._hoist_due = due
                self._one_graphs[(p, inm, due)].replay()
            else:
                self._hoist_dp_segments(p, inm, due)
        elif graph:
            self._use_set(p)
            self._hgraphs[(p, inm, due)].replay()
        else:
            self._hoist_body(p, inm, due)
        self.hoisted_steps += inm == "H"
        self._hoist_ready = True
        self._note_presample()                         # the replay the next batch was sampled from
        self._step_done(graph)

    def _chunk_len(self) -> int:
        if not self.hoist or self.dp:     # (no multi-step chunk graph at DP: run_steps -> step)
            return 1
        return max(1, int(getattr(self.cfg.learner, "graph_chunk", 1)))

    def run_steps(self, n: int) -> None:
        """``n`` learner steps, the same work and results as ``n`` calls of ``step``.  In the
        hoisted graph mode a run of ``learner.graph_chunk`` steps that starts at an even step,
        follows a hoisted step with no replay write since (``_hoist_fresh``; writes happen between
        calls, so never inside a chunk) and has no target sync inside replays as ONE captured graph
        (the hoisted bodies back to back on the same streams): the ~5 us boundary between two
        graph replays (profiles/r06_step_timeline.txt) is paid once per chunk."""
        m = self._chunk_len()
        while n > 0:
            k = self.steps_done
            off = self._dev_step_off
            if (n >= m and m > 1 and self.graph and self._cgraph is not None
                    and (k & 1) == 0 and self._hoist_fresh() and off is not None
                    and not any(self._due(k + j + off) for j in range(m))):
                self._use_set(0)
                self._cgraph.replay()
                self.chunks_run += 1
                self._use_set((m - 1) & 1)
                self._hoist_due = False
                self.hoisted_steps += m
                self._note_presample()
                self.steps_done += m
                n -= m
            else:
                self.step()
                n -= 1

    # ------------------------------------------------------------------ segments
    def _sync(self):
        if self._gsync is None:
            from ..parallel.grad_sync import GradSync
            self._gsync = GradSync(self.grad, self.world, self.pg, self.cfg.dist.grad_dtype,
                                   use_stream=self.cfg.dist.overlap_allreduce, force=self.dp)
        return self._gsync

    def _seg_core(self):
        self._forward_loss()
        self._backward_core()

    def _seg_fwd_head(self):       # DP global sampling: everything before the TD (gather in flight)
        self._forward_rest(tail=False)

    def _seg_core_tail(self):      # ... and from the heads / TD on (gathered stats joined)
        self._forward_tail()
        self._backward_core()

    def _seg_torso(self):
        # the update that follows (same segment) sums the slabs itself when folded
        self._backward_torso(defer_reduce=self._fold_tq is not None)

    def _single_body(self, timer=None, _presampled: bool = False):
        """The world == 1 step as stream operations (eager or captured).  (Running the priority
        refresh + tree repair on a side stream beside the BPTT was measured neutral and removed:
        profiles/r03_prio_side_stream_ab.txt.)"""
        ph = _phase(timer)
        with ph("forward+td"):
            self._forward_loss(_presampled)
        with ph("backward_core"):
            self._backward_core()
        with ph("backward_torso"):
            self._seg_torso()
        with ph("update"):
            self._update()
        with ph("priorities"):
            self._priorities()

    # DP (world > 1): the priority refresh + tree repair need only the forward's TD errors, so
    # they run while the torso bucket is all-reduced; the update and the step counter follow
    def _seg_prio(self):
        self._priorities(end=False)

    def _seg_update(self):
        self._update()
        self.replay.step_end()

    # ------------------------------------------------------------------ public API
    def _step_done(self, graph: bool) -> None:
        """The host bookkeeping every step of ``step`` / ``step_eager`` ends with: count it, then
        (DP steps replayed from graphs) let the one-graph rollout look at it."""
        self.steps_done += 1
        if graph and self.dp:
            self._dp_rollout_after_step()

    def step_eager(self, timer=None, _presampled: bool = False):
        """One step without the graph.  ``timer``: optional utils.profiling.PhaseTimer -- every
        phase is bracketed by HIP events and a roctx range (bench.py --profile-phases).
        ``_presampled`` (private, plain single-rank step only): the caller already sampled this
        step's batch with ``_sample()``, so the step does not sample at its start."""
        L = self.layout
        if _presampled and (self.hoist or self.dp):
            raise ValueError("_presampled: the plain single-rank step only")
        if self.hoist:     # (no per-phase timer: the step's phases overlap on two streams)
            self._hoist_step(graph=False)
            return
        if not self.dp:
            self._single_body(timer, _presampled)
        else:
            ph = _phase(timer)
            with ph("forward+td"):
                self._forward_loss()      # (DP global sampling: includes the stats all-gather)
            with ph("backward_core"):
                self._backward_core()
            self._sync().start(0, L.torso_offset)        # core bucket: overlaps the conv backward
            with ph("backward_torso"):
                self._seg_torso()
            self._sync().start(L.torso_offset, L.padded)  # torso bucket: overlaps the priority tail
            with ph("priorities"):
                self._seg_prio()
            with ph("allreduce_wait"):
                self._sync().finish()
            with ph("update"):
                self._seg_update()
        self._step_done(graph=False)

    def _capture_graph(self, fn, *args, pool=None):
        """``fn(*args)`` captured into a new graph in ``pool`` (None: a pool of its own)."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool, capture_error_mode=self._capture_mode()):
            fn(*args)
        return g

    def _capture_graphs(self, jobs, pool=None):
        """{key: graph} of ``jobs`` = (key, fn, args) in order, all in ``pool`` or else the first one's."""
        out = {}
        for key, fn, args in jobs:
            out[key] = g = self._capture_graph(fn, *args, pool=pool)
            pool = g.pool()
        return out

    @contextlib.contextmanager
    def _keep_set(self):
        """Around a batch of captures: the bodies switch the sample set and the baked due decision,
        so put back what the steps since the last one left (also when a capture raises)."""
        cur, due = self._cur, self._hoist_due
        try:
            yield
        finally:
            self._use_set(cur)
            self._hoist_due = due

    def capture(self, warmup: int = 2):
        """Capture the step into HIP graphs, every variant a step can ask for now and none inside
        a step loop.  world == 1: one graph for the whole step (hoisted: one per variant, and the
        chunk graph).  world > 1 with dist.hoist_dp: ``_capture_hoist_dp``.  world > 1 otherwise:
        four graphs (core fwd/bwd | conv bwd | priorities | update), the two bucket all-reduces
        issued between them on the communication stream; with global sampling the core graph is
        split after the sampling launch (the shard stats are all-gathered from there on, on their
        own stream beside the torso / x-projection / LSTM graph) and again before the heads / TD,
        where the gather is joined (six graphs)."""
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.step_eager()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self.graphs = []
        self._one_dp_graph = False
        self._cgraph = None
        if self.dp:     # segment graphs now; the one graph follows after dist.one_graph_warm steps
            self._make_rollout()
        if self.hoist and self.dp:
            self._capture_hoist_dp()
        elif self.hoist:
            # the hoisted step's graph variants: (sample set, sampled by the previous step or
            # not, target sync due) -- all eight captured now, none inside a timed loop
            with self._keep_set():
                self._hgraphs = self._capture_graphs((key, self._hoist_body, key) for key in _HOIST_VARIANTS)
                # runs of graph_chunk steps starting at an even step, none due, previous step
                # sampled (run_steps): one graph, so the inter-replay boundary is paid once per chunk
                m = self._chunk_len()
                if m > 1:
                    self._cgraph = self._capture_graph(self._hoist_chunk, m,
                                                       pool=self._hgraphs[_HOIST_VARIANTS[0]].pool())
                    _graph_upload(self._cgraph)
        else:
            segs = self._dp_segs() if self.dp else [self._single_body]
            self.graphs += self._capture_graphs((i, fn, ()) for i, fn in enumerate(segs)).values()
            self._seg_replays = [g.replay for g in self.graphs]
        torch.cuda.synchronize(self.device)
        self.graph = True

    def _make_rollout(self) -> None:
        """The segment graphs first; the whole DP step as ONE graph (collectives captured on their
        side streams) replaces them after dist.one_graph_warm steps and, at world > 1, a
        validation window (parallel/graph_rollout.py)."""
        from ..parallel.graph_rollout import GraphRollout
        dc = self.cfg.dist
        one = dc.graph_collectives and (self.world == 1 or dc.graph_collectives_multi)
        self._rollout = GraphRollout(self.pg, self.rank, self.world,
                                     enabled=one and self._pg_backend() == "nccl",
                                     warm=int(dc.one_graph_warm), validate=int(dc.one_graph_validate),
                                     device=self.device)

    def _capture_mode(self) -> str:
        """Graph capture error mode: with a process group the RCCL watchdog thread polls the events
        of earlier collectives while this thread captures, which global mode turns into a capture
        error (hipErrorStreamCaptureUnsupported on the watchdog, seen as a flaky forced-DP test);
        thread-local mode confines the capture rules to this thread."""
        return "thread_local" if self.dp else "global"

    def _pg_backend(self) -> str:
        """Backend of the DP process group (only RCCL collectives can be graph-captured; gloo
        ones -- CPU tests, ranks sharing a GPU -- stay between segment graphs)."""
        import torch.distributed as dist
        try:
            return str(dist.get_backend(self.pg))
        except (RuntimeError, ValueError):
            return ""

    def _dp_segs(self):
        """The serial DP step's segments in order; ``capture`` makes a graph of each."""
        segs = [self._seg_core, self._seg_torso, self._seg_prio, self._seg_update]
        if self.dp_global:
            segs = [self._sample, self._seg_fwd_head, self._seg_core_tail] + segs[1:]
        return segs

    def _dp_step_body(self, segs=None):
        """The DP step as stream operations (capturable): the segments in order, the collectives on
        their side streams with event fork / join.  ``segs``: the replays of the segment graphs
        (``step``: the same operations, the host between the graphs) instead of their bodies."""
        L = self.layout
        if segs is None:
            segs = self._dp_segs()
        if self.dp_global:
            sample, fwd_head, core, torso, prio, update = segs
            sample()
            self._gather_fork()     # beside the torso / x-projection / LSTM segment
            fwd_head()
            self._gather_join()
        else:
            core, torso, prio, update = segs
        core()
        self._sync().start(0, L.torso_offset)
        torso()
        self._sync().start(L.torso_offset, L.padded)
        prio()
        self._sync().finish()
        update()

    def _capture_one_dp(self) -> None:
        """The whole DP step in ONE graph: the bucket all-reduces and the shard-stats all-gather
        are captured on their side streams (fork / join as graph edges), so the ~15 us gap of
        every segment boundary disappears.  The hoisted DP step (dist.hoist_dp): one such graph
        per (sample set, 'P' / 'H', due) variant, the same collectives in the same order in each."""
        torch.cuda.synchronize(self.device)
        pool = self.graphs[0].pool() if self.graphs else None
        if self.hoist:
            with self._keep_set():
                gs = self._capture_graphs(((key, self._hoist_dp_body, key) for key in _HOIST_VARIANTS), pool)
            torch.cuda.synchronize(self.device)
            self._one_graphs = gs
        else:
            g = self._capture_graph(self._dp_step_body, pool=pool)
            torch.cuda.synchronize(self.device)
            self._one_graph = g
        self._one_dp_graph = True

    def _dp_checksum(self) -> torch.Tensor:
        """A fingerprint of this rank's weights (0-d float64, on the device): equal on every rank
        while the ranks stay in lock-step."""
        return self.master.double().sum() + 3.0 * self.target.double().sum()

    def _dp_repair(self) -> None:
        """After a one-graph validation mismatch: every rank takes rank 0's weights and optimizer
        state, re-packs its kernel layouts and (hoisted DP step) drops the pre-sampled batch."""
        import torch.distributed as dist
        src = dist.get_global_rank(self.pg, 0) if hasattr(dist, "get_global_rank") else 0
        for t in (self.master, self.target, self.opt_a, self.opt_b):
            dist.broadcast(t, src=src, group=self.pg)
        self._pack(always=True)
        self._one_dp_graph = False
        self.invalidate_hoist()     # the pre-sampled batch's target frames used the old weights

    def _dp_rollout_after_step(self) -> None:
        ro = self._rollout
        if ro is None:
            return
        if ro.validating():
            if ro.record(self._dp_checksum(), self.err, self.steps_done) is False:
                self._dp_repair()
        elif ro.want_promote(self.steps_done):
            err = None
            try:
                self._capture_one_dp()
            except Exception as e:   # noqa: BLE001 -- the runtime refused the capture
                err = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:120] if str(e) else "")
                self._one_graph, self._one_dp_graph = None, False
                # host-side step state a half-captured body may have left behind
                self._pack_deferred = None
                self._gsync = None
                torch.cuda.synchronize(self.device)
            if ro.agree(err is None):
                ro.promoted()
            else:
                self._one_graph, self._one_dp_graph = None, False
                ro.refused(err or "on another rank")

    def dp_graph_label(self) -> Optional[str]:
        """How the DP step is replayed (bench.py JSON): segment graphs, the one graph (validated
        or still validating), or the fallback after a mismatch; None without DP."""
        if not self.dp:
            return None
        return self._rollout.label() if self._rollout is not None else "eager"

    def step(self):
        if not self.graph:
            self.step_eager()
        elif self.hoist:
            self._hoist_step(graph=True)
        else:
            if not self.dp:
                self.graphs[0].replay()
            elif self._rollout is not None and self._rollout.mode == "one":
                self._one_graph.replay()
            else:
                self._dp_step_body(self._seg_replays)
            self._step_done(graph=True)
