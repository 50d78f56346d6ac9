"""The hoisted learner step on data-parallel ranks (dist.hoist_dp, engine/learner_engine.py
"the hoisted step on data-parallel ranks"): the shard stats folded into the fused priority tail +
sample launch (replay.hip r2_prio_tail_sample_dp), and the hoisted DP step against the serial DP
step, bit for bit -- over RCCL at one forced rank (eager, segment graphs, the one graph) and over
gloo with two ranks sharing this GPU, one of which drops its pre-sampled batch mid-run so the two
replay different variants of the same step."""
import os
import socket
from datetime import timedelta

import pytest
import torch

from pytorch_r2d2_amd.config import get_config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PG_TIMEOUT = timedelta(seconds=120)     # a collective-order bug raises instead of hanging


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("B", [8, 64, 256])
@pytest.mark.parametrize("skip", [0, 2])
def test_tail_sample_shard_stats_match_separate_launch(skip, B):
    """r2_prio_tail_sample_dp: the launch's last sampler workgroup writes [root, n_valid, min_b
    probs[b]] of the batch it just sampled -- the three floats of r2_dp_local_stats run after the
    plain fused launch, bit for bit -- and everything else the launch writes is unchanged.  Three
    rounds: the sync words are back to 0 after each, so rounds 2 and 3 prove the ticket reset.
    B = 8: less than a wave of probabilities; 256: several sequences per sampler workgroup and
    four probabilities per lane of the min."""
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    from pytorch_r2d2_amd.ops._lib import check, kernels, ptr, stream_handle
    cfg = get_config("atari57", **{"replay.capacity": 64000, "replay.n_subrings": 8})
    a = HBMReplay(cfg, DEV)
    a.fill_synthetic(episode_len=200, seed=3)
    b = HBMReplay(cfg, DEV)
    b.fill_synthetic(episode_len=200, seed=3)
    H, Tn = cfg.model.hidden, cfg.replay.seq_len + cfg.replay.n_step
    g = torch.Generator(device=DEV).manual_seed(9)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)   # noqa: E731
    for rnd in range(3):
        idx = z(B, dt=torch.int32)
        a.sample(B, idx, z(B))
        pr = torch.rand(a.capacity, generator=g, device=DEV) * 3
        outs = []
        for r in (b, a):         # b: the plain fused launch + the separate stats launch
            r.priority.copy_(pr)
            st, pb, rows = z(B, dt=torch.int32), z(B), z(Tn * B, dt=torch.int32)
            hs = [(r.hs_cs, 0, z(B, H), z(B, H)), (r.target_hs_cs, 5, z(B, H), z(B, H)),
                  (r.hs_cs, 5, z(B, H), z(B, H))]
            q = torch.full((4,), 7, dtype=torch.int32, device=DEV)
            buf = torch.full((3,), float("nan"), device=DEV)
            outs.append((st, pb, rows, hs, q, buf))
            args = (idx, B, 40, 80, st, pb, rows, Tn, hs, True, q)
            if r is b:
                if not r.prio_tail_sample(*args, skip_xcds=skip):
                    assert B != 64 and rnd == 0, "the bench batch may not be refused"
                    pytest.skip("prio_tail_sample refuses B=%d here without dp_out as well" % B)
                root = r.tree[int(r.tree_offs[-1]): int(r.tree_offs[-1]) + 1]
                check(kernels().r2_dp_local_stats(ptr(root), ptr(r.n_valid), ptr(pb), B, ptr(buf),
                                                  stream_handle()), "dp_local_stats")
            else:
                assert r.prio_tail_sample(*args, skip_xcds=skip, dp_out=buf)
        torch.cuda.synchronize()
        (s1, p1, r1, h1, q1, d1), (s0, p0, r0, h0, q0, d0) = outs
        print("round", rnd, "stats fused", d0.tolist(), "separate", d1.tolist())
        assert not torch.isnan(d0).any() and not torch.isnan(d1).any()
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))
        assert d0[2].item() == p0.min().item() and d0[1].item() == float(a.n_valid.item())
        assert torch.equal(a.tree, b.tree) and torch.equal(a.step, b.step)
        assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(r0, r1)
        for (_, _, ha, ca), (_, _, hb, cb) in zip(h0, h1):
            assert torch.equal(ha, hb) and torch.equal(ca, cb)
        assert q0.tolist() == q1.tolist() == [0, 0, 7, 7]
        assert a.prio_sync.tolist() == [0] * 8, a.prio_sync.tolist()
        assert b.prio_sync.tolist() == [0] * 8, b.prio_sync.tolist()
        assert int(a.dirty_count.item()) == 0 and int(a.step.item()) == rnd + 1


# ---------------------------------------------------------------- engines under test
def _engine(pg, rank=0, world=1, fill_seed=3, **over):
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    kw = {"seed": 1234, "learner.batch_size": 16, "learner.target_update_interval": 3}
    kw.update(over)
    cfg = get_config("atari57", **kw)
    rp = HBMReplay(cfg, DEV, capacity=64000)
    rp.fill_synthetic(episode_len=200, seed=fill_seed)
    return rp, LearnerEngine(cfg, rp, DEV, rank=rank, world=world, process_group=pg)


def _state(rp, eng):
    """tests/test_hoist_gpu.py's state set (master, target, both moments, every packed layout by
    name, priorities, tree, step counter, loss) + the DP step's own outputs."""
    out = {"master": eng.master, "target": eng.target, "opt_a": eng.opt_a, "opt_b": eng.opt_b,
           "lstm_b": eng.lstm_b, "lstm_b_t": eng.lstm_b_t, "priority": rp.priority,
           "tree": rp.tree, "step": rp.step, "loss": eng.loss,
           "dp_recv": eng.dp_recv, "dp_params": eng.dp_params, "is_w": eng.is_w,
           "starts": eng.starts}
    for tag, (bf, f32) in {"": (eng.bf, eng.f32), "_t": (eng.bf_t, eng.f32_t)}.items():
        for plane in range(bf.shape[0]):
            for k, v in eng.layout.packed_views(bf[plane], f32).items():
                out["%s%s.%d" % (k, tag, plane)] = v
    return out


def _same(i, rp0, e0, rp1, e1):
    torch.cuda.synchronize()
    a, b = _state(rp0, e0), _state(rp1, e1)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (i, bad)


# ---------------------------------------------------------------- 2. one forced rank over RCCL
_MODES = {"eager": {"learner.use_graph": False},
          "segments": {"learner.use_graph": True, "dist.graph_collectives": False},
          "one": {"learner.use_graph": True, "dist.graph_collectives": True},
          "eager-local": {"learner.use_graph": False, "dist.global_sampling": False}}


def _forced_worker(rank, port, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0), timeout=PG_TIMEOUT)
    over = dict(_MODES[mode], **{"dist.force_dp": True})
    pg = dist.group.WORLD
    rp0, serial = _engine(pg, **over, **{"dist.hoist_dp": False})
    rp1, hoist = _engine(pg, **over, **{"dist.hoist_dp": True})
    assert serial.dp and not serial.hoist
    assert hoist.dp and hoist.hoist
    assert hoist.dp_global == (mode != "eager-local")
    graph = bool(over["learner.use_graph"])
    if graph:
        serial.capture(warmup=0)
        hoist.capture(warmup=0)
    for i in range(10):
        if i == 6:
            hoist.invalidate_hoist()
        serial.step()
        hoist.step()
        _same(i, rp0, serial, rp1, hoist)
    assert serial.error_word() == 0 and hoist.error_word() == 0
    assert hoist.hoisted_steps == 8, hoist.hoisted_steps
    if graph:
        want = "one" if mode == "one" else "segments"
        assert hoist._rollout.mode == want, hoist.dp_graph_label()
        assert serial._rollout.mode == want, serial.dp_graph_label()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", list(_MODES))
def test_forced_dp_hoisted_step_is_bitwise_the_serial_dp_step(mode):
    """The N-GPU step at ONE rank over RCCL (dist.force_dp), target sync every 3 steps, one
    invalidation before step 6 (that step samples at its start): after each of 10 steps the hoisted
    DP engine's weights, moments, packed layouts, priorities, tree, counter, loss, gathered stats,
    IS parameters and weights, and batch equal the serial DP engine's.  ``one``: steps 0-2 replay
    the segment graphs (dist.one_graph_warm), 3-9 the one graph of each variant."""
    import torch.multiprocessing as tmp
    tmp.spawn(_forced_worker, args=(_free_port(), mode), nprocs=1, join=True)


# ---------------------------------------------------------------- 3. two ranks over gloo
def _two_rank_worker(rank, port, outdir, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE="2", LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", timeout=PG_TIMEOUT)
    pg = dist.group.WORLD
    over = {"learner.use_graph": graph}
    rp0, serial = _engine(pg, rank, 2, fill_seed=3 + rank, **over, **{"dist.hoist_dp": False})
    rp1, hoist = _engine(pg, rank, 2, fill_seed=3 + rank, **over, **{"dist.hoist_dp": True})
    assert serial.dp and serial.dp_global and not serial.hoist
    assert hoist.dp and hoist.dp_global and hoist.hoist
    if graph:
        serial.capture(warmup=0)
        hoist.capture(warmup=0)
    for i in range(8):
        if i == 4 and rank == 1:
            hoist.invalidate_hoist()     # rank 0 replays an 'H' variant of step 4, rank 1 a 'P'
        serial.step()
        hoist.step()
        _same(i, rp0, serial, rp1, hoist)
    assert serial.error_word() == 0 and hoist.error_word() == 0
    torch.save({"master": hoist.master.cpu(), "loss": hoist.loss_value(),
                "hoisted_steps": hoist.hoisted_steps},
               os.path.join(outdir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_two_ranks_hoisted_dp_matches_serial_dp(tmp_path, graph):
    """Two ranks on this GPU over gloo, different replay shards: a serial-DP and a hoisted-DP
    engine step alternately on each rank and stay bitwise equal for 8 steps, although rank 1 drops
    its pre-sampled batch before step 4 and so replays another variant of that step than rank 0
    (the collectives still pair up: the run ends within the group timeout)."""
    import torch.multiprocessing as tmp
    tmp.spawn(_two_rank_worker, args=(_free_port(), str(tmp_path), graph), nprocs=2, join=True)
    a = torch.load(tmp_path / "rank0.pt", weights_only=True)
    b = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(a["master"], b["master"])
    assert a["loss"] != b["loss"]
    assert a["hoisted_steps"] == 7 and b["hoisted_steps"] == 6


# ---------------------------------------------------------------- 4. off by default
def _default_worker(rank, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0), timeout=PG_TIMEOUT)
    cfg = get_config("atari57", **{"learner.batch_size": 8, "replay.burn_in": 4, "replay.learn": 4,
                                   "replay.overlap": 4, "seed": 11, "dist.force_dp": True})
    assert cfg.learner.hoist and not cfg.dist.hoist_dp
    rp = HBMReplay(cfg, DEV, capacity=8 * 200, n_subrings=8)
    rp.fill_synthetic(episode_len=50, seed=0)
    eng = LearnerEngine(cfg, rp, DEV, process_group=dist.group.WORLD)
    assert eng.dp and eng.dp_global and not eng.hoist
    assert len(eng._sets) == 1
    eng.capture(warmup=1)
    assert len(eng.graphs) == 6
    eng.step()
    torch.cuda.synchronize()
    assert eng.error_word() == 0 and eng.hoisted_steps == 0
    dist.destroy_process_group()


def test_hoist_dp_is_off_by_default():
    """Forced DP without the knob is the serial DP step: no hoist, the six segment graphs."""
    import torch.multiprocessing as tmp
    tmp.spawn(_default_worker, args=(_free_port(),), nprocs=1, join=True)
