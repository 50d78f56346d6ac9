"""The oracle of the evaluator's launches (pytorch_r2d2_amd/eval_ref.py) against a plain per-env
Python loop, every entry of ``MUTATIONS`` against ``check``, the result aggregation, the
constructor's refusals and the public switches (EvalConfig, ``main.py --mode eval``).

Also holds the scripted case and its builders, which the GPU test (test_eval_gpu.py) shares.
"""
import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import eval_ref as er
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.config import PRESETS, get_config
from pytorch_r2d2_amd.evaluator import BatchedEvaluator, aggregate, check_eval_params
from pytorch_r2d2_amd.refnum import bf16_bits

E, H, K, N = 5, 8, 2, 12
EPS = np.asarray([0.0, 1.0, 0.4, 0.0, 0.4], np.float32)
SEED = 0x9E3779B97F4A7C15 ^ 0x1234567
# env 0 finishes 3 episodes (one past the quota), env 1 none, envs 2 and 3 finish on step 5
DONE_AT = {0: (2, 6, 10), 1: (), 2: (5,), 3: (5, 11), 4: (7,)}
SIZES = (6, 18)


def make_logs(A):
    rng = np.random.default_rng(100 + A)
    q = (rng.integers(-3, 4, size=(N, E, A)) * 0.5).astype(np.float32)      # a few levels: ties
    q[:, 0, :] = np.minimum(q[:, 0, :], 1.0)
    q[:, 0, 2] = q[:, 0, A - 1] = 2.0          # env 0 (eps 0): the maximum at 2 and at the last index
    q[:, 3, :] = -0.25                          # env 3 (eps 0): every action ties
    q[N // 2:, 3, A - 1] = 0.75                 # ... later a single maximum, the last index
    done = np.zeros((N, E), bool)
    for e, steps in DONE_AT.items():
        done[list(steps), e] = True
    reward = rng.integers(0, 2, size=(N, E)).astype(np.float32)
    finished = np.where(done, rng.normal(size=(N, E)) * 7, np.nan).astype(np.float32)
    h_new = rng.normal(size=(N, E, H)).astype(np.float32)
    c_new = rng.normal(size=(N, E, H)).astype(np.float32)
    return er.EvalLogs(q=q, h_new=h_new, c_new=c_new, reward=reward, done=done, finished=finished,
                       eps=EPS, seed=SEED)


LOGS = {A: make_logs(A) for A in SIZES}


def poison_init():
    """What the launches' output buffers hold before the first step: poison where the kernels
    write before they read, zero for the counters they read."""
    return dict(act=np.full(E, -1, np.int64), h32=np.full((E, H), np.nan, np.float32),
                c=np.full((E, H), np.nan, np.float32), h_bf=np.full((E, H), 0x7FC0, np.uint16),
                ret=np.full((E, K), np.nan, np.float32), ep_len=np.full((E, K), -1, np.int32),
                n_done=np.zeros(E, np.int32), len=np.zeros(E, np.int32),
                total_done=np.zeros(1, np.int32), counted_steps=np.zeros(1, np.int64),
                t=np.zeros(1, np.int64))


def as_kernel(o, init):
    """``EvalRef.at`` as the memory a kernel with that behaviour leaves: the init's bits in every
    cell it has not written."""
    g = {}
    for name in ("h32", "c", "h_bf"):
        g[name] = np.asarray(o[name]).copy() if o["carried_w"] else init[name].copy()
    for name in ("ret", "ep_len"):
        g[name] = np.where(o["ret_w"], o[name], init[name]).astype(init[name].dtype)
    g["act"] = init["act"].copy() if o["act"] is None else o["act"].astype(np.int64)
    for name in ("n_done", "len"):
        g[name] = o[name].astype(np.int32)
    g["total_done"] = np.asarray([o["total_done"]], np.int32)
    g["counted_steps"] = np.asarray([o["counted_steps"]], np.int64)
    g["t"] = np.asarray([o["t"]], np.int64)
    return g


# ------------------------------------------------------------------ the oracle itself
def plain_loop(lg, S):
    """The state after S steps, one env at a time, written from the rules."""
    A = lg.q.shape[2]
    out = dict(act=np.zeros(E, np.int64), h32=np.zeros((E, H), np.float32), c=np.zeros((E, H), np.float32),
               ret=np.full((E, K), np.nan, np.float32), ep_len=np.full((E, K), -1, np.int32),
               n_done=np.zeros(E, np.int32), len=np.zeros(E, np.int32))
    total = counted = 0
    for e in range(E):
        h, c = np.zeros(H, np.float32), np.zeros(H, np.float32)
        n_done = length = act = 0
        for t in range(S):
            row = lg.q[t, e]
            best = 0
            for i in range(1, A):
                if row[i] > row[best]:
                    best = i
            u = float(rr.uniform(lg.seed, t, np.asarray([2 * e]))[0])
            u2 = np.float32(rr.uniform(lg.seed, t, np.asarray([2 * e + 1]))[0])
            act = min(int(np.float32(u2 * np.float32(A))), A - 1) if u < float(lg.eps[e]) else best
            length += 1
            if n_done < K:
                counted += 1
            if lg.done[t, e]:
                if n_done < K:
                    out["ret"][e, n_done] = lg.finished[t, e]
                    out["ep_len"][e, n_done] = length
                    n_done += 1
                    total += 1
                length = 0
                h, c = np.zeros(H, np.float32), np.zeros(H, np.float32)
            else:
                h, c = lg.h_new[t, e], lg.c_new[t, e]
        out["act"][e], out["h32"][e], out["c"][e] = act, h, c
        out["n_done"][e], out["len"][e] = n_done, length
    out["h_bf"] = bf16_bits(out["h32"])
    out.update(total_done=total, counted_steps=counted, t=S)
    return out


def test_the_case_has_what_it_is_for():
    for A in SIZES:
        lg = LOGS[A]
        assert lg.q.shape == (N, E, A) and lg.eps.tolist() == [0.0, 1.0, 0.4000000059604645, 0.0, 0.4000000059604645]
        ends = lg.done.sum(axis=0).tolist()
        assert ends == [3, 0, 1, 2, 1] and ends[0] == K + 1
        assert lg.done[5].sum() == 2                                   # two envs finish on one step
        top = lg.q == lg.q.max(axis=2, keepdims=True)
        assert (top.sum(axis=2) > 1).any() and (top[:, 0, A - 1] & top[:, 0, 2]).all()   # ties, last index
        ref = er.EvalRef(lg, K)
        assert (ref.act[:, 0] == 2).all(), "eps 0 with a tie at the last index takes the first maximum"
        assert (ref.act[: N // 2, 3] == 0).all() and (ref.act[N // 2:, 3] == A - 1).all()
        # eps 1 always draws: not every action is the greedy one
        assert (ref.act[:, 1] != np.argmax(lg.q[:, 1], axis=1)).any()


@pytest.mark.parametrize("A", SIZES)
def test_oracle_agrees_with_a_plain_loop(A):
    lg = LOGS[A]
    ref = er.EvalRef(lg, K)
    init = poison_init()
    for S in range(N + 1):
        want, plain = ref.at(S), plain_loop(lg, S)
        for name in ("h32", "c", "h_bf", "n_done", "len"):
            assert np.array_equal(np.asarray(want[name]).view(np.uint8), np.asarray(plain[name]).astype(
                np.asarray(want[name]).dtype).view(np.uint8)), (S, name)
        for name in ("total_done", "counted_steps", "t"):
            assert want[name] == plain[name], (S, name)
        if S:
            assert np.array_equal(want["act"], plain["act"])
        w = want["ret_w"]
        assert np.array_equal(w, plain["ep_len"] >= 0)
        assert np.array_equal(want["ret"][w].view(np.uint32), plain["ret"][w].view(np.uint32))
        assert np.array_equal(want["ep_len"][w], plain["ep_len"][w])
        assert er.check(as_kernel(want, init), want, init) == len(er.EXACT)
    end = ref.at(N)
    assert end["n_done"].tolist() == [2, 0, 1, 2, 1] and end["total_done"] == 6
    assert end["ep_len"][0].tolist() == [3, 4] and end["ep_len"][3].tolist() == [6, 6]
    # env 0 stops counting with its second episode (step 6), env 3 with the last step
    assert end["counted_steps"] == 7 + N + N + N + N


SHOWN = dict(last_max="first maximum", past_quota="quota", no_state_reset="reset", t_twice="t")


@pytest.mark.parametrize("A", SIZES)
@pytest.mark.parametrize("mutation", er.MUTATIONS)
def test_check_rejects_a_mutated_result(mutation, A):
    assert set(SHOWN) == set(er.MUTATIONS)
    lg = LOGS[A]
    ref, bad = er.EvalRef(lg, K), er.EvalRef(lg, K, mutation)
    init = poison_init()
    rejected = 0
    for S in range(1, N + 1):
        try:
            er.check(as_kernel(bad.at(S), init), ref.at(S), init)
        except AssertionError:
            rejected += 1
    assert rejected > 0, f"{mutation} passes every check"


def test_check_rejects_a_cell_written_too_early():
    lg = LOGS[6]
    ref, init = er.EvalRef(lg, K), poison_init()
    got = as_kernel(ref.at(3), init)
    got["ret"][1, 0] = 1.0                        # env 1 never finishes
    with pytest.raises(AssertionError):
        er.check(got, ref.at(3), init)


# ------------------------------------------------------------------ aggregation
def test_aggregate_with_unfinished_cells():
    ret = np.asarray([[1.0, 3.0], [5.0, 99.0], [77.0, 88.0]], np.float32)      # 99, 77, 88: stale cells
    ln = np.asarray([[4, 6], [8, 123], [5, 5]], np.int32)
    out = aggregate(ret, ln, [2, 1, 0], counted_steps=31)
    assert out["episodes"] == 3 and not out["complete"] and out["env_steps"] == 31
    assert out["mean_return"] == 3.0 and out["min_return"] == 1.0 and out["max_return"] == 5.0
    assert out["std_return"] == pytest.approx(np.std([1.0, 3.0, 5.0]), rel=1e-15)
    assert out["mean_length"] == 6.0
    assert np.array_equal(np.isnan(out["returns"]), [[False, False], [False, True], [True, True]])
    assert out["lengths"].tolist() == [[4, 6], [8, -1], [-1, -1]]
    assert ret[1, 1] == 99.0, "the input tables are left as they are"
    full = aggregate(ret, ln, [2, 2, 2], 40)
    assert full["complete"] and full["episodes"] == 6
    none = aggregate(ret, ln, [0, 0, 0], 0)
    assert none["episodes"] == 0 and not none["complete"] and np.isnan(none["mean_return"])


# ------------------------------------------------------------------ constructor, config, CLI
class _Env:
    def __init__(self, n):
        self.E, self.frames, self.episode_len = n, torch.zeros(n, 4, dtype=torch.uint8), 8

    def reset_all(self):
        raise AssertionError("a refused constructor touches nothing")

    step = reset_all


@pytest.mark.parametrize("n, kw", [(257, {}), (4, dict(episodes_per_env=0)), (4, dict(epsilon=1.5)),
                                   (4, dict(epsilon=-0.1)), (4, dict(epsilon=[0.0, 0.1, 0.2])),
                                   (4, dict(epsilon=[0.0, 0.1, float("nan"), 0.2]))])
def test_constructor_refusals(n, kw):
    with pytest.raises(ValueError):
        BatchedEvaluator(get_config("atari57"), _Env(n), None, **kw)


def test_constructor_refuses_an_env_without_the_contract():
    with pytest.raises(TypeError):
        BatchedEvaluator(get_config("atari57"), object(), None)


def test_epsilon_scalar_or_vector():
    assert check_eval_params(3, 1, 0.25).tolist() == [0.25] * 3
    assert check_eval_params(256, 2, 1.0).shape == (256,)
    v = check_eval_params(2, 1, [0.0, 1.0])
    assert v.dtype == np.float32 and v.tolist() == [0.0, 1.0]


def test_eval_config_in_every_preset_and_overridable():
    for name in PRESETS:
        ec = get_config(name).eval
        assert (ec.envs, ec.episodes_per_env, ec.epsilon, ec.every) == (64, 1, 0.0, 0)
        assert isinstance(ec.seed, int)
    cfg = get_config("pong", **{"eval.envs": 8, "eval.every": "50", "eval.epsilon": "0.05"})
    assert (cfg.eval.envs, cfg.eval.every, cfg.eval.epsilon) == (8, 50, 0.05)
    assert cfg.to_dict()["eval"]["envs"] == 8


def test_main_parser_accepts_eval_mode():
    import main
    a = main.build_parser().parse_args(["--mode", "eval", "--checkpoint", "save/7_save.pt", "--episodes", "3",
                                        "--eval-eps", "0.01", "--set", "eval.envs=8"])
    assert (a.mode, a.checkpoint, a.episodes, a.eval_eps) == ("eval", "save/7_save.pt", 3, 0.01)
    with pytest.raises(SystemExit):
        main.run(["--mode", "eval"])            # no checkpoint


def test_run_native_refuses_eval_with_the_concurrent_driver():
    from pytorch_r2d2_amd.runner import run_native
    with pytest.raises(ValueError, match="serial loop"):
        run_native(get_config("pong"), steps=1, concurrent=True, eval_every=2)
