"""fp32 inference (``actor.compute_dtype`` / ``eval.compute_dtype``) without a GPU: the knobs and
their command-line path, every refusal at construction, the hi / lo weight planes of
``PackedWeights(split=True)`` and ``engine_weights``, and the ctypes entry of the new step kernel."""
import inspect
import types

import pytest
import torch

import main
from pytorch_r2d2_amd import actor_batched as ab
from pytorch_r2d2_amd.config import ActorConfig, EvalConfig, get_config
from pytorch_r2d2_amd.engine.layout import ParamLayout
from pytorch_r2d2_amd.evaluator import BatchedEvaluator
from pytorch_r2d2_amd.ops import _lib


def test_defaults_stay_bf16_and_the_knobs_parse():
    assert ActorConfig().compute_dtype == "bf16" and EvalConfig().compute_dtype == "bf16"
    for preset in ("reference", "cartpole", "pong", "atari57", "seaquest8", "dmlab30"):
        c = get_config(preset)
        assert c.actor.compute_dtype == "bf16" and c.eval.compute_dtype == "bf16"
    c = get_config("pong", **{"actor.compute_dtype": "fp32", "eval.compute_dtype": "fp32"})
    assert c.actor.compute_dtype == "fp32" and c.eval.compute_dtype == "fp32"
    assert c.to_dict()["actor"]["compute_dtype"] == "fp32"


def test_the_knobs_reach_the_runners_through_set(monkeypatch):
    """main.py --set actor.compute_dtype=fp32 / eval.compute_dtype=fp32 in --mode native (serial and
    --concurrent) and --mode eval: the configuration the runner receives carries them."""
    from pytorch_r2d2_amd import runner
    seen = []
    monkeypatch.setattr(runner, "run_native", lambda cfg, **kw: seen.append((cfg, kw)) or {})
    monkeypatch.setattr(runner, "run_eval", lambda cfg, ckpt, **kw: seen.append((cfg, kw)) or {})
    sets = ["--set", "actor.compute_dtype=fp32", "eval.compute_dtype=fp32", "eval.every=5"]
    main.run(["--mode", "native", "--config", "pong", "--steps", "1", *sets])
    main.run(["--mode", "native", "--config", "pong", "--steps", "1", "--concurrent", *sets])
    main.run(["--mode", "eval", "--config", "pong", "--checkpoint", "x.pt", *sets])
    assert len(seen) == 3 and seen[1][1]["concurrent"] is True
    for cfg, _ in seen:
        assert cfg.actor.compute_dtype == "fp32" and cfg.eval.compute_dtype == "fp32" and cfg.eval.every == 5


class _W:
    def __init__(self, lo):
        self.pk, self.pk_lo, self.lstm_b, self.flat = {}, ({} if lo else None), None, None


REFUSALS = {
    "another string": ("atari57", {}, "fp16", True),
    "dmlab30 geometry": ("dmlab30", {}, "fp32", True),
    "mlp torso": ("cartpole", {}, "fp32", True),
    "hidden 512": ("atari57", {"model.hidden": 512}, "fp32", True),
    "weights without lo planes": ("atari57", {}, "fp32", False),
}


@pytest.mark.parametrize("what", list(REFUSALS))
@pytest.mark.parametrize("knob", ["actor.compute_dtype", "eval.compute_dtype"])
def test_refusals_name_the_knob(knob, what):
    preset, over, value, lo = REFUSALS[what]
    cfg = get_config(preset, **over, **{knob: value})
    with pytest.raises(ValueError, match=knob.replace(".", r"\.")):
        ab.check_compute_dtype(knob, value, cfg, (_W(lo),))
    # at construction, before anything is allocated or any library is loaded
    with pytest.raises(ValueError, match=knob.replace(".", r"\.")):
        if knob.startswith("actor"):
            ab.BatchedActor(cfg, None, None, _W(lo), _W(True))
        else:
            env = types.SimpleNamespace(frames=torch.zeros(4, 1), step=None, reset_all=None, E=4)
            BatchedEvaluator(cfg, env, _W(lo))


def test_accepted_settings():
    cfg = get_config("atari57")
    assert ab.check_compute_dtype("actor.compute_dtype", "bf16", cfg, (_W(False),)) is False
    assert ab.check_compute_dtype("actor.compute_dtype", "fp32", cfg, (_W(True), _W(True))) is True
    for H in (64, 128, 256):
        c = get_config("atari57", **{"model.hidden": H})
        assert ab.check_compute_dtype("eval.compute_dtype", "fp32", c, (_W(True),)) is True


def test_packed_weights_and_engine_weights_expose_the_lo_planes():
    assert "split" in inspect.signature(ab.PackedWeights.__init__).parameters
    eng = types.SimpleNamespace(pk={"a": 1}, pk_t={"a": 2}, pk_lo={"a": 3}, pk_t_lo={"a": 4},
                                lstm_b=5, lstm_b_t=6, master=7, target=8)
    on, tg = ab.engine_weights(eng)
    assert (on.pk, on.pk_lo, on.lstm_b, on.flat) == ({"a": 1}, {"a": 3}, 5, 7)
    assert (tg.pk, tg.pk_lo, tg.lstm_b, tg.flat) == ({"a": 2}, {"a": 4}, 6, 8)
    eng.pk_lo = eng.pk_t_lo = None            # a bf16 engine
    assert ab.engine_weights(eng)[0].pk_lo is None and ab.engine_weights(eng)[1].pk_lo is None
    cfg = get_config("atari57")
    L = ParamLayout(cfg.model, cfg.env)
    plain, split = ab.PackedWeights(L, "cpu"), ab.PackedWeights(L, "cpu", split=True)
    assert plain.pk_lo is None and plain.bf.shape == (L.bf_numel,)
    assert split.bf.shape == (2, L.bf_numel) and set(split.pk_lo) == set(split.pk)
    for k, v in split.pk.items():
        lo = split.pk_lo[k]
        assert lo.shape == v.shape and lo.stride() == v.stride()
        if v.dtype == torch.bfloat16:         # the lo plane sits one plane behind the hi plane
            assert lo.data_ptr() - v.data_ptr() == 2 * L.bf_numel
        else:                                 # fp32 entries (biases, the last head layer) are shared
            assert lo.data_ptr() == v.data_ptr()


def test_step_kernel_entry_is_declared():
    assert len(_lib._SIGS["r2_lstm_fwd_sp"]) == 7
    assert _lib._SIGS["r2_lstm_fwd_sp"] == _lib._SIGS["r2_lstm_fwd"]
    if not _lib.available():
        pytest.skip("kernel library not built")
    k = _lib.kernels()
    with pytest.raises(TypeError):
        k.r2_lstm_fwd_sp(0, 1, 1, 1, 64, 0)
    # refused before anything is read: n_chains 0, B 0, H 96
    assert k.r2_lstm_fwd_sp(0, 0, 4, 1, 64, 0, 0) == -1
    assert k.r2_lstm_fwd_sp(0, 1, 0, 1, 64, 0, 0) == -1
