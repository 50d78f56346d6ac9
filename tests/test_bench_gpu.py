"""bench.py --dump-outputs on the GPU: the paper batch on a small replay, a few steps."""
import json
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

NAMES = {"loss", "q_online", "td_abs", "online_params", "target_params", "opt_a", "opt_b",
         "replay_priority"}


def _run(tmp_path, capsys, tag, steps):
    out = tmp_path / tag
    bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--capacity", "200000",
                "--dump-outputs", str(out)])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(line) == 1
    return json.loads(line[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_dump_outputs_writes_the_last_steps_results_and_repeats(tmp_path, capsys):
    """Two runs with the same arguments see the same inputs: every dumped array is float32,
    finite, within 64 MB in all, and bitwise the same in both runs (the step has no
    order-dependent accumulation: tests/test_hoist_gpu.py compares it bitwise too).  One step
    more changes the weights and the loss: --steps sets the number of steps that really run.
    The result line keeps its contract fields."""
    res, a = _run(tmp_path, capsys, "a", 3)
    _, b = _run(tmp_path, capsys, "b", 3)
    _, c = _run(tmp_path, capsys, "c", 4)
    assert set(a) == NAMES
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        assert np.array_equal(v, b[k]), k
    assert a["q_online"].shape == (40 * 64, 6) and a["td_abs"].shape == (40 * 64,)
    assert a["online_params"].size >= 2037095 and np.abs(a["opt_b"]).max() > 0
    assert not np.array_equal(a["online_params"], c["online_params"])
    assert not np.array_equal(a["loss"], c["loss"])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["metric"] == "learner_steps_per_sec" and res["higher_is_better"] is True
    assert res["dtype"] == "fp32" and res["kernel_error_word"] == 0
    assert res["final_loss"] == float(a["loss"][0])
