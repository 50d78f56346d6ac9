"""dist.hoist_dp (the hoisted learner step on data-parallel ranks): the config knob and the
collective order of the step (engine/learner_engine.py dp_hoist_plan).  Ranks decide on their own
replay whether a step samples at its start ('P') or trains on the batch the previous step's side
branch sampled ('H'), so two ranks may replay different variants of the same step: the sequence of
collectives must not depend on the variant."""
import pytest

from pytorch_r2d2_amd.config import DistConfig, get_config


def _collectives(plan):
    return [name for kind, name in plan if kind == "collective"]


def test_knob_exists_and_is_off_by_default():
    assert DistConfig().hoist_dp is False
    assert get_config("atari57").dist.hoist_dp is False
    assert get_config("seaquest8").dist.hoist_dp is False


def test_knob_parses_through_the_dotted_override():
    assert get_config("atari57", **{"dist.hoist_dp": "true"}).dist.hoist_dp is True
    assert get_config("atari57", **{"dist.hoist_dp": "false"}).dist.hoist_dp is False
    assert get_config("atari57", **{"dist.hoist_dp": True}).dist.hoist_dp is True


@pytest.mark.parametrize("dp_global", [True, False])
def test_collective_order_does_not_depend_on_the_variant(dp_global):
    from pytorch_r2d2_amd.engine.learner_engine import dp_hoist_plan
    p, h = dp_hoist_plan(dp_global, "P"), dp_hoist_plan(dp_global, "H")
    assert _collectives(p) == _collectives(h)
    want = ["all_reduce_core", "all_reduce_torso"]
    assert _collectives(p) == (["all_gather"] + want if dp_global else want)
    # the variants differ only by the sample segment at the start of 'P'
    assert p[0] == ("segment", "sample") and p[1:] == h
    assert ("segment", "sample") not in h


def test_plan_without_global_sampling_has_no_all_gather():
    from pytorch_r2d2_amd.engine.learner_engine import dp_hoist_plan
    for inm in "PH":
        assert "all_gather" not in _collectives(dp_hoist_plan(False, inm))


def test_plan_order_of_segments_and_collectives():
    """The all-gather is issued before the forward it runs beside and joined before the segment
    with the TD launch; the side branch lives inside that segment (no priority segment, no
    collective of its own); the core bucket follows it, the torso bucket the torso backward."""
    from pytorch_r2d2_amd.engine.learner_engine import dp_hoist_plan
    names = [n for _, n in dp_hoist_plan(True, "P")]
    assert names == ["sample", "all_gather", "fwd_head", "core_side", "all_reduce_core", "torso",
                     "all_reduce_torso", "update"]
    with pytest.raises(ValueError):
        dp_hoist_plan(True, "X")
