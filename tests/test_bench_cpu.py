"""bench.py pieces that need no GPU: the size cap of --dump-outputs and the option surface."""
import itertools

import pytest

import bench


@pytest.mark.parametrize("budget", [1, 7, 64, 1000])
def test_dump_cap_keeps_the_total_within_budget(budget):
    """Every multiset of sizes from a small alphabet: whole arrays while they fit (cap None), else
    the capped total is within the budget and no more than one share (len(sizes) elements of
    rounding) below it."""
    for sizes in itertools.combinations_with_replacement([1, 3, 8, 50, 400, 5000], 4):
        cap = bench.dump_cap(sizes, budget)
        if sum(sizes) <= budget:
            assert cap is None or sum(min(n, cap) for n in sizes) == sum(sizes), (sizes, cap)
            continue
        assert cap is not None, sizes
        total = sum(min(n, cap) for n in sizes)
        assert budget - len(sizes) <= total <= budget, (sizes, cap, total)


def test_full_and_dump_outputs_are_options(capsys):
    with pytest.raises(SystemExit) as e:
        bench.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text
