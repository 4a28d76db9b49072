"""tests/depsim.py, the sequential restatement of src/inter_dc_dep_vnode.erl:94-154, 187-238 that is the
contract of am_dep: the literal outputs of the hand cases pin it to that reading of the reference, the
reversed queue order swaps the two late-bump cases, and the clock is set, not maxed."""
import pytest

from tests import depcases
from tests.depsim import DepSim

CASES = depcases.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_give_their_literal_outputs(case):
    _, n_dc, own, order, steps = case
    sim = DepSim(n_dc, own, order)
    for (_, dc, ts, snap, ping, tag), now, delivered, clock in steps:
        assert sim.handle((dc, ts, snap, ping, tag), now) == delivered
        assert sim.clock == clock


def test_reversed_order_swaps_the_late_bump_cases():
    by = {c[0]: [d for _, _, d, _ in c[4]] for c in CASES}
    assert by["late-bump"] == [[], [], [depcases.A]] and by["late-bump-reversed"] == [[], [depcases.A], []]
    assert by["late-bump-mirrored"] == [[], [depcases.A]] and by["late-bump-mirrored-reversed"] == [[], []]


def test_chain_takes_eight_rounds_and_grows_with_its_length():
    for links, rounds in ((6, 8), (12, 14)):
        arr, ping, want = depcases.chain(links)
        sim = DepSim(4, 0)
        for t in arr:
            assert sim.handle(t[1:], 100) == []
        before = sim.rounds
        assert sim.handle(ping[1:], 100) == want
        assert sim.rounds - before == rounds
        assert sim.clock == {1: 2 * links - 1, 2: 2 * links, 3: 1}


def test_clock_is_set_not_maxed_under_decreasing_timestamps():
    sim = DepSim(3, 0)
    assert sim.handle((1, 9, {}, False, 1), 0) == [1] and sim.clock == {1: 9}
    assert sim.handle((1, 4, {}, False, 2), 0) == [2] and sim.clock == {1: 4}
    assert sim.handle((1, 3, {2: 1}, False, 3), 0) == [] and sim.clock == {1: 2}
    assert sim.handle((1, 1, {}, True, 4), 0) == [] and sim.clock == {1: 2} and sim.queued(1) == [3, 4]
    assert sim.handle((2, 1, {}, True, 5), 0) == [3] and sim.clock == {1: 1, 2: 1}


def test_own_entry_appears_only_when_set_or_named_as_origin():
    sim = DepSim(3, 0)
    sim.handle((1, 5, {0: 7}, False, 1), 7)
    assert 0 not in sim.clock
    sim.set_dependency_clock({0: 3, 2: 8})
    assert sim.clock == {0: 3, 2: 8}
    sim.handle((0, 6, {}, False, 2), 7)
    assert sim.clock == {0: 6, 2: 8}


def test_drop_ping_pops_without_a_clock_change_and_timestamp_zero_is_rejected():
    sim = DepSim(3, 0)
    sim.set_drop_ping(True)
    assert sim.handle((1, 5, {}, True, 1), 0) == [] and sim.clock == {} and sim.queued(1) == []
    sim.set_drop_ping(False)
    assert sim.handle((1, 0, {}, True, 2), 0) == [] and sim.clock == {1: 0}
    with pytest.raises(ValueError):
        sim.handle((1, 0, {}, False, 3), 0)


def test_conditioned_histories_meet_the_conditions_the_gpu_tests_state():
    for n_dc, n_part in ((1, 1), (2, 2), (3, 1), (8, 2)):
        script, m = depcases.conditioned_history(n_dc, n_part, 120, [0, 1, 2, 63, 64, 65, 200])
        assert m.delivered * 10 >= m.nonping * 9
        assert m.first_try_failed() * 3 >= m.nonping if n_dc > 1 else m.first_try_failed() == 0
        assert sum(len(c[1]) for c in script if c[0] == "deliver") > 120
