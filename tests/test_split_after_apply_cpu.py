"""The host model of tests/test_gpu_split_after_apply.py (tests/splitapply.py) reaches its cases
without a GPU: per (type, D) the three states' merged logs over the slot offsets of the room rule,
with every key where the table puts it, the view statistics, routing flips and lag-only counts by
view_counts' definition, and the inclusion pass's list sizes and edges by the host rule over the
store's slots (segment_lists with slot offsets) -- every size, a whole segment, lists across a
tile and a segment edge, inside one quad, and after the prunes a window op in the last 32 slots
before a freed region.  The GPU module asserts the same on the log the store gives back, so the
two cannot drift apart."""
import numpy as np
import pytest

from antidote_amd import abi
from tests import splitapply as sa
from tests.test_gpu_incl_compact import segment_lists


@pytest.mark.parametrize("t,n_dc", sa.CASES)
def test_split_after_apply_model_reaches_the_cases(t, n_dc):
    m = sa.model(t, n_dc)
    assert len(m.states) == 3 and len(m.lay) == sa.N_KEYS
    # the room rule, restated: a quarter of the ops, four at least; offsets are running sums
    lens0 = m.lens(0)
    assert sa.cap_of(70) == 87 and sa.cap_of(3) == 7 and sa.cap_of(1000) == 1250
    assert [int(x) for x in np.diff(m.slot_off)] == [n + max(n // 4, 4) for n in lens0] and m.slot_off[0] == 0
    for s in range(3):
        log = m.host_log(s)
        clocks, stats = sa.check_state(m, s, log)
        assert 11 <= len(clocks) <= 14
        assert stats["ops"] == sum(m.lens(s))
        ids = m.states[s][1]
        assert all(len(i) == n and all(b > a for a, b in zip(i, i[1:])) for i, n in zip(ids, m.lens(s)))
    # every round is an apply of touched keys that fit; round A prunes nothing, round B does
    (ta, na, pa), (tb, nb, pb) = m.rounds
    assert not pa and pb and all(len(x) for x in na) and any(len(x) == 0 for x in nb) and any(len(x) for x in nb)
    assert set(m.idx["n"]).isdisjoint(ta) and set(m.idx["n"]).isdisjoint(tb)
    touched = set(ta) | set(tb)
    fillers = set(m.idx[None])
    assert fillers & touched and fillers - touched  # some fillers touched, some not
    if n_dc > 1:  # the escaped quad of key j: ops appended in round A, in one lane's four slots
        j, q = m.key["j"], m.j_quad
        assert q >= lens0[j] and (int(m.slot_off[j]) + q) % 4 == 0


def test_split_after_apply_slot_offsets_shift_the_segments():
    """segment_lists cuts a key's segments from its first slot in the store: with slot offsets the
    same ops give the lists of the dense log moved by the key's shift inside its 32-slot group,
    and without them nothing changes."""
    m = sa.model(abi.AM_AWSET, 3)
    log, k = m.host_log(0), m.key["c"]
    clock = [sa.T0 + 55_000] * 3
    dense = segment_lists(log, k, clock)
    assert [list(w) for w in segment_lists(log, k, clock, None, None)] == [list(w) for w in dense]
    assert [list(w) for w in segment_lists(log, k, clock, None, log.key_off)] == [list(w) for w in dense]
    moved = segment_lists(log, k, clock, None, m.slot_off)

    def at(segs, first):  # the listed ops as indices within the key (segments come newest first)
        t0 = int(first) // 32 * 32
        return sorted(t0 + (len(segs) - 1 - j) * sa.SEG + int(x) - int(first) for j, w in enumerate(segs) for x in w)
    assert at(dense, log.key_off[k]) == at(moved, m.slot_off[k])  # the same ops of the key
    assert int(log.key_off[k]) % 32 != int(m.slot_off[k]) % 32 and len(at(dense, log.key_off[k])) > sa.SEG
