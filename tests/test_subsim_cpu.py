"""tests/subsim.py, the contract of the subscriber buffer, against the hand cases' literal outputs (worked
from src/inter_dc_sub_buf.erl by hand), and the generators of tests/subcases.py against the conditions
the device tests state on their inputs."""
import random

import pytest

from tests import subcases
from tests.subcases import Model
from tests.subsim import BUFFERING, NORMAL, RESP_END, RESP_TXN, TXN, SubSim

CASES = subcases.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_literal_outputs(case):
    _, n_dc, logging, steps, dropped, unexpected = case
    m = Model(n_dc, 1, logging)
    for i, s in enumerate(steps):
        if s[0] != "row":
            subcases.serve(m, [s])
            continue
        _, row, tags, gap, (dc, last, mode, queue) = s
        got, gaps, cnt = m.process([row])
        assert got == [tags], (i, got)
        assert gaps == ([gap] if gap else []), (i, gaps)
        assert m.stream(0, dc) == (last, mode, queue), (i, m.stream(0, dc))
        assert cnt["delivered"] == len(tags) and cnt["gaps"] == len(gaps) and cnt["queued"] == m.sim.queued()
    assert (m.sim.dropped, m.sim.unexpected) == (dropped, unexpected)


def test_the_hand_cases_cover_the_issue_list():
    names = {c[0] for c in CASES}
    assert len(names) == len(CASES) >= 15
    assert any(not c[2] for c in CASES) and any(s[0] == "set_last" for c in CASES for s in c[3])
    assert any(s[0] == "set_reachable" for c in CASES for s in c[3])


def test_a_ping_ignores_its_last_opid_column():
    for garbage in (0, 1, 999, subcases.U64_MAX):
        s = SubSim(1, 1)
        s.handle(subcases.t(0, 4, 1, dc=0))
        assert [r[8] for r in s.handle(subcases.ping(4, 2, dc=0, garbage=garbage))[0]] == [2]
        assert s.stream(0, 0) == (4, NORMAL, [])


def test_invalid_rows_are_refused_and_an_invalid_batch_changes_nothing():
    m = Model(2, 2)
    m.process([subcases.t(0, 2, 1), subcases.t(5, 6, 2)])
    before = m.state()
    for bad in ((TXN, 2, 0, 0, 1, 1, {}, False, 9), (TXN, 0, 2, 0, 1, 1, {}, False, 9), (3, 0, 0, 0, 1, 1, {}, False, 9),
                (TXN, 0, 0, 0, 1, 0, {}, False, 9), (RESP_TXN, 0, 0, 0, 1, 0, {}, False, 9)):
        with pytest.raises(ValueError):
            m.process([subcases.t(2, 3, 8), bad])
        assert m.state() == before
    m.process([(RESP_END, 0, 0, 0, 0, 0, {}, False, 0), subcases.ping(0, 3, dc=0)])  # timestamp 0 is legal on these
    assert m.process([]) == ([[], []], [], dict(zip(subcases.COUNTS, (0, 0, 0, 0, 1))))


def test_clear_and_set_last():
    m = Model(2, 1)
    m.process([subcases.t(0, 2, 1), subcases.t(5, 6, 2)])
    assert m.stream(0, 1) == (2, BUFFERING, [2])
    m.clear()
    assert m.state() == {} and m.size() == (0,)
    m.set_last(0, 1, 5)
    assert m.process([subcases.t(5, 6, 2)])[0] == [[2]]


SHAPES = [(1, 1, 600), (1, 3, 600), (2, 8, 3000), (65, 3, 3000), (65, 32, 3000), (1, 32, 600), (2, 1, 3000), (2, 3, 3000),
          (65, 1, 3000), (2, 32, 3000)]


@pytest.mark.parametrize("n_part,n_dc,length", SHAPES)
def test_lossy_histories_meet_the_conditions_of_the_device_tests(n_part, n_dc, length):
    for seed in range(3):
        rows, sim, sent = subcases.lossy_history(random.Random(seed), n_dc, n_part, length)
        m = Model(n_dc, n_part)
        gaps = sum(len(m.process([r])[1]) for r in rows)
        assert m.state() == subcases.state_of(sim, n_dc, n_part)
        assert len(rows) >= length
        assert gaps * 100 >= len(rows), (gaps, len(rows))
        assert sim.dropped * 100 >= len(rows), (sim.dropped, len(rows))
        assert sim.released >= gaps
        assert sim.delivered * 10 >= sent * 9, (sim.delivered, sent)
        # responses answer real gaps with the sender's transactions of the range
        kinds = [r[0] for r in rows]
        assert kinds.count(RESP_END) == gaps and kinds.count(RESP_TXN) >= gaps
        assert sim.unexpected == 0 and all(s.mode == NORMAL for s in sim.streams.values())


def test_tile_history_shapes():
    for n in (63, 64, 65, 129):
        rows, e = subcases.tile_history(n)
        m = Model(2, 1)
        out, gaps, cnt = m.process(rows)
        assert out == [[1]] and gaps == [(0, 1, 2, 5)] and cnt["queued"] == n + 1
        out, gaps, cnt = m.process([e])
        assert out == [[2] + [100 + i for i in range(n)]] and not gaps and cnt["queued"] == 0
        for at in sorted({0, 62, 63, 64, n - 1} & set(range(n))):
            rows, e = subcases.tile_history(n, dup_at=at)
            m = Model(2, 1)
            m.process(rows)
            out, gaps, cnt = m.process([e])
            assert out == [[2] + [100 + i for i in range(n) if i != at]] and cnt["dropped"] == 1 and not gaps
            rows, e = subcases.tile_history(n, hole_at=at)
            m = Model(2, 1)
            m.process(rows)
            out, gaps, cnt = m.process([e])
            assert out == [[2] + [100 + i for i in range(at)]] and len(gaps) == 1 and cnt["queued"] == n - at
            assert m.stream(0, 1)[1] == BUFFERING


def test_history_text_round_trip_shape():
    script = [("set_last", 0, 1, 7), ("process", [subcases.t(7, 8, 1, snap={0: 3})]), ("set_reachable", [1]), ("clear",)]
    text = subcases.history_text(script, 2, 1)
    assert text.splitlines() == ["C 2 1 1", "L 0 1 7", "P 1 0 0 1 7 8 5 0 1 3 0", "R 2", "Z", "X"]
