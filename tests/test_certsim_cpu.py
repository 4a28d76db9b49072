"""tests/certsim.py, the sequential checker of write-write certification, against the reference's own outcomes
(tests/golden/suite_certification.json, transcribed from test/multidc/clocksi_SUITE.erl) and the
rules of src/clocksi_vnode.erl:450-632 case by case."""
import json
import os

import pytest

from tests import certsim
from tests.certsim import NO_UPDATES, OK, WRITE_CONFLICT, CertSim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "suite_certification.json")
CASES = json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_certsim_replays_the_reference_suites(case):
    assert case["source"].startswith("test/multidc/clocksi_SUITE.erl:")
    sim = CertSim(case["record_commits"])
    assert certsim.replay(case, sim.prepare, sim.finish, sim.read_ready) == []
    assert sim.min_prepared() is None  # every suite ends with nothing in flight


def test_golden_suite_holds_the_five_histories():
    assert [c["name"] for c in CASES] == ["clocksi_certification_test", "clocksi_cert_property_test",
                                          "clocksi_multiple_certification_test", "clocksi_prepare_test",
                                          "clocksi_read_time_test"]


def test_last_commit_wins_with_decreasing_commit_times():
    sim = CertSim()
    assert sim.prepare([(1, 10, 50, False, [4]), (2, 10, 51, False, [4])]) == [OK, OK]  # stacked, not certified
    assert sim.finish([(1, 90, True, [4]), (2, 70, True, [4])]) == [OK, OK]
    assert sim.key_info(4) == (70, [])  # ets:insert overwrites: not the maximum
    assert sim.prepare([(3, 80, 100, True, [4])]) == [OK]  # 70 > 80 is false
    assert sim.prepare([(4, 60, 101, True, [5, 4])]) == [WRITE_CONFLICT]


def test_abort_of_a_transaction_that_holds_nothing():
    sim = CertSim()
    assert sim.finish([(9, 0, False, [1, 2])]) == [OK]
    assert sim.key_info(1) == (0, []) and sim.key_info(2) == (0, []) and sim.min_prepared() is None


def test_abort_leaves_another_owners_entry():
    sim = CertSim()
    assert sim.prepare([(1, 10, 20, True, [7, 8]), (2, 11, 21, True, [8, 9])]) == [OK, WRITE_CONFLICT]
    assert sim.finish([(2, 0, False, [8, 9])]) == [OK]  # case 3 of :533-555: M's record stays
    assert sim.key_info(8) == (0, [(1, 20)]) and sim.key_info(9) == (0, [])
    assert sim.min_prepared() == 20
    assert sim.finish([(1, 30, True, [7, 8])]) == [OK]
    assert sim.key_info(8) == (30, []) and sim.min_prepared() is None


def test_empty_write_set_with_and_without_certify():
    sim = CertSim()
    assert sim.prepare([(1, 10, 20, True, []), (2, 10, 21, False, [])]) == [NO_UPDATES, NO_UPDATES]
    assert sim.finish([(1, 30, True, []), (2, 0, False, [])]) == [NO_UPDATES, NO_UPDATES]
    assert sim.prepared == {} and sim.committed == {}


def test_record_commits_off_never_touches_the_commit_table():
    sim = CertSim(record_commits=False)
    assert sim.prepare([(1, 10, 20, True, [3])]) == [OK]
    assert sim.finish([(1, 99, True, [3])]) == [OK]
    assert sim.key_info(3) == (0, [])
    assert sim.prepare([(2, 5, 30, True, [3])]) == [OK]  # no commit time to lose against


def test_repeated_key_enters_once_and_list_order_is_the_references():
    sim = CertSim()
    assert sim.prepare([(1, 10, 20, False, [3, 3, 4, 3]), (2, 10, 25, False, [3])]) == [OK, OK]
    assert sim.key_list(3) == [(2, 25), (1, 20)]  # set_prepared prepends
    assert sim.key_info(3) == (0, [(1, 20), (2, 25)]) and sim.key_info(4) == (0, [(1, 20)])
    assert sim.read_ready([(3, 19), (3, 20), (3, 24), (4, 30), (5, 30), (3, 2001)], 1000) == [0, 10, 10, 10, 0, 2]
