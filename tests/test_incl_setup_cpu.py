"""The inputs of tests/test_gpu_incl_setup.py, checked without a GPU: the hand-made logs
(tests/incl_setup_cases.py) do put the reads where the lane-parallel set-up of the inclusion pass can
go wrong.  By the rule replicated on the host log (test_gpu_incl_compact.segment_lists) every case has
reads with a non-empty window list, reads that take a second round and reads whose bound a sure-in op
raised before the rounds; neighbouring keys differ in time base and in every lag base; and the oracle
gives the sparse batch its error statuses and the escape batch its 64-bit maxima."""
import numpy as np
import pytest

from antidote_amd import abi
from oracle import amo
from antidote_amd.oplog import HostBatch, Read
from tests import randlog
from tests.incl_setup_cases import LATE, PLAIN, case, coverage, host_view, key_bases
from tests.test_gpu_lagcadence import view_counts

PARAMS = [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3), (abi.AM_MVREG, 3), (abi.AM_AWSET, 5), (abi.AM_MVREG, 5)]


def oracle(log, keys, t, n_dc, clock, pres=None, cap=512):
    reads = [Read(k, t, {d: clock[d] for d in range(n_dc) if pres is None or (pres >> d) & 1}) for k in range(len(keys))]
    return amo.materialize(log, HostBatch(n_dc, reads, randlog.caps_for(reads, n_dc, cap)))


@pytest.mark.parametrize("t,n_dc", PARAMS)
def test_mixed_batch_inputs(t, n_dc):
    keys, log, clocks = case("mixed", t, n_dc)
    assert 40 <= len(keys) <= 70 and all(int(o) % 32 for o in log.key_off[1:-1])
    ks = key_bases(log)
    _, lbs, _ = host_view(log)
    for k in range(1, len(keys)):  # a slot that leaks into its neighbour holds other values throughout
        assert ks[k] != ks[k - 1]
        assert all(int(lbs[k][d]) != int(lbs[k - 1][d]) for d in range(n_dc) if lbs[k][d] or lbs[k - 1][d])
    assert sum(1 for lb in lbs if (lb < 0).any()) >= len(keys) // 2 and any((lb > 0).any() for lb in lbs)
    st, routed, lag_only = view_counts(log)
    assert st["routed_keys"] == 0 and st["lag_only_esc_ops"] == 0 and st["pk_esc_ops"] == 0, st
    cov = coverage(log, clocks)
    assert min(cov["listed"], cov["second_round"], cov["sure_raised"]) >= 1, cov
    # the clocks lie in the middle of keys: reads neither empty nor whole, many per clock
    for clock, pres in clocks[:3]:
        ref = oracle(log, keys, t, n_dc, clock, pres)
        part = sum(1 for i in range(len(keys)) if 0 < ref.result(i)[5] < len(keys[i]))
        assert part >= 8, (clock, part)


def test_edge_clock_inputs():
    t, n_dc = abi.AM_AWSET, 8
    keys, log, clocks = case("edges", t, n_dc)
    ks = key_bases(log)
    below = sum(1 for k in ks if clocks[0][0][0] < k)
    assert 0 < below < len(keys)  # the clock lies below some keys' K only
    counts = []
    for clock, pres in clocks:
        ref = oracle(log, keys, t, n_dc, clock, pres)
        assert all(ref.result(i)[0] == "ok" for i in range(len(keys)))
        counts.append([ref.result(i)[5] for i in range(len(keys))])
        if pres is not None:  # a missing DC: the flag on every read with candidate ops, nothing included
            assert all(ref.result(i)[6] == abi.AM_FLAG_MISSING_DC_LOGGED for i in range(len(keys)))
    assert not any(counts[0]) and not any(counts[1]) and not any(counts[2]) and not any(counts[4])
    assert counts[3] == [len(k) for k in keys]


@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_sparse_batch_inputs(t):
    n_dc = 8
    keys, log, clocks = case("sparse", t, n_dc)
    assert len(keys) == 69 and len(keys) % 32 == 5
    lens = [len(k) for k in keys]
    assert all(64 < lens[i] <= 8192 for i in (0, 31, 32))
    assert min(lens) <= 20 and max(lens) > 8192
    st, routed, _ = view_counts(log)
    assert st["routed_keys"] == 2 and routed[10] and routed[46] and not routed[[0, 31, 32]].any(), st
    ref = oracle(log, keys, t, n_dc, *clocks[0])
    bad = [i for i in range(len(keys)) if ref.result(i)[0] != "ok"]
    # the reads of the keys of another type; the keys over the op limit may run out of result room
    assert {14, 66} <= set(bad) <= {6, 14, 38, 66}, bad
    assert all(ref.result(i)[1] == abi.AM_ERR_CORRUPTED_OPS_CACHE for i in (14, 66))
    for b in (range(0, 32), range(32, 64), range(64, 69)):  # every batch: eligible slots apart from each other
        assert sum(1 for i in b if i in PLAIN["sparse"]) >= 3 and any(i not in PLAIN["sparse"] for i in b)
    cov = coverage(log, clocks, PLAIN["sparse"])
    assert min(cov["listed"], cov["second_round"], cov["sure_raised"]) >= 1, cov


def test_segment_inputs():
    t, n_dc = abi.AM_AWSET, 8
    keys, log, clocks = case("segments", t, n_dc)
    assert len(keys[0]) == 1025 and int(log.key_off[0]) == 0 and len(keys[5]) == 2300
    assert sum(1 for k in keys if len(k) == 40) >= 10
    a, b = int(log.key_off[5]), int(log.key_off[6])
    assert (b - 1 - (a & ~31)) // 1024 == 2  # three segments
    cov = coverage(log, clocks, [0, 5])
    assert min(cov.values()) >= 1, cov  # with a bound carried into an older segment that has window ops


@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 3)])
def test_escape_inputs(t, n_dc):
    keys, log, clocks = case("escapes", t, n_dc)
    st, routed, lag_only = view_counts(log)
    assert st["routed_keys"] == 0 and st["lag_only_esc_ops"] == 1 and st["pk_esc_ops"] == 3, st
    ks = key_bases(log)
    ref = oracle(log, keys, t, n_dc, *clocks[0])
    for k in (7, 31):  # the escaped newest op is included and holds every DC's maximum, 2^32 and more above K
        r = ref.result(k)
        assert r[0] == "ok" and r[5] == len(keys[k])
        assert all(v - ks[k] >= 1 << 32 for v in r[3].values()) and keys[k][-1].commit_time - keys[k][0].commit_time == LATE
        inview = max(op.commit_time for op in keys[k][:-1])
        assert all(v > inview for v in r[3].values())
    assert ref.result(3)[5] == len(keys[3]) and ref.result(11)[5] == len(keys[11])  # the planted escapes are included
    ref = oracle(log, keys, t, n_dc, *clocks[1])
    assert 0 < ref.result(7)[5] < len(keys[7])  # and excluded beside included in-view ops
    cov = coverage(log, clocks, PLAIN["escapes"])
    assert min(cov["listed"], cov["second_round"], cov["sure_raised"]) >= 1, cov
    assert np.count_nonzero(lag_only) == 1
