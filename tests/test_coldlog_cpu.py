"""CPU checks of the device log's boundary and of the cold-path restatement the GPU tests compare
with: include/antidote_mat.h declares the am_plog calls and the library exports them, the ABI
version is still 15, the calls reject missing arguments before touching a device, and
tests/coldlog.py (logging_vnode:get_up_to_time/5 restated) gives, on hand-written logs of 2-4
transactions, the results the reference's rules give when worked out by hand."""
import ctypes

import pytest

from antidote_amd import abi
from oracle import ref_materializer as R
from tests import coldlog
from tests.test_abi import HDR, declared_functions

PL_FNS = ["am_plog_create", "am_plog_destroy", "am_plog_append_host", "am_plog_size", "am_plog_key_ops", "am_plog_read",
          "am_plog_read_host"]
CASES = coldlog.hand_cases()


def test_header_declares_and_library_exports_the_log_calls():
    fns = declared_functions()
    L = abi.lib()
    names = {n for n, _, _ in abi.SIGNATURES}
    for fn in PL_FNS:
        assert fn in fns, fn
        assert fn in names, fn
        assert hasattr(L, fn), fn
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_log_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    cm, b, r = abi.am_commits(), abi.am_read_batch(), abi.am_read_result()
    assert L.am_plog_create(None, 2, 4, 8, 8, ctypes.byref(out)) == abi.AM_ERR_INVALID
    assert L.am_plog_create(None, 2, 4, 8, 8, None) == abi.AM_ERR_INVALID
    assert L.am_plog_destroy(None) == abi.AM_OK
    assert L.am_plog_append_host(None, ctypes.byref(cm)) == abi.AM_ERR_INVALID
    assert L.am_plog_size(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == abi.AM_ERR_INVALID
    assert L.am_plog_key_ops(None, 0, 0, 0, None, ctypes.byref(n)) == abi.AM_ERR_INVALID
    assert L.am_plog_read(None, None, ctypes.byref(b), None, ctypes.byref(r)) == abi.AM_ERR_INVALID
    assert L.am_plog_read_host(None, None, ctypes.byref(b), None, ctypes.byref(r)) == abi.AM_ERR_INVALID


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_helper_gives_the_hand_worked_results(case):
    _, _, log, reads, expect = case
    assert len(reads) == len(expect)
    for (key, type_, clock, txid, horizon), want in zip(reads, expect):
        assert coldlog.cold_result(log, key, type_, clock, txid, horizon) == want, (key, clock, horizon)


def test_helper_response_shape_and_ids():
    """The response of the `filtered` case: ids 0, 1 over the two survivors, newest first, the base
    new() with last_op_id 0 under the clock {} (a clock, not ignore), never the newest snapshot."""
    _, _, log, reads, _ = CASES[0]
    key, type_, clock, _, _ = reads[0]
    resp = coldlog.get_up_to_time(log, key, type_, clock)
    assert [i for i, _ in resp.ops_list] == [1, 0] and resp.number_of_ops == 2
    assert [p.op_param for _, p in resp.ops_list] == [4, 1]
    assert [p.commit_time for _, p in resp.ops_list] == [(1, 12), (0, 10)]
    assert resp.snapshot_time == {} and resp.snapshot_time != R.IGNORE and resp.is_newest_snapshot is False
    assert (resp.materialized_snapshot.last_op_id, resp.materialized_snapshot.value) == (0, R.crdt_new(type_))
    assert coldlog.get_up_to_time(log, key, type_, clock, horizon=1).number_of_ops == 1


def run_history_on_oracle(monkeypatch, seed, n_dc):
    lv = coldlog.LoggedVnode().use(monkeypatch)
    _, steps = coldlog.history(seed, n_dc)
    for step in steps:
        if step[0] == "commit":
            for tx in step[1]:
                lv.commit(tx)
        else:
            for (k, t, clock), sg in zip(step[1], step[2]):
                lv.read(k, t, clock, sg)
        lv.mark_dead(coldlog.N_KEYS)
    return lv


def test_generator_of_the_gpu_vnode_test_meets_its_conditions(monkeypatch):
    """The random histories of tests/test_gpu_coldvnode.py against the helper alone: no oracle
    exception, and the conditions that test asserts -- per seed at least 8 reader cold reads, at
    least 1 cold GC read from a commit and at most a quarter of the keys left out; over the seeds at
    least 2 cold reads with ShouldGC -- so nothing there passes vacuously."""
    should_gc = 0
    for seed, n_dc in coldlog.HISTORY_SEEDS:
        lv = run_history_on_oracle(monkeypatch, seed, n_dc)
        print(seed, n_dc, "cold reads", lv.cold_reads, "with ShouldGC", lv.cold_should_gc, "cold GC reads",
              lv.cold_gc_reads, "left out", sorted(lv.dead), "log", len(lv.log))
        assert lv.cold_reads >= coldlog.MIN_COLD_READS, (seed, lv.cold_reads)
        assert lv.cold_gc_reads >= coldlog.MIN_COLD_GC_READS, (seed, lv.cold_gc_reads)
        assert len(lv.dead) <= coldlog.N_KEYS // 4, (seed, lv.dead)
        should_gc += lv.cold_should_gc
    assert should_gc >= coldlog.MIN_COLD_SHOULD_GC


def test_logged_vnode_reads_the_log_where_the_oracle_raises(monkeypatch):
    """A cached snapshot above the read clock: the oracle raises LogColdPath, the logged vnode
    returns the value from the log; materialize_snapshot stores it iff ShouldGC."""
    PN = abi.AM_PN
    lv = coldlog.LoggedVnode().use(monkeypatch)
    for i in range(8):
        lv.commit((0, 100 + 10 * i, {0: 95 + 10 * i}, None, [(3, PN, 1)]))
    # three GC reads: the dict keeps its SNAPSHOT_MIN newest entries, the initial {} leaves
    for at, want in ((135, 4), (155, 6), (175, 8)):
        assert lv.internal_read(3, PN, {0: at}, R.IGNORE, True) == ("ok", want)
    assert [c for c, _ in lv.st.snapshot_cache[3][0]] == [{0: 170}, {0: 150}, {0: 130}]
    assert lv.cold_reads == 0
    plain = R.VnodeState()
    plain.ops_cache, plain.snapshot_cache = lv.st.ops_cache, lv.st.snapshot_cache
    monkeypatch.undo()
    with pytest.raises(R.LogColdPath):
        R.internal_read(3, PN, {0: 125}, R.IGNORE, False, plain)
    lv.use(monkeypatch)
    assert lv.internal_read(3, PN, {0: 125}, R.IGNORE, False) == ("ok", 3)
    assert (lv.cold_reads, lv.cold_should_gc) == (1, 0)
    assert [c for c, _ in lv.st.snapshot_cache[3][0]] == [{0: 170}, {0: 150}, {0: 130}]
    # with ShouldGC the cold snapshot goes through internal_store_ss: insert_bigger refuses a clock
    # below the newest entry, snapshot_insert_gc runs all the same
    assert lv.internal_read(3, PN, {0: 125}, R.IGNORE, True) == ("ok", 3)
    assert (lv.cold_reads, lv.cold_should_gc) == (2, 1)
    assert [c for c, _ in lv.st.snapshot_cache[3][0]] == [{0: 170}, {0: 150}, {0: 130}]
