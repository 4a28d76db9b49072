"""The split fresh read (csrc/am_group_split.h: k_grp_incl, then k_grp_spans or k_grp_recs) on a
store ingested in place.  Every other test of that path reads a store mat.store(log) has just
built: a dense CSR, every view written by one build pass.  A vnode's store has room behind every
key (am_store_reserve) and am_store_apply rewrites the touched keys in place (csrc/am_apply.hip
k_writeback): the lag view under new lag bases, the routing mark, the records, groups and spans,
key_end inside the key's slots, AM_PK_ESC on the slots a shrunk key frees, the explicit op id
column.  Here such a store (no zone index, so launch_d takes launch_split) is read in three
states -- reserved, after a round of appends, after a round of prunes with some appends; the model
of tests/splitapply.py says what each round does and what each state must hold:

  key  reserved -> after round A -> after round B (positions from t0 = slot offset & ~31)
  a    1000 -> 1024 exactly -> 1025: one segment, full to the op, then two
  b    250 -> 257: a tile edge inside a segment
  c    2040 -> 2049 -> 2054: the bitmap past 64 words
  d    1100 -> pruned below 1024: two segments -> one, freed slots in the old second segment
  e    600 -> its newer third: survivors moved to the front, stale commit words behind key_end
  f    quiet-DC lags 1 and 1 + 65535; round A appends lag 0: every lag re-encoded, one lag-only escape
  g    a lag-only escape 65536 above a base one old op sets; round B prunes that op: back in the view
  h    300 tight ops + 48 lag-only escapes: unrouted -> routed, among clean reads (second wave batch)
  i    400 ops, 60 lag-only escapes in the first 150; round B prunes those: routed -> unrouted
  j    round A writes a lag-only and a packed escape into one lane's four slots, among window ops
  k    shuffled; round B keeps non-consecutive ops: the store gains the explicit op id column
  l    pruned to empty in round B, read beside live reads
  m    MV only, 1020 -> 1030 ops: past AM_BIG_MIN_OPS, wave tier -> big tier in place
  n    untouched, at batch slots 0, 31 and 32 and behind d and e: t0 windows over a neighbour's room
  o    4200 ops + 20: the walk path past 16 tiles
  (D = 1 has no escapes and no routing: rows f - j are fillers there and the counts must be zero.)

Per state: the store's downloaded log equals the model's merged ops and op ids (and the oracle
reads the downloaded log, not the model); the view statistics equal the definition's
(test_gpu_lagcadence.view_counts) with the flips above; lag_ct is AM_PK_ESC on every slot behind a
key's end up to its capacity, on every op of a routed key and on the escaped ops only elsewhere;
about a dozen batch clocks -- steered so that key a's list holds 0, 1, 63, 64, 65 and 129 entries,
below and above every op, two quantiles, inside every key, one lacking a DC -- are read three ways
(test_gpu_inclwindow.three_ways: lag view, packed instantiation, C oracle; every column and the
pairs bit-equal) with no read out of capacity; the coverage conditions of splitapply.check_state
hold on the downloaded log.  The last state is also read from a fresh mat.store of the merged ops
with the same op ids: every column equal."""
import numpy as np
import pytest

from antidote_amd import abi
from tests import splitapply as sa
from tests.test_gpu_inclwindow import read_columns, same_columns, three_ways
from tests.test_gpu_lagcadence import _download_u32, _download_u64, view_counts
from tests.test_gpu_zones import _DownLog

pytestmark = pytest.mark.gpu

CAP = 512  # pairs per read: above every key's value (the 48 elements key h gains are the most)


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


class DownLog(_DownLog):
    """The downloaded log, also as view_counts and segment_lists read a host log."""

    def __init__(self, D, n_dc):
        super().__init__(D, n_dc)
        self.key_off, self.commit_time, self.op_meta = D["key_off"], D["commit_time"], D["op_meta"]


def check_applied(m, s, D):
    """The store's log is the model's: lengths, commit vectors, metas, op ids."""
    want = m.host_log(s)
    n = want.n_ops
    assert [int(x) for x in np.diff(D["key_off"].astype(np.int64))] == m.lens(s)
    assert np.array_equal(D["commit_time"], want.commit_time[:n])
    assert np.array_equal(D["op_meta"], want.op_meta[:n])
    assert np.array_equal(D["snap_vc"], want.snap_vc[:, :n])
    assert [int(x) for x in D["op_id"]] == [i for ids in m.states[s][1] for i in ids]


def check_lag_ct(m, s, mat, dlog, log):
    """lag_ct over the store's slots: escaped behind every key's end up to its capacity (free and
    freed slots alike), on every op of a routed key, and on the escaped ops only of every other."""
    stride = int(dlog.snap_stride) or int(dlog.n_ops)
    lag_ct = _download_u32(mat, dlog.lag_ct, stride)
    _, routed, lag_only = view_counts(log)
    so, ko, lens = m.slot_off, np.asarray(log.key_off).astype(np.int64), m.lens(s)
    assert stride >= int(so[-1])
    freed = 0
    for k in range(sa.N_KEYS):
        a, e, b = int(so[k]), int(so[k]) + lens[k], int(so[k + 1])
        assert (lag_ct[e:b] == abi.AM_PK_ESC).all(), (s, k, m.lay[k][0])
        freed += max(m.lens(s - 1)[k] - lens[k], 0) if s else 0
        esc = lag_only[ko[k]:ko[k + 1]].copy()
        if m.lay[k][0] == "j" and s >= 1:
            esc[m.j_quad + 2] = True  # escaped from the packed view too
        assert np.array_equal(lag_ct[a:e] == abi.AM_PK_ESC, esc | bool(routed[k])), (s, k, m.lay[k][0])
    assert (freed > 500) == (s == 2)  # round B frees slots that held commit words


@pytest.mark.parametrize("t,n_dc", sa.CASES)  # D = 5: no template width, the runtime-width instantiation
def test_gpu_split_after_apply(mat, t, n_dc):
    m = sa.model(t, n_dc)
    base = mat.store(m.host_log(0))
    st = base.reserve()
    base.close()
    fresh = None
    try:
        st.index(abi.AM_INDEX_NONE)
        cols = {}
        for s in range(3):
            if s:
                touched, new_log, prune = m.apply_args(s)
                applied, _ = st.apply(touched, new_log=new_log, prune=prune)
                assert applied, (s, "a rebuild fallback would hide the path under test")
            dlog = st.device_log()
            assert dlog.lag_ct and not dlog.zone_vc  # launch_d takes launch_split
            # the room rule, restated on the host (am_gc.hip slack_cap): the slots never move
            ko = _download_u64(mat, dlog.key_off, sa.N_KEYS + 1).astype(np.int64)
            assert np.array_equal(ko, m.slot_off), (s, ko, m.slot_off)
            D = st.download()
            assert D["explicit_op_id"] == (s == 2), s
            check_applied(m, s, D)
            log = DownLog(D, n_dc)
            clocks, want = sa.check_state(m, s, log)
            assert st.view_stats() == want, (s, st.view_stats(), want)
            check_lag_ct(m, s, mat, dlog, log)
            keys = m.states[s][0]
            for clock, pres, kind in clocks:
                three_ways(mat, dlog, log, keys, t, n_dc, clock, pres, cap=CAP)
                _, h = read_columns(mat, dlog, sa.N_KEYS, n_dc, t, clock, pres, CAP)
                assert (h["status"] == 0).all(), (s, kind, h["status"])
                cols[s, tuple(clock), pres] = h
        # the last state from a store just built of the merged ops (their op ids kept)
        fresh = mat.store(m.host_log(2, ids=True))
        fresh.index(abi.AM_INDEX_NONE)
        flog = fresh.device_log()
        assert flog.lag_ct and not flog.zone_vc and not flog.key_end
        assert fresh.view_stats() == want
        for clock, pres, kind in clocks:
            _, h = read_columns(mat, flog, sa.N_KEYS, n_dc, t, clock, pres, CAP)
            same_columns(cols[2, tuple(clock), pres], h, ("fresh store", kind, clock, pres))
    finally:
        st.close()
        if fresh is not None:
            fresh.close()
