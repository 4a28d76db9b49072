"""The per-key lag width: a store's private column (am_store_lag_width) and the commit-word window
the inclusion pass of the split fresh read sizes by it (csrc/am_inclwin.h, csrc/am_group_split.h
k_grp_incl<.., LAG = true>).

1. The column from its definition: read back and compared with numpy over the host log
   (tests/lagwidth_cases.definition) on tests/randlog logs, the hand-made cases and small synthetic
   stores; routed keys, keys with lag-only escapes, empty keys; no column without a lag view (D = 17).
2. Reads three ways: the store's own log (the widths are used), the same log with its key_lag row
   copied into a fresh allocation (the reader does not know the widths: the 16-bit window) and the C
   oracle; every result column equal.  tests/test_lagwidth_cpu.py asserts on the host what the cases'
   reads meet.
3. am_store_apply keeps the column current: a wider op raises a key's width, an op that makes the key
   routed, a GC prune that removes the widest op.
4. Two stores in one context, one destroyed."""
import ctypes
import random

import numpy as np
import pytest

from antidote_amd import abi, synth
from antidote_amd.oplog import HostLog
from tests import randlog
from tests.lagwidth_cases import T0, WMAX, case, definition, key_ops
from tests.test_gpu_inclwindow import read_columns, same_columns
from tests.test_gpu_lagcadence import _DownLog, check_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


class CopiedKeyLag:
    """The device log with its key_lag row copied into a fresh am_dev_alloc block: the same view, but
    not the store's columns, so a reader takes the format's 16 bits for every key."""

    def __init__(self, mat, dlog):
        self.mat = mat
        nbytes = max(int(dlog.n_keys) * int(dlog.n_dc) * 4, 4)
        host = np.zeros(nbytes, np.uint8)
        abi.check(mat.L.am_memcpy_d2h(mat.ctx, host.ctypes.data, dlog.key_lag, nbytes), "d2h")
        self.p = ctypes.c_void_p()
        abi.check(mat.L.am_dev_alloc(mat.ctx, nbytes, ctypes.byref(self.p)), "am_dev_alloc")
        abi.check(mat.L.am_memcpy_h2d(mat.ctx, self.p, host.ctypes.data, nbytes), "h2d")
        self.log = abi.am_op_log()
        ctypes.memmove(ctypes.byref(self.log), ctypes.byref(dlog), ctypes.sizeof(abi.am_op_log))
        self.log.key_lag = self.p.value  # (a c_void_p field: an int, or None)
        assert self.log.key_lag and self.log.key_lag != dlog.key_lag

    def free(self):
        if self.p:
            self.mat.L.am_dev_free(self.mat.ctx, self.p)
            self.p = ctypes.c_void_p()


def three_ways(mat, dlog, log, keys, t, n_dc, clock, cap=512, copied=None):
    own = copied is None
    cp = CopiedKeyLag(mat, dlog) if own else copied
    try:
        _, a = read_columns(mat, dlog, len(keys), n_dc, t, clock, None, cap)
        _, b = read_columns(mat, cp.log, len(keys), n_dc, t, clock, None, cap)
        same_columns(a, b, clock)
        check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=cap)
    finally:
        if own:
            cp.free()


def check_column(st, log, lens=None):
    v = definition(log, lens)
    got = st.lag_width()
    assert np.array_equal(got.astype(np.int64), v["width"]), (np.nonzero(got != v["width"])[0][:8], got[:8], v["width"][:8])
    return v


# ---------------------------------------------------------------- 1. the column
@pytest.mark.parametrize("n_dc", [1, 3, 8])
@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG, abi.AM_PN])
def test_gpu_lagwidth_column_random_logs(mat, t, n_dc):
    rng = random.Random(10_200 + 10 * t + n_dc)
    keys = [randlog.rand_key_ops(rng, t, n_dc, rng.choice([0, 1, 5, 64, 65, 300])) for _ in range(64)]
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        v = check_column(st, log)
        assert (v["width"][[len(k) == 0 for k in keys]] == WMAX).all() and (v["width"] <= 12).sum() >= 32
    finally:
        st.close()


@pytest.mark.parametrize("name,t,n_dc", [("batch", abi.AM_AWSET, 8), ("batch", abi.AM_MVREG, 3), ("lists", abi.AM_AWSET, 8),
                                         ("sparse", abi.AM_MVREG, 8), ("segments", abi.AM_AWSET, 8)])
def test_gpu_lagwidth_column_cases(mat, name, t, n_dc):
    keys, log, clocks, v = case(name, t, n_dc)
    st = mat.store(log)
    try:
        check_column(st, log)
        assert st.view_stats()["routed_keys"] == int(v["routed"].sum())
    finally:
        st.close()


@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_gpu_lagwidth_column_synthetic(mat, t):
    """Small synthetic stores (am_synth_store, the benchmark's generator): the column against the
    definition over the generator's host log, plain and with GST-cadence snapshots (routed keys)."""
    for gst in (0, 250_000):
        p = synth.params(256, 8, t, ops_per_key=300)
        p.gst_ppm = gst
        st = mat.synth_store(p)
        try:
            v = check_column(st, synth.host_log(p, 0, 256))
            assert (int(v["routed"].sum()) > 0) == (gst > 0)
            assert (v["width"] < WMAX).sum() >= 64
        finally:
            st.close()


def test_gpu_lagwidth_no_lag_view(mat):
    rng = random.Random(10_217)
    keys = [randlog.rand_key_ops(rng, abi.AM_AWSET, 17, 70) for _ in range(8)]
    st = mat.store(HostLog(17, keys, key_types=[abi.AM_AWSET] * 8))
    try:
        assert not st.device_log().lag_ct
        out = np.zeros(8, np.uint16)
        assert mat.L.am_store_lag_width(mat.ctx, st.handle, out.ctypes.data) == abi.AM_ERR_INVALID
        with pytest.raises(abi.AmError):
            st.lag_width()
    finally:
        st.close()


# ---------------------------------------------------------------- 2. reads three ways
def run_case(mat, name, t, n_dc):
    keys, log, clocks, v = case(name, t, n_dc)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        check_column(st, log)
        dlog = st.device_log()
        assert dlog.lag_ct and not dlog.zone_vc
        cp = CopiedKeyLag(mat, dlog)
        try:
            for clock in clocks:
                three_ways(mat, dlog, log, keys, t, n_dc, clock, copied=cp)
        finally:
            cp.free()
    finally:
        st.close()


# n_dc 5: the runtime-width instantiation of D = 8 (pad DCs)
@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3), (abi.AM_MVREG, 5)])
def test_gpu_lagwidth_batch(mat, t, n_dc):
    run_case(mat, "batch", t, n_dc)


@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3)])
def test_gpu_lagwidth_lists(mat, t, n_dc):
    run_case(mat, "lists", t, n_dc)


def test_gpu_lagwidth_segments(mat):
    run_case(mat, "segments", abi.AM_AWSET, 8)


@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_gpu_lagwidth_sparse(mat, t):
    run_case(mat, "sparse", t, 8)


# ---------------------------------------------------------------- 3. apply
def test_gpu_lagwidth_apply(mat):
    """A reserved store of 96 narrow keys (width 100), then three am_store_apply rounds: ops whose
    lag exceeds the key's width (it rises to 5000), ops that make a key routed (0xFFFF), and a GC
    prune that removes a key's widest op (its width falls).  After each round the column equals the
    definition over the downloaded log, and the reads are equal three ways."""
    rng = random.Random(10_250)
    t, n_dc, n_keys = abi.AM_AWSET, 8, 96
    lens = [rng.choice([70, 97, 131]) for _ in range(n_keys)]
    hist = [key_ops(rng, t, n_dc, lens[k] + 3, T0 + 503 * k, 300, 100, k) for k in range(n_keys)]
    for k in range(n_keys):
        for j, op in enumerate(hist[k][lens[k]:]):  # appended ops: one add of a new token each
            op.effect = [(j, [5000 + j], [])]
    wide, routed, pruned = [3, 40, 41], [7, 60], [11, 70]
    for k in wide:  # the appended ops trail by up to 5000 us on a DC the key does not commit at
        d = (k + 1) % n_dc
        base = min(o.commit_time - o.snap[d] for o in hist[k][:lens[k]])
        hist[k][lens[k] + 1].snap[d] = hist[k][lens[k] + 1].commit_time - (base + 5000)
    for k in routed:  # lag-only escapes on more than an eighth of the merged key
        d = (k + 1) % n_dc
        base = min(o.commit_time - o.snap[d] for o in hist[k][:lens[k]])
        lens[k] = 13
        for op in hist[k][13:16]:
            op.snap[d] = op.commit_time - (base + 70_000)
    for k in pruned:  # the key's widest op is its oldest: 8000 above the base
        d = (k + 1) % n_dc
        base = min(o.commit_time - o.snap[d] for o in hist[k][1:lens[k]])
        hist[k][0].snap[d] = hist[k][0].commit_time - (base + 8000)
    keys = [hist[k][:lens[k]] for k in range(n_keys)]
    log0 = HostLog(n_dc, keys, key_types=[t] * n_keys)
    base_st = mat.store(log0)
    st = base_st.reserve()
    try:
        v0 = check_column(st, log0)
        # (a key's first ops need not hold the op that attains its width of 100)
        assert all(v0["width"][k] <= 100 for k in wide + routed) and all(v0["width"][k] == 8000 for k in pruned)
        merged = [list(k) for k in keys]
        hi = max(op.commit_time for ops in hist for op in ops) + 10

        def after(what):
            D = st.download()
            assert [int(x) for x in np.diff(D["key_off"].astype(np.int64))] == [len(m) for m in merged]
            mlog = _DownLog(D, n_dc)
            v = check_column(st, mlog)
            dlog = st.device_log()
            for clock in ([hi] * n_dc, [T0 + 24_000] * n_dc, [T0 + 40_000] * n_dc):
                three_ways(mat, dlog, mlog, merged, t, n_dc, clock)
            return v

        # round 1: wider ops; round 2: the ops that route a key
        for touched, want in ((wide, (5000, 5100)), (routed, (WMAX, WMAX))):  # (the appended ops may lower the base)
            new_ops = [hist[k][lens[k]:lens[k] + 3] for k in touched]
            ok, _ = st.apply(touched, new_log=HostLog(n_dc, new_ops, key_types=[t] * len(touched)))
            assert ok
            for k, ops in zip(touched, new_ops):
                merged[k] = merged[k] + ops
            v = after(touched)
            assert all(want[0] <= v["width"][k] <= want[1] for k in touched), (touched, v["width"][touched])
            assert all(bool(v["routed"][k]) == (want[0] == WMAX) for k in touched)
        # round 3: a prune of the oldest ops of two keys, their widest among them
        mask = np.zeros(n_keys, np.uint8)
        thr_vc = np.zeros((n_dc, n_keys), np.uint64)
        thr_pres = np.zeros(n_keys, np.uint32)
        for k in pruned:
            mask[k] = 1
            for d in range(n_dc):  # ops 0 .. 4 lie under the threshold on every DC (entries may run ahead of
                # the commit times); op 5 lies above it at the committing DC
                thr_vc[d, k] = max(op.commit_time if op.commit_dc == d else op.snap[d] for op in keys[k][:5])
            assert keys[k][5].commit_time > thr_vc[keys[k][5].commit_dc, k]
            thr_pres[k] = (1 << n_dc) - 1
        ok, _ = st.apply(pruned, new_log=HostLog(n_dc, [[] for _ in pruned], key_types=[t] * len(pruned)),
                         prune=(mask, thr_vc, thr_pres))
        assert ok
        for k in pruned:
            merged[k] = keys[k][5:]
        v = after(pruned)
        assert all(v["width"][k] <= 100 for k in pruned), v["width"][pruned]
    finally:
        st.close()
        base_st.close()


# ---------------------------------------------------------------- 4. two stores, one destroyed
def test_gpu_lagwidth_two_stores(mat):
    t, n_dc = abi.AM_AWSET, 8
    keys1, log1, clocks1, _ = case("batch", t, n_dc)
    keys2, log2, clocks2, _ = case("lists", t, n_dc)
    st1, st2 = mat.store(log1), mat.store(log2)
    try:
        st1.index(abi.AM_INDEX_NONE)
        st2.index(abi.AM_INDEX_NONE)
        check_column(st1, log1)
        check_column(st2, log2)
        three_ways(mat, st1.device_log(), log1, keys1, t, n_dc, clocks1[1])
        three_ways(mat, st2.device_log(), log2, keys2, t, n_dc, clocks2[2])
        cp = CopiedKeyLag(mat, st2.device_log())
        st1.close()  # its blocks go back to the context's allocator; the survivor keeps its own widths
        try:
            check_column(st2, log2)
            for clock in clocks2[:4]:
                three_ways(mat, st2.device_log(), log2, keys2, t, n_dc, clock, copied=cp)
            # a third store takes the freed blocks: the survivor and the copied log still read the same
            st3 = mat.store(log1)
            try:
                st3.index(abi.AM_INDEX_NONE)
                check_column(st3, log1)
                three_ways(mat, st3.device_log(), log1, keys1, t, n_dc, clocks1[0])
                three_ways(mat, st2.device_log(), log2, keys2, t, n_dc, clocks2[0], copied=cp)
            finally:
                st3.close()
        finally:
            cp.free()
    finally:
        st1.close()
        st2.close()
