"""Reads under GST-cadence snapshot clocks: ops whose lags do not fit the lag view's 16 bits but
whose packed u32 entries do (lag-only escapes), and keys routed to the packed view because most of
their ops are such (include/antidote_mat.h, the lag view's reader contract).

1. Boundaries: hand-made logs near 1.7e15 us where one remote DC's lag above the key's minimum is
   65535 (fits), 65536, 65537, 2^20, 2^30 - 100 (lag-only escapes, inside the packed window of
   am_pk_base) or 2^31 (escaped from the packed view too: the escape row), read at clocks swept
   across each such entry at +-1, in three regimes (tight / sparse / heavy) whose view counters
   (am_store_view_stats) must equal the counts computed here in numpy from the definition.
2. Escaped ops read with a clock that lacks a DC, in every tier's escape walk.
3. Synthetic populations with gst_ppm (csrc/synth.h am_syn_snap_g): full parity over every key.
4. In place: am_store_apply carries the routing decision and frees slots as escaped.
Every result is compared with the oracle (oracle/am_oracle.c)."""
import random

import numpy as np
import pytest
import torch

import bench
from antidote_amd import abi, synth
from antidote_amd.devbatch import DeviceReads, materialize
from antidote_amd.oplog import HostBatch, HostLog, Read
from oracle import amo
from tests import fullpop, randlog

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000
BOUNDS = [65535, 65536, 65537, 1 << 20, (1 << 30) - 100]  # lag above the key's minimum; [0] still fits
FAR = 1 << 31                                                # outside the packed window
ESC = 0xFFFFFFFF


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


# ---------------------------------------------------------------- the view, from its definition
def view_counts(log: HostLog, lens=None):
    """am_store_view_stats from the definition, in numpy: the packed view's escapes (am_pk_base /
    am_pk_rel), the lag bases (minimum of ct - X[d] over the key's packed ops), the lag-only
    escapes (a lag more than 0xFFFF above its base, or a base outside (INT32_MIN, INT32_MAX]) and the routing
    (lag-only escapes above AM_LAG_ROUTE_NUM / AM_LAG_ROUTE_DEN = 1 / 8 of the packed ops).
    Returns (stats dict, routed[n_keys], lag_only[n_ops])."""
    nd, n = log.n_dc, log.n_ops
    ko = log.key_off.astype(np.int64)
    ct = log.commit_time[:n].astype(np.int64)
    dc = (log.op_meta[:n] & 0x1F).astype(np.int64)
    bad = (log.op_meta[:n] & 0x80) != 0
    X = log.snap_vc[:, :n].astype(np.int64).copy()
    X[dc, np.arange(n)] = ct
    routed = np.zeros(log.n_keys, bool)
    lag_only = np.zeros(n, bool)
    pk_esc = np.zeros(n, bool)
    for k in range(log.n_keys):
        a, b = int(ko[k]), int(ko[k + 1])
        if lens is not None:
            b = a + int(lens[k])
        if b <= a:
            continue
        lo, floor = int(ct[a]), max(int(ct[a]) - 0x7FFFFFFF, 0)
        for d in range(nd):
            if d != dc[a] and floor <= X[d, a] < lo:
                lo = int(X[d, a])
        base = lo - 0x40000000 if lo > 0x40000000 else 0
        rel = X[:, a:b] - base
        esc = ((rel < 0) | (rel >= ESC)).any(axis=0) | bad[a:b]
        pk_esc[a:b] = esc
        if esc.all():
            continue
        lag = ct[a:b][None, :] - X[:, a:b]
        lb = lag[:, ~esc].min(axis=1)
        fit = bool(((lb > -(1 << 31)) & (lb < (1 << 31))).all())  # (INT32_MIN is the routing mark)
        over = ((lag - lb[:, None] > 0xFFFF) | (lag - lb[:, None] < 0)).any(axis=0) | (not fit)
        lag_only[a:b] = over & ~esc
        npk, nlo = int((~esc).sum()), int((over & ~esc).sum())
        routed[k] = (not fit) or nlo * 8 > npk
    klen = np.diff(ko) if lens is None else np.asarray(lens, np.int64)
    stats = {"ops": int(klen.sum()), "pk_esc_ops": int(pk_esc.sum()), "lag_only_esc_ops": int(lag_only.sum()),
             "routed_keys": int(routed.sum()), "routed_ops": int(klen[routed].sum())}
    return stats, routed, lag_only


# ---------------------------------------------------------------- hand-made logs
def make_keys(rng, t, n_dc, lens, regime, n_first=None):
    """Keys of the given lengths near T0 and the boundaries (value, key, dc, entry) to sweep read
    clocks across.  tight: lags of 1..12 us.  heavy: every remote entry lags 0.1-1.2 s in steps of
    0.1 s (every key is routed).  sparse and heavy: a key of >= 12 ops gets one FAR entry, one
    65535 entry and lag-only escapes of the other BOUNDS values on distinct ops -- in sparse as many
    as stay under 1/8 of its packed ops ((n - 2) // 8, the values rotating with the key's index so
    that the short keys share them out), so nothing is routed; keys of >= 300 ops get n // 50 more
    (about 2% of the ops over all).  Keys past the first n_first (repeated lengths) take boundaries
    only where they are short (<= 16 ops)."""
    keys, sweeps = [], []
    n_first = len(lens) if n_first is None else n_first
    for ki, n in enumerate(lens):
        ops = randlog.rand_key_ops(rng, t, n_dc, n, t0=T0 + rng.randint(0, 100))
        if regime == "heavy":
            for i, op in enumerate(ops):
                for d in range(n_dc):
                    if d != op.commit_dc:
                        op.snap[d] = op.commit_time - (100_000 + ((i * 7 + d) % 12) * 100_000 + d)
        if regime != "tight" and n_dc > 1 and n >= 12 and (ki < n_first or n <= 16):
            room = min(len(BOUNDS) - 1, (n - 2) // 8 if regime == "sparse" else len(BOUNDS) - 1)
            vals = [FAR, BOUNDS[0]] + [BOUNDS[1 + (ki + j) % (len(BOUNDS) - 1)] for j in range(room)]
            extra = n // 50 if n >= 300 else 0
            picks = rng.sample(range(n), len(vals) + extra)
            for j, i in enumerate(picks):
                op = ops[i]
                r = (op.commit_dc + 1 + rng.randrange(n_dc - 1)) % n_dc
                kmin = min(0 if o.commit_dc == r else o.commit_time - o.snap[r] for o in ops)
                val = vals[j] if j < len(vals) else rng.choice(BOUNDS[1:])
                op.snap[r] = op.commit_time - (kmin + val)
                if j < len(vals):
                    sweeps.append((val, ki, r, op.snap[r]))
        keys.append(ops)
    return keys, sweeps


def check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=512, sel=None, pres=None):
    """One batch-clock read of the keys `sel` (every key when None) against the oracle.  pres: the
    mask of the DCs the clock holds (every DC when None)."""
    sel = list(range(len(keys))) if sel is None else list(sel)
    n = len(sel)
    kt = torch.tensor(sel, dtype=torch.int64, device="cuda")
    dr = DeviceReads(n, n_dc, t, clock, pres=pres, set_cap=cap, keys=kt)
    torch.cuda.synchronize()
    materialize(mat, dlog, dr)
    mat.sync()
    h = dr.host()
    reads = [Read(k, t, {d: clock[d] for d in range(n_dc) if pres is None or (pres >> d) & 1}) for k in sel]
    ref = amo.materialize(log, HostBatch(n_dc, reads, randlog.caps_for(reads, n_dc, cap)))
    ok = [i for i in range(n) if ref.result(i)[0] == "ok"]
    vals = dr.values(np.asarray(ok, np.int64)) if ok else []
    for i in range(n):
        r = ref.result(i)
        if r[0] != "ok":
            assert int(h["status"][i]) == r[1], (sel[i], int(h["status"][i]), r)
            continue
        assert int(h["status"][i]) == 0, (sel[i], int(h["status"][i]), r)
        ct = None if h["last_ct_ignore"][i] else {d: int(h["last_ct"][d, i]) for d in range(n_dc)
                                                  if (int(h["last_ct_pres"][i]) >> d) & 1}
        got = ("ok", vals[ok.index(i)], int(h["new_last_op"][i]), ct, bool(h["is_new_ss"][i]), int(h["count"][i]),
               int(h["flags"][i]))
        assert got == r, (sel[i], len(keys[sel[i]]), clock, got, r)


def span(keys):
    return (min(op.commit_time for ops in keys for op in ops), max(op.commit_time for ops in keys for op in ops) + 10)


def at_entry(hi, n_dc, r, x):
    """The clock with DC r at x and every other DC past the newest op: the entries of DC r alone
    decide the ops."""
    c = [hi] * n_dc
    c[r] = x
    return c


def check_stats(st, log, regime):
    want, routed, lag_only = view_counts(log)
    got = st.view_stats()
    assert got == want, (regime, got, want)
    if regime == "tight":
        assert got["lag_only_esc_ops"] == 0 and got["routed_keys"] == 0
    elif regime == "sparse":
        assert got["routed_keys"] == 0 and got["pk_esc_ops"] > 0
        assert 0.005 < got["lag_only_esc_ops"] / got["ops"] < 0.04, got
    else:
        assert got["routed_keys"] == log.n_keys and got["routed_ops"] == got["ops"], got
        assert got["lag_only_esc_ops"] > got["ops"] // 2
    return routed


CASES = [(abi.AM_AWSET, 8, [3, 12, 16, 40, 64, 65, 300, 1024, 1500, 5000, 9000], True),
         (abi.AM_MVREG, 8, [3, 12, 16, 40, 64, 65, 300, 1024, 1500, 5000, 9000], True),
         (abi.AM_BCOUNTER, 16, [3, 40, 64, 70, 300, 2500, 4096, 5000], False),
         (abi.AM_PN, 3, [3, 16, 20, 64, 300], False),
         (abi.AM_LWW, 3, [3, 16, 20, 64, 300], False)]


@pytest.mark.parametrize("regime", ["tight", "sparse", "heavy"])
@pytest.mark.parametrize("t,n_dc,lens,incremental", CASES)
def test_gpu_lag_boundaries(mat, t, n_dc, lens, incremental, regime):
    rng = random.Random(7100 + 10 * t + len(regime))
    keys, sweeps = make_keys(rng, t, n_dc, lens + lens[:4], regime, n_first=len(lens))
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        check_stats(st, log, regime)
        dlog = st.device_log()
        lo, hi = span(keys)
        quantiles = [[lo + (hi - lo) * 3 // 4] * n_dc, [lo + (hi - lo) // 2] * n_dc, [hi] * n_dc]
        for clock in quantiles:
            check_batch(mat, dlog, log, keys, t, n_dc, clock)
        # every recorded boundary entry e, at e - 1, e, e + 1: its own key read alone (the tier of
        # that key's length), and for each value the last such entry also with every key in the batch
        last = {val: (ki, r, e) for val, ki, r, e in sweeps}
        for val, ki, r, e in sweeps:
            for x in (e - 1, e, e + 1):
                check_batch(mat, dlog, log, keys, t, n_dc, at_entry(hi, n_dc, r, x), sel=[ki])
                if last[val] == (ki, r, e):
                    check_batch(mat, dlog, log, keys, t, n_dc, at_entry(hi, n_dc, r, x))
        if incremental:
            # per-read clocks (the general kernels): a read below the 0.75 quantile, then reads
            # against that result as their base -- at every quantile clock, and for every boundary
            # value at e - 1, e, e + 1 with each key at its own entry of that value (a key without
            # one reads past every op)
            n = len(keys)
            caps = [512] * n
            c0 = {d: quantiles[0][d] - (quantiles[0][d] - T0) // 2 for d in range(n_dc)}
            r0 = [Read(k, t, c0) for k in range(n)]
            h0 = mat.read_batch(st, r0, caps)
            ref0 = amo.materialize(log, HostBatch(n_dc, r0, caps))
            for i in range(n):
                assert h0.result(i) == ref0.result(i), (i, h0.result(i), ref0.result(i))
            rounds = [[q] * n for q in quantiles]
            for val in BOUNDS + [FAR]:
                own = {ki: (r, e) for v, ki, r, e in sweeps if v == val}
                if own:
                    rounds += [[at_entry(hi, n_dc, own[k][0], own[k][1] + dx) if k in own else [hi] * n_dc
                                for k in range(n)] for dx in (-1, 0, 1)]
            for clocks in rounds:
                r1 = []
                for k in range(n):
                    _, val, nlo, ct, _, _, _ = ref0.result(k)
                    r1.append(Read(k, t, {d: clocks[k][d] for d in range(n_dc)}, None, ct, nlo, val))
                h1 = mat.read_batch(st, r1, caps)
                ref1 = amo.materialize(log, HostBatch(n_dc, r1, caps))
                for i in range(n):
                    assert h1.result(i) == ref1.result(i), (i, len(keys[i]), clocks[i], h1.result(i), ref1.result(i))
    finally:
        st.close()


# ---------------------------------------------------------------- escaped ops, a DC missing
# lengths of CASES that reach each type's row, wave, workgroup and big tiers
MISSING_DC = [(abi.AM_BCOUNTER, 16, [40, 300, 5000]),
              (abi.AM_AWSET, 8, [40, 300, 1500, 9000]),
              (abi.AM_PN, 3, [16, 64, 300])]


@pytest.mark.parametrize("every", [False, True], ids=["sparse", "all_escaped"])
@pytest.mark.parametrize("t,n_dc,lens", MISSING_DC)
def test_gpu_escape_missing_dc(mat, t, n_dc, lens, every):
    """Escaped ops read with a clock that lacks a DC ("Could not find DC in SS": the op is excluded
    and AM_FLAG_MISSING_DC_LOGGED set).  sparse: make_keys' sparse regime, a few lag-only escapes
    and one FAR escape per key, nothing routed.  all_escaped: every op has one remote entry FAR
    below its commit time, so every op is outside the packed view and the escape reader alone
    decides each read.  Every key is read at a clock past its newest op with every DC present and
    with DC 0, DC n_dc - 1 and a middle DC absent."""
    rng = random.Random(7400 + 10 * t + every)
    keys, _ = make_keys(rng, t, n_dc, lens, "tight" if every else "sparse")
    if every:
        for ops in keys:
            for op in ops:
                op.snap[(op.commit_dc + 1) % n_dc] = op.commit_time - FAR
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        stats = st.view_stats()
        assert stats == view_counts(log)[0], stats
        if every:
            assert stats["pk_esc_ops"] == stats["ops"] == sum(lens), stats
        else:
            assert stats["routed_keys"] == 0 and stats["pk_esc_ops"] > 0 and stats["lag_only_esc_ops"] > 0, stats
        dlog = st.device_log()
        _, hi = span(keys)
        full = (1 << n_dc) - 1
        for pres in [None] + [full & ~(1 << d) for d in (0, n_dc - 1, n_dc // 2)]:
            check_batch(mat, dlog, log, keys, t, n_dc, [hi] * n_dc, pres=pres)
    finally:
        st.close()


# ---------------------------------------------------------------- synthetic populations
def _shape(name):
    cfg = dict(bench.CONFIGS[name])
    if name == "c3":
        cfg["n_keys"] = 2048
    elif name == "c4":
        cfg["n_keys"] = 65536
    else:
        cfg["n_keys"], cfg["total_ops"], cfg["hot_cap"] = 16384, 64 * 16384, 8192
    return cfg


@pytest.mark.parametrize("esc", [0, 100000])
@pytest.mark.parametrize("gst", [1_000_000, 250_000])
@pytest.mark.parametrize("name", ["c3", "c4", "c5"])
def test_gpu_gst_population_parity(mat, name, gst, esc):
    cfg = _shape(name)
    p = bench.synth_params(cfg)
    p.gst_ppm, p.esc_ppm = gst, esc
    st = mat.synth_store(p)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        ko, kt = bench.key_columns(mat, dlog, cfg["n_keys"])
        lens = np.diff(ko.astype(np.int64))
        stats = st.view_stats()
        multi = int((lens > 1).sum())
        assert stats["ops"] == int(lens.sum())
        assert stats["routed_keys"] > 0, stats
        if gst == 1_000_000:
            assert stats["routed_keys"] >= multi * 9 // 10, (stats, multi)
        else:
            assert stats["routed_keys"] < multi * 4 // 10, (stats, multi)  # unrouted keys present
            assert 0.15 < stats["routed_ops"] / stats["ops"] < 0.35, stats
        if esc:
            assert stats["pk_esc_ops"] > 0
        clock = synth.read_clock(p, bench.Q)
        th = cfg["type"] if cfg["type"] in range(1, 6) else 0
        types = torch.from_numpy(kt.copy()).cuda() if not th else None
        cap = max(cfg["set_cap"], 1)
        dr = DeviceReads(cfg["n_keys"], cfg["n_dc"], th, clock, set_cap=cap, types=types)
        torch.cuda.synchronize()
        materialize(mat, dlog, dr)
        mat.sync()
        dev = fullpop.device_results(dr)
        dev["_key_type"] = kt
        n_reads, n_ops, bad = fullpop.full_parity(p, clock, cap, dev, lens)
        assert n_reads == cfg["n_keys"] and len(bad) == 0, (name, gst, esc, len(bad), bad[:8])
    finally:
        st.close()


# ---------------------------------------------------------------- in place
class _DownLog:
    """A downloaded device log (Store.download: dense CSR, explicit op ids) as a host log the C
    oracle and view_counts read."""

    def __init__(self, D, n_dc):
        self.D, self.n_dc = D, n_dc
        self.snap_vc = np.ascontiguousarray(D["snap_vc"], np.uint64)
        self.key_off, self.commit_time, self.op_meta = D["key_off"], D["commit_time"], D["op_meta"]
        self.n_keys = len(D["key_off"]) - 1
        self.n_ops = int(D["key_off"][-1])

    def as_struct(self):
        D = self.D
        s = abi.am_op_log()
        s.n_dc, s.n_keys, s.n_ops = self.n_dc, self.n_keys, self.n_ops
        s.n_var = len(D["var_data"]) if D["var_off"] is not None else 0
        s.snap_stride = self.snap_vc.shape[1]
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        s.key_off, s.key_type, s.key_flags = p(D["key_off"]), p(D["key_type"]), p(D["key_flags"])
        s.op_meta, s.commit_time, s.snap_vc, s.snap_pres = (p(D["op_meta"]), p(D["commit_time"]), p(self.snap_vc),
                                                            p(D["snap_pres"]))
        s.op_txid, s.op_id, s.p0, s.p1 = p(D["op_txid"]), p(D["op_id"]), p(D["p0"]), p(D["p1"])
        s.var_off = p(D["var_off"]) if D["var_off"] is not None and s.n_var else None
        s.var_data = p(D["var_data"]) if D["var_off"] is not None and s.n_var else None
        self._s = s
        return s


def _download_u64(mat, ptr, n):
    a = np.zeros(n, np.uint64)
    abi.check(mat.L.am_memcpy_d2h(mat.ctx, a.ctypes.data, ptr, n * 8), "d2h")
    return a


def _download_u32(mat, ptr, n):
    a = np.zeros(n, np.uint32)
    abi.check(mat.L.am_memcpy_d2h(mat.ctx, a.ctypes.data, ptr, n * 4), "d2h")
    return a


def test_gpu_apply_carries_routing(mat):
    """am_store_apply on a reserved c3-shaped store of 512 keys: GST-lagged ops appended to tight
    keys (they become routed where they exceed an eighth), tight ops appended to routed keys (they
    stay routed), one routed key pruned to empty and one tight key pruned to its newer half; reads
    match the oracle on the merged log, the counters match the numpy count, and the slots the two
    pruned keys freed read AM_PK_ESC in lag_ct -- the tight key's held commit entries before."""
    rng = random.Random(7300)
    t, n_dc, n_keys = abi.AM_AWSET, 8, 512
    lens = [rng.choice([3, 16, 40, 70, 130]) for _ in range(n_keys)]

    def stepped(ops, i0, i1):  # make_keys' heavy regime on ops [i0, i1)
        for i in range(i0, i1):
            op = ops[i]
            for d in range(n_dc):
                if d != op.commit_dc:
                    op.snap[d] = op.commit_time - (100_000 + ((i * 7 + d) % 12) * 100_000 + d)

    # each key's whole history in one piece (one causal token history): its first lens[k] ops
    # are the store's, its last 3 the ops appended below -- lagged where the key is tight
    # (k < 256) and tight where it is lagged
    hist = [randlog.rand_key_ops(rng, t, n_dc, lens[k] + 3, t0=T0 + rng.randint(0, 100)) for k in range(n_keys)]
    for k in range(n_keys):
        stepped(hist[k], *((lens[k], lens[k] + 3) if k < 256 else (0, lens[k])))
        for j, op in enumerate(hist[k][lens[k]:]):  # appended ops: one add of a new token each, so
            op.effect = [(j, [5000 + j], [])]       # the key's record room (2 per free slot) holds them
    keys = [hist[k][:lens[k]] for k in range(n_keys)]
    base = mat.store(HostLog(n_dc, keys, key_types=[t] * n_keys))
    st = base.reserve()
    try:
        log0 = HostLog(n_dc, keys, key_types=[t] * n_keys)
        assert st.view_stats() == view_counts(log0)[0]
        touched = sorted(rng.sample(range(0, 256), 24) + rng.sample(range(256, 512), 24))
        gone = touched[-1]  # a routed key, pruned to empty
        # a tight key (every lag_ct a commit entry), pruned to its newer half: no appends
        shrunk = next(k for k in range(256) if k not in touched and lens[k] >= 40)
        touched = sorted(touched + [shrunk])
        cut = lens[shrunk] // 2  # ops [0, cut] go: X <= the threshold on every DC (snapshot entries < ct)
        new_ops = [[] if k in (gone, shrunk) else hist[k][lens[k]:] for k in touched]
        mask = np.zeros(n_keys, np.uint8)
        thr_vc = np.zeros((n_dc, n_keys), np.uint64)
        thr_pres = np.zeros(n_keys, np.uint32)
        mask[gone] = 1
        thr_vc[:, gone] = max(o.commit_time for o in keys[gone]) + 10
        thr_pres[gone] = (1 << n_dc) - 1
        mask[shrunk] = 1
        thr_vc[:, shrunk] = keys[shrunk][cut].commit_time
        thr_pres[shrunk] = (1 << n_dc) - 1
        d0 = st.device_log()
        stride = int(d0.snap_stride) or int(d0.n_ops)
        lag_before = _download_u32(mat, d0.lag_ct, stride)
        ko0 = _download_u64(mat, d0.key_off, n_keys + 1).astype(np.int64)  # slot offsets (room included)
        ok, _ = st.apply(touched, new_log=HostLog(n_dc, new_ops, key_types=[t] * len(touched)),
                         prune=(mask, thr_vc, thr_pres))
        assert ok
        merged = [list(keys[k]) for k in range(n_keys)]
        for k, ops in zip(touched, new_ops):
            merged[k] = merged[k] + ops
        merged[gone] = []
        merged[shrunk] = keys[shrunk][cut + 1:]
        D = st.download()  # the store's own log (dense CSR, its op ids): what the oracle reads
        assert [int(x) for x in np.diff(D["key_off"].astype(np.int64))] == [len(m) for m in merged]
        assert [int(x) for x in D["commit_time"]] == [op.commit_time for ops in merged for op in ops]
        mlog = _DownLog(D, n_dc)
        want, routed, _ = view_counts(mlog)
        assert st.view_stats() == want, (st.view_stats(), want)
        # routed keys stay routed under tight appends; a tight key turns routed when the lagged
        # appends exceed an eighth of it (3 of 6, 3 of 19) and stays unrouted otherwise (3 of 43)
        assert all(routed[k] for k in touched if k >= 256 and k != gone) and not routed[gone]
        assert not routed[shrunk]
        assert routed[256:].sum() == 255 and not routed[[k for k in range(256) if k not in touched]].any()
        was_tight = [k for k in touched if k < 256 and k != shrunk]
        assert any(routed[k] for k in was_tight) and not all(routed[k] for k in was_tight)
        dlog = st.device_log()
        hi = max(op.commit_time for ops in merged for op in ops) + 10
        for clock in ([hi] * n_dc, [T0 + 60] * n_dc):
            check_batch(mat, dlog, mlog, merged, t, n_dc, clock)
        # the slots the pruned keys freed: the routed key's, and the tight key's, whose slots
        # held commit entries before and whose survivors (moved to the front) still do
        lag_ct = _download_u32(mat, dlog.lag_ct, stride)
        a, b = int(ko0[gone]), int(ko0[gone]) + len(keys[gone])
        assert b > a and (lag_ct[a:b] == ESC).all()
        a, b = int(ko0[shrunk]), int(ko0[shrunk]) + lens[shrunk]
        left = len(merged[shrunk])
        assert 0 < left < lens[shrunk] and (lag_before[a:b] != ESC).all()
        assert (lag_ct[a:a + left] != ESC).all() and (lag_ct[a + left:b] == ESC).all()
    finally:
        st.close()
        base.close()
