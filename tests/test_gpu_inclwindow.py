"""The split fresh read's inclusion pass over the lag view loads lags only inside the commit-word
window (csrc/am_inclwin.h).  Every batch is read three ways -- through the lag view, through the
same device log with lag_ct nulled (the packed instantiation; every result column and the pairs
bit-equal) and by the C oracle -- on keys whose ops fall on every side of the rule: tiles the
commit word decides, tiles with window and decided ops, lags of exactly 0 and 65535, a negative
lag base, unsorted logs, escapes and routed keys.  The rule is replicated here on the host log
(with the bound that needs no lag load, the least the kernel knows), so a case that never
leaves the window fails instead of passing."""
import ctypes
import random

import numpy as np
import pytest
import torch

import bench
from antidote_amd import abi, synth
from antidote_amd.devbatch import DeviceReads, materialize
from antidote_amd.oplog import HostLog
from tests import fullpop, randlog
from tests.test_gpu_lagcadence import check_batch, check_stats, make_keys, span

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000
STEP = 1000                                   # us between ops: 65535 us of lag room is ~65 ops
LENS = [300, 65, 256, 257, 255, 513, 1024, 1100]  # every key past the lane tier; starts not 32-aligned
LATE = {0: 700}                               # key 0 starts 700 steps late: a prefix clock decides all of it
TILE, LAGMAX = 256, 0xFFFF


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


# ---------------------------------------------------------------- logs
def timeline(rng, n, n_dc, kind, start=0):
    """(commit_time, commit_dc, {dc: ct - snapshot entry}) of n ops in log order.  asc: one
    timeline, ascending.  shuffled: the same, in random log order.  inter: two DC timelines, the
    second 40 ms ahead, interleaved op by op (commit times go back and forth).  DC n_dc - 1 never
    commits on the key; its entries trail by 1 .. 65536 us with both ends present (lags 0 and
    65535 above the base); DC 0's entry of one op lies AHEAD of its commit time (a negative lag
    base); ops DC 0 commits have lag 0 there."""
    quiet = n_dc - 1 if n_dc > 1 else None
    committers = [d for d in range(n_dc) if d != quiet]
    out = []
    for i in range(n):
        if kind == "inter":
            dc = committers[i % 2 % len(committers)]
            ct = T0 + (start + (i // 2) * 2) * STEP + (i % 2) * 40_000 + rng.randrange(STEP)
        else:
            dc = rng.choice(committers)
            ct = T0 + (start + i) * STEP + rng.randrange(STEP)
        back = {d: rng.randint(1, 9000) for d in range(n_dc)}
        out.append((ct, dc, back))
    if n_dc > 1:
        i0, i1, i2 = rng.sample(range(n), 3)
        out[i0][2][quiet] = 1            # the base of the quiet DC ...
        out[i1][2][quiet] = 1 + LAGMAX   # ... and the largest lag that fits
        if out[i2][1] == 0 and len(committers) > 1:
            out[i2] = (out[i2][0], committers[1], out[i2][2])
        if out[i2][1] != 0:
            out[i2][2][0] = -500         # a remote entry ahead of the commit time
    if kind == "shuffled":
        rng.shuffle(out)
    return out


def make_log(rng, t, n_dc, kind):
    keys = []
    for ki, n in enumerate(LENS):
        ops = randlog.rand_key_ops(rng, t, n_dc, n)
        for op, (ct, dc, back) in zip(ops, timeline(rng, n, n_dc, kind, LATE.get(ki, 0))):
            op.commit_dc, op.commit_time = dc, ct
            op.snap = {d: ct - back[d] for d in range(n_dc)}
        keys.append(ops)
    return keys, HostLog(n_dc, keys, key_types=[t] * len(keys))


# ---------------------------------------------------------------- the rule, on the host log
def rule_classes(log, clock, pres=None):
    """Per key, per 256-op tile (32-aligned from the key's start, as the kernel cuts them, newest
    first): the ops the commit word decides as out / in, and the window ops, with cmax from the
    bound without loads only.  Returns [(n_out, n_in, n_window)] over every tile of every key."""
    nd, n = log.n_dc, log.n_ops
    ct = log.commit_time[:n].astype(np.int64)
    dc = (log.op_meta[:n] & 0x1F).astype(np.int64)
    X = log.snap_vc[:, :n].astype(np.int64).copy()
    X[dc, np.arange(n)] = ct
    ko = log.key_off.astype(np.int64)
    tiles = []
    for k in range(log.n_keys):
        a, b = int(ko[k]), int(ko[k + 1])
        lb = (ct[a:b][None, :] - X[:, a:b]).min(axis=1)      # key_lag (nothing escapes here)
        never = pres is not None and pres != (1 << nd) - 1
        cin = min(int(clock[d]) + int(lb[d]) for d in range(nd))
        hi = cin + LAGMAX
        if never:
            cin, hi = -1 - LAGMAX, -1
        cmax = None
        t0 = a & ~31
        for t in range(t0 + (b - 1 - t0) // TILE * TILE, t0 - 1, -TILE):
            c = ct[max(t, a):min(t + TILE, b)]
            sure = c[c <= cin]
            if len(sure):
                cmax = max(cmax if cmax is not None else -(1 << 62), int(sure.max()) - LAGMAX)
            lim = min(cin, cmax) if cmax is not None else -(1 << 62)
            n_out, n_in = int((c > hi).sum()), int((c <= lim).sum())
            tiles.append((n_out, n_in, len(c) - n_out - n_in))
    return tiles


# ---------------------------------------------------------------- three ways
def packed_only(dlog):
    """The same device log without its lag view: the packed instantiation streams it."""
    d2 = abi.am_op_log()
    ctypes.memmove(ctypes.byref(d2), ctypes.byref(dlog), ctypes.sizeof(abi.am_op_log))
    d2.lag_ct = None
    return d2


def read_columns(mat, dlog, n, n_dc, t, clock, pres, cap, types=None):
    dr = DeviceReads(n, n_dc, t, clock, pres=pres, set_cap=cap, types=types)
    torch.cuda.synchronize()
    materialize(mat, dlog, dr)
    mat.sync()
    h = dr.host()
    if dr.set_len is not None:
        sl = dr.set_len.cpu().numpy()
        so = dr.set_off.cpu().numpy()
        sa, sb = dr.set_a.cpu().numpy(), dr.set_b.cpu().numpy()
        keep = np.zeros(len(sa), bool)
        for i in range(n):
            if h["status"][i] == 0:
                keep[int(so[i]):int(so[i]) + int(sl[i])] = True
        h.update(set_len=sl, set_a=np.where(keep, sa, 0), set_b=np.where(keep, sb, 0))
    return dr, h


def same_columns(a, b, what):
    ok = a["status"] == 0
    assert np.array_equal(a["status"], b["status"]), what
    for col in a:
        if col in ("set_a", "set_b", "flags", "status"):
            assert np.array_equal(a[col], b[col]), (what, col)
        else:
            assert np.array_equal(a[col][..., ok], b[col][..., ok]), (what, col)


def three_ways(mat, dlog, log, keys, t, n_dc, clock, pres=None, cap=512):
    _, lagv = read_columns(mat, dlog, len(keys), n_dc, t, clock, pres, cap)
    _, pkv = read_columns(mat, packed_only(dlog), len(keys), n_dc, t, clock, pres, cap)
    same_columns(lagv, pkv, (clock, pres))
    check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=cap, pres=pres)


@pytest.mark.parametrize("kind", ["asc", "shuffled", "inter"])
@pytest.mark.parametrize("n_dc", [1, 3, 8])
@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_gpu_inclwindow_three_ways(mat, t, n_dc, kind):
    rng = random.Random(9100 + 100 * t + 10 * n_dc + len(kind))
    keys, log = make_log(rng, t, n_dc, kind)
    assert all(int(o) % 32 for o in log.key_off[1:-1])  # neighbouring keys share bitmap words
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        stats = st.view_stats()  # the lag view holds every key and every op
        assert stats["routed_keys"] == 0 and stats["lag_only_esc_ops"] == 0 and stats["pk_esc_ops"] == 0, stats
        dlog = st.device_log()
        assert dlog.lag_ct and not dlog.zone_vc
        lo, hi = span(keys)
        full = (1 << n_dc) - 1
        r = n_dc - 1
        probe = keys[-1][700]  # an op of the longest key: the clock at its entry on DC r and 1 us below
        entry = probe.commit_time if probe.commit_dc == r else probe.snap[r]
        mid = [T0 + 500 * STEP] * n_dc
        clocks = [([hi] * n_dc, None),                       # past every op
                  ([T0 - 10] * n_dc, None),                  # before every op: count 0
                  (mid, None),                               # a prefix
                  ([hi] * r + [entry], None), ([hi] * r + [entry - 1], None),
                  ([hi - 30_000] * n_dc, None)]              # nothing of the longest key is sure-out
        if n_dc > 1:
            clocks.append((mid, full & ~2))                  # a clock that lacks a DC: nothing passes
        seen = []
        for clock, pres in clocks:
            tiles = rule_classes(log, clock, pres)
            seen += tiles
            if clock is mid and pres is None:  # the prefix read alone meets every kind of tile and op
                assert any(w == 0 and o + i > 0 for o, i, w in tiles), "no tile the commit word decides"
                assert any(w > 0 and o + i > 0 for o, i, w in tiles), "no tile with window and decided ops"
                assert all(sum(x[j] for x in tiles) > 0 for j in range(3)), "a class is empty"
            three_ways(mat, dlog, log, keys, t, n_dc, clock, pres)
        assert all(sum(x[j] for x in seen) > 0 for j in range(3))
    finally:
        st.close()


def test_gpu_inclwindow_lag_only_escapes(mat):
    """Hand-made keys whose lag view holds clean ops beside lag-only escapes and ops escaped from
    the packed view (test_gpu_lagcadence's sparse regime: nothing routed)."""
    rng = random.Random(9300)
    t, n_dc = abi.AM_AWSET, 8
    keys, _ = make_keys(rng, t, n_dc, [300, 1024, 1500], "sparse")
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        check_stats(st, log, "sparse")
        stats = st.view_stats()
        assert stats["lag_only_esc_ops"] > 0 and stats["pk_esc_ops"] > 0 and stats["routed_keys"] == 0, stats
        dlog = st.device_log()
        lo, hi = span(keys)
        for clock in ([hi] * n_dc, [lo + (hi - lo) // 2] * n_dc, [lo - 5] * n_dc):
            three_ways(mat, dlog, log, keys, t, n_dc, clock)
    finally:
        st.close()


@pytest.mark.parametrize("esc,gst", [(3000, 0), (0, 250_000), (100_000, 250_000)])
def test_gpu_inclwindow_synthetic_escapes(mat, esc, gst):
    """A c3-shaped synthetic store (1000 us steps: most tiles are decided by the commit word) with
    escaped ops in and outside the window (esc_ppm) and routed keys next to lag keys (gst_ppm):
    full parity with the oracle, and the packed instantiation bit-equal."""
    cfg = dict(bench.CONFIGS["c3"])
    cfg["n_keys"] = 192
    p = bench.synth_params(cfg)
    p.gst_ppm, p.esc_ppm = gst, esc
    st = mat.synth_store(p)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        ko, kt = bench.key_columns(mat, dlog, cfg["n_keys"])
        lens = np.diff(ko.astype(np.int64))
        stats = st.view_stats()
        if esc:
            assert stats["pk_esc_ops"] > 0, stats
        if gst:
            assert 0 < stats["routed_keys"] < cfg["n_keys"], stats  # routed keys next to lag keys
        else:
            assert stats["routed_keys"] == 0, stats
        clock = synth.read_clock(p, bench.Q)
        n, nd, t, cap = cfg["n_keys"], cfg["n_dc"], cfg["type"], cfg["set_cap"]
        dr, lagv = read_columns(mat, dlog, n, nd, t, clock, None, cap)
        _, pkv = read_columns(mat, packed_only(dlog), n, nd, t, clock, None, cap)
        same_columns(lagv, pkv, (esc, gst))
        dev = fullpop.device_results(dr)
        dev["_key_type"] = kt
        n_reads, _, bad = fullpop.full_parity(p, clock, cap, dev, lens)
        assert n_reads == n and len(bad) == 0, (esc, gst, len(bad), bad[:8])
    finally:
        st.close()
