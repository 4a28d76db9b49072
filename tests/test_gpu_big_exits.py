"""The big-read tier's overflow exits (am_big.hip) and the exact 128-bit sums at the int64 edges,
on the hand-made logs of tests/bigexits.py (their shape is proven without a GPU by
tests/test_bigexits_cpu.py).  Every output column is compared bit for bit with oracle/am_oracle.c,
after the oracle alone has answered ok -- or the error the key is built for -- at the same capacity.

Exits (the key that takes each is the first of its log: chunk c = ops [1024 c, 1024 c + 1024)):
  1 LDS birth list full (birth_s -> gbirth)                test_gpu_exit_aw_births_overflow
  2 LDS kill list full (kills -> gkill)                    test_gpu_exit_aw_kills_overflow
  3 MV token hash full / over-probed (hash_kill -> gkill)  test_gpu_exit_mv_hash_overflow
  4 grouped MV: gset_insert gives up (-> atomicOr)         test_gpu_exit_mv_gset_overflow
  5 more than SCAP survivors, capacity edges (k_big_finish) test_gpu_exit_many_survivors
Each key is read past every op, before every op and at a middle clock inside a chunk, through the
batch-clock (fast) variants and the general ones (per-read clocks, cached bases), beside short keys
of its type.
Sums: PN (rows, k_stream, the lane tier of a mixed batch), the bounded counter (rows with both
deferral amounts, the wave tier / k_sets, the big tier's per-chunk slots and their flush) and both
through the snapshot cache."""
import random

import numpy as np
import pytest
import torch

from antidote_amd import abi
from antidote_amd.devbatch import DeviceReads, materialize
from antidote_amd.oplog import HostBatch, HostLog, Read
from oracle import amo
from tests import bigexits as bx
from tests import randlog
from tests.bigexits import AW, BC, MV, PN

pytestmark = pytest.mark.gpu

OVF = ("error", abi.AM_ERR_OVERFLOW)
CAPERR = ("error", abi.AM_ERR_CAPACITY)


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def key_ngrp(mat, st, k):
    out = np.zeros(k + 1, np.uint32)
    abi.check(mat.L.am_memcpy_d2h(mat.ctx, out.ctypes.data, st.device_log().key_ngrp, out.nbytes), "am_memcpy_d2h")
    return int(out[k])


def check_fast(mat, dlog, log, n_dc, sel, types, clock, caps):
    """One batch-clock read (the fast variants: no bases, TxIds or per-read clocks) of the keys
    `sel` with room caps[i] against the oracle; returns the oracle's results."""
    n = len(sel)
    hint = types[0] if len(set(types)) == 1 else 0
    dr = DeviceReads(n, n_dc, hint, clock, set_cap=1, keys=torch.tensor(sel, dtype=torch.int64, device="cuda"),
                     types=torch.tensor(types, dtype=torch.uint8, device="cuda"))
    if dr.set_off is not None:
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum(caps)
        dr.set_off = torch.from_numpy(off).cuda()
        dr.set_a = torch.zeros(max(int(off[-1]), 1), dtype=torch.int64, device="cuda")
        dr.set_b = torch.zeros(max(int(off[-1]), 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    materialize(mat, dlog, dr)
    mat.sync()
    h = dr.host()
    reads = [Read(k, t, {d: clock[d] for d in range(n_dc)}) for k, t in zip(sel, types)]
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    want = [ref.result(i) for i in range(n)]
    ok = [i for i in range(n) if want[i][0] == "ok" and int(h["status"][i]) == 0]
    vals = dict(zip(ok, dr.values(np.asarray(ok, np.int64)))) if ok else {}
    for i in range(n):
        if int(h["status"][i]) != 0:
            got = ("error", int(h["status"][i]))
        else:
            ct = None if h["last_ct_ignore"][i] else {d: int(h["last_ct"][d, i]) for d in range(n_dc)
                                                      if (int(h["last_ct_pres"][i]) >> d) & 1}
            got = ("ok", vals.get(i), int(h["new_last_op"][i]), ct, bool(h["is_new_ss"][i]), int(h["count"][i]),
                   int(h["flags"][i]))
        assert got == want[i], (sel[i], types[i], clock[0], got[:1], want[i][:1], _diff(got, want[i]))
    return want


def check_general(mat, st, log, n_dc, reads, caps):
    """read_batch (per-read clocks: the general variants) against the oracle; returns the oracle's
    results."""
    got = mat.read_batch(st, reads, caps)
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    want = [ref.result(i) for i in range(len(reads))]
    for i in range(len(reads)):
        a = got.result(i)
        assert a == want[i], (i, reads[i].key, reads[i].type, a[:1], want[i][:1], _diff(a, want[i]))
    return want


def _diff(a, b):
    """A short account of where two results differ (the values may hold thousands of pairs)."""
    if a[0] != "ok" or b[0] != "ok":
        return (a if a[0] != "ok" else a[0], b if b[0] != "ok" else b[0])
    out = [(j, x, y) for j, (x, y) in enumerate(zip(a[2:], b[2:]), 2) if x != y]
    if a[1] != b[1]:
        va, vb = a[1], b[1]
        if isinstance(va, list) and isinstance(vb, list):
            first = next((j for j, (x, y) in enumerate(zip(va, vb)) if x != y), min(len(va), len(vb)))
            out.append(("value", len(va), len(vb), first, va[first:first + 2], vb[first:first + 2]))
        else:
            out.append(("value", va, vb))
    return out


def shorts(t, n_dc, seed, lens=(0, 5, 40, 300)):
    rng = random.Random(seed)
    return [randlog.rand_key_ops(rng, t, n_dc, n, t0=bx.T0) for n in lens]


def all_ok(want):
    bad = [(i, r) for i, r in enumerate(want) if r[0] != "ok"]
    assert not bad, bad


def dict_clock(c, n_dc):
    return {d: c[d] for d in range(n_dc)}


def run_exit(mat, t, n_dc, big, mid, cap, ngrp=None, base_after=None, fresh=True):
    """The key `big` (key 0) beside four short keys of its type: fast and general reads past every
    op, before every op and after `mid` ops; base_after: the general reads again over the result
    of the read after that many ops as the cached base.  fresh=False: only the reads over the base
    (the key's fresh reads belong to another path)."""
    keys = [big] + shorts(t, n_dc, 50 + n_dc)
    types = [t] * len(keys)
    log = HostLog(n_dc, keys, key_types=types)
    st = mat.store(log)
    try:
        if ngrp == "big":  # the chunked token-group view, whatever its group count
            assert key_ngrp(mat, st, 0) != bx.NGRP_NONE and key_ngrp(mat, st, 0) & bx.NGRP_BIG, hex(key_ngrp(mat, st, 0))
        elif ngrp is not None:
            assert key_ngrp(mat, st, 0) == ngrp, hex(key_ngrp(mat, st, 0))
        dlog = st.device_log()
        clocks = [bx.clock_after(big, m, n_dc) for m in (len(big), 0, mid)]
        sel, caps = list(range(len(keys))), [cap] * len(keys)
        if fresh:
            for clock in clocks:
                all_ok(check_fast(mat, dlog, log, n_dc, sel, types, clock, caps))
        # one batch: the big key at its three clocks, each short key at a clock of its own
        reads = [Read(0, t, dict_clock(c, n_dc)) for c in clocks]
        for k in range(1, len(keys)):
            hi = keys[k][-1].commit_time if keys[k] else bx.T0 + 50
            reads.append(Read(k, t, {d: bx.T0 + (hi - bx.T0) * (k + 1) // 5 + d for d in range(n_dc)}))
        if fresh:
            all_ok(check_general(mat, st, log, n_dc, reads, [cap] * len(reads)))
        if base_after is not None:
            first = [Read(k, t, dict_clock(bx.clock_after(big, base_after, n_dc), n_dc)) for k in range(len(keys))]
            res = check_general(mat, st, log, n_dc, first, [cap] * len(first))
            all_ok(res)
            assert len(res[0][1]) > 0, "the base has pairs"
            over = [Read(r.key, t, r.clock, None, res[r.key][3], res[r.key][2], res[r.key][1]) for r in reads
                    if all(r.clock[d] >= first[0].clock[d] for d in range(n_dc))]
            assert sum(r.key == 0 for r in over) == 2  # past every op, and the middle clock
            all_ok(check_general(mat, st, log, n_dc, over, [cap] * len(over)))
    finally:
        st.close()


@pytest.mark.parametrize("n_dc", [3, 17])
def test_gpu_exit_aw_births_overflow(mat, n_dc):
    """bigexits.aw_births_overflow: every chunk births 4 x LB pairs; most of a chunk's kills hit
    births that were exported unresolved.  More than 12000 pairs survive."""
    run_exit(mat, AW, n_dc, bx.aw_births_overflow(n_dc), 2600, 16384, base_after=500)


@pytest.mark.parametrize("n_dc", [3, 17])
def test_gpu_exit_aw_kills_overflow(mat, n_dc):
    """bigexits.aw_kills_overflow: every full chunk holds 3072 kills for LK = 2048 list slots; the
    overflowed ones are the only kill of births of the same chunk."""
    run_exit(mat, AW, n_dc, bx.aw_kills_overflow(n_dc), 2600, 4096, base_after=500)


@pytest.mark.parametrize("variant", ["born_twice", "cached_base"])
def test_gpu_exit_mv_hash_overflow(mat, variant):
    """bigexits.mv_hash_overflow through k_big_chunk's LDS token hash (about 2760 distinct killed
    tokens per chunk for 2048 slots).  born_twice: the key is AM_NGRP_NONE and its fresh reads go
    there.  cached_base: the key is grouped (its fresh reads take the grouped mode, read here as
    well); read over the result after 40 ops -- a base with pairs -- it goes through k_big_chunk."""
    twice = variant == "born_twice"
    big = bx.mv_hash_overflow(3, born_twice=twice)
    ngrp = bx.NGRP_NONE if twice else "big"  # (tokens that are overridden but never born count as groups too)
    run_exit(mat, MV, 3, big, 1500, 1024, ngrp=ngrp, base_after=40)


@pytest.mark.parametrize("n_dc", [3, 17])
def test_gpu_exit_mv_gset_overflow(mat, n_dc):
    """bigexits.mv_gset_overflow: about 127 group ids of chunk 3 compete for 63 slots of the born
    set, 80 of their kills for the same slots of the kill set; the middle clock includes the
    births and about 40 of the kills."""
    big = bx.mv_gset_overflow(n_dc)
    run_exit(mat, MV, n_dc, big, bx.GSET_CHUNK * bx.CHUNK + 170, 1024, ngrp=bx.NGRP_BIG | bx.GSET_OPS)


BASE_OPS = 500


@pytest.mark.parametrize("n", [bx.SCAP, bx.SCAP + 1, 3000])
@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_exit_many_survivors(mat, t, n):
    """Exactly n survivors (SCAP: the last count sorted in LDS; SCAP + 1 and 3000: the sort in
    global scratch, for AW with the token payload) with room n (ok) and n - 1 (AM_ERR_CAPACITY on
    both sides), fresh (MV: the grouped finish) and over the base taken after 500 ops (base pairs
    among the survivors; MV: the ungrouped path and its de-duplicating write), fast and general;
    then the usual three clocks."""
    n_dc = 3
    big = (bx.aw_many_survivors if t == AW else bx.mv_many_survivors)(n, n_dc)
    keys = [big] + shorts(t, n_dc, 60 + n % 7)
    types = [t] * len(keys)
    log = HostLog(n_dc, keys, key_types=types)
    full = bx.clock_after(big, len(big), n_dc)
    st = mat.store(log)
    try:
        dlog = st.device_log()
        sel = [0, 0] + list(range(1, len(keys)))  # the key twice: with room, one short of it
        caps = [n, n - 1] + [512] * (len(keys) - 1)
        want = check_fast(mat, dlog, log, n_dc, sel, [t] * len(sel), full, caps)
        assert want[0][0] == "ok" and len(want[0][1]) == n and want[1] == CAPERR
        all_ok(want[2:])
        reads = [Read(k, t, dict_clock(full, n_dc)) for k in sel]
        want = check_general(mat, st, log, n_dc, reads, caps)
        assert want[0][0] == "ok" and len(want[0][1]) == n and want[1] == CAPERR
        early = dict_clock(bx.clock_after(big, BASE_OPS, n_dc), n_dc)
        first = check_general(mat, st, log, n_dc, [Read(0, t, early)], [n])[0]
        assert first[0] == "ok" and len(first[1]) > 100
        over = [Read(0, t, dict_clock(full, n_dc), None, first[3], first[2], first[1]) for _ in range(2)] + reads[2:]
        wb = check_general(mat, st, log, n_dc, over, caps)
        assert wb[0][0] == "ok" and wb[0][1] == want[0][1] and wb[1] == CAPERR
    finally:
        st.close()
    run_exit(mat, t, n_dc, big, 2600, 4096)


# ---------------------------------------------------------------- sums
def sum_reads(keys, t, n_dc, n_ops):
    """Per key: the read at the newest clock over its base (when it has one) and a fresh read at a
    middle clock of its own."""
    full = dict_clock([bx.T0 + 3 * n_ops] * n_dc, n_dc)
    base0 = {d: 0 for d in range(n_dc)}
    reads = []
    for i, k in enumerate(keys):
        reads.append(Read(i, t, full, None, None if k["base"] is None else base0, 0, k["base"]))
        reads.append(Read(i, t, dict_clock(bx.clock_after(k["ops"], n_ops // 2 + i % 3, n_dc), n_dc)))
    return reads


def check_sum_keys(mat, t, n_dc, n_ops, keys, extra):
    """Fast reads past every op, before every op and at the middle; general reads (sum_reads).
    The oracle's status at the newest clock is the one each key is built for."""
    all_keys = [k["ops"] for k in keys] + extra
    types = [t] * len(all_keys)
    log = HostLog(n_dc, all_keys, key_types=types)
    cap = n_dc * n_dc + n_dc if t == BC else 1
    st = mat.store(log)
    try:
        dlog = st.device_log()
        sel, caps = list(range(len(all_keys))), [cap] * len(all_keys)
        for m in (n_ops, 0, n_ops // 2):
            want = check_fast(mat, dlog, log, n_dc, sel, types, bx.clock_after(keys[0]["ops"], m, n_dc), caps)
            if m == n_ops:
                for k, r in zip(keys, want):
                    if k["base"] is None:
                        assert (r == OVF) if k["want"] == "overflow" else r[0] == "ok", (k["name"], r[:2])
            if m == 0:
                all_ok(want)
        reads = sum_reads(keys, t, n_dc, n_ops)
        want = check_general(mat, st, log, n_dc, reads, [cap] * len(reads))
        for i, k in enumerate(keys):
            r = want[2 * i]
            assert (r == OVF) if k["want"] == "overflow" else r[0] == "ok", (k["name"], r[:2])
    finally:
        st.close()


@pytest.mark.parametrize("n_ops", [3, 64, 65, 700])
@pytest.mark.parametrize("n_dc", [1, 3, 17])
def test_gpu_pn_edge_sums(mat, n_dc, n_ops):
    """PN sums of exactly INT64_MAX / INT64_MIN (ok), one beyond each, +-2^64 (low word 0) and a
    climb past the int64 range that returns to 7, and bases of INT64_MAX / INT64_MIN: 3 and 64 ops
    (the row tier), 65 and 700 (k_stream: wave_sum_i128 / add128)."""
    check_sum_keys(mat, PN, n_dc, n_ops, bx.pn_edge_keys(n_ops, n_dc), shorts(PN, n_dc, 70, (0, 5, 100)))


def test_gpu_pn_edge_sums_lane_tier(mat):
    """A five-type batch whose PN edge keys have 3 and 40 ops: the lane tier (am_lanes.hip) sums
    them.  General (read_batch, with the bases) and fast (one batch clock)."""
    n_dc = 3
    pn = bx.pn_edge_keys(3, n_dc) + bx.pn_edge_keys(40, n_dc)
    keys, types = [k["ops"] for k in pn], [PN] * len(pn)
    rng = random.Random(71)
    for t in (abi.AM_LWW, AW, MV, BC):
        for n in (5, 30, 60):
            keys.append(randlog.rand_key_ops(rng, t, n_dc, n, t0=bx.T0))
            types.append(t)
    log = HostLog(n_dc, keys, key_types=types)
    caps = [64] * len(keys)
    full = [bx.T0 + 3 * 40] * n_dc
    st = mat.store(log)
    try:
        reads = [Read(i, types[i], dict_clock(full, n_dc)) for i in range(len(keys))]
        for i, k in enumerate(pn):
            if k["base"] is not None:
                reads[i] = Read(i, PN, dict_clock(full, n_dc), None, {d: 0 for d in range(n_dc)}, 0, k["base"])
        want = check_general(mat, st, log, n_dc, reads, caps)
        for k, r in zip(pn, want):
            assert (r == OVF) if k["want"] == "overflow" else (r[0] == "ok" and r[1] == k["total"]), (k["name"], r[:2])
        all_ok(want[len(pn):])
        want = check_fast(mat, st.device_log(), log, n_dc, list(range(len(keys))), types, full, caps)
        for k, r in zip(pn, want):
            if k["base"] is None:
                assert (r == OVF) if k["want"] == "overflow" else (r[0] == "ok" and r[1] == k["total"]), (k["name"], r[:2])
    finally:
        st.close()


@pytest.mark.parametrize("n_ops", [40, 48, 49, 300, 4096, 4097, 5000])
@pytest.mark.parametrize("n_dc", [3, 13, 17])
def test_gpu_bc_edge_sums(mat, n_dc, n_ops):
    """Bounded-counter slots on the int64 edges (bigexits.bc_edge_keys): 40 and 48 ops = the row
    tier (am_bcrows / k_rows in list mode above 16 DCs; 2^56 defers, 2^56 - 1 does not), 49 .. 4096
    = the wave tier (am_bcwave, 3 and 13 DCs) or k_sets (17 DCs), 4097 and 5000 = the big tier
    (k_big_run's LDS slots, their flush into the read's 128-bit global slots -- the key `flush`
    carries only there -- and the slots' start from a base snapshot)."""
    check_sum_keys(mat, BC, n_dc, n_ops, bx.bc_edge_keys(n_ops, n_dc), shorts(BC, n_dc, 72, (0, 5, 60)))


def test_gpu_edge_sums_through_snapshot_cache(mat):
    """am_snapcache_read: a PN key and a bounded-counter key read at three ever newer clocks.  The
    first read (30 ops, INT64_MAX - 10) is stored; the second adds ten ops of 1 to that cached base
    (exactly INT64_MAX, ok, stored too); the third adds one more (AM_ERR_OVERFLOW).  Each value
    equals the oracle's fresh read at the same clock."""
    n_dc = 3
    amounts = [1 << 62, (1 << 62) - 11 - 28] + [1] * 28 + [1] * 10 + [1]
    assert sum(amounts[:30]) == bx.INT64_MAX - 10 and sum(amounts[:40]) == bx.INT64_MAX
    keys = [bx.stamp(PN, amounts, n_dc), bx.stamp(BC, [("transfer", v, 1, 0) for v in amounts], n_dc)]
    types = [PN, BC]
    log = HostLog(n_dc, keys, key_types=types)
    store = mat.store(log)
    cache = mat.snapshot_cache(store, 2)
    try:
        for m, ok in ((30, True), (40, True), (41, False)):
            clock = dict_clock(bx.clock_after(keys[0], m, n_dc), n_dc)
            reads = [Read(k, types[k], clock) for k in range(2)]
            caps = [16, 16]
            got = cache.read(reads, set_capacity=caps)
            ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
            for k in range(2):
                g, r = got.result(k), ref.result(k)
                if ok:
                    assert r[0] == "ok" and g[0] == "ok" and g[1] == r[1], (m, k, g, r)
                else:
                    assert r == OVF and g == OVF, (m, k, g, r)
            if ok:  # the read left a snapshot for the next one to start from (newest first, by its last op id)
                assert all(cache.entries(k)[0][1] == m for k in range(2)), [cache.entries(k) for k in range(2)]
    finally:
        cache.close()
        store.close()
