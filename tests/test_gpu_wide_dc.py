"""Reads at 13, 17 and 32 data centres: the kernel widths no other module opens.

Every read kernel is compiled per clock width D in {1, 2, 3, 4, 8, 16, 32} and picked by
`nd <= 16 ? 16 : 32`; 13 is the padded D = 16 variant, 17 the padded D = 32 one (the first width
past every `n_dc <= 16` guard) and 32 the exact one, whose presence mask is 0xFFFFFFFF and whose
last DC is bit 31 of every mask and value 31 of op_meta's five DC bits.

Above 16 DCs the read path differs in kind, not only in width (all checked below):
  * the store has no lag view (am_pack.hip LAG_MAX_DC = 16): lag_ct is null, no op is a lag-only
    escape, no key is routed, AW / MV wave reads stay on the packed view;
  * a bounded counter has neither am_bcrows nor am_bcwave (both need n_dc <= 16): its chain is
    k_rows in list mode (am_rows.hip RowSmem<32>::SLOTS == false), then k_sets over
    n_dc^2 + n_dc <= 1056 slots, then the big tier.
Every output column is compared bit for bit with oracle/am_oracle.c."""
import random

import numpy as np
import pytest
import torch

from antidote_amd import abi
from antidote_amd.devbatch import DeviceReads, materialize
from antidote_amd.oplog import HostBatch, HostLog, Op, Read
from oracle import amo
from tests import randlog
from tests.test_gpu_lagcadence import FAR, T0, at_entry, check_batch, make_keys, span, view_counts

pytestmark = pytest.mark.gpu

PN, LWW, AW, MV, BC = abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER
WIDTHS = [13, 17, 32]
# AW / MV: the lane tier (<= 64 ops, am_lanes.hip LBITS), the wave tier, the workgroup tier and
# k_sets; 1024 | 1025 is AM_BIG_MIN_OPS (an MV key past it has the chunked big view), 4097 and 5000
# are past AM_SETS_BIG_OPS = 4096 (the big tier), 2200 is past AM_GRP_MAX_REC = 2048 records;
# 255 | 256 | 257 and 1024 | 1025 straddle a 256-op tile.
SET_LENS = [0, 1, 3, 17, 64, 65, 255, 256, 257, 300, 1024, 1025, 1100, 2200, 4097, 5000]
# bounded counter: 0 .. 48 = the row tier (am_plan.hip ROWS_BC = 48; list mode above 16 DCs);
# 49 .. 4096 = at 13 DCs the wave tier (AM_BCWAVE_OPS = 4096), above 16 DCs k_sets
# (AM_SETS_BIG_OPS = 4096); 4097 and 5000 = the big tier.
BC_LENS = [0, 3, 40, 48, 49, 64, 70, 130, 300, 2500, 4096, 4097, 5000]
# PN / LWW: <= 64 the row tier (ROWS_SCALAR = 64), longer k_stream (am_stream.h)
SCALAR_LENS = [0, 3, 16, 20, 64, 65, 300, 700]
LENS = {AW: SET_LENS, MV: SET_LENS, BC: BC_LENS, PN: SCALAR_LENS, LWW: SCALAR_LENS}
# Room per set read.  An AW effect adds at most 2 tokens to each of at most 2 elements and an MV
# assign one value, so a 5000-op key has at most 20000 survivors; the keys drawn here stay far
# below that (512 was too few for the 5000-op AW key at 32 DCs: the oracle returned
# AM_ERR_CAPACITY).  Every parity case asserts that the oracle returns ok for every read.
CAP = 8192


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def full_mask(n_dc):
    return (1 << n_dc) - 1


def check_ok(mat, dlog, log, keys, t, n_dc, clock, sel=None, pres=None):
    """check_batch, after the oracle alone has returned ok for every read (no capacity error hides
    a value)."""
    ks = list(range(len(keys))) if sel is None else list(sel)
    reads = [Read(k, t, {d: clock[d] for d in range(n_dc) if pres is None or (pres >> d) & 1}) for k in ks]
    ref = amo.materialize(log, HostBatch(n_dc, reads, randlog.caps_for(reads, n_dc, CAP)))
    bad = [(ks[i], ref.result(i)) for i in range(len(ks)) if ref.result(i)[0] != "ok"]
    assert not bad, bad
    check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=CAP, sel=sel, pres=pres)


def entry(op, d):
    return op.commit_time if op.commit_dc == d else op.snap[d]


def check_store(st, log, n_dc, regime):
    """The counters and views that tell the paths apart."""
    got, want = st.view_stats(), view_counts(log)[0]
    dlog = st.device_log()
    if n_dc <= 16:
        assert dlog.lag_ct, "a store of <= 16 DCs has the lag view"
        assert got == want, (got, want)
    else:
        assert not dlog.lag_ct and not dlog.lag, "no lag view above LAG_MAX_DC"
        assert got["lag_only_esc_ops"] == 0 and got["routed_keys"] == 0 and got["routed_ops"] == 0, got
        assert (got["ops"], got["pk_esc_ops"]) == (want["ops"], want["pk_esc_ops"]), (got, want)
    if regime == "tight":
        assert got["pk_esc_ops"] == 0, got
    else:
        assert got["pk_esc_ops"] > 0, got
    return dlog


def extra_bc_keys(n_dc):
    """Bounded-counter keys of at most 48 ops (the row tier) at its two exits:
    [0] one amount of 2^56 + 5 among small ones: in slot-array mode (n_dc <= 16) the row defers the
        read to the next tier, in list mode it takes the exact 128-bit pass;
    [1] three increments of 2^62 into the last DC's own P slot: AM_ERR_OVERFLOW;
    [2] 48 ops that all land in two slots (P[n_dc-1][n_dc-1] and D[n_dc-1]): the longest entry
        list a lane scans for one slot.
    An effect is one (slot, amount) entry (increment: P[id][id], decrement: D[id], transfer:
    P[from][to]), so a row read of <= 48 ops never exceeds the list's RK = 64 entries: the list
    overflow exit of k_rows cannot be reached through am_materialize."""
    last = n_dc - 1

    def ops_of(effs):
        return [Op(BC, i % n_dc, T0 + 10 + 3 * i, {d: T0 + 9 + 3 * i - (d % 5) for d in range(n_dc)}, e)
                for i, e in enumerate(effs)]
    big = [("increment", 7, last) if i != 11 else ("increment", (1 << 56) + 5, last) for i in range(20)]
    big[3] = ("transfer", 9, 0, last)
    ovf = [("increment", 1 << 62, last)] * 3 + [("decrement", 4, 0)]
    two = [("increment", 3 + i, last) if i % 2 else ("decrement", 1 + i, last) for i in range(48)]
    return [ops_of(big), ops_of(ovf), ops_of(two)]


@pytest.mark.parametrize("regime", ["tight", "sparse"])
@pytest.mark.parametrize("n_dc", WIDTHS)
@pytest.mark.parametrize("t", randlog.TYPES)
def test_gpu_wide_fast_path(mat, t, n_dc, regime):
    """The fast variants (batch clock, full-clock log, no bases) over one key per length of LENS
    (the tier each length reaches is noted there), read
      1. past every op, 2. before every op, 3. at a middle clock,
      4. per key, with DC n_dc - 1 exactly on its middle op's entry and one below, every other DC
         past the newest op (at 32 the entry of bit 31 alone decides) -- each key alone, and the
         longest key's entry over the whole batch,
      5. past every op with DC 0, DC n_dc - 1 and a middle DC absent from the clock,
      and once more past every op after the zone index is dropped (AM_INDEX_NONE).
    sparse: one FAR escape and a few lag-only boundaries per key of >= 12 ops (make_keys), so each
    tier's escape walk runs.  Bounded counter: half of the effects move rights among DCs 0, 16, 30,
    31 and n_dc - 1; above 16 DCs the lengths 0, 3, 40 and 48 and the three keys of extra_bc_keys
    stay in the row tier's list mode (ROWS_BC = 48), every longer one is handed on."""
    rng = random.Random(8100 + 100 * t + n_dc + len(regime))
    keys, _ = make_keys(rng, t, n_dc, LENS[t], regime)
    if t == BC:
        for ops in keys:
            randlog.far_bc_effects(rng, n_dc, ops)
        keys += extra_bc_keys(n_dc)
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        dlog = check_store(st, log, n_dc, regime)
        lo, hi = span(keys)
        last = n_dc - 1
        if t == BC:  # the overflow key is an error at every clock that includes it: compared by check_batch
            ovf = len(LENS[t]) + 1
            ok_keys = [k for k in range(len(keys)) if k != ovf]
            check_batch(mat, dlog, log, keys, t, n_dc, [hi] * n_dc, cap=CAP, sel=[ovf])
            r = amo.materialize(log, HostBatch(n_dc, [Read(ovf, t, {d: hi for d in range(n_dc)})],
                                               [n_dc * n_dc + n_dc])).result(0)
            assert r == ("error", abi.AM_ERR_OVERFLOW), r
        else:
            ok_keys = list(range(len(keys)))
        for clock in ([hi] * n_dc, [lo - 20] * n_dc, [lo + (hi - lo) // 2] * n_dc):
            check_ok(mat, dlog, log, keys, t, n_dc, clock, sel=ok_keys)
        for k in ok_keys:
            if keys[k]:
                e = entry(keys[k][len(keys[k]) // 2], last)
                for x in (e, e - 1):
                    check_ok(mat, dlog, log, keys, t, n_dc, at_entry(hi, n_dc, last, x), sel=[k])
        longest = max(ok_keys, key=lambda k: len(keys[k]))
        e = entry(keys[longest][len(keys[longest]) // 2], last)
        for x in (e, e - 1):
            check_ok(mat, dlog, log, keys, t, n_dc, at_entry(hi, n_dc, last, x), sel=ok_keys)
        for d in (0, last, n_dc // 2):
            check_ok(mat, dlog, log, keys, t, n_dc, [hi] * n_dc, sel=ok_keys, pres=full_mask(n_dc) & ~(1 << d))
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        check_ok(mat, dlog, log, keys, t, n_dc, [hi] * n_dc, sel=ok_keys)
        check_ok(mat, dlog, log, keys, t, n_dc, [lo + (hi - lo) // 2] * n_dc, sel=ok_keys)
    finally:
        st.close()


@pytest.mark.parametrize("t,lens", [(BC, [40, 300, 5000]), (AW, [40, 300, 1500, 5000])])
def test_gpu_wide_all_escaped_missing_dc(mat, t, lens):
    """32 DCs, every op outside the packed view (one remote entry FAR below its commit time): the
    escape reader alone decides each read, at D = 32, with every DC present and with DC 0, DC 31
    and DC 16 absent (the op is excluded and AM_FLAG_MISSING_DC_LOGGED set)."""
    n_dc = 32
    rng = random.Random(8400 + t)
    keys, _ = make_keys(rng, t, n_dc, lens, "tight")
    for ops in keys:
        randlog.far_bc_effects(rng, n_dc, ops)
        for op in ops:
            op.snap[(op.commit_dc + 1) % n_dc] = op.commit_time - FAR
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        stats = st.view_stats()
        assert stats["pk_esc_ops"] == stats["ops"] == sum(lens), stats
        assert stats["lag_only_esc_ops"] == 0 and not st.device_log().lag_ct
        dlog = st.device_log()
        _, hi = span(keys)
        for pres in [None] + [0xFFFFFFFF & ~(1 << d) for d in (0, 31, 16)]:
            check_ok(mat, dlog, log, keys, t, n_dc, [hi] * n_dc, pres=pres)
    finally:
        st.close()


def test_gpu_wide_default_mask_is_all_ones(mat):
    """DeviceReads' default presence mask at AM_MAX_DC is 0xFFFFFFFF on the device (it used to be
    built as an int32 literal, which 2^32 - 1 overflows), and a read through it sees DC 31."""
    dr = DeviceReads(4, 32, PN, [100] * 32)
    assert dr.read_pres.dtype == torch.int32
    assert int(dr.read_pres.cpu().numpy().view(np.uint32)[0]) == 0xFFFFFFFF
    for n_dc in (1, 13, 17, 31):
        small = DeviceReads(1, n_dc, PN, [100] * n_dc)
        assert int(small.read_pres.cpu().numpy().view(np.uint32)[0]) == (1 << n_dc) - 1
    given = DeviceReads(1, 32, PN, [1] * 32, pres=0x80000001)
    assert int(given.read_pres.cpu().numpy().view(np.uint32)[0]) == 0x80000001
    # one op committed at DC 31 whose snapshot needs DC 31 at 50: included only if bit 31 is read
    ops = [Op(PN, 31, 60, {d: 50 for d in range(32)}, 5)]
    keys = [ops] * 4
    log = HostLog(32, keys, key_types=[PN] * 4)
    st = mat.store(log)
    try:
        check_batch(mat, st.device_log(), log, keys, PN, 32, [100] * 32)
        torch.cuda.synchronize()
        materialize(mat, st.device_log(), dr)
        mat.sync()
        assert dr.values(range(4)) == [5] * 4 and (dr.host()["flags"] == 0).all()
    finally:
        st.close()


def test_gpu_wide_capacity_one_short(mat):
    """32 DCs: an AW key whose room is one pair below its survivor count reports AM_ERR_CAPACITY,
    the same key read beside it with room is exact.  Three lengths: the lane tier (40), the
    wave / workgroup tiers (300) and k_sets past AM_GRP_MAX_REC records (2200); through the fast
    variants (DeviceReads with its offsets narrowed) and the general ones (read_batch)."""
    n_dc, t = 32, AW
    rng = random.Random(8500)
    lens = [40, 300, 2200]
    keys, _ = make_keys(rng, t, n_dc, lens, "tight")
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    _, hi = span(keys)
    clock = {d: hi for d in range(n_dc)}
    sel = [0, 0, 1, 1, 2, 2]  # each key twice: short of room, then with room
    reads = [Read(k, t, clock) for k in sel]
    full = amo.materialize(log, HostBatch(n_dc, reads, [CAP] * 6))
    surv = [len(full.result(i)[1]) for i in range(6)]
    assert all(full.result(i)[0] == "ok" for i in range(6)) and min(surv) >= 2, surv
    caps = [surv[i] - 1 if i % 2 == 0 else surv[i] for i in range(6)]
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    for i in range(6):
        want = ("error", abi.AM_ERR_CAPACITY) if i % 2 == 0 else full.result(i)
        assert ref.result(i) == want, (i, ref.result(i))
    st = mat.store(log)
    try:
        got = mat.read_batch(st, reads, caps)
        for i in range(6):
            assert got.result(i) == ref.result(i), (i, got.result(i), ref.result(i))
        dr = DeviceReads(6, n_dc, t, [hi] * n_dc, set_cap=CAP, keys=torch.tensor(sel, dtype=torch.int64, device="cuda"))
        off = np.zeros(7, np.int64)
        off[1:] = np.cumsum(caps)
        dr.set_off = torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        materialize(mat, st.device_log(), dr)
        mat.sync()
        h = dr.host()
        assert [int(x) for x in h["status"]] == [abi.AM_ERR_CAPACITY, 0] * 3
        ok = [1, 3, 5]
        for i, v in zip(ok, dr.values(ok)):
            r = full.result(i)
            ct = {d: int(h["last_ct"][d, i]) for d in range(n_dc) if (int(h["last_ct_pres"][i]) >> d) & 1}
            assert ("ok", v, int(h["new_last_op"][i]), ct, bool(h["is_new_ss"][i]), int(h["count"][i]),
                    int(h["flags"][i])) == r, (i, r)
    finally:
        st.close()


# ---------------------------------------------------------------- general variants
def _compare(mat, st, log, reads, n_dc, cap):
    caps = randlog.caps_for(reads, n_dc, cap)
    got = mat.read_batch(st, reads, caps)
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    for i in range(len(reads)):
        a, b = got.result(i), ref.result(i)
        assert a == b, (i, reads[i].key, reads[i].type, a, b)
    return got


@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("n_dc", WIDTHS)
@pytest.mark.parametrize("t", randlog.TYPES)
def test_gpu_wide_random_batches(mat, t, n_dc, seed):
    """The GENERAL instantiations (per-read clocks, TxIds, partial op clocks, cached bases) and, on
    the partial logs, the non-packed ones, at D = 16 padded and D = 32: test_gpu_random_batches'
    shape with the bounded counter at the full width.  seed 0: full clocks and TxIds; seed 1:
    partial op clocks (snap_pres), partial read clocks and 0.2 % bad effects.  Then every ok read
    again from its own result as the cached base."""
    rng = random.Random(8600 + seed * 7 + 31 * t + n_dc)
    partial = seed == 1
    lens = [0, 1, 3, 17, 64, 255, 256, 257, 400] if t in (AW, MV) else [0, 1, 3, 17, 64, 255, 256, 257, 700]
    keys, reads = [], []
    for k in range(60):
        n_ops = lens[k % len(lens)] if k % 5 else rng.randint(0, 48)
        ops = randlog.rand_key_ops(rng, t, n_dc, n_ops, partial=partial, txids=seed == 0,
                                   bad_rate=0.002 if seed == 1 else 0.0, t0=rng.randint(0, 100))
        keys.append(randlog.far_bc_effects(rng, n_dc, ops))
        hi = ops[-1].commit_time if ops else 50
        # (a read clock lacks each DC with chance 1 / n_dc: with the default 0.2 every read of 32
        # DCs would lack some DC that each op names, and include nothing)
        clock = randlog.rand_clock(rng, n_dc, hi // 3, hi + 5, partial=partial, miss=1.0 / n_dc)
        reads.append(Read(k, t, clock, rng.choice([None, 1, 3]) if seed == 0 else None))
    log = HostLog(n_dc, keys, key_types=[t] * len(keys), partial=partial or None)
    st = mat.store(log)
    try:
        first = _compare(mat, st, log, reads, n_dc, 1024)
        oks = [first.result(i) for i in range(60) if first.result(i)[0] == "ok"]
        assert len(oks) >= 40 and sum(r[5] > 0 for r in oks) >= 15, "reads that include ops"
        reads2 = []
        for i, r in enumerate(reads):
            res = first.result(i)
            if res[0] == "ok":
                clock2 = {d: v + rng.randint(0, 200) for d, v in r.clock.items()}
                reads2.append(Read(r.key, t, clock2, None, res[3], res[2], res[1]))
        _compare(mat, st, log, reads2, n_dc, 1024)
    finally:
        st.close()


@pytest.mark.parametrize("n_dc", [17, 32])
def test_gpu_wide_mixed_batch_planner(mat, n_dc):
    """One log with keys of all five types read in one batch of 1100 reads (type_hint = 0: two
    1024-read planner blocks), so the lane tier, k_plan_*, the three set chains on their
    sub-streams and both scalar chains run at D = 32.  Lengths on either side of the lane tier's
    hand-off (a lane read holds 64 inclusion bits from its 4-op-aligned start: am_lanes.hip LBITS,
    lopl = 4 above D = 8): 60 .. 66; an MV key of 1100 ops (past AM_BIG_MIN_OPS = 1024: the early
    big-MV class); bounded-counter keys on both sides of ROWS_BC (the early chain).  Twenty reads
    name an unknown type or a key past the log: AM_ERR_INVALID from the planner (the oracle has
    no such read: asserted directly); twenty name another type than the key's: corrupted."""
    rng = random.Random(8700 + n_dc)
    lens = [0, 1, 7, 16, 48, 49, 60, 61, 62, 63, 64, 65, 66, 90, 300]
    keys, types = [], []
    for k in range(200):
        t = randlog.TYPES[k % 5]
        n_ops = lens[(k // 5) % len(lens)]
        if k == 198:
            assert t == MV
            n_ops = 1100
        ops = randlog.rand_key_ops(rng, t, n_dc, n_ops, t0=T0 + rng.randint(0, 100))
        keys.append(randlog.far_bc_effects(rng, n_dc, ops))
        types.append(t)
    log = HostLog(n_dc, keys, key_types=types)
    n_reads = 1100
    reads, invalid = [], set()
    for i in range(n_reads):
        k = rng.randrange(200)
        hi = keys[k][-1].commit_time if keys[k] else T0 + 50
        clock = randlog.rand_clock(rng, n_dc, T0 + (hi - T0) // 2, hi + 5)
        t = types[k]
        if i % 55 == 7:
            invalid.add(i)
            if i % 2:
                t = rng.choice([0, 6, 9])
            else:
                k = 200 + rng.randrange(5)
        elif i % 55 == 9:
            t = randlog.TYPES[(k + 1) % 5]
        reads.append(Read(k, t, clock))
    assert len(invalid) == 20
    st = mat.store(log)
    try:
        assert not st.device_log().lag_ct
        caps = randlog.caps_for(reads, n_dc, 2048)
        got = mat.read_batch(st, reads, caps)
        valid = [i for i in range(n_reads) if i not in invalid]
        vreads = [reads[i] for i in valid]
        ref = amo.materialize(log, HostBatch(n_dc, vreads, randlog.caps_for(vreads, n_dc, 2048)))
        for i in invalid:
            assert got.result(i) == ("error", abi.AM_ERR_INVALID), (i, reads[i].key, reads[i].type, got.result(i))
        n_err = 0
        for j, i in enumerate(valid):
            a, b = got.result(i), ref.result(j)
            assert a == b, (i, reads[i].key, reads[i].type, len(keys[reads[i].key]), a, b)
            n_err += b[0] == "error"
        assert n_err >= 10  # the wrong-type reads of non-empty keys: corrupted_ops_cache
        assert all(ref.result(j)[0] == "ok" for j, i in enumerate(valid) if reads[i].type == types[reads[i].key])
        # the second batch from the cached bases (base pairs: the LDS-sort tier, the general kernels)
        reads2 = []
        for j, i in enumerate(valid):
            res = ref.result(j)
            if res[0] == "ok":
                r = reads[i]
                later = {d: v + 40 for d, v in r.clock.items()}
                reads2.append(Read(r.key, r.type, later, None, res[3], res[2], res[1]))
        _compare(mat, st, log, reads2, n_dc, 2048)
    finally:
        st.close()


# ---------------------------------------------------------------- stable time
def test_gpu_wide_gst(mat):
    """am_gst_local_min / am_gst_finalize at 32 DCs against amo_gst_min / amo_update_stable, with
    partitions that lack DC 31, DC 0, both, or nothing, and undefined partitions (test_gpu_gst
    draws 1-5 DCs)."""
    nd = 32
    rng = np.random.default_rng(32)
    for trial in range(12):
        npart = int(rng.integers(1, 9))
        vc = rng.integers(0, 1000, size=(npart, nd)).astype(np.uint64)
        pres = np.full(npart, 0xFFFFFFFF, np.uint32)
        if trial % 4 == 1:
            pres[rng.integers(0, npart)] &= np.uint32(0x7FFFFFFF)          # DC 31 absent somewhere
        elif trial % 4 == 2:
            pres[rng.integers(0, npart)] &= np.uint32(0xFFFFFFFE)          # DC 0 absent somewhere
        elif trial % 4 == 3:
            pres = rng.integers(0, 1 << 32, size=npart, dtype=np.uint64).astype(np.uint32)
        undef = (rng.random(npart) < 0.1).astype(np.uint8)
        out = np.zeros(nd, np.uint64)
        op = np.zeros(1, np.uint32)
        amo.lib().amo_gst_min(nd, npart, vc.ctypes.data, pres.ctypes.data, undef.ctypes.data, out.ctypes.data,
                              op.ctypes.data)
        if trial % 4 == 0 and not undef.any():
            assert int(op[0]) == 0xFFFFFFFF
        d_vc = torch.from_numpy(vc.view(np.int64)).cuda()
        d_pres = torch.from_numpy(pres.view(np.int32)).cuda()
        d_undef = torch.from_numpy(undef).cuda()
        lanes = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        abi.check(mat.L.am_gst_local_min(mat.ctx, nd, npart, d_vc.data_ptr(), d_pres.data_ptr(), d_undef.data_ptr(),
                                         lanes.data_ptr()), "local_min")
        mat.sync()
        ln = lanes.cpu().numpy().view(np.uint64)
        for d in range(nd):
            want = out[d] if (int(op[0]) >> d) & 1 else np.uint64(0xFFFFFFFFFFFFFFFF)
            assert ln[d] == want, (trial, d, ln[d], want)
        last = rng.integers(0, 800, size=nd).astype(np.uint64)
        lastp = np.array([rng.integers(0, 1 << 32, dtype=np.uint64)], np.uint64).astype(np.uint32)
        if trial % 3 == 0:
            lastp[0] = 0xFFFFFFFF
        h_last, h_lastp = last.copy(), lastp.copy()
        changed_ref = amo.lib().amo_update_stable(nd, h_last.ctypes.data, h_lastp.ctypes.data, out.ctypes.data,
                                                  int(op[0]))
        d_last = torch.from_numpy(last.view(np.int64)).cuda()
        d_lastp = torch.from_numpy(lastp.view(np.int32)).cuda()
        o_vc = torch.zeros(nd, dtype=torch.int64, device="cuda")
        o_p = torch.zeros(1, dtype=torch.int32, device="cuda")
        ch = torch.zeros(1, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        abi.check(mat.L.am_gst_finalize(mat.ctx, nd, lanes.data_ptr(), d_last.data_ptr(), d_lastp.data_ptr(), 0,
                                        o_vc.data_ptr(), o_p.data_ptr(), ch.data_ptr()), "finalize")
        mat.sync()
        assert int(ch.item()) == changed_ref, trial
        assert int(d_lastp.item()) & 0xFFFFFFFF == int(h_lastp[0]), trial
        gv = d_last.cpu().numpy().view(np.uint64)
        for d in range(nd):
            if (int(h_lastp[0]) >> d) & 1:
                assert gv[d] == h_last[d], (trial, d)
