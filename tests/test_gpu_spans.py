"""The group-span view (include/antidote_mat.h key_nspan / gspan / gsrc) and the span record pass of
the split fresh read (csrc/am_group_split.h k_grp_spans; k_grp_recs shares its batch structure).

1. The view from its definition: key_nspan, gspan and gsrc read back from the device and compared
   with a construction from the host log in Python (births in record order, effective kills, the
   output ranks taken from grp), on random logs and on the synthetic AW and MV logs.
2. Reader cases on hand-made logs, each read three ways: through the spans, through rec_g (the same
   log with the span pointers nulled: every result column must be equal) and by the C oracle.
3. Fallback: a key whose token two ops effectively kill has no spans and reads next to keys that do;
   batch edges: such keys and capacity overflows at the first and last reads of the waves' batches.
4. Apply: am_store_apply keeps a touched key's spans current, flips it to the sentinel on a second
   effective kill, and a GC prune leaves a readable key.
Single-type batches on device stores, the batch clock, no zone index; every key is longer than the
lane tier's short-read hand-off (64 ops), so the wave tier takes it."""
import random

import numpy as np
import pytest
import torch

from antidote_amd import abi, synth
from antidote_amd.devbatch import DeviceReads, materialize
from antidote_amd.oplog import HostLog, Op
from tests import randlog
from tests.test_gpu_lagcadence import _DownLog, check_batch

pytestmark = pytest.mark.gpu

NONE = abi.AM_NSPAN_NONE
RCAP = 2048  # AM_GRP_MAX_REC
NGRP_NONE = 0xFFFFFFFF  # AM_NGRP_NONE
T0 = 1_700_000_000_000_000
TYPES = [abi.AM_AWSET, abi.AM_MVREG]


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def d2h(mat, ptr, n, dt):
    a = np.zeros(max(n, 1), dt)
    abi.check(mat.L.am_memcpy_d2h(mat.ctx, a.ctypes.data, ptr, a.nbytes), "am_memcpy_d2h")
    return a[:n]


def no_spans(dlog):
    """The same device log with one span pointer nulled: the reads go through rec_g."""
    d = abi.am_op_log.from_buffer_copy(dlog)
    d.gspan = None
    return d


# ---------------------------------------------------------------- the view, from its definition
def key_records(log, k):
    """Key k's records in record order (op order; within an op MV: kills then the birth, AW per
    entry: births then kills): (op, is_kill, kill key, pair)."""
    if getattr(log, "_cols", None) is None:  # the columns as Python lists, once per log
        log._cols = tuple(np.asarray(x).tolist() for x in (log.key_off, log.op_meta, log.var_off, log.var_data,
                                                           log.p0, log.p1))
    key_off, op_meta, var_off, var_data, p0, p1 = log._cols
    t = int(log.key_type[k])
    a, b = key_off[k], key_off[k + 1]
    recs = []
    for p in range(a, b):
        meta = op_meta[p]
        if meta & 0x80:
            continue
        w = var_data[var_off[p]:var_off[p + 1]]
        if t == abi.AM_MVREG:
            recs += [(p - a, True, tok, None) for tok in w]
            if (meta >> 5) & 3 != 1:  # not a reset
                recs.append((p - a, False, p1[p], (p0[p], p1[p])))
        else:
            q = 0
            while q < len(w):
                e, na, nr = w[q], w[q + 1], w[q + 2]
                recs += [(p - a, False, (e, x), (e, x)) for x in w[q + 3:q + 3 + na]]
                recs += [(p - a, True, (e, x), None) for x in w[q + 3 + na:q + 3 + na + nr]]
                q += 3 + na + nr
    return recs


def key_spans(log, k, rank_of):
    """(NB or NONE, gspan words, gsrc words) of key k from the definition; rank_of: pair -> the
    group's output rank (from the device's grp)."""
    recs = key_records(log, k)
    n_ops = int(log.key_off[k + 1]) - int(log.key_off[k])
    births = {}
    for i, (op, kill, kk, _) in enumerate(recs):
        if not kill:
            if kk in births:
                return NONE, [], []  # a token born twice: ungrouped
            births[kk] = (op, i)
    if len(recs) > RCAP or n_ops >= 65535:
        return NONE, [], []
    kills = {}
    for op, kill, kk, _ in recs:
        if kill and kk in births and op > births[kk][0]:
            kills.setdefault(kk, []).append(op)
    if any(len(v) > 1 for v in kills.values()):
        return NONE, [], []
    gspan, gsrc = [], []
    for i, (op, kill, kk, pair) in enumerate(recs):
        if kill:
            continue
        gspan.append(op | (kills[kk][0] if kk in kills else op) << 16)
        gsrc.append(rank_of[pair] | i << 16)
    return len(gspan), gspan, gsrc


def check_view(mat, dlog, log, keys=None):
    """The device's span view of the keys against key_spans; returns (key_nspan, key_ngrp)."""
    nk = log.n_keys
    assert dlog.key_nspan and dlog.gspan and dlog.gsrc
    rko = d2h(mat, dlog.rec_key_off, nk + 1, np.uint64).astype(np.int64)
    rke = d2h(mat, dlog.rec_key_end, nk, np.uint64).astype(np.int64) if dlog.rec_key_end else rko[1:]
    n_rec = int(rko[-1])
    ngrp = d2h(mat, dlog.key_ngrp, nk, np.uint32)
    nspan = d2h(mat, dlog.key_nspan, nk, np.uint32)
    gspan = d2h(mat, dlog.gspan, n_rec, np.uint32)
    gsrc = d2h(mat, dlog.gsrc, n_rec, np.uint32)
    grp = d2h(mat, dlog.grp, 2 * n_rec, np.uint64)
    for k in (range(nk) if keys is None else keys):
        r0 = int(rko[k])
        if int(ngrp[k]) == NGRP_NONE or int(ngrp[k]) & 0x80000000:
            assert int(nspan[k]) == NONE, k
            continue
        G = int(ngrp[k])
        rank_of = {(int(grp[2 * (r0 + g)]), int(grp[2 * (r0 + g) + 1])): g for g in range(G)}
        nb, ws, wr = key_spans(log, k, rank_of)
        assert int(nspan[k]) == nb, (k, int(nspan[k]), nb)
        if nb != NONE:
            assert nb <= int(rke[k]) - r0
            assert [int(x) for x in gspan[r0:r0 + nb]] == ws, k
            assert [int(x) for x in gsrc[r0:r0 + nb]] == wr, k
    return nspan, ngrp


@pytest.mark.parametrize("t", TYPES)
def test_view_random_log(mat, t):
    rng = random.Random(9100 + t)
    lens = [0, 1, 3, 40, 65, 70, 97, 130, 300, 700] * 3
    keys = [randlog.rand_key_ops(rng, t, 3, n, t0=T0, bad_rate=0.02 if i % 5 == 0 else 0.0) for i, n in enumerate(lens)]
    log = HostLog(3, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        nspan, _ = check_view(mat, st.device_log(), log)
        assert (nspan != NONE).sum() >= 10
    finally:
        st.close()


@pytest.mark.parametrize("t,n_dc,ops,nk", [(abi.AM_AWSET, 8, 1024, 192), (abi.AM_MVREG, 3, 300, 256)])
def test_view_synthetic_log(mat, t, n_dc, ops, nk):
    p = synth.params(nk, n_dc, t, ops_per_key=ops)
    st = mat.synth_store(p)
    try:
        st.index(abi.AM_INDEX_NONE)
        nspan, ngrp = check_view(mat, st.device_log(), synth.host_log(p, 0, nk))
        # a causal log: every grouped key has spans
        assert ((nspan == NONE) == (ngrp == NGRP_NONE)).all() and (nspan != NONE).sum() > nk // 2
    finally:
        st.close()


# ---------------------------------------------------------------- hand-made logs
# events: ("add", elem | value, token, [tokens removed / overridden]), ("rm", elem, [tokens]),
# ("nop",); a trailing "x" marks an op that the split clock (below) excludes on its own
def effect(t, ev):
    if t == abi.AM_AWSET:
        return {"add": lambda: [(ev[1], [ev[2]], list(ev[3]))], "rm": lambda: [(ev[1], [], list(ev[2]))],
                "nop": lambda: [(50, [], [])]}[ev[0]]()
    return {"add": lambda: ("assign", ev[1], ev[2], list(ev[3])), "rm": lambda: ("reset", list(ev[2])),
            "nop": lambda: ("reset", [])}[ev[0]]()


def make_ops(t, n_dc, events, t0):
    """One op per event, 3 us apart, committed at DC 0; every remote entry is 5 (far below any
    clock) except DC 1's entry of an "x" op, its commit time - 1: the clock split() leaves such an
    op out and takes every other op."""
    ops = []
    for i, ev in enumerate(events):
        ct = t0 + 3 * (i + 1)
        x = ev[-1] == "x"
        snap = {d: (ct - 1 if d == 0 or (x and d == 1) else 5) for d in range(n_dc)}
        ops.append(Op(type=t, commit_dc=0, commit_time=ct, snap=snap, effect=effect(t, ev[:-1] if x else ev)))
    return ops


def nops(n):
    return [("nop",)] * n


def chain(n, n_elems, tok0=1000):
    """n adds, each of a new token of elem i % n_elems that removes the elem's previous token: every
    token has at most one kill and n_elems (at most n) survive."""
    ev, live = [], {}
    for i in range(n):
        e = i % n_elems
        ev.append(("add", e, tok0 + i, [live[e]] if e in live else []))
        live[e] = tok0 + i
    return ev


def case_events(t=abi.AM_AWSET):
    """The reader cases, one key each.  Two of them do not run in every instance:
    - "past_prefetch" is NB = 1100 for AW, past the 1024 prefetched span words (the second span
      pass).  An MV key of more than 1024 ops has the chunked view and no spans, so the MV key has
      NB = 1024: exactly the prefetched words, the second pass is AW's alone.
    - "kill_excluded" (and the fallback's "only the later kill included") needs a clock that is
      no prefix of the key's ops, which takes a second DC (clocks()): at D = 1 these keys read
      under prefix clocks only, the split clock runs at D = 3 and D = 8.
    AW has one key more, "long_bitmap" (an MV key over 1024 ops leaves this tier, as above): 2180
    ops, so its inclusion bitmap has more than 64 words -- the words past the prefetched 64 are
    staged straight from memory -- with births in the first and in the last of them."""
    n_long = 1100 if t == abi.AM_AWSET else 1024
    long_bitmap = {"long_bitmap": chain(40, 5) + nops(2100) + chain(40, 7, tok0=9000)} if t == abi.AM_AWSET else {}
    return {
        "no_groups": nops(70),
        "one_add": [("add", 1, 101, [])] + nops(66),
        "same_op_kill": [("add", 1, 101, [101])] + nops(70),
        "kill_before_birth": [("rm", 1, [101])] + nops(3) + [("add", 1, 101, [])] + nops(65),
        "unborn_kill": [("rm", 1, [999]), ("add", 1, 101, [])] + nops(63),
        "kill_excluded": [("add", 1, 101, []), ("nop",), ("rm", 1, [101], "x")] + nops(70),
        "len65": chain(65, 7), "len95": chain(95, 11), "len97": chain(97, 97), "len129": chain(129, 5),
        "nb255": chain(255, 40), "nb256": chain(256, 40), "nb257": chain(257, 40),
        "two_rounds": chain(300, 300),      # more than RLIST = 256 survivors
        "past_prefetch": chain(n_long, 900),  # AW: NB beyond the 1024 prefetched spans; 900 survive
        **long_bitmap,
    }


def hand_log(t, n_dc, events_by_key):
    keys = [make_ops(t, n_dc, ev, T0 + 17 * i) for i, ev in enumerate(events_by_key)]
    return keys, HostLog(n_dc, keys, key_types=[t] * len(keys))


def clocks(keys, n_dc):
    """Past every op; a prefix (half the time range); and, with a second DC, the split clock: DC 1
    at 10, past the ordinary ops' entry there and below every "x" op's."""
    lo = min(op.commit_time for ops in keys for op in ops)
    hi = max(op.commit_time for ops in keys for op in ops) + 10
    out = [[hi] * n_dc, [lo + (hi - lo) // 2] * n_dc]
    if n_dc > 1:
        out.append([hi, 10] + [hi] * (n_dc - 2))
    return out


COLS = ["status", "new_last_op", "last_ct", "last_ct_pres", "last_ct_ignore", "is_new_ss", "count", "flags"]


def raw_read(mat, dlog, n_dc, t, clock, sel, cap, types=None):
    kt = torch.tensor(list(sel), dtype=torch.int64, device="cuda")
    dr = DeviceReads(len(sel), n_dc, t, clock, set_cap=cap, keys=kt, types=types)
    torch.cuda.synchronize()
    materialize(mat, dlog, dr)
    mat.sync()
    h = dr.host()
    out = {c: h[c].copy() for c in COLS}
    sl = dr.set_len.cpu().numpy().copy()
    sa, sb = dr.set_a.cpu().numpy(), dr.set_b.cpu().numpy()
    ok = out["status"] == 0
    out["set_len"] = np.where(ok, sl, 0)
    out["pairs"] = [(sa[i * cap:i * cap + int(sl[i])].tolist(), sb[i * cap:i * cap + int(sl[i])].tolist()) if ok[i]
                    else None for i in range(len(sel))]
    return out


def same_as_records(mat, dlog, n_dc, t, clock, sel, cap, types=None):
    """The read through the spans and through rec_g: every result column equal."""
    a = raw_read(mat, dlog, n_dc, t, clock, sel, cap, types)
    b = raw_read(mat, no_spans(dlog), n_dc, t, clock, sel, cap, types)
    for c in COLS + ["set_len"]:
        assert np.array_equal(a[c], b[c]), (c, clock)
    assert a["pairs"] == b["pairs"], clock
    return a


def three_ways(mat, dlog, log, keys, t, n_dc, clock, cap, sel=None):
    sel = list(range(len(keys))) if sel is None else sel
    check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=cap, sel=sel)
    check_batch(mat, no_spans(dlog), log, keys, t, n_dc, clock, cap=cap, sel=sel)
    return same_as_records(mat, dlog, n_dc, t, clock, sel, cap)


@pytest.mark.parametrize("n_dc", [1, 3, 8])
@pytest.mark.parametrize("t", TYPES)
def test_reader_cases(mat, t, n_dc):
    cases = case_events(t)
    names = list(cases)
    keys, log = hand_log(t, n_dc, [cases[n] for n in names])
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        nspan, _ = check_view(mat, dlog, log)
        want = {"no_groups": 0, "one_add": 1, "same_op_kill": 1, "kill_before_birth": 1, "unborn_kill": 1,
                "kill_excluded": 1, "nb255": 255, "nb256": 256, "nb257": 257, "two_rounds": 300,
                "past_prefetch": 1100 if t == abi.AM_AWSET else 1024}
        if "long_bitmap" in names:
            want["long_bitmap"] = 80
        for n, nb in want.items():
            assert int(nspan[names.index(n)]) == nb, n
        # (the keys start at op slots 70, 137, 208, ...: most share bitmap words with their neighbours)
        ko = log.key_off.astype(np.int64)
        assert (ko[1:-1] % 32 != 0).sum() >= 10
        cl = clocks(keys, n_dc)
        split = cl[2] if n_dc > 1 else None
        if "long_bitmap" in names:  # (it doubles the keys' time range: the prefix of the others' range too)
            ko_l = ko[names.index("long_bitmap"):]
            assert ko_l[1] - ko_l[0] == 2180 and (ko_l[1] - 1) // 32 - ko_l[0] // 32 >= 64
            cl.append(clocks(keys[:names.index("long_bitmap")], n_dc)[1])
        for ci, clock in enumerate(cl):
            a = three_ways(mat, dlog, log, keys, t, n_dc, clock, 1024)
            sl = dict(zip(names, a["set_len"].tolist()))
            if ci == 0:  # past every op
                assert (sl["no_groups"], sl["one_add"], sl["same_op_kill"], sl["kill_before_birth"],
                        sl["unborn_kill"], sl["kill_excluded"]) == (0, 1, 1, 1, 1, 0)
                assert sl["two_rounds"] == 300 and sl["past_prefetch"] == 900 and sl["nb257"] == 40
                assert sl.get("long_bitmap", 12) == 12  # the first chain's 5 tokens and the last one's 7
            elif clock is split:  # the kill op alone is out: the token lives
                assert sl["kill_excluded"] == 1
        hi = clocks(keys, n_dc)[0]
        # capacity below the survivors: AM_ERR_CAPACITY for those reads, the others unchanged
        a = three_ways(mat, dlog, log, keys, t, n_dc, hi, 8)
        st8 = dict(zip(names, a["status"].tolist()))
        assert st8["two_rounds"] == abi.AM_ERR_CAPACITY and st8["nb256"] == abi.AM_ERR_CAPACITY and st8["one_add"] == 0
        # a subset of the keys, out of order
        sel = [names.index(n) for n in ("past_prefetch", "one_add", "len97", "kill_excluded", "nb256")]
        three_ways(mat, dlog, log, keys, t, n_dc, hi, 1024, sel=sel)
    finally:
        st.close()


def test_read_selection_mixed_types(mat):
    """A batch of AW and MV reads without a type hint: the planner hands each type's kernels a
    selection (S.idx) over its share of the reads."""
    n_dc = 3
    ev = [chain(70 + 3 * i, 5 + i) for i in range(12)] + [case_events()["kill_excluded"]]
    kt = [abi.AM_AWSET if i % 3 else abi.AM_MVREG for i in range(len(ev))]
    keys = [make_ops(kt[i], n_dc, e, T0 + 17 * i) for i, e in enumerate(ev)]
    log = HostLog(n_dc, keys, key_types=kt)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        check_view(mat, dlog, log)
        types = torch.tensor(kt, dtype=torch.uint8, device="cuda")
        for clock in clocks(keys, n_dc):
            a = same_as_records(mat, dlog, n_dc, 0, clock, range(len(keys)), 128, types=types)
            assert (a["status"] == 0).all()
            for t in TYPES:  # each type's reads alone (a type hint) give the same pairs, and the oracle's
                sel = [i for i in range(len(keys)) if kt[i] == t]
                check_batch(mat, dlog, log, keys, t, n_dc, clock, cap=128, sel=sel)
                b = raw_read(mat, dlog, n_dc, t, clock, sel, 128)
                assert b["pairs"] == [a["pairs"][i] for i in sel]
    finally:
        st.close()


# ---------------------------------------------------------------- fallback
@pytest.mark.parametrize("n_dc", [1, 3, 8])
@pytest.mark.parametrize("t", TYPES)
def test_fallback_two_kills(mat, t, n_dc):
    """Two ops remove one token (concurrent removes): the key has no spans and reads through rec_g
    in the batch of its neighbours, which have spans.  Under the split clock only the later kill is
    included."""
    twice = chain(40, 4) + [("rm", 0, [1036], "x"), ("nop",), ("rm", 0, [1036])] + nops(30)
    ev = [chain(80, 6), twice, chain(90, 9), chain(66, 66), twice, chain(70, 3)]
    keys, log = hand_log(t, n_dc, ev)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        nspan, _ = check_view(mat, dlog, log)
        assert [int(x) == NONE for x in nspan] == [False, True, False, False, True, False]
        for ci, clock in enumerate(clocks(keys, n_dc)):
            a = three_ways(mat, dlog, log, keys, t, n_dc, clock, 128)
            assert (a["status"] == 0).all()
            if ci != 1:  # past every op, and the split clock: the later kill is included, 3 of 4 elems left
                assert a["set_len"][1] == 3 and a["set_len"][4] == 3
    finally:
        st.close()


@pytest.mark.parametrize("t", TYPES)
def test_batch_edges(mat, t):
    """70 reads in one launch: the waves take 32, 32 and 6 of them.  Keys without spans sit at the
    batches' edges (reads 0, 31, 32, 69) and keys with more survivors than the capacity next to
    them (reads 1, 30, 32, 68): AM_ERR_CAPACITY for exactly those reads and every other read the
    oracle's, in order and with the selection reversed.  Read 32 is both: a key without spans
    whose survivors exceed the capacity."""
    n_dc, cap = 3, 8
    kills = [("rm", 0, [1036], "x"), ("nop",), ("rm", 0, [1036])] + nops(30)  # 1036: elem 0's newest token
    twice, twice_big = chain(40, 4) + kills, chain(40, 12) + kills            # 3 and 11 survivors
    fallback, over = (0, 31, 32, 69), (1, 30, 32, 68)
    ev = [chain(66 + 7 * i % 65, 3 + i % 6) for i in range(70)]  # 66 - 130 ops, 3 - 8 survivors
    for i in over:
        ev[i] = chain(66 + 7 * i % 65, 20)
    for i in fallback:
        ev[i] = twice_big if i in over else twice
    keys, log = hand_log(t, n_dc, ev)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        dlog = st.device_log()
        nspan, _ = check_view(mat, dlog, log)
        assert [i for i in range(70) if int(nspan[i]) == NONE] == list(fallback)
        hi = clocks(keys, n_dc)[0]
        fwd = three_ways(mat, dlog, log, keys, t, n_dc, hi, cap)
        assert [i for i in range(70) if fwd["status"][i] == abi.AM_ERR_CAPACITY] == sorted(over)
        assert all(fwd["status"][i] == 0 for i in range(70) if i not in over)
        assert fwd["set_len"][0] == 3 and fwd["set_len"][31] == 3 and fwd["set_len"][69] == 3
        rev = three_ways(mat, dlog, log, keys, t, n_dc, hi, cap, sel=list(range(69, -1, -1)))
        assert rev["status"].tolist() == fwd["status"].tolist()[::-1] and rev["pairs"] == fwd["pairs"][::-1]
    finally:
        st.close()


# ---------------------------------------------------------------- apply
@pytest.mark.parametrize("t", TYPES)
def test_apply_keeps_spans(mat, t):
    """A reserved store: appends of births and single kills keep the spans current; an append that
    kills a token a second time flips its key to the sentinel; a GC prune leaves a readable key."""
    n_dc, nk = 3, 12
    ev = [chain(70 + i, 4 + i) for i in range(nk)]
    hist = []
    for i in range(nk):
        last = 1000 + 70 + i - 1  # the newest token (of elem (69 + i) % (4 + i))
        e = (69 + i) % (4 + i)
        dead = 1000  # elem 0's first token, killed by elem 0's second add
        if i % 3 == 1:    # a second effective kill of a token already removed
            extra = [("add", e, 5000 + i, [last]), ("rm", 0, [dead])]
        elif i % 3 == 2:  # births and single kills
            extra = [("add", e, 5000 + i, [last]), ("rm", e, [5000 + i])]
        else:
            extra = []
        hist.append(make_ops(t, n_dc, ev[i] + extra, T0 + 17 * i))
    keys = [hist[i][:len(ev[i])] for i in range(nk)]
    log0 = HostLog(n_dc, keys, key_types=[t] * nk)
    base = mat.store(log0)
    st = base.reserve()
    try:
        st.index(abi.AM_INDEX_NONE)
        assert (check_view(mat, st.device_log(), log0)[0] != NONE).all()
        touched = [i for i in range(nk) if i % 3]
        new_ops = [hist[i][len(ev[i]):] for i in touched]
        ok, _ = st.apply(touched, new_log=HostLog(n_dc, new_ops, key_types=[t] * len(touched)))
        assert ok
        merged = [hist[i] if i % 3 else keys[i] for i in range(nk)]
        mlog = HostLog(n_dc, merged, key_types=[t] * nk)
        dlog = st.device_log()
        nspan, _ = check_view(mat, dlog, mlog)
        for i in range(nk):
            assert (int(nspan[i]) == NONE) == (i % 3 == 1), i
            if i % 3 == 2:
                assert int(nspan[i]) == len(ev[i]) + 1
        for clock in clocks(merged, n_dc)[:2]:
            three_ways(mat, dlog, mlog, merged, t, n_dc, clock, 128)
        # GC: key 3 (untouched so far) pruned to its newer half, key 5 appended to again
        cut = len(merged[3]) // 2
        mask = np.zeros(nk, np.uint8)
        thr_vc = np.zeros((n_dc, nk), np.uint64)
        thr_pres = np.zeros(nk, np.uint32)
        mask[3], thr_vc[:, 3], thr_pres[3] = 1, merged[3][cut].commit_time, (1 << n_dc) - 1
        more = make_ops(t, n_dc, [("add", 0, 7000, [])], merged[5][-1].commit_time)
        ok, _ = st.apply([3, 5], new_log=HostLog(n_dc, [[], more], key_types=[t] * 2), prune=(mask, thr_vc, thr_pres))
        assert ok
        merged[3], merged[5] = merged[3][cut + 1:], merged[5] + more
        D = st.download()
        assert [int(x) for x in np.diff(D["key_off"].astype(np.int64))] == [len(m) for m in merged]
        dl = _DownLog(D, n_dc)
        dl.key_type, dl.var_off, dl.var_data, dl.p0, dl.p1 = D["key_type"], D["var_off"], D["var_data"], D["p0"], D["p1"]
        dlog = st.device_log()
        nspan, _ = check_view(mat, dlog, dl)
        assert int(nspan[3]) != NONE and int(nspan[5]) == len(ev[5]) + 2
        for clock in clocks(merged, n_dc)[:2]:
            check_batch(mat, dlog, dl, merged, t, n_dc, clock, cap=128)
            check_batch(mat, no_spans(dlog), dl, merged, t, n_dc, clock, cap=128)
            same_as_records(mat, dlog, n_dc, t, clock, range(nk), 128)
    finally:
        st.close()
        base.close()
