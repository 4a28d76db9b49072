"""The hand-made logs of tests/bigexits.py have the shape that makes each exit of the big-read tier
reachable, and the oracle alone answers every read of tests/test_gpu_big_exits.py with ok / the
stated error at the capacities that module uses (no capacity error stands in for a value).  No GPU:
the preconditions are computed from the ops and the read clock by the models of bigexits."""
import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostBatch, HostLog, Read
from oracle import amo
from tests import bigexits as bx
from tests.bigexits import AW, BC, MV, PN

N_DC = 3
OVF = ("error", abi.AM_ERR_OVERFLOW)
CAPERR = ("error", abi.AM_ERR_CAPACITY)


def oracle(n_dc, ops, t, clock, cap, base=None):
    """The oracle's result of one read of a one-key log; base = (clock dict, last op, value)."""
    log = HostLog(n_dc, [ops], key_types=[t])
    rd = Read(0, t, {d: clock[d] for d in range(n_dc)})
    if base is not None:
        rd = Read(0, t, rd.clock, None, base[0], base[1], base[2])
    return amo.materialize(log, HostBatch(n_dc, [rd], [cap])).result(0)


def three_clocks(ops, mid, n_dc=N_DC):
    return [bx.clock_after(ops, m, n_dc) for m in (len(ops), 0, mid)]


def test_mirrored_constants():
    """The mirrors agree with the sources they name (a changed kernel constant must change them)."""
    import os
    import re
    root = os.path.join(os.path.dirname(__file__), "..")
    big = open(os.path.join(root, "antidote_amd", "csrc", "am_big.hip")).read()
    for name, val in (("LB", bx.LB), ("LK", bx.LK), ("SCAP", bx.SCAP), ("HPROBES", bx.HPROBES)):
        assert re.search(r"constexpr uint32_t %s = %d;" % (name, val), big), name
    assert "constexpr uint32_t GH = LK;" in big and "for (uint32_t pr = 0; pr < 32; ++pr)" in big
    assert "return (g * 0x9E3779B1u) >> 21;" in big and "constexpr int OPL = 4;" in big
    assert "constexpr int SBLOCK = 256;" in open(os.path.join(root, "antidote_amd", "csrc", "am_block.h")).read()
    internal = open(os.path.join(root, "antidote_amd", "csrc", "am_internal.h")).read()
    assert "AM_BCWAVE_OPS = %d;" % bx.AM_BCWAVE_OPS in internal and "AM_SETS_BIG_OPS = %d;" % bx.AM_SETS_BIG_OPS in internal
    plan = open(os.path.join(root, "antidote_amd", "csrc", "am_plan.hip")).read()
    assert "ROWS_SCALAR = %d, ROWS_BC = %d;" % (bx.ROWS_SCALAR, bx.ROWS_BC) in plan
    hdr = open(os.path.join(root, "include", "antidote_mat.h")).read()
    assert "#define AM_GRP_MAX_REC 2048u" in hdr and "#define AM_BIG_MIN_OPS (AM_GRP_MAX_REC / 2)" in hdr
    assert bx.AM_BIG_MIN_OPS == 1024 and bx.CHUNK == 256 * 4


def test_aw_births_overflow_shape():
    ops = bx.aw_births_overflow(N_DC)
    assert len(ops) > bx.AM_SETS_BIG_OPS
    for clock, full_chunks in zip(three_clocks(ops, 2600), (4, 0, 2)):
        incl = bx.included(ops, clock)
        per = bx.list_overflow_witnesses(AW, ops, incl, "births")
        for c, (nb, nk, wit) in enumerate(per):
            assert nk <= bx.LK, (c, nk)
            if c < full_chunks:  # 4 x LB births; most of the chunk's own kills hit exported births
                assert nb == 4 * bx.LB and len(wit) >= 400, (c, nb, len(wit))
        if full_chunks:
            # kills of an earlier chunk's tokens: chunk 2 holds ops 2048 .. 3071, op 2100 kills op 1000's
            chunks = bx.chunk_records(AW, ops, incl)
            born = {b: p for bs, _ in chunks for p, b in bs}
            cross = [k for p, k in chunks[1][1] + chunks[2][1]
                     if (k[1], k[0]) in born and born[(k[1], k[0])] // bx.CHUNK < p // bx.CHUNK]
            assert len(cross) >= 100, len(cross)
        surv = bx.survivors(AW, ops, incl)
        births = sum(nb for nb, _, _ in per)
        assert (births == 0 and not surv) or 0 < len(surv) < births  # survivors and dead births
        r = oracle(N_DC, ops, AW, clock, 16384)
        assert r[0] == "ok" and set(r[1]) == surv and len(r[1]) == len(surv), (r[0], len(surv))


def test_aw_kills_overflow_shape():
    ops = bx.aw_kills_overflow(N_DC)
    assert len(ops) > bx.AM_SETS_BIG_OPS
    for clock, full_chunks in zip(three_clocks(ops, 2600), (4, 0, 2)):
        incl = bx.included(ops, clock)
        per = bx.list_overflow_witnesses(AW, ops, incl, "kills")
        for c, (nb, nk, wit) in enumerate(per):
            assert nb <= bx.LB, (c, nb)
            if c < full_chunks:  # 3 kills per op; the last third of the chunk's kills finds the list full
                assert nk == 3 * bx.CHUNK > bx.LK and len(wit) >= 200, (c, nk, len(wit))
        surv = bx.survivors(AW, ops, incl)
        births = sum(nb for nb, _, _ in per)
        assert (births == 0 and not surv) or 0 < len(surv) < births
        if full_chunks == 4:  # the kinds of removed tokens: same chunk, earlier chunks, never born
            kills = [k for _, ks in bx.chunk_records(AW, ops, incl) for _, k in ks]
            assert sum(k[0] >= bx.NEVER for k in kills) > 4000
            # tokens j % 5 == 2: no op of their own chunk removes them
            assert sum(k[0] < bx.NEVER and (k[0] - bx.TOK) % 5 == 2 for k in kills) > 1000
        r = oracle(N_DC, ops, AW, clock, 4096)
        assert r[0] == "ok" and set(r[1]) == surv and len(r[1]) == len(surv), (r[0], len(surv))


@pytest.mark.parametrize("born_twice", [True, False])
def test_mv_hash_overflow_shape(born_twice):
    ops = bx.mv_hash_overflow(N_DC, born_twice=born_twice)
    assert 2 * bx.CHUNK < len(ops) <= 3 * bx.CHUNK
    toks = [op.effect[2] for op in ops]
    assert (len(set(toks)) < len(toks)) == born_twice
    for clock, full_chunks in zip(three_clocks(ops, 1500), (2, 0, 1)):
        incl = bx.included(ops, clock)
        per = bx.mv_hash_failures(ops, incl)
        for c, (distinct, failed, wit) in enumerate(per):
            if c < full_chunks:  # more tokens than slots: at least distinct - LK kills leave the table
                assert distinct > bx.LK + 500 and len(failed) >= distinct - bx.LK and len(wit) >= 50, (c, distinct, len(wit))
        surv = bx.survivors(MV, ops, incl)
        assert (not any(incl) and not surv) or 50 < len(surv) < sum(incl) - 100
        r = oracle(N_DC, ops, MV, clock, 1024)
        assert r[0] == "ok" and r[1] == sorted(surv), (r[0], len(surv))
    # the cached-base variant: the base is the read after 40 ops (it has pairs), the second read
    # includes every later op, two full chunks' worth of kills among them
    if not born_twice:
        c0 = bx.clock_after(ops, 40, N_DC)
        first = oracle(N_DC, ops, MV, c0, 1024)
        assert first[0] == "ok" and len(first[1]) >= 3
        r = oracle(N_DC, ops, MV, bx.clock_after(ops, len(ops), N_DC), 1024, base=(first[3], first[2], first[1]))
        assert r[0] == "ok" and r[1] == sorted(bx.survivors(MV, ops, bx.included(ops, bx.clock_after(ops, len(ops), N_DC))))
        assert r[5] == len(ops) - 40  # ops applied over the base


GSET_MID = bx.GSET_CHUNK * bx.CHUNK + 170  # inside chunk 3: the window's births and about 40 of its kills


def test_mv_gset_overflow_shape():
    s0, win = bx.gset_window(bx.GSET_OPS)
    m = len(win)
    reach = 2 * bx.GPROBES - 1
    assert m >= bx.GSET_KILLED + bx.GSET_LATER + 5 and m > reach + 30, m  # about 127 ids for 63 slots
    assert all((bx.gslot(g) - s0) % bx.GH < bx.GPROBES for g in win)
    ops = bx.mv_gset_overflow(N_DC)
    assert len(ops) == bx.GSET_OPS
    assert sorted(op.effect[1] for op in ops) == list(range(bx.GSET_OPS))      # group id = value
    assert len({op.effect[2] for op in ops}) == bx.GSET_OPS                     # no token twice: grouped
    for clock, kills in zip(three_clocks(ops, GSET_MID), (bx.GSET_KILLED, 0, GSET_MID - bx.GSET_CHUNK * bx.CHUNK - m)):
        incl = bx.included(ops, clock)
        fails = bx.gset_failures(ops, incl)
        if any(incl):
            chunk = bx.chunk_records(MV, ops, incl)[bx.GSET_CHUNK]
            nwin = sum(b[0] in set(win) for _, b in chunk[0])
            assert nwin == m and fails[bx.GSET_CHUNK][0] >= m - reach, fails[bx.GSET_CHUNK]  # for every insertion order
            w0 = bx.TOK + bx.GSET_CHUNK * bx.CHUNK  # the window's tokens: [w0, w0 + m)
            wkills = sum(1 for _, k in chunk[1] if w0 <= k[0] < w0 + m)
            assert wkills == kills
            if kills > reach:
                assert fails[bx.GSET_CHUNK][1] >= kills - reach
            assert all(f == (0, 0) for c, f in enumerate(fails) if c != bx.GSET_CHUNK), fails  # ordinary chains
        surv = bx.survivors(MV, ops, incl)
        assert (not any(incl) and not surv) or 20 < len(surv) < sum(incl) - 100
        if sum(incl) == len(ops):  # the window's tokens: 80 + 20 dead, the rest alive
            alive = sum(1 for v, _ in surv if v in set(win))
            assert alive == m - bx.GSET_KILLED - bx.GSET_LATER
        r = oracle(N_DC, ops, MV, clock, 1024)
        assert r[0] == "ok" and r[1] == sorted(surv), (r[0], len(surv))


SURVIVORS = [bx.SCAP, bx.SCAP + 1, 3000]
BASE_OPS = 500  # the base of the many-survivor reads: the read after 500 ops


@pytest.mark.parametrize("n", SURVIVORS)
@pytest.mark.parametrize("t", [AW, MV])
def test_many_survivors_shape(t, n):
    ops = (bx.aw_many_survivors if t == AW else bx.mv_many_survivors)(n, N_DC)
    assert len(ops) > bx.AM_SETS_BIG_OPS
    full = bx.clock_after(ops, len(ops), N_DC)
    incl = bx.included(ops, full)
    surv = bx.survivors(t, ops, incl)
    births = sum(len(bx.records(t, op)[0]) for op in ops)
    assert len(surv) == n < births
    r = oracle(N_DC, ops, t, full, n)
    assert r[0] == "ok" and len(r[1]) == n and set(r[1]) == surv
    assert oracle(N_DC, ops, t, full, n - 1) == CAPERR
    if t == AW:  # elements with many live tokens, from different ops and two from one op
        per = {}
        for e, x in r[1]:
            per.setdefault(e, []).append(x)
        assert len(per) == 5 and min(len(v) for v in per.values()) > 300
        assert any(x % 2 == 1 and x - 1 in v for v in per.values() for x in v)
    else:        # equal values under different tokens
        assert len({v for v, _ in r[1]}) <= 50
    # over the base taken after BASE_OPS ops: the same survivors, base pairs among them
    first = oracle(N_DC, ops, t, bx.clock_after(ops, BASE_OPS, N_DC), n)
    assert first[0] == "ok" and len(first[1]) > 100
    base = (first[3], first[2], first[1])
    rb = oracle(N_DC, ops, t, full, n, base=base)
    assert rb[0] == "ok" and rb[1] == r[1] and rb[5] == len(ops) - BASE_OPS
    assert len(set(first[1]) & surv) > 100  # base pairs that survive
    assert oracle(N_DC, ops, t, full, n - 1, base=base) == CAPERR
    # the middle clock of the GPU module
    mid = bx.clock_after(ops, 2600, N_DC)
    rm = oracle(N_DC, ops, t, mid, 4096)
    assert rm[0] == "ok" and set(rm[1]) == bx.survivors(t, ops, bx.included(ops, mid))


PN_LENS = [3, 40, 64, 65, 700]
BC_LENS = [40, 48, 49, 300, 4096, 4097, 5000]
BASE0 = {d: 0 for d in range(N_DC)}  # a base clock below every op: the read applies every included op


@pytest.mark.parametrize("n_ops", PN_LENS)
def test_pn_edge_keys(n_ops):
    keys = bx.pn_edge_keys(n_ops, N_DC)
    assert {k["name"] for k in keys} == set(bx.edge_sums(n_ops)) | {"base_max", "base_min"}
    pos = set(bx.edge_positions(n_ops))
    planted = set()
    for k in keys:
        ops = k["ops"]
        assert len(ops) == n_ops
        big = [p for p, op in enumerate(ops) if abs(op.effect) > 1000]
        planted |= set(big)
        assert sum(op.effect for op in ops) + (k["base"] or 0) == k["total"]
        base = None if k["base"] is None else (BASE0, 0, k["base"])
        r = oracle(N_DC, ops, PN, bx.clock_after(ops, n_ops, N_DC), 1, base=base)
        assert r == OVF if k["want"] == "overflow" else (r[0] == "ok" and r[1] == k["total"]), (k["name"], r)
        if k["name"] == "climb" and n_ops >= 11:  # the running sum passes 2^65
            run = peak = 0
            for op in ops:
                run += op.effect
                peak = max(peak, run)
            assert peak > 1 << 65 and k["total"] == 7
    totals = {k["name"]: k["total"] for k in keys}
    assert totals["max_ok"] == bx.INT64_MAX and totals["max_ovf"] == bx.INT64_MAX + 1
    assert totals["min_ok"] == bx.INT64_MIN and totals["min_ovf"] == bx.INT64_MIN - 1
    assert totals["p64"] == 1 << 64 and totals["m64"] == -(1 << 64)
    assert totals["base_max"] == bx.INT64_MAX - 5 and totals["base_min"] == bx.INT64_MIN + 5
    if len(pos) >= 3:  # the boundaries are used: both sides of some 256-op boundary hold an edge amount
        assert {0, n_ops - 1} <= planted and any(b - 1 in planted and b in planted for b in range(256, n_ops, 256))


@pytest.mark.parametrize("n_dc", [3, 13, 17])
@pytest.mark.parametrize("n_ops", BC_LENS)
def test_bc_edge_keys(n_ops, n_dc):
    keys = bx.bc_edge_keys(n_ops, n_dc)
    names = [k["name"] for k in keys]
    assert set(names) >= set(bx.edge_sums(n_ops)) | {"neg", "defer", "nodefer", "flush", "base_max", "base_max_ovf",
                                                     "base_neg", "base_neg_ovf"}
    np_ = n_dc * n_dc
    assert {k["slot"] for k in keys} == {1, np_ - 1, np_ + n_dc - 1}
    full = [bx.T0 + 3 * n_ops] * n_dc
    reads, caps = [], []
    for i, k in enumerate(keys):
        base = k["base"]
        bclock = None if base is None else {d: 0 for d in range(n_dc)}
        reads.append(Read(i, BC, {d: full[d] for d in range(n_dc)}, None, bclock, 0, base))
        caps.append(np_ + n_dc)
    log = HostLog(n_dc, [k["ops"] for k in keys], key_types=[BC] * len(keys))
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    for i, k in enumerate(keys):
        ops, slot = k["ops"], k["slot"]
        incl = [True] * n_ops
        b0 = 0
        if k["base"] is not None:
            pd, dd = k["base"]
            b0 = dd[slot - np_] if slot >= np_ else pd[divmod(slot, n_dc)]
        assert bx.bc_slot_sum(n_dc, ops, incl, slot, b0) == k["total"], k["name"]
        small = {}
        for op in ops:
            s = bx.bc_slot_of(n_dc, op.effect)
            small[s] = small.get(s, 0) + op.effect[1]
        assert all(0 <= x <= 50 * n_ops for s, x in small.items() if s != slot)
        r = ref.result(i)
        if k["want"] == "overflow":
            assert r == OVF, (k["name"], r)
        else:
            assert r[0] == "ok", (k["name"], r)
            pd, dd = r[1]
            got = dd[slot - np_] if slot >= np_ else pd[divmod(slot, n_dc)]
            assert got == k["total"], (k["name"], got)
    by = dict(zip(names, keys))
    amounts = lambda k: [op.effect[1] for op in k["ops"]]  # noqa: E731
    assert bx.DEFER in amounts(by["defer"]) and max(amounts(by["nodefer"])) == bx.DEFER - 1
    assert by["neg"]["total"] == -3 and min(amounts(by["neg"])) < 0
    at = [p for p, op in enumerate(by["flush"]["ops"]) if op.effect[1] == 1 << 62]
    assert len(at) == 4 and by["flush"]["total"] == 1 << 64
    if n_ops > bx.AM_BCWAVE_OPS:  # four different chunks, each chunk's own sum within 64 bits
        assert len({p // bx.CHUNK for p in at}) == 4
