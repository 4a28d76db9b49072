"""Downstream generation on the device (am_generate_downstream / _host, am_update_objects_*):
clocksi_downstream:generate_downstream_op/6 for a batch, the states never leaving the GPU.

The expected effect comes from the restatement below: tests/dcsim.downstream for what it covers
(PN, add-wins-set add / remove, MV assign, the bounded counter with bcounter_mgr's permission
check), extended here for what no suite issues -- add-wins-set reset ({E, [], Tokens} per element
in state order), MV reset ({reset, Tokens}), LWW assign ({Ts, Value}) -- and for the statuses of
include/antidote_mat.h.  Comparison is on the decoded effect, token order included."""
import ctypes
import os
import random
from collections import Counter

import numpy as np
import pytest

from antidote_amd import abi
from antidote_amd.oplog import Effects, HostBatch, Op, Read, Updates, WriteSet
from oracle import ref_materializer as R
from tests import dcsim, randlog
from tests.kat_util import load

pytestmark = pytest.mark.gpu

PN, LWW, AW, MV, BC = abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BASES = (0, 1, 63, 64, 65, 255, 256, 257, 1027)
COUNTS = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def err(st):
    return ("error", st)


# ---- the restatement ----
def ref_downstream(t, upd, value, n_dc, toks):
    """(effect | ('error', status), avail) of one update on a value in HostBatch.value's shape;
    toks: the fresh tokens the update takes, in order."""
    it = iter(toks)
    token = lambda: next(it)  # noqa: E731
    op = upd[0]
    if t == PN:
        if op == "decrement" and upd[1] == I64_MIN:
            return err(abi.AM_ERR_OVERFLOW), 0
        return dcsim.downstream(PN, op, upd[1], None, 0, token), 0
    if t == LWW:
        return (upd[1], upd[2]), 0
    state = randlog.base_state_term(t, value)
    if t == AW:
        if op == "reset":
            return [(e, [], list(tk)) for e, tk in state], 0
        return dcsim.downstream(AW, op, upd[1], state, 0, token), 0
    if t == MV:
        if op == "reset":
            return ("reset", [tk for _, tk in state]), 0
        return dcsim.downstream(MV, op, upd[1], state, 0, token), 0
    assert t == BC
    if op == "transfer":
        amount, to, frm = upd[1]
        dc, arg = frm, (amount, to, frm)
        if to >= n_dc:
            return err(abi.AM_ERR_INVALID), 0
    else:
        amount, dc = upd[1]
        arg = amount
        if op == "increment" and amount < 0:   # src/bcounter_mgr.erl:89-90
            if amount == I64_MIN:
                return err(abi.AM_ERR_OVERFLOW), 0
            op, amount, arg = "decrement", -amount, -amount
    if dc >= n_dc or amount <= 0:
        return err(abi.AM_ERR_INVALID), 0
    if op == "increment":
        return dcsim.downstream(BC, op, arg, state, dc, token), 0
    avail = dcsim.local_permissions(dc, state)
    if not I64_MIN <= avail <= I64_MAX:
        return err(abi.AM_ERR_OVERFLOW), 0
    try:
        return dcsim.downstream(BC, op, arg, state, dc, token), avail
    except dcsim.NoPermissions:
        return err(abi.AM_ERR_NO_PERMISSIONS), avail


def expected(n_dc, values, ups: Updates, in_status=None):
    out, av = [], []
    for i, (row, t, upd) in enumerate(ups.entries):
        if in_status is not None and in_status[row] != 0 and t not in (PN, LWW):
            e, a = err(int(in_status[row])), 0
        else:
            e, a = ref_downstream(t, upd, values[row][1], n_dc, ups.tokens[i])
        out.append(e)
        av.append(a)
    return out, av


def check_invariant(eff: Effects):
    """Every failed update has zero words and AM_META_BAD; offsets are a scan ending at n_var."""
    n = eff.n_up
    assert list(eff.eff_off) == list(range(n + 1))
    assert int(eff.var_off[0]) == 0
    for i in range(n):
        assert int(eff.var_off[i]) <= int(eff.var_off[i + 1])
        if eff.status[i] != 0:
            assert int(eff.var_off[i]) == int(eff.var_off[i + 1]) and eff.eff_meta[i] & abi.AM_META_BAD, i
        else:
            assert not eff.eff_meta[i] & abi.AM_META_BAD, i
    if int(eff.n_var[0]) <= eff.var_cap:
        assert int(eff.var_off[n]) == int(eff.n_var[0])


def run(mat, n_dc, values, entries, in_status=None, var_cap=None, tokens=None):
    fresh = iter(range(10 ** 9, 2 * 10 ** 9))
    ups = Updates(entries, tokens or (lambda: next(fresh)))
    effs, avail, eff = mat.generate_downstream(n_dc, values, ups, in_status=in_status, var_cap=var_cap)
    check_invariant(eff)
    return ups, effs, avail, eff


# ---- bases ----
def aw_base(n, rng):
    """n (elem, token) pairs, elements ascending from 10 in steps of 3 (so absent elements lie
    between, below and above); at n >= 100 one element holds a 70-token run: pairs [187 or 200,
    +70) across the 256-pair boundary at n >= 257, pairs [30, 100) across the 64-pair one else."""
    long_at = min(200, n - 70) if n >= 257 else 30 if n >= 100 else None
    pairs, e, tok = [], 10, 5000
    while len(pairs) < n:
        run = 70 if len(pairs) == long_at else rng.choice([1, 1, 1, 2, 3])
        if long_at is not None and len(pairs) < long_at:
            run = min(run, long_at - len(pairs))
        for _ in range(min(run, n - len(pairs))):
            tok += rng.randint(1, 9)
            pairs.append((e, tok * 7919 % 100003))   # tokens in no order
        e += 3
    return pairs


def mv_base(n, rng):
    return sorted((rng.randint(0, 40), 7000 + i) for i in range(n))


def pick_elems(base, ne, rng):
    """ne distinct elements: the 70-token one, the base's first and last, one below and one above
    them, the label extremes, then a mix of present and absent ones."""
    count = Counter(e for e, _ in base)
    have = sorted(count)
    lo, hi = (have[0], have[-1]) if have else (10, 10)
    cand = [e for e in have if count[e] == 70] + [lo, hi, lo - 1, hi + 1, 0, 2 ** 64 - 1]
    must = list(dict.fromkeys(cand))[:ne]
    pool = [x for x in range(1, hi + 3 * ne + 10) if x not in set(must)]
    return must + rng.sample(pool, ne - len(must))


@pytest.fixture(scope="module")
def edge_run(mat):
    """One call over every base size x element count x {add, remove}, plus reset and MV assign /
    reset over every base: the shared result of the edge tests."""
    rng = random.Random(4242)
    values, entries = [], []
    for n in BASES:
        base = aw_base(n, rng)
        for ne in COUNTS:
            for op in ("add_all", "remove_all"):
                entries.append((len(values), AW, (op, pick_elems(base, ne, rng))))
                values.append((AW, base))
        entries.append((len(values), AW, ("reset",)))
        values.append((AW, base))
        m = mv_base(n, rng)
        for upd in (("assign", 9), ("reset",)):
            entries.append((len(values), MV, upd))
            values.append((MV, m))
    ups, effs, avail, eff = run(mat, 2, values, entries)
    return values, ups, effs, eff


def test_gpu_downstream_add_remove_over_base_and_count_edges(edge_run):
    values, ups, effs, eff = edge_run
    exp, _ = expected(2, values, ups)
    seen = set()
    for i, (row, t, upd) in enumerate(ups.entries):
        if t == AW and upd[0] != "reset":
            assert effs[i] == exp[i], (i, len(values[row][1]), upd[0], len(upd[1]))
            seen.add((len(values[row][1]), len(effs[i]), upd[0]))
            if len(values[row][1]) >= 100 and len(upd[1]) >= 1:   # the 70-token run came whole, in state order
                assert any(len(rm) == 70 for _, _, rm in effs[i])
    assert seen == {(n, c, op) for n in BASES for c in COUNTS for op in ("add_all", "remove_all")}
    assert (eff.status[:eff.n_up] == 0).all() and int(eff.n_var[0]) == int(eff.var_off[eff.n_up])


def test_gpu_downstream_reset_and_mv_assign_over_every_base(edge_run):
    values, ups, effs, _ = edge_run
    exp, _ = expected(2, values, ups)
    sizes = {AW: [], MV: []}
    for i, (row, t, upd) in enumerate(ups.entries):
        if upd[0] == "reset" or t == MV:
            assert effs[i] == exp[i], (i, t, upd, len(values[row][1]))
            sizes[t].append(len(values[row][1]))
            if not values[row][1]:   # an empty base: the empty list / no overridden tokens
                assert effs[i] == ([] if t == AW else ("reset", []) if upd[0] == "reset" else
                                   ("assign", 9, ups.tokens[i][0], []))
    assert sizes[AW] == list(BASES) and sizes[MV] == [n for n in BASES for _ in range(2)]


# ---- bounded counter ----
def bc_values(n_dc, rng):
    out = []
    for _ in range(12):
        p = {(f, t): rng.randint(0, 50) for f in range(n_dc) for t in range(n_dc) if rng.random() < 0.6}
        d = {i: rng.randint(0, 30) for i in range(n_dc) if rng.random() < 0.6}
        out.append((p, d))
    out.append(({}, {}))
    out.append(({(0, 0): 5}, {0: 9}))                                   # negative permissions
    if n_dc >= 2:
        big = I64_MAX
        # partial sums leave int64, the result fits: 2 big in, 1 big out, 1 big - 7 decremented
        out.append(({(0, 0): big, (1, 0): big, (0, 1): big}, {0: big - 7}))
        out.append(({(0, 0): I64_MIN, (1, 0): big, (0, 1): I64_MIN + 5}, {0: 3}))   # -(INT64_MIN + 5) is exact
        out.append(({(0, 0): big, (1, 0): big}, {}))                    # 2^64 - 2: outside int64
        out.append(({(0, 0): I64_MIN}, {0: 1}))                         # below INT64_MIN
    else:
        out.append(({(0, 0): I64_MAX}, {0: I64_MIN}))                   # 2^63 - 1 + 2^63: outside int64
    return out


@pytest.mark.parametrize("n_dc", [1, 3, 16, 32])
def test_gpu_downstream_bounded_counter(mat, n_dc):
    rng = random.Random(100 + n_dc)
    states = bc_values(n_dc, rng)
    values, entries = [], []

    def add(state, upd):
        entries.append((len(values), BC, upd))
        values.append((BC, state))
    for s in states:
        term = randlog.base_state_term(BC, s)
        for dc in sorted({0, n_dc - 1, rng.randrange(n_dc)}):
            av = dcsim.local_permissions(dc, term)
            to = (dc + 1) % n_dc
            for n in {av, av + 1, 1, max(av - 1, 1)}:
                if I64_MIN <= n <= I64_MAX:
                    add(s, ("decrement", (n, dc)))
                    add(s, ("transfer", (n, to, dc)))
            add(s, ("increment", (7, dc)))
            add(s, ("increment", (-max(min(av, I64_MAX), 1), dc)))      # a decrement of exactly avail
            add(s, ("increment", (-3, dc)))
    s0 = states[0]
    for upd in (("increment", (0, 0)), ("decrement", (0, 0)), ("decrement", (-5, 0)), ("increment", (I64_MIN, 0)),
                ("decrement", (1, n_dc)), ("increment", (1, n_dc)), ("transfer", (1, n_dc, 0)), ("transfer", (1, 0, n_dc)),
                ("transfer", (0, 0, 0))):
        add(s0, upd)
    ups, effs, avail, eff = run(mat, n_dc, values, entries)
    exp, exp_av = expected(n_dc, values, ups)
    assert effs == exp
    assert avail == exp_av   # dcsim.local_permissions for every decrement and transfer
    got = {e[1] if isinstance(e, tuple) and e[0] == "error" else 0 for e in effs}
    assert {0, abi.AM_ERR_NO_PERMISSIONS, abi.AM_ERR_OVERFLOW, abi.AM_ERR_INVALID} <= got
    kinds = {e[0] for e in effs if e[0] != "error"}
    assert kinds == ({"increment", "decrement", "transfer"})
    if n_dc >= 2:   # the exact near-2^63 sums came out as numbers, and were granted at N == avail
        i = next(k for k, (r, _, u) in enumerate(ups.entries) if values[r][1] is states[-4] and u == ("decrement", (7, 0)))
        assert avail[i] == 7 and effs[i] == ("decrement", 7, 0)
    assert int(eff.n_var[0]) == 0


# ---- statuses ----
def test_gpu_downstream_statuses_and_pass_through(mat):
    base = [(10, 1), (10, 2), (13, 3)]
    values = [(AW, base), (MV, [(1, 5), (2, 6)]), (BC, ({(0, 0): 9}, {})), (PN, 4), (LWW, (5, 6, False)),
              (AW, base), (AW, base), (AW, base), (PN, 0), (AW, base), (MV, []), (AW, base), (AW, base)]
    ist = [abi.AM_ERR_COLD_PATH, abi.AM_ERR_CAPACITY, abi.AM_ERR_COLD_PATH, abi.AM_ERR_COLD_PATH,
           abi.AM_ERR_CORRUPTED_OPS_CACHE, 0, 0, 0, 0, 0, 0, 0, 0]
    entries = [
        (0, AW, ("remove", 10)), (1, MV, ("assign", 3)), (2, BC, ("increment", (1, 0))),   # failed rows pass through
        (3, PN, ("increment", 8)), (4, LWW, ("assign", 77, 9)),                            # ... but not for PN / LWW
        (5, AW, ("raw", abi.AM_UP_AW_REMOVE, 0, 0, [13, 10])),                             # unsorted
        (6, AW, ("raw", abi.AM_UP_AW_REMOVE, 0, 0, [10, 10])),                             # repeated element
        (7, AW, ("raw", 3, 0, 0, [])),                                                     # unknown op
        (8, PN, ("decrement", I64_MIN)),
        (9, AW, ("raw", abi.AM_UP_AW_ADD, 0, 0, [10, 900, 13])),                           # half a pair
        (10, MV, ("raw", 2, 0, 0, [])),                                                    # unknown op
        (11, 9, ("raw", 0, 0, 0, [])),                                                     # unknown type
        (12, AW, ("remove_all", [10, 11, 13])),
    ]
    ups, effs, avail, eff = run(mat, 1, values, entries, in_status=ist)
    inv = err(abi.AM_ERR_INVALID)
    assert effs == [err(abi.AM_ERR_COLD_PATH), err(abi.AM_ERR_CAPACITY), err(abi.AM_ERR_COLD_PATH), 8, (77, 9),
                    inv, inv, inv, err(abi.AM_ERR_OVERFLOW), inv, inv, inv, [(10, [], [1, 2]), (11, [], []), (13, [], [3])]]
    assert avail == [0] * len(entries)
    # a repeated row fails the call
    with pytest.raises(abi.AmError, match="rc=-1"):
        mat.generate_downstream(1, values, [(0, AW, ("remove", 10)), (0, AW, ("remove", 13))])
    # no input set columns: a state-dependent update is invalid, PN / LWW are not
    ups2 = Updates([(0, AW, ("reset",)), (1, PN, ("increment", 2)), (2, BC, ("increment", (1, 0)))])
    e2 = Effects(ups2, 8)
    u, e, vin = ups2.as_struct(), e2.as_struct(), abi.am_values()
    abi.check(mat.L.am_generate_downstream_host(mat.ctx, 1, ctypes.byref(u), ctypes.byref(vin), None, ctypes.byref(e),
                                                e2.status.ctypes.data), "am_generate_downstream_host")
    check_invariant(e2)
    assert e2.effects() == [inv, 2, inv]


def test_gpu_downstream_capacity_is_all_or_nothing(mat):
    rng = random.Random(77)
    base, m = aw_base(300, rng), mv_base(40, rng)
    values = [(AW, base), (PN, 1), (MV, m), (AW, base), (MV, []), (BC, ({(0, 0): 4}, {})), (AW, base), (LWW, None)]
    entries = [(0, AW, ("remove_all", [10, 13, 11])), (1, PN, ("increment", 3)), (2, MV, ("assign", 1)),
               (3, AW, ("reset",)), (4, MV, ("assign", 2)), (5, BC, ("decrement", (4, 0))), (6, AW, ("remove_all", [])),
               (7, LWW, ("assign", 5, 6))]
    ups, effs, _, eff = run(mat, 1, values, entries)
    total = int(eff.n_var[0])
    exp, _ = expected(1, values, ups)
    assert effs == exp and total == sum(len(eff.words(i)) for i in range(eff.n_up)) > 300
    fresh = iter(ups.tokens[2] + ups.tokens[4])
    _, e_exact, _, eff_exact = run(mat, 1, values, entries, var_cap=total, tokens=lambda: next(fresh))
    assert e_exact == exp and int(eff_exact.n_var[0]) == total
    fresh = iter(ups.tokens[2] + ups.tokens[4])
    eff_short = Effects(Updates(entries, lambda: next(fresh)), total - 1)
    eff_short.var_data[:] = 0xDEAD
    u, e = eff_short.updates.as_struct(), eff_short.as_struct()
    hin = HostBatch(1, [Read(i, t, {}, base_value=b) for i, (t, b) in enumerate(values)])
    b, _ = hin.structs()
    abi.check(mat.L.am_generate_downstream_host(mat.ctx, 1, ctypes.byref(u), ctypes.byref(b.base), None, ctypes.byref(e),
                                                eff_short.status.ctypes.data), "am_generate_downstream_host")
    check_invariant(eff_short)
    cap = err(abi.AM_ERR_CAPACITY)
    # every update with variable words fails; the scalar ones and the empty ones stay
    assert eff_short.effects() == [cap, 3, cap, cap, exp[4], exp[5], [], (5, 6)]
    assert int(eff_short.n_var[0]) == total and int(eff_short.var_off[-1]) == 0
    assert (eff_short.var_data == 0xDEAD).all(), "no variable word is written"


# ---- composition: the effect pinned through update/2 ----
def rand_value(t, rng, n_dc):
    if t == PN:
        return rng.randint(-100, 100)
    if t == LWW:
        return (rng.randint(1, 50), rng.randint(0, 9), False) if rng.random() < 0.8 else None
    if t == AW:
        return aw_base(rng.choice([0, 3, 40, 130, 300]), rng)
    if t == MV:
        return mv_base(rng.choice([0, 1, 5, 70, 290]), rng)
    return ({(f, t2): rng.randint(0, 40) for f in range(n_dc) for t2 in range(n_dc) if rng.random() < 0.5},
            {i: rng.randint(0, 20) for i in range(n_dc) if rng.random() < 0.5})


def rand_update(t, v, rng, n_dc):
    if t == PN:
        return (rng.choice(["increment", "decrement"]), rng.randint(-50, 50))
    if t == LWW:
        return ("assign", rng.randint(1, 100), rng.randint(0, 9))
    if t == AW:
        k = rng.random()
        if k < 0.15:
            return ("reset",)
        have = sorted({e for e, _ in v}) or [10]
        el = rng.sample(have, min(len(have), rng.randint(0, 5))) + [rng.randint(1, 500) for _ in range(rng.randint(0, 4))]
        return (rng.choice(["add_all", "remove_all"]), el)
    if t == MV:
        return ("reset",) if rng.random() < 0.2 else ("assign", rng.randint(0, 40))
    k = rng.choice(["increment", "decrement", "transfer"])
    if k == "transfer":
        return (k, (rng.randint(1, 30), rng.randrange(n_dc), rng.randrange(n_dc)))
    return (k, (rng.randint(1, 30), rng.randrange(n_dc)))


def dev_array(mat, arr):
    return mat.device_array(np.ascontiguousarray(arr))


def test_gpu_downstream_effects_compose_with_materialize_eager(mat):
    rng = random.Random(2025)
    n_dc, n = 3, 200
    values = []
    for _ in range(n):
        t = rng.choice(randlog.TYPES)
        values.append((t, rand_value(t, rng, n_dc)))
    rows = rng.sample(range(n), n)    # every row once, shuffled
    entries = [(r, values[r][0], rand_update(values[r][0], values[r][1], rng, n_dc)) for r in rows]
    ups, effs, _, eff = run(mat, n_dc, values, entries)
    exp, _ = expected(n_dc, values, ups)
    assert effs == exp
    assert {t for _, t, _ in entries} == set(randlog.TYPES)
    # the restated effects through the reference's update/2
    caps = [2048] * n
    ref_vals = []
    for i, (r, t, _) in enumerate(entries):
        if isinstance(exp[i], tuple) and exp[i] and exp[i][0] == "error":
            ref_vals.append(None)
            continue
        s = R.materialize_eager(t, randlog.base_state_term(t, values[r][1]), [randlog.effect_term(t, exp[i])])
        ref_vals.append(randlog.canon_state(t, s))
    # host path: Effects.as_writeset() into am_materialize_eager_host
    ws = eff.as_writeset()
    hb = mat.materialize_eager_rows(n_dc, values, ws, caps)
    for i in range(n):
        if ref_vals[i] is None:
            assert int(hb.status[i]) == abi.AM_ERR_UNEXPECTED_OPERATION   # AM_META_BAD: never half-applied
        else:
            assert int(hb.status[i]) == 0 and hb.value(i) == ref_vals[i], (i, entries[i])
    assert sum(v is None for v in ref_vals) > 0 and sum(v is not None for v in ref_vals) > 150
    # device path: the am_effects columns as a device am_writeset straight into am_materialize_eager
    hin = HostBatch(n_dc, [Read(i, t, {}, base_value=b) for i, (t, b) in enumerate(values)])
    hout = HostBatch(n_dc, [Read(i, t, {}) for i, (_, t, _) in enumerate(entries)], caps)
    cap = eff.var_cap
    bufs = {}
    try:
        for name, arr in (("row", ups.row), ("type", ups.type), ("op", ups.op), ("a0", ups.a0), ("a1", ups.a1),
                          ("uvo", ups.var_off), ("uvd", ups.var_data), ("v0", hin.b_v0), ("v1", hin.b_v1),
                          ("vf", hin.b_vflag), ("so", hin.b_set_off), ("sl", hin.b_set_len), ("sa", hin.b_set_a),
                          ("sb", hin.b_set_b), ("oso", hout.o_set_off)):
            bufs[name] = dev_array(mat, arr)
        for name, nbytes in (("eo", (n + 1) * 8), ("em", n), ("p0", n * 8), ("p1", n * 8), ("vo", (n + 1) * 8),
                             ("vd", max(cap, 1) * 8), ("nv", 8), ("av", n * 8), ("st", n * 4), ("ost", n * 4),
                             ("ov0", n * 8), ("ov1", n * 8), ("ovf", n), ("osl", n * 4),
                             ("osa", int(hout.o_set_off[-1]) * 8), ("osb", int(hout.o_set_off[-1]) * 8)):
            bufs[name] = dev_array(mat, np.zeros(nbytes, np.uint8))
        p = lambda k: bufs[k].ptr  # noqa: E731
        du = abi.am_updates()
        du.n_up, du.n_var = ups.n_up, ups.n_var
        du.row, du.type, du.op, du.a0, du.a1, du.var_off, du.var_data = (p("row"), p("type"), p("op"), p("a0"), p("a1"),
                                                                         p("uvo"), p("uvd"))
        dv = abi.am_values()
        dv.v0, dv.v1, dv.vflag, dv.set_off, dv.set_len, dv.set_a, dv.set_b = (p("v0"), p("v1"), p("vf"), p("so"), p("sl"),
                                                                              p("sa"), p("sb"))
        de = abi.am_effects()
        de.var_cap = cap
        de.eff_off, de.eff_meta, de.p0, de.p1, de.var_off, de.var_data, de.n_var, de.avail = (
            p("eo"), p("em"), p("p0"), p("p1"), p("vo"), p("vd"), p("nv"), p("av"))
        abi.check(mat.L.am_generate_downstream(mat.ctx, n_dc, ctypes.byref(du), ctypes.byref(dv), None, ctypes.byref(de),
                                               p("st")), "am_generate_downstream")
        dw = abi.am_writeset()   # row, type and the effect columns: a write set as they stand
        dw.n_ws = dw.n_eff = n
        dw.n_var = cap           # an upper bound of *n_var, which stays on the device
        dw.row, dw.type, dw.eff_off, dw.eff_meta, dw.p0, dw.p1, dw.var_off, dw.var_data = (
            p("row"), p("type"), p("eo"), p("em"), p("p0"), p("p1"), p("vo"), p("vd"))
        do = abi.am_values()
        do.v0, do.v1, do.vflag, do.set_off, do.set_len, do.set_a, do.set_b = (p("ov0"), p("ov1"), p("ovf"), p("oso"),
                                                                              p("osl"), p("osa"), p("osb"))
        abi.check(mat.L.am_materialize_eager(mat.ctx, n_dc, ctypes.byref(dw), ctypes.byref(dv), None, ctypes.byref(do),
                                             p("ost")), "am_materialize_eager")
        mat.sync()
        for name, arr in (("ost", hout.status), ("ov0", hout.v0), ("ov1", hout.v1), ("ovf", hout.vflag),
                          ("osl", hout.o_set_len), ("osa", hout.o_set_a), ("osb", hout.o_set_b)):
            bufs[name].download(arr)
        st = np.zeros(n, np.int32)
        bufs["st"].download(st)
        assert st.tolist() == eff.status[:n].tolist()
        for c in ("status", "v0", "v1", "vflag", "o_set_len"):
            assert np.array_equal(getattr(hout, c)[:n], getattr(hb, c)[:n]), c
        for i in range(n):
            if ref_vals[i] is not None:
                assert hout.value(i) == ref_vals[i], i
        # the device entry point reports a repeated row on every update (no host readback)
        rows2 = ups.row.copy()
        rows2[5] = rows2[9]
        bufs["row"].free()
        bufs["row"] = dev_array(mat, rows2)
        du.row = p("row")
        abi.check(mat.L.am_generate_downstream(mat.ctx, n_dc, ctypes.byref(du), ctypes.byref(dv), None, ctypes.byref(de),
                                               p("st")), "am_generate_downstream")
        mat.sync()
        bufs["st"].download(st)
        assert (st == abi.AM_ERR_INVALID).all()
    finally:
        for b in bufs.values():
            b.free()


# ---- a transaction's updates one after another ----
def test_gpu_update_rounds_equal_the_sequential_restatement(mat):
    values = [(AW, [(5, 50), (8, 80)]), (MV, [(1, 10), (2, 20)]), (PN, 3)]
    tx = [(0, AW, ("add", 7)), (1, MV, ("assign", 4)), (0, AW, ("remove", 7)), (2, PN, ("increment", 2)),
          (1, MV, ("assign", 5)), (0, AW, ("add", 7)), (1, MV, ("assign", 6)), (0, AW, ("remove_all", [5, 7]))]
    fresh = iter(range(900, 1000))
    got = mat.update_rounds(1, values, tx, tokens=lambda: next(fresh))
    # the host restatement, one update at a time, each seeing the write set so far
    state = {r: randlog.base_state_term(t, v) for r, (t, v) in enumerate(values)}
    by_round = sorted(range(len(tx)), key=lambda q: (sum(1 for p in range(q) if tx[p][0] == tx[q][0]), q))
    toks = {}
    nxt = iter(range(900, 1000))
    for q in by_round:   # update_rounds draws tokens round by round
        toks[q] = [next(nxt)] if tx[q][2][0] in ("add", "assign") and tx[q][1] != PN else []
    exp = []
    for q, (r, t, upd) in enumerate(tx):
        e, _ = ref_downstream(t, upd, randlog.canon_state(t, state[r]), 1, toks[q])
        exp.append(e)
        state[r] = R.materialize_eager(t, state[r], [randlog.effect_term(t, e)])
    assert got == exp
    assert exp[2] == [(7, [], [toks[0][0]])] and exp[5] == [(7, [toks[5][0]], [])]
    assert exp[6] == ("assign", 6, toks[6][0], [toks[4][0]])
    assert exp[7] == [(5, [], [50]), (7, [], [toks[5][0]])]


# ---- the reference's suites with the device generating every downstream ----
class DeviceClient:
    """tests/test_gpu_system_suites.Client with Type:downstream/2 on the device: the state read
    from the vnode stays in labels, Materializer.update_rounds generates the transaction's
    effects, and the effects go into the ops cache as they come."""

    def __init__(self, mat, type_):
        from antidote_amd.codec import Codec
        self.mat, self.t, self.codec, self.vn = mat, type_, Codec(), mat.vnode(1, 1)
        self.clock = 1000

    def close(self):
        self.vn.close()
        self.codec.close()

    def labels(self):
        r = self.vn.read([Read(0, self.t, {0: self.clock})], set_capacity=[4096]).result(0)
        assert r[0] == "ok", r
        return r[1]

    def state(self):
        return self.codec.value(self.t, self.labels())

    def commit(self, updates):
        from tests.test_gpu_system_suites import _term
        t = self.t
        terms, n_tok = [], 0
        for op, arg in updates:
            arg = _term(arg)
            if t == AW:
                terms += [arg] if op == "add" else list(arg)
                n_tok += 1 if op == "add" else len(arg)
            elif t in (LWW, MV):
                terms.append(arg)
                n_tok += t == MV
        tokens = [os.urandom(20) for _ in range(n_tok)]   # fresh 20-byte binaries, interned before the call
        rl = self.codec.intern(terms + tokens)[1] if terms or tokens else False
        if rl:
            old, nw = self.codec.take_relabel()
            self.vn.relabel(old, nw)
        lab = self.codec.label
        tx = []
        for op, arg in updates:
            arg = _term(arg)
            if t == AW:
                tx.append((0, t, (op, lab(arg) if op == "add" else [lab(x) for x in arg])))
            elif t == LWW:
                tx.append((0, t, ("assign", self.clock * 1000 + 1, lab(arg))))
            elif t == MV:
                tx.append((0, t, ("assign", lab(arg))))
            else:
                tx.append((0, t, (op, int(arg))))
        it = iter(tokens)
        effs = self.mat.update_rounds(1, [(t, self.labels())], tx, tokens=lambda: lab(next(it)))
        snap = self.clock
        self.clock += 10
        assert not any(isinstance(e, tuple) and e and e[0] == "error" for e in effs), effs
        self.vn.insert([[Op(type=t, commit_dc=0, commit_time=self.clock, snap={0: snap}, effect=e) for e in effs]], [t])


SYSTEM = [c for c in load("system_suites.json")["cases"] if "txns" in c]


@pytest.mark.parametrize("case", SYSTEM, ids=lambda c: c["name"])
def test_gpu_system_suite_values_with_device_downstream(mat, case):
    from tests.test_gpu_system_suites import TYPES, _term, _value
    t = TYPES[case["type"]]
    cl = DeviceClient(mat, t)
    try:
        for txn in case["txns"]:
            cl.commit(txn)
        st = cl.state()
        v = _value(t, st)
        exp = case["expect"]
        if "value" in exp:
            assert v == _term(exp["value"]), (case["name"], v)
        if "length" in exp:
            assert len(v) == exp["length"] and all(_term(x) in v for x in exp["contains"]), v
        if t in (AW, MV):   # the tokens are the interned binaries
            toks = [tk for _, tks in st for tk in tks] if t == AW else [tk for _, tk in st]
            assert all(isinstance(tk, bytes) and len(tk) == 20 for tk in toks)
    finally:
        cl.close()


BC_CASES = [c for c in load("multidc_suites.json")["cases"] if set(c["keys"].values()) == {"counter_b"}]


@pytest.mark.parametrize("case", BC_CASES, ids=lambda c: c["name"])
def test_gpu_bounded_counter_scenarios_with_device_downstream(mat, case, monkeypatch):
    """bcounter_mgr's scenarios with every generate_downstream on the device: the state read from
    the DC's vnode, am_generate_downstream_host, {error, no_permissions} as dcsim.NoPermissions."""
    n_dc = case["n_dc"]
    host = dcsim.downstream
    calls = {"ok": 0, "refused": []}

    def device_downstream(type_, op, arg, state, dc, token):
        if type_ != dcsim.BCOUNTER:
            return host(type_, op, arg, state, dc, token)
        upd = (op, tuple(arg)) if op == "transfer" else (op, (int(arg), dc))
        effs, avail, _ = mat.generate_downstream(n_dc, [(BC, (dict(state[0]), dict(state[1])))], [(0, BC, upd)])
        frm = arg[2] if op == "transfer" else dc
        if op != "increment":
            assert avail[0] == dcsim.local_permissions(frm, state)
        if effs[0] == err(abi.AM_ERR_NO_PERMISSIONS):
            calls["refused"].append((upd, avail[0]))
            raise dcsim.NoPermissions()
        calls["ok"] += 1
        try:
            assert effs[0] == host(type_, op, arg, state, dc, token)
        except dcsim.NoPermissions:
            raise AssertionError(("the device granted what the restatement refuses", upd, state))
        return effs[0]

    monkeypatch.setattr(dcsim, "downstream", device_downstream)
    checks = dcsim.run_case(case, lambda nd, keys: dcsim.GpuBackend(nd, keys, mat))
    assert checks
    if any("txn" in s for s in dcsim._expand(case["steps"])):   # new_bcounter_test only reads
        assert calls["ok"] > 0
    for where, got, exp in checks:
        assert got == exp, where
    n_refused = sum(1 for w, g, _ in checks if g == "no_permissions")
    assert len(calls["refused"]) >= n_refused
    if any("expect_error" in s.get("txn", {}) for s in dcsim._expand(case["steps"])):
        assert n_refused > 0 and all(av < upd[1][0] for upd, av in calls["refused"])


# ---- the coordinator-level call ----
def _update_for(t, ops, rng, n_dc):
    if t == AW:
        seen = sorted({e for op in ops for e, _, _ in op.effect}) or [1]
        return rng.choice([("remove_all", rng.sample(seen, min(len(seen), 3)) + [999]), ("add", rng.choice(seen)),
                           ("reset",)])
    if t == MV:
        return rng.choice([("assign", 3), ("reset",)])
    if t == PN:
        return ("decrement", 4)
    if t == LWW:
        return ("assign", 10 ** 9, 5)
    return rng.choice([("decrement", (rng.randint(1, 40), rng.randrange(n_dc))), ("increment", (2, 0)),
                       ("transfer", (rng.randint(1, 40), 0, 1))])


def test_gpu_update_objects_equals_read_then_generate(mat):
    from antidote_amd.readbatch import PartitionedReader
    from tests.test_gpu_eager_reads import _objects, _own_effects, _raw
    from tests.test_gpu_vnode import KeyGen
    rng = random.Random(919)
    n_dc, n_part = 3, 3
    keys, objects = _objects(rng, 60, n_dc)
    cold = 7777   # 200 ops: four write-triggered GC reads drop the initial snapshot, a read below them is cold
    objects[cold] = (PN, KeyGen(rng, PN, n_dc, 10).ops(200))
    keys.append(cold)
    assert {objects[k][0] for k in keys} == set(randlog.TYPES)
    rd, plain = PartitionedReader(mat, n_part, n_dc, objects), PartitionedReader(mat, n_part, n_dc, objects)
    fresh = [10 ** 7]
    try:
        hi = max(op.commit_time for _, ops in objects.values() for op in ops)
        saw_cold = applied = 0
        for rnd in range(4):
            clock = {d: rng.randint(hi // 2, hi + 10) for d in range(n_dc)} if rnd else {d: 1 for d in range(n_dc)}
            req_keys = rng.sample([k for k in keys if k != cold], 36) + [cold]
            req = [(k, objects[k][0]) for k in req_keys]
            wkeys = rng.sample(req_keys[:-1], 10)
            write_set = {k: _own_effects(rng, objects[k][0], objects[k][1], n_dc, fresh) for k in wkeys}
            upd_rows = sorted(set(rng.sample(range(len(req) - 1), len(req) // 3))
                              | {len(req) - 1, req_keys.index(wkeys[0])})   # a written key and the cold one among them
            upds = {i: _update_for(req[i][1], objects[req[i][0]][1], rng, n_dc) for i in upd_rows}
            tk = iter(range(5 * 10 ** 8 + 1000 * rnd, 6 * 10 ** 8))
            ou = [(k, t, upds.get(i)) for i, (k, t) in enumerate(req)]
            if rnd % 2 == 0:   # am_update_objects_submit + am_ticket_wait
                effs, avail, eff = rd.update_objects(ou, clock, write_set=write_set, tokens=lambda: next(tk))
                check_invariant(eff)
                got = [(effs[i], avail[i]) for i in upd_rows]
            else:              # am_update_objects_host
                parts = np.zeros(len(req), np.uint32)
                reads = []
                for i, (key, t) in enumerate(req):
                    parts[i], local = rd.where[key]
                    reads.append(Read(local, t, dict(clock)))
                hb = HostBatch(n_dc, reads, [4096] * len(reads))
                b, _ = hb.structs()
                ups = Updates([(i, req[i][1], upds[i]) for i in upd_rows], lambda: next(tk))
                eff = Effects(ups, 8 * 4096 * len(upd_rows))
                ws = WriteSet([(i, t, write_set[k]) for i, (k, t) in enumerate(req) if k in write_set])
                u, e, w = ups.as_struct(), eff.as_struct(), ws.as_struct()
                abi.check(mat.L.am_update_objects_host(rd.vnode.handle, n_part, rd.part_key_base.ctypes.data,
                                                       parts.ctypes.data, ctypes.byref(b), hb.o_set_off.ctypes.data,
                                                       ctypes.byref(w), ctypes.byref(u), ctypes.byref(e),
                                                       eff.status.ctypes.data), "am_update_objects_host")
                check_invariant(eff)
                got = [(eff.effect(q), int(eff.avail[q])) for q in range(len(upd_rows))]
            # the same in two steps: the read with the write set, then the host generate call
            ws = WriteSet([(i, t, write_set[k]) for i, (k, t) in enumerate(req) if k in write_set])
            hb2 = _raw(plain, mat, req, clock, ws.as_struct(), True)
            vals = [(t, hb2.value(i) if hb2.status[i] == 0 else None) for i, (_, t) in enumerate(req)]
            tk2 = iter(range(5 * 10 ** 8 + 1000 * rnd, 6 * 10 ** 8))
            e2, a2, _ = mat.generate_downstream(n_dc, vals, [(i, req[i][1], upds[i]) for i in upd_rows],
                                                tokens=lambda: next(tk2), in_status=hb2.status[:len(req)])
            assert got == list(zip(e2, a2)), rnd
            for i, (g, _) in zip(upd_rows, got):
                if hb2.status[i] == abi.AM_ERR_COLD_PATH:
                    assert g == (err(abi.AM_ERR_COLD_PATH) if req[i][1] not in (PN, LWW) else g)
                    saw_cold += 1
                applied += not (isinstance(g, tuple) and g and g[0] == "error")
            if rnd == 0:   # the cold key is a PN counter: its read fails, its update does not need it
                assert hb2.status[len(req) - 1] == abi.AM_ERR_COLD_PATH and got[-1][0] == -4
        assert applied > 20 and saw_cold > 0
        # requests naming one key twice are refused: one key's updates are separate calls
        k0 = req_keys[0]
        with pytest.raises(abi.AmError, match="rc=-1"):
            rd.update_objects([(k0, objects[k0][0], None), (k0, objects[k0][0], None)], clock)
    finally:
        rd.close()
        plain.close()
