"""materializer:materialize_eager/3 on the device (am_materialize_eager_host) against
oracle.ref_materializer.materialize_eager: the reference's known answers, every base size
around the two kernel shapes' tiles, the write-set limits, the per-type edge cases and a random
mixed batch whose write sets are generated against the running state (tests/dcsim.downstream)."""
import functools
import random

import pytest

from antidote_amd import abi
from antidote_amd.oplog import WriteSet
from oracle import ref_materializer as R
from tests import dcsim, randlog
from tests.kat_util import load

PN, LWW, AW, MV, BC = abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TW, TG = abi.AM_EAGER_TILE_WAVE, abi.AM_EAGER_TILE_WG
# bases of 0, 1, 63, 64, 65, T-1, T, T+1 and 4T+3 pairs for both tiles
SIZES = sorted({0, 1, 63, 64, 65, TW - 1, TW, TW + 1, 4 * TW + 3, TG - 1, TG, TG + 1, 4 * TG + 3})


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def oracle(t, base, effs):
    """The oracle's outcome in the ABI's rendering: a value, or ('error', status).  The
    reference's integers never overflow: a result outside int64 is AM_ERR_OVERFLOW."""
    terms = [("bad_effect", "x") if e == "bad" else randlog.effect_term(t, e) for e in effs]
    r = R.materialize_eager(t, randlog.base_state_term(t, base), terms)
    if isinstance(r, tuple) and len(r) == 2 and r[0] == "error":
        return ("error", abi.AM_ERR_UNEXPECTED_OPERATION)
    v = randlog.canon_state(t, r)
    ints = [v] if t == PN else (list(v[0].values()) + list(v[1].values()) if t == BC else [])
    if any(not I64_MIN <= x <= I64_MAX for x in ints):
        return ("error", abi.AM_ERR_OVERFLOW)
    return v


def got(hb, i):
    st = int(hb.status[i])
    return ("error", st) if st != 0 else hb.value(i)


def check(mat, n_dc, entries, caps=None):
    """Every entry (type, base, effects) through one am_materialize_eager_host call."""
    hb = mat.materialize_eager(n_dc, entries, caps or [max(4096, n_dc * n_dc + n_dc)] * len(entries))
    for i, (t, base, effs) in enumerate(entries):
        assert got(hb, i) == oracle(t, base, effs), (i, t, len(base or []) if t in (AW, MV) else base, effs)
    return hb


# ---------------------------------------------------------------- known answers
@pytest.mark.gpu
def test_gpu_eager_known_answers(mat):
    cases = load("kat_materialize.json")["materialize_eager"]
    assert len(cases) == 6
    entries = [(c["type"], None, ["bad" if "expect_error" in c else e for e in c["effects"]]) for c in cases]
    hb = mat.materialize_eager(1, entries)
    for i, c in enumerate(cases):
        if "expect_error" in c:
            assert got(hb, i) == ("error", abi.AM_ERR_UNEXPECTED_OPERATION)
        else:
            assert got(hb, i) == c["expect"]
        assert got(hb, i) == oracle(*entries[i])


# ---------------------------------------------------------------- base sizes
def aw_base(n):
    """n (elem, token) pairs: elems 10, 20, ... with 1-3 tokens each, state order."""
    out, e, tok = [], 10, 1000
    while len(out) < n:
        for _ in range(min(1 + (e // 10) % 3, n - len(out))):
            out.append((e, tok))
            tok += 1
        e += 10
    return out


def mv_base(n):
    return sorted((i % 7, 2000 + i) for i in range(n))


PAD = list(range(900000, 900200))  # tokens no state holds: a write set of the workgroup shape


def aw_write_sets(base):
    elems = sorted({e for e, _ in base})
    toks = lambda e: [t for x, t in base if x == e]  # noqa: E731
    lo, mid, hi = 5, 15, 10 ** 6
    first = elems[0] if elems else 10
    last = elems[-1] if elems else 20
    # every token of `first` removed (it vanishes); token 3 of `last` added and removed at once (it stays)
    ends = ([(first, [], toks(first)), (mid, [2], []), (last, [3], [3] + toks(last)[:1])] if first != last
            else [(first, [3], [3] + toks(first)), (mid, [2], [])])
    one = [[(lo, [1], [])] + ends + [(hi, [4], [])]]
    several = one + [
        [(mid, [5, 6], [2])],                    # the add of effect 0 removed, two tokens added
        [(lo, [], [1]), (mid, [], [5])],         # lo vanishes again; one of the two goes
        [(first, [7], []), (hi, [8], [4])],      # a vanished elem comes back; hi's token replaced
    ]
    return [[], one, several]


def mv_write_sets(base):
    toks = [t for _, t in base]
    keep = base[len(base) // 2] if base else (3, 2000)
    one = [("assign", 3, 1, toks[: len(toks) // 2])]
    several = [
        ("assign", keep[0], keep[1], []),            # repeats a surviving {Value, Token} pair
        ("assign", 2, 2, toks[:3]),
        ("assign", 9, 3, [2]),                       # overrides the assign before it
        ("assign", 2, 4, []), ("assign", 2, 4, []),  # the same pair twice
        ("assign", 0, 5, toks[-2:]),
    ]
    reset = [("assign", 1, 6, []), ("reset", toks + [6]), ("assign", 4, 7, [])]
    return [[], one, several, reset]


@pytest.mark.gpu
def test_gpu_eager_base_sizes_both_shapes(mat):
    entries = []
    for n in SIZES:
        for effs in aw_write_sets(aw_base(n)):
            entries.append((AW, aw_base(n), effs))
            entries.append((AW, aw_base(n), [[(1, [], PAD)]] + effs))
        for effs in mv_write_sets(mv_base(n)):
            entries.append((MV, mv_base(n), effs))
            entries.append((MV, mv_base(n), [("reset", PAD)] + effs))
    check(mat, 3, entries)
    # the cases are what they claim to be
    a = oracle(AW, aw_base(65), aw_write_sets(aw_base(65))[1][:])
    assert a[0] == (5, 1) and a[-1] == (10 ** 6, 4) and 10 not in {e for e, _ in a} and (15, 2) in a
    last = aw_base(65)[-1][0]
    assert (last, 3) in a, "a token added and removed by one effect stays"
    s = oracle(AW, aw_base(65), aw_write_sets(aw_base(65))[2])
    assert (15, 2) not in s and (15, 6) in s and (15, 5) not in s and 5 not in {e for e, _ in s}
    m = oracle(MV, mv_base(64), mv_write_sets(mv_base(64))[2])
    assert len(m) == len(set(m)) and mv_base(64)[32] in m
    assert oracle(MV, mv_base(64), mv_write_sets(mv_base(64))[3]) == [(4, 7)]


# ---------------------------------------------------------------- limits
@pytest.mark.gpu
def test_gpu_eager_write_set_limits_and_output_capacity(mat):
    NB, NK = abi.AM_EAGER_MAX_BIRTHS, abi.AM_EAGER_MAX_KILLS
    base = aw_base(5)
    entries = [
        (AW, base, [[(7, list(range(1, NB + 1)), [])]]),            # births at the limit
        (AW, base, [[(7, list(range(1, NB + 2)), [])]]),            # one token over
        (AW, base, [[(7, [], list(range(1, NK + 1)))]]),            # kills at the limit
        (AW, base, [[(7, [], list(range(1, NK + 2)))]]),
        (MV, mv_base(5), [("reset", list(range(1, NK + 1)))]),
        (MV, mv_base(5), [("reset", list(range(1, NK + 2)))]),
        (AW, base, [[(7, [1], [])]]),                               # 6 pairs out
        (AW, base, [[(7, [1], [])]]),
        (MV, mv_base(5), [("assign", 9, 1, [])]),
        (MV, mv_base(5), [("assign", 9, 1, [])]),
        (BC, ({(0, 0): 5}, {1: 2}), [("increment", 1, 2)]),         # 3 slots out
        (BC, ({(0, 0): 5}, {1: 2}), [("increment", 1, 2)]),
    ]
    caps = [NB + 5, NB + 6, 5, 5, 5, 5, 6, 5, 6, 5, 3, 2]
    hb = mat.materialize_eager(3, entries, caps)
    CAP = ("error", abi.AM_ERR_CAPACITY)
    want = [None, CAP, None, CAP, None, CAP, None, CAP, None, CAP, None, CAP]
    for i, (t, b, e) in enumerate(entries):
        assert got(hb, i) == (want[i] or oracle(t, b, e)), i
    assert len(got(hb, 0)) == NB + 5


# ---------------------------------------------------------------- per-type edge cases
@pytest.mark.gpu
def test_gpu_eager_counters_and_registers(mat):
    U = ("error", abi.AM_ERR_UNEXPECTED_OPERATION)
    O = ("error", abi.AM_ERR_OVERFLOW)
    entries = [
        # bounded counter: a zero amount makes its slot present; keyed adds; overflow at 2^63
        (BC, None, [("increment", 0, 1)]),
        (BC, None, [("decrement", 0, 2), ("transfer", 0, 0, 1)]),
        (BC, ({(0, 0): 10, (1, 2): 4}, {0: 3}), [("increment", 5, 0), ("transfer", 2, 2, 1), ("decrement", 1, 0),
                                                 ("decrement", 7, 2), ("increment", 1, 1)]),
        (BC, ({(0, 0): I64_MAX}, {}), [("increment", 1, 0)]),
        (BC, ({(0, 0): I64_MAX}, {}), [("increment", 1, 0), "bad"]),
        (BC, ({(0, 0): I64_MAX}, {}), [("increment", 1, 1)]),
        # PN: sums at +-2^63, exact through an intermediate excess, a bad effect beats the overflow
        (PN, I64_MAX - 1, [1]), (PN, I64_MAX - 1, [1, 1]), (PN, I64_MIN + 1, [-1]), (PN, I64_MIN + 1, [-1, -1]),
        (PN, I64_MAX, [1, -1]), (PN, I64_MAX, [I64_MAX, I64_MIN, I64_MIN + 2]), (PN, I64_MAX, [1, "bad"]),
        (PN, None, []), (PN, 7, []),
        # LWW: equal timestamps compare the values; the initial {0, <<>>} sorts above every integer
        (LWW, (7, 5, False), [(7, 9)]), (LWW, (7, 5, False), [(7, 3)]), (LWW, (7, 5, False), [(7, 5)]),
        (LWW, None, [(0, 4)]), (LWW, None, [(1, 4)]), (LWW, None, []), (LWW, (3, 1, False), [(2, 9), (3, 2), (3, 0)]),
        (LWW, (3, 1, False), [(9, 9), "bad"]),
    ]
    hb = check(mat, 3, entries)
    assert got(hb, 0) == ({(1, 1): 0}, {}) and got(hb, 1) == ({(1, 0): 0}, {2: 0})
    assert got(hb, 3) == O and got(hb, 4) == U and got(hb, 5) == ({(0, 0): I64_MAX, (1, 1): 1}, {})
    assert [got(hb, i) for i in range(6, 13)] == [I64_MAX, O, I64_MIN, O, I64_MAX, 0, U]
    assert got(hb, 15) == (7, 9, False) and got(hb, 16) == (7, 5, False) and got(hb, 18) == (0, 0, True)
    # a transfer at D = 16 (the workgroup shape: 272 slots)
    e16 = [(BC, ({(3, 3): 50, (15, 15): 9}, {15: 1}), [("transfer", 5, 15, 3), ("transfer", 2, 3, 15),
                                                       ("decrement", 4, 15), ("increment", 0, 7)])]
    assert got(check(mat, 16, e16), 0) == ({(3, 3): 50, (3, 15): 5, (7, 7): 0, (15, 3): 2, (15, 15): 9}, {15: 5})


@pytest.mark.gpu
def test_gpu_eager_payload_rows_and_pass_through(mat):
    """A malformed variable payload, a non-identity row map over a longer value batch, the
    in_status pass-through and a mixed-type batch, in one call."""
    values = [(PN, 100), (AW, aw_base(70)), (MV, mv_base(3)), (LWW, (4, 4, False)), (BC, ({(1, 1): 3}, {})),
              (AW, aw_base(2)), (PN, 5), (AW, aw_base(4)), (MV, mv_base(2))]
    in_status = [0, 0, 0, 0, 0, abi.AM_ERR_CAPACITY, 5, 0, 0]
    ent = [(7, AW, [[(10, [1], [])]]),            # payload truncated below
           (3, LWW, [(4, 5)]),
           (1, AW, [[(15, [9], [])]]),
           (6, PN, [1]),                          # in_status 5: passed through
           (0, PN, [-1, -2]),
           (5, AW, [[(10, [1], [])]]),            # in_status AM_ERR_CAPACITY
           (4, BC, [("decrement", 1, 1)]),
           (2, MV, [("assign", 5, 9, [2000])]),
           (8, MV, [("assign", 5, 9, [2000])])]
    ws = WriteSet(ent)
    q = int(ws.var_off[int(ws.eff_off[0])])
    assert list(ws.var_data[q:q + 4]) == [10, 1, 0, 1]
    ws.var_data[q + 1] = 5                        # n_add beyond the effect's words
    hb = mat.materialize_eager_rows(3, values, ws, [4096] * len(ent), in_status)
    U = ("error", abi.AM_ERR_UNEXPECTED_OPERATION)
    want = [U, oracle(LWW, (4, 4, False), [(4, 5)]), oracle(AW, aw_base(70), ent[2][2]), ("error", 5),
            97, ("error", abi.AM_ERR_CAPACITY), oracle(BC, ({(1, 1): 3}, {}), ent[6][2]),
            oracle(MV, mv_base(3), ent[7][2]), oracle(MV, mv_base(2), ent[8][2])]
    assert [got(hb, i) for i in range(len(ent))] == want
    assert int(hb.o_set_len[3]) == 0 and int(hb.o_set_len[5]) == 0 and int(hb.o_set_len[0]) == 0


# ---------------------------------------------------------------- random batch
@functools.lru_cache(maxsize=None)
def random_batch(n=2000, n_dc=3, seed=0xEA6E):
    """(type, base, effects) per entry: the base is the oracle's state after a random causal
    history, the write set 0-6 downstream effects generated against the running state (fresh
    tokens, observed removes).  Nothing is filtered out."""
    rng = random.Random(seed)
    tok = [10 ** 6]

    def token():
        tok[0] += 1
        return tok[0]

    out = []
    for i in range(n):
        t = randlog.TYPES[i % 5]
        state = R.crdt_new(t)
        for op in randlog.rand_key_ops(rng, t, n_dc, rng.choice([0, 1, 5, 40, 150] if t in (AW, MV) else [0, 3, 20])):
            state = R.crdt_update(t, randlog.effect_term(t, op.effect), state)
        if t in (AW, MV) and rng.random() < 0.3:  # a wide state: concurrent adds / assigns nobody observed
            for k in range(rng.choice([70, 300])):
                wide = [(rng.randrange(400), [token()], [])] if t == AW else ("assign", rng.randint(0, 4), token(), [])
                state = R.crdt_update(t, randlog.effect_term(t, wide), state)
        base = randlog.canon_state(t, state)
        effs = []
        for _ in range(rng.choice([0, 1, 1, 1, 2, 2, 3, 6])):
            dc = rng.randrange(n_dc)
            if t == PN:
                eff = dcsim.downstream(t, rng.choice(["increment", "decrement"]), rng.randint(0, 1000), state, dc, token)
            elif t == LWW:
                eff = (rng.randint(0, 70), rng.randint(0, 5))
            elif t == AW:
                present = [e for e, _ in state]
                op = rng.choice(["add", "remove", "add_all", "remove_all"])
                pool = present + list(range(8)) if op.startswith("add") else (present or [3]) + [77]
                arg = rng.choice(pool) if op in ("add", "remove") else rng.sample(pool, min(len(pool), rng.randint(1, 3)))
                eff = dcsim.downstream(t, op, arg, state, dc, token)
            elif t == MV:
                eff = dcsim.downstream(t, "assign", rng.randint(0, 4), state, dc, token)
            else:
                try:
                    kind = rng.choice(["increment", "decrement", "transfer"])
                    arg = (rng.randint(0, 30), rng.randrange(n_dc), dc) if kind == "transfer" else rng.randint(0, 30)
                    eff = dcsim.downstream(t, kind, arg, state, dc, token)
                except dcsim.NoPermissions:
                    eff = dcsim.downstream(t, "increment", rng.randint(0, 30), state, dc, token)
            effs.append(eff)
            state = R.crdt_update(t, randlog.effect_term(t, eff), state)
        out.append((t, base, effs))
    return out


def test_eager_random_batch_is_accepted_by_the_oracle():
    batch = random_batch()
    assert len(batch) == 2000 and {t for t, _, _ in batch} == set(randlog.TYPES)
    sizes = set()
    for t, base, effs in batch:
        r = oracle(t, base, effs)
        assert not (isinstance(r, tuple) and len(r) == 2 and r[0] == "error"), (t, base, effs, r)
        if t in (AW, MV):
            sizes.add(len(base) > abi.AM_EAGER_TILE_WAVE)
    assert sizes == {False, True}, "bases on both sides of one tile"


@pytest.mark.gpu
def test_gpu_eager_random_batch(mat):
    check(mat, 3, list(random_batch()))


@pytest.mark.gpu
def test_gpu_eager_random_batch_32_dcs(mat):
    """The same batch shape at AM_MAX_DC: bounded counters are CLS_BIG from 11 DCs on (am_eager.hip),
    their slots run to 32 * 32 + 31, and write sets name DC 31."""
    batch = list(random_batch(600, 32, 0xEA6E + 32))
    slots = {f * 32 + to for t, base, _ in batch if t == BC for f, to in base[0]}
    dcs = {e[-1] for t, _, effs in batch if t == BC for e in effs}
    assert max(slots) > 16 * 32 and 31 in dcs, "bases past slot 16 * n_dc, effects at DC 31"
    check(mat, 32, batch)
