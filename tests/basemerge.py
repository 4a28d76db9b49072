"""Host side of tests/test_gpu_base_merge.py: hand-made add-wins-set and MV-register keys that are
read over a cached base snapshot at the size limits of every tier that folds new ops into a base.

A read over a base with pairs is refused by the row, lane and workgroup kernels (am_group.h
has_base_pairs) and lands in
  the wave tier      am_group.h base_merge: at most KB base pairs and KB new survivors, no TxId
                     (base_ok); base pairs on lanes j and j + 64, a two-word alive mask; output
                     through birth records when the key has at most VGB groups (by_birth)
  the LDS-sort tier  am_sets.hip k_sets: the base pairs are births at -1; at most BCAP births
                     with the base, KCAP kills
  the big-read tier  am_big.hip: whatever outgrows those.
The random logs of tests/randlog.py hold bases of a dozen pairs.  Each builder here returns cases
with exact counts: a base phase, a new phase and what the read over the base holds.  The base value
of a case is always the C oracle's own result at the base clock (base_of); nothing here needs a
GPU.  tests/test_basemerge_cpu.py proves with the oracle that every case is what it claims."""
import random

from antidote_amd import abi
from antidote_amd.oplog import HostBatch, HostLog, Op, Read
from oracle import amo

AW, MV = abi.AM_AWSET, abi.AM_MVREG

# ---------------------------------------------------------------- mirrors of the kernels' constants
KB = 120                # am_group.h `constexpr uint32_t KB = 120;`
VGB = 1024              # am_group.h `constexpr uint32_t VGB = VG / 2;` with `VG = AM_GRP_MAX_REC` (2048)
BCAP = 1024             # am_sets.hip `constexpr uint32_t BCAP = 1024;`
KCAP = 2048             # am_sets.hip `constexpr uint32_t KCAP = 2048;`
AM_SETS_BIG_OPS = 4096  # am_internal.h `constexpr uint64_t AM_SETS_BIG_OPS = 4096;`
GRP_MAX_REC = 2048      # include/antidote_mat.h `#define AM_GRP_MAX_REC 2048u`: more records, and the key is not grouped
AM_BIG_MIN_OPS = 1024   # include/antidote_mat.h `#define AM_BIG_MIN_OPS (AM_GRP_MAX_REC / 2)`: a longer MV key is chunked

# ---------------------------------------------------------------- timeline and clocks
T0 = 1_700_000_000_000_000
_SNAPS = {}


def stamp(t, effects, n_dc, txids=None, first=0):
    """Op i commits at DC i % n_dc at T0 + 3 i, its snapshot 1 .. 3 us below on every DC: a clock
    with every DC at c includes exactly the ops committed at or before c (a prefix).  first: the
    position of effects[0] in its key (ops appended to a stamped key)."""
    snaps = _SNAPS.setdefault(n_dc, [])  # shared among the keys (never changed)
    for i in range(len(snaps), first + len(effects)):
        snaps.append({d: T0 + 3 * i - 1 - ((i + d) % 3) for d in range(n_dc)})
    return [Op(t, i % n_dc, T0 + 3 * i, snaps[i], e, txid=None if txids is None else txids[i - first])
            for i, e in enumerate(effects, first)]


def clock_after(ops, m, n_dc=None):
    """The clock (a dict over every DC) that includes exactly the first m ops of a stamped key."""
    n_dc = len(ops[0].snap) if n_dc is None else n_dc
    c = ops[m - 1].commit_time if m > 0 else T0 - 10
    return {d: c for d in range(n_dc)}


# ---------------------------------------------------------------- cases
TOK = 1 << 20       # tokens of the base phase
NEW = 1 << 22       # tokens of the new phase
PAD = 1 << 24       # tokens of the padding chain
TAIL = 1 << 26      # tokens of the ops past the read clock
SCRATCH = 10 ** 12  # the padding's element / value, above every other


def case(name, t, hist, n_base, n_read, nb, nout, ns=None, ops=None, txid=None, fresh=True):
    """hist: the stamped history the base is taken from (after n_base ops) and the read clock is
    counted in (after n_read ops); ops: the key as the log holds it (hist unless pruned);
    nb / nout: pairs of the base / of the read over it; ns: new survivors among them (None: not
    stated); count: the ops the read applies;
    fresh: the read over the base equals the fresh read of the log at the same clock."""
    return dict(name=name, t=t, hist=hist, ops=hist if ops is None else ops, n_base=n_base, n_read=n_read, nb=nb,
                nout=nout, ns=ns, count=n_read - n_base, txid=txid, fresh=fresh)


def oracle_read(n_dc, ops, t, clock, cap, base=None, txid=None):
    """The C oracle's result of one read of a one-key log; base = (clock, last op, value)."""
    log = HostLog(n_dc, [ops], key_types=[t])
    b = base if base is not None else (None, 0, None)
    rd = Read(0, t, dict(clock), txid, b[0], b[1], b[2])
    return amo.materialize(log, HostBatch(n_dc, [rd], [cap])).result(0)


def base_of(c, n_dc):
    """(base clock, base last op, base value) of a case: the oracle's read of its history at the
    base clock (LastOpCt, NewLastOp and the value, as the snapshot cache stores them)."""
    if "base" not in c:
        r = oracle_read(n_dc, c["hist"], c["t"], clock_after(c["hist"], c["n_base"], n_dc), c["nb"] + 8)
        assert r[0] == "ok" and len(r[1]) == c["nb"], (c["name"], r[0], r[0] == "ok" and len(r[1]), c["nb"])
        c["base"] = (r[3], r[2], r[1])
    return c["base"]


def read_clock(c, n_dc):
    return clock_after(c["hist"], c["n_read"], n_dc)


def read_of(c, key, n_dc, based=True):
    """The case's read of log key `key`: over its base, or (based=False) fresh at the same clock."""
    if not based:
        return Read(key, c["t"], read_clock(c, n_dc), c["txid"])
    b = base_of(c, n_dc)
    return Read(key, c["t"], read_clock(c, n_dc), c["txid"], b[0], b[1], b[2])


def n_groups(t, ops):
    """The token groups of a key (am_group.hip's builder): one per distinct AW (elem, token), one
    per MV token -- born or only removed."""
    g = set()
    for op in ops:
        if t == AW:
            for e, add, rm in op.effect:
                g |= {(e, x) for x in add} | {(e, x) for x in rm}
        elif op.effect[0] == "reset":
            g |= set(op.effect[1])
        else:
            g |= {op.effect[2]} | set(op.effect[3])
    return len(g)


def with_ids(keys):
    """The keys with an explicit op id on every op (HostLog takes ids for all ops or for none):
    ops that have none get the dense one, position + 1."""
    if not any(op.op_id is not None for k in keys for op in k):
        return keys
    return [[op if op.op_id is not None else Op(op.type, op.commit_dc, op.commit_time, op.snap, op.effect, op.txid, i + 1)
             for i, op in enumerate(k)] for k in keys]


# ---------------------------------------------------------------- sizes
def _elem(j):
    """Base element / value j: 1000, 2000, ..."""
    return 1000 * (j + 1)


def _new_elem(i, nb):
    """New element / value i: spread over the nb + 1 gaps around the base's (gap 0 lies below every
    base element, gap nb above), so the merge's rank search ends at lo = 0, lo = nb and between.
    (1 .. 99 stay free for ops appended later that must sort below every pair.)"""
    return 1000 * (i % (nb + 1)) + 100 + i // (nb + 1)


def default_kills(nb):
    """Holes on both sides of bit 64 of the alive mask and at both ends."""
    return sorted({j for j in (0, 63, 64, nb // 2, nb - 1) if j < nb})


def _aw_ops(entries, per, rng):
    """AW entries (elem, adds, removes) of distinct elems -> effects of at most `per` entries each,
    in a shuffled order, every effect sorted by elem."""
    entries = list(entries)
    rng.shuffle(entries)
    return [sorted(entries[i:i + per]) for i in range(0, len(entries), per)]


def _pads(t, n, first):
    """n padding ops that leave no pair behind and one record each (a chain that replaces its own
    token would cost two records per op, and a key of more than GRP_MAX_REC records is not grouped):
    each removes / resets a token that was never born -- a group of its own, without a birth."""
    return [[(SCRATCH, [], [PAD + first + k])] if t == AW else ("reset", [PAD + first + k]) for k in range(n)]


def n_records(t, ops):
    """Births + kills of a key: an upper bound of its records in the token-group view (one per
    birth, one slot per kill)."""
    n = 0
    for op in ops:
        if t == AW:
            n += sum(len(add) + len(rm) for _, add, rm in op.effect)
        else:
            n += len(op.effect[1]) if op.effect[0] == "reset" else 1 + len(op.effect[3])
    return n


def wave_tier_key(t, ops):
    """The key can be read by the wave tier: grouped in LDS (at most GRP_MAX_REC records and
    groups), and an MV key not past AM_BIG_MIN_OPS ops (it would get the chunked view, which the
    wave tier refuses like an ungrouped key)."""
    return n_records(t, ops) <= GRP_MAX_REC and (t == AW or len(ops) <= AM_BIG_MIN_OPS)


def sizes(t, nb, ns, n_dc, kills=None, base_ops=None, new_ops=None, extra=(), extra_ns=0, name=None):
    """Exactly nb base pairs (AW: distinct elements _elem(j) under token TOK + j; MV: concurrent
    assigns of the values _elem(j)), exactly ns new survivors (_new_elem(i, nb) under NEW + i) and
    the base pairs at the positions `kills` removed by new ops (AW: removes that name them; MV:
    the first new assigns override them, a reset when ns == 0).  The read holds nb - len(kills) +
    ns pairs.  AW effects carry several entries (8, or 32 when the key is wide), so 1025 elements
    need 33 ops.  base_ops / new_ops: the phases padded to that many ops (_pads, first in the
    phase).  extra: more new-phase AW entries / MV effects that leave extra_ns survivors.  Two ops
    past the read clock add a pair and remove base pair 1: the read must not see them."""
    rng = random.Random(1000 * nb + ns + 7 * t)
    kills = default_kills(nb) if kills is None else sorted(kills)
    assert all(0 <= j < nb for j in kills)
    per = 8 if nb + ns <= 300 else 32
    order = list(range(nb))
    rng.shuffle(order)
    if t == AW:
        base = _aw_ops([(_elem(j), [TOK + j], []) for j in order], per, rng)
        ents = [(_new_elem(i, nb), [NEW + i], []) for i in range(ns)] + [(_elem(j), [], [TOK + j]) for j in kills]
        new = _aw_ops(ents + list(extra), per, rng)
        tail = [[(SCRATCH + 5, [TAIL], [])], [(_elem(1), [], [TOK + 1])] if nb > 1 else [(SCRATCH + 6, [TAIL + 1], [])]]
    else:
        base = [("assign", _elem(j), TOK + j, []) for j in order]
        ovr = [[] for _ in range(ns)]
        for q, j in enumerate(kills if ns else ()):
            ovr[q % ns].append(TOK + j)
        new = [("assign", _new_elem(i, nb), NEW + i, ovr[i]) for i in range(ns)]
        if not ns and kills:
            new = [("reset", [TOK + j for j in kills])]
        new += list(extra)
        rng.shuffle(new)
        tail = [("assign", SCRATCH + 5, TAIL, []), ("assign", SCRATCH + 6, TAIL + 1, [TOK + 1] if nb > 1 else [])]
    if base_ops is not None:
        assert base_ops > len(base)
        base = _pads(t, base_ops - len(base), 0) + base
    if new_ops is not None:
        assert new_ops > len(new)
        new = _pads(t, new_ops - len(new), 5000) + new
    hist = stamp(t, base + new + tail, n_dc)
    return case(name or "sizes-%d-%d" % (nb, ns), t, hist, len(base), len(base) + len(new), nb,
                nb - len(kills) + ns + extra_ns, ns=ns + extra_ns)


# ---------------------------------------------------------------- interleave
def interleave(t, n_dc):
    """New pairs below, above and between the base's, and every way an element's token list is put
    together (docstrings of _interleave_aw / _interleave_mv)."""
    return _interleave_aw(n_dc) if t == AW else _interleave_mv(n_dc)


GAPS = (1, 10, 62, 63, 64, 65, 69)  # new elements / values at _elem(j) + 500: interior rank positions


def _interleave_aw(n_dc):
    """Base, 78 pairs over 73 elements: 70 singles _elem(0 .. 69); element 31500 with four tokens
    from four ops (state order: newest first); 45500 and 20500 with two each.
    New ops, 16 survivors:
      below / above / between   elements 1, 2, 3; 10^9 + 1, 10^9 + 2; _elem(j) + 500 for j in GAPS
      ties                      45500 gets a token from each of two ops and keeps its base tokens:
                                [newest, older, base newest, base older]; _elem(4) gets two tokens
                                in one effect: [first, second, base token]
      partly killed             31500 loses its newest and its third token, the other two stay
      vanishing                 20500 loses both tokens and gets none
      killed singles            0, 63, 64 and 69
    -> 78 - 8 + 16 = 86 pairs."""
    rng = random.Random(41)
    b = [[(_elem(j), [TOK + j], [])] for j in range(70)]
    b += [[(31500, [TOK + 100 + k], [])] for k in range(4)]
    b += [[(45500, [TOK + 110 + k], [])] for k in range(2)] + [[(20500, [TOK + 120 + k], [])] for k in range(2)]
    rng.shuffle(b)
    n = [[(e, [NEW + e], [])] for e in (1, 2, 3, 10 ** 9 + 1, 10 ** 9 + 2)]
    n += [[(_elem(j), [], [TOK + j]), (_elem(j) + 500, [NEW + 50 + j], [])] if j in (63, 64, 69)
          else [(_elem(j) + 500, [NEW + 50 + j], [])] for j in GAPS]
    n += [[(_elem(0), [], [TOK])], [(20500, [], [TOK + 120, TOK + 121]), (31500, [], [TOK + 103, TOK + 101])]]
    n += [[(_elem(4), [NEW + 22, NEW + 23], [])]]
    rng.shuffle(n)
    n.insert(3, [(45500, [NEW + 20], [])])
    n.append([(45500, [NEW + 21], [])])  # the newest: first in the element's list
    hist = stamp(AW, b + n, n_dc)
    return case("interleave", AW, hist, len(b), len(b) + len(n), 78, 86, ns=16)


def _interleave_mv(n_dc):
    """Base, 71 pairs: values _elem(0 .. 69) under TOK + j, and (5000, TOK + 500) beside (5000,
    TOK + 4).  New ops, 15 survivors:
      below / above / between   values 1, 2, 3; 10^9 + 1, 10^9 + 2; _elem(j) + 500 for j in GAPS
      equal values              5000 under tokens 7 (below TOK + 4), TOK + 200 (between the base's
                                two) and TOK + 900 (above both)
      an overriding assign      64500 (one of GAPS) overrides the base pairs at the sorted
                                positions 0, 62, 63, 64, 65 and 70: both sides of bit 64, both ends
    -> 71 - 6 + 15 = 80 pairs."""
    rng = random.Random(43)
    pairs = [(_elem(j), TOK + j) for j in range(70)] + [(5000, TOK + 500)]
    b = [("assign", v, x, []) for v, x in pairs]
    rng.shuffle(b)
    srt = sorted(pairs)
    ovr = [srt[p][1] for p in (0, 62, 63, 64, 65, 70)]
    n = [("assign", v, NEW + 200 + k, []) for k, v in enumerate((1, 2, 3, 10 ** 9 + 1, 10 ** 9 + 2))]
    n += [("assign", _elem(j) + 500, NEW + 50 + j, ovr if j == 63 else []) for j in GAPS]
    n += [("assign", 5000, x, []) for x in (7, TOK + 200, TOK + 900)]
    rng.shuffle(n)
    hist = stamp(MV, b + n, n_dc)
    return case("interleave", MV, hist, len(b), len(b) + len(n), 71, 80, ns=15)


# ---------------------------------------------------------------- unborn
def unborn(t, n_dc):
    """A base with tokens whose births the log no longer holds: the history is sizes(100 base
    pairs, 24 new survivors, 7 kills), the log only its ops after the base, their op ids explicit
    and continuing the numbering (a pruned ops cache).  The new ops kill base pairs 0, 1, 50, 63,
    64, 98 and 99 (AW: removes that name the tokens; MV: assigns that override them) -- kills of
    groups with no birth in the log, which the builder keeps -- and AW adds a token to base element
    10, whose base token stays: [new, base].  117 pairs (AW 118)."""
    extra = [(_elem(10), [NEW + 999], [])] if t == AW else []
    c = sizes(t, 100, 24, n_dc, kills=(0, 1, 50, 63, 64, 98, 99), extra=extra, extra_ns=len(extra), name="unborn")
    h = c["hist"]
    c["ops"] = [Op(op.type, op.commit_dc, op.commit_time, op.snap, op.effect, op.txid, i + 1)
                for i, op in enumerate(h) if i >= c["n_base"]]
    return c


# ---------------------------------------------------------------- churn
CHURN_OPS, CHURN_BASE = 1000, 500


def churn(t, n_dc):
    """1000 ops of observe-and-replace on 100 elements (AW) / 100 concurrent slots of values (MV):
    op i writes slot i % 100 (past the base clock, after 500 ops: i % 90, so ten slots keep their
    base pairs) under token TOK + i and removes what the slot holds, except every 13th op, which
    removes nothing (a concurrent add: the slot then holds two); every 25th op also removes a
    token that was never born.  1040 groups -- more than VGB, so the wave tier reads the
    survivors' pairs from the group table, not from birth records -- in about 1930 records: the
    key is still grouped (GRP_MAX_REC; an MV key must also stay within AM_BIG_MIN_OPS ops, so its
    groups past 1024 can only be tokens without a birth)."""
    live = {}
    effs, at_base = [], None
    for i in range(CHURN_OPS):
        if i == CHURN_BASE:
            at_base = sum(len(v) for v in live.values())
        s = i % 100 if i < CHURN_BASE else i % 90
        cur = live.setdefault(s, [])
        rm = [] if i % 13 == 5 else list(cur)
        live[s] = [TOK + i] + [x for x in cur if x not in rm]
        rm = rm + ([PAD + i] if i % 25 == 0 else [])
        if t == AW:
            effs.append([(_elem(s), [TOK + i], rm)])
        else:
            effs.append(("assign", _elem(s) + (i // 100) % 3, TOK + i, rm))
    nout = sum(len(v) for v in live.values())
    ns = sum(x >= TOK + CHURN_BASE for v in live.values() for x in v)
    assert 100 <= at_base <= KB and 90 <= ns <= KB, (at_base, ns)
    return case("churn", t, stamp(t, effs, n_dc), CHURN_BASE, CHURN_OPS, at_base, nout, ns=ns)


# ---------------------------------------------------------------- TxIds
def txid_dup(t, n_dc, txid=5):
    """60 base ops (op j adds element / value 100 (j + 1) under token 1000 + j) and 10 new ones
    (100 (j + 1) + 50), every op with a TxId 1 .. 4 but base ops 10 and 20, which belong to
    transaction 5.  The read names TxId 5: both ops are candidates although the base holds them,
    and re-applying them puts (1100, 1010) and (2100, 1020) into the AW value twice (72 pairs:
    outside the closed form of base_merge, which must refuse the read); the MV register drops the
    copies (70 pairs).  txid=9: a transaction with no op in the key -- the plain 70 pairs."""
    def eff(e, x):
        return [(e, [x], [])] if t == AW else ("assign", e, x, [])

    effs = [eff(100 * (j + 1), 1000 + j) for j in range(60)] + [eff(100 * (j + 1) + 50, 2000 + j) for j in range(10)]
    tx = [5 if j in (10, 20) else 1 + j % 4 for j in range(70)]
    dup = 2 if txid == 5 else 0
    c = case("txid-%d" % txid, t, stamp(t, effs, n_dc, tx), 60, 70, 60, 70 + (dup if t == AW else 0), txid=txid,
             fresh=False)
    c["count"] = 10 + dup
    return c


# ---------------------------------------------------------------- the LDS-sort tier's edges
def lds_edge(t, n_dc):
    """Reads the wave tier refuses (more than KB base pairs) at the LDS-sort tier's birth limit:
      sum-1024    121 base pairs + 903 births of included ops = BCAP: the last read k_sets keeps
      sum-1025    121 + 904: one more than its list holds -- retried in the big-read tier
      base-1024   the base alone fills the list (5 kills, no birth)
      base-1025   the base alone is past it (`bl > BCAP`)
    An AW key's base phase is padded to 300 ops (ops inside the base are no candidates: their
    births do not count); an MV key has one op per pair (1026 .. 1030 ops)."""
    pad = dict(base_ops=300) if t == AW else {}
    return [sizes(t, 121, BCAP - 121, n_dc, name="sum-1024", **pad), sizes(t, 121, BCAP - 120, n_dc, name="sum-1025", **pad),
            sizes(t, BCAP, 0, n_dc, name="base-1024", **pad), sizes(t, BCAP + 1, 0, n_dc, name="base-1025", **pad)]
