"""Host side of tests/test_gpu_big_exits.py: hand-made logs that take the big-read tier's overflow
exits (antidote_amd/csrc/am_big.hip) and keys whose exact sums sit on the int64 edges.

The random logs of tests/randlog.py reach the tier but not its fallbacks: a chunk of 1024 ops whose
births or kills outgrow the workgroup's LDS lists, an MV chunk whose token hash fills, a grouped MV
chunk whose group-id hash set cannot place an id, more survivors than k_big_finish sorts in LDS, and
128-bit slot sums whose high word is not the sign of the low one.  Each builder below returns the
ops of one key that is to be the FIRST key of its log: then key_off == 0 and chunk c of the tier is
ops [1024 c, 1024 c + 1024).  The models (included, chunk_records, survivors, ...) restate from the
ops and a read clock what a chunk sees, in op order -- the device fills its lists through atomics,
in about that order; where it matters a condition is stated so that it holds for every order
(pigeonhole) -- and tests/test_bigexits_cpu.py asserts with them, without a GPU, that every key has
the shape its docstring claims and that the oracle alone answers ok / the stated error."""
import random

from antidote_amd import abi
from antidote_amd.oplog import Op

PN, AW, MV, BC = abi.AM_PN, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER

# ---------------------------------------------------------------- mirrors of the kernels' constants
CHUNK = 1024          # am_big.hip `constexpr uint64_t CHUNK = (uint64_t)BLOCK * OPL` (256 threads x 4 ops)
LB = 1024             # am_big.hip `constexpr uint32_t LB = 1024;   // LDS births per chunk`
LK = 2048             # am_big.hip `constexpr uint32_t LK = 2048;   // LDS kills per chunk`
HPROBES = 64          # am_big.hip `constexpr uint32_t HPROBES = 64;` (probes of the MV token hash)
GH = 2048             # am_big.hip `constexpr uint32_t GH = LK;` (slots per group-id hash set)
GPROBES = 32          # am_big.hip gset_insert: `for (uint32_t pr = 0; pr < 32; ++pr)`
SCAP = 2048           # am_big.hip `constexpr uint32_t SCAP = 2048; // survivors sorted in LDS by k_big_finish`
AM_BIG_MIN_OPS = 1024   # include/antidote_mat.h `#define AM_BIG_MIN_OPS (AM_GRP_MAX_REC / 2)`
AM_SETS_BIG_OPS = 4096  # am_internal.h `constexpr uint64_t AM_SETS_BIG_OPS = 4096;`
AM_BCWAVE_OPS = 4096    # am_internal.h `constexpr uint64_t AM_BCWAVE_OPS = 4096;`
ROWS_SCALAR = 64      # am_plan.hip `constexpr uint32_t ROWS_SCALAR = 64, ROWS_BC = 48;`
ROWS_BC = 48          # (the same line)
NGRP_BIG = 0x80000000   # include/antidote_mat.h `#define AM_NGRP_BIG 0x80000000u`
NGRP_NONE = 0xFFFFFFFF  # include/antidote_mat.h `#define AM_NGRP_NONE 0xFFFFFFFFu`
DEFER = 1 << 56       # the row tier's deferral amount (tests/test_gpu_wide_dc.py extra_bc_keys)

M64 = (1 << 64) - 1
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def key_hash(a, b):
    """am_big.hip key_hash."""
    h = ((a * 0x9E3779B97F4A7C15) & M64) ^ ((((b + 0x632BE59BD9B4E019) & M64) * 0xC2B2AE3D27D4EB4F) & M64)
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & M64
    return h ^ (h >> 32)


def tok_slot(t):
    """am_big.hip tok_slot: the MV token hash's start slot."""
    return key_hash(t, 0) & (LK - 1)


def gslot(g):
    """am_big.hip gslot: `(g * 0x9E3779B1u) >> 21`, 11 bits."""
    return ((g * 0x9E3779B1) & 0xFFFFFFFF) >> 21


# ---------------------------------------------------------------- timeline and clocks
T0 = 1000
_SNAPS = {}


def stamp(t, effects, n_dc, txid=None):
    """Op i commits at DC i % n_dc at T0 + 3 i, its snapshot 1 .. 3 us below on every DC: a clock
    with every DC at c includes exactly the ops committed at or before c (a prefix)."""
    snaps = _SNAPS.setdefault(n_dc, [])  # shared among the keys (never changed)
    for i in range(len(snaps), len(effects)):
        snaps.append({d: T0 + 3 * i - 1 - ((i + d) % 3) for d in range(n_dc)})
    return [Op(t, i % n_dc, T0 + 3 * i, snaps[i], e, txid=txid) for i, e in enumerate(effects)]


def clock_after(ops, m, n_dc):
    """The batch clock that includes the first m ops of a stamped key (none: below T0)."""
    c = ops[m - 1].commit_time if m > 0 else T0 - 10
    return [c] * n_dc


def included(ops, clock):
    """Per op: is it in a fresh read at `clock` (a list over every DC)?  materializer:is_op_in_snapshot
    without a base or TxId."""
    out = []
    for op in ops:
        ent = dict(op.snap)
        ent[op.commit_dc] = op.commit_time
        out.append(all(clock[d] >= x for d, x in ent.items()))
    return out


# ---------------------------------------------------------------- records and survivors
def records(t, op):
    """(births [(a, b)], kills [kill key]) of one op in the order the kernels emit them
    (am_block.h set_effects): AW births (elem, tok), kills (tok, elem); MV kills (tok, 0) first, then
    the birth (value, tok)."""
    if t == AW:
        b = [(e, x) for e, add, _ in op.effect for x in add]
        k = [(x, e) for e, _, rm in op.effect for x in rm]
        return b, k
    eff = op.effect
    if eff[0] == "reset":
        return [], [(x, 0) for x in eff[1]]
    return [(eff[1], eff[2])], [(x, 0) for x in eff[3]]


def kill_key(t, birth):
    a, b = birth
    return (b, a) if t == AW else (b, 0)


def chunk_records(t, ops, incl):
    """Per 1024-op chunk: (births [(pos, (a, b))], kills [(pos, key)]) of the included ops, in op
    order -- the order in which a chunk's workgroup claims its LDS list slots, lane by lane."""
    out = []
    for c0 in range(0, len(ops), CHUNK):
        bs, ks = [], []
        for p in range(c0, min(c0 + CHUNK, len(ops))):
            if incl[p]:
                b, k = records(t, ops[p])
                if t == MV:  # kills first
                    ks += [(p, x) for x in k]
                    bs += [(p, x) for x in b]
                else:        # entry by entry: births, then kills; the two lists are independent
                    bs += [(p, x) for x in b]
                    ks += [(p, x) for x in k]
        out.append((bs, ks))
    return out


def kill_counts(t, ops, incl):
    """kill key -> number of included kills of it in the whole key."""
    n = {}
    for p, op in enumerate(ops):
        if incl[p]:
            for k in records(t, op)[1]:
                n[k] = n.get(k, 0) + 1
    return n


def survivors(t, ops, incl, base=()):
    """The surviving pairs of a read that includes `incl` over the base pairs `base`, by the
    sequential definition (antidote_crdt_set_aw / register_mv update): a set, unordered."""
    live = {}
    for a, b in base:
        live.setdefault(kill_key(t, (a, b)), set()).add((a, b))
    for p, op in enumerate(ops):
        if not incl[p]:
            continue
        b, k = records(t, op)
        for x in k:
            live.pop(x, None)
        for x in b:
            live.setdefault(kill_key(t, x), set()).add(x)
    return {x for s in live.values() for x in s}


# ---------------------------------------------------------------- 1 / 2: AW list overflows
TOK = 1 << 20      # tokens of the hand-made keys
NEVER = 1 << 30    # tokens no op adds


def _aw_effect(adds, rms):
    """[(elem, [add tokens], [remove tokens])] sorted by elem from (elem, tok) lists."""
    ents = {}
    for e, x in adds:
        ents.setdefault(e, ([], []))[0].append(x)
    for e, x in rms:
        ents.setdefault(e, ([], []))[1].append(x)
    return [(e, a, r) for e, (a, r) in sorted(ents.items())]


def aw_births_overflow(n_dc, n_ops=4200):
    """An AW key whose every chunk births 4 x LB pairs: op i adds tokens 4i, 4i + 1 to element
    i % 6 and 4i + 2, 4i + 3 to element 6 + i % 5 (two tokens per element in one effect).  About
    three quarters of a chunk's births find the LDS list full and are exported unresolved
    (am_big.hip birth_s -> gbirth).  Kills, one per op at most (<= LK per chunk):
      i % 3 != 0: token 4 (i - 2) + i % 4, born two ops earlier -- in the same chunk but for a
                  chunk's first two ops; its only kill, so past the first LB / 4 ops of a chunk
                  only the global pass (k_big_hash / k_big_kill) can apply it;
      i % 3 == 0, i >= 1100: token 4 (i - 1100) + 1, a live token of an earlier chunk.
    Roughly 3 of 4 births survive (more than SCAP: the read also sorts outside LDS)."""
    def elem(j, k):
        return j % 6 if k < 2 else 6 + j % 5

    effs = []
    for i in range(n_ops):
        adds = [(elem(i, k), TOK + 4 * i + k) for k in range(4)]
        rms = []
        if i % 3 != 0 and i >= 2:
            rms.append((elem(i - 2, i % 4), TOK + 4 * (i - 2) + i % 4))
        elif i % 3 == 0 and i >= 1100:
            rms.append((elem(i - 1100, 1), TOK + 4 * (i - 1100) + 1))
        effs.append(_aw_effect(adds, rms))
    return stamp(AW, effs, n_dc)


def aw_kills_overflow(n_dc, n_ops=4200):
    """An AW key whose every full chunk holds 3 x 1024 kills (> LK) and 1024 births (<= LB): op i
    adds token i to element i % 7 and removes three tokens:
      a. token i - 3 (i % 5 != 0; its only kill; the same chunk but for a chunk's first three ops),
         else a token never born -- so the tokens j with j % 5 == 2 outlive their chunk;
      b. i >= 1100: the live token j <= i - 1100 with j % 5 == 2 nearest below, if j % 10 == 2 (a
         live token of an earlier chunk; the other half stays alive), else a token never born;
      c. a token never born.
    The kills past the first LK of a chunk go straight to the global records (am_big.hip kills ->
    gkill): those of kind a are the only kill of a birth of that same chunk."""
    effs = []
    for i in range(n_ops):
        rms = []
        if i % 5 != 0 and i >= 3:
            rms.append(((i - 3) % 7, TOK + i - 3))
        else:
            rms.append((i % 7, NEVER + 3 * i))
        j = i - 1100
        j -= (j - 2) % 5
        if i >= 1100 and j >= 0 and j % 10 == 2:
            rms.append((j % 7, TOK + j))
        else:
            rms.append(((i + 1) % 7, NEVER + 3 * i + 1))
        rms.append(((i + 2) % 7, NEVER + 3 * i + 2))
        effs.append(_aw_effect([(i % 7, TOK + i)], rms))
    return stamp(AW, effs, n_dc)


def list_overflow_witnesses(t, ops, incl, which):
    """Per chunk, the births of the chunk that only the global pass can kill because a list was
    full, in the op-order model: which == "births": births at list index >= LB whose single kill
    sits later in the same chunk; which == "kills": births whose single kill sits later in the same
    chunk at kill-list index >= LK.  -> [(n births, n kills, [witness pairs])]."""
    total = kill_counts(t, ops, incl)
    out = []
    for bs, ks in chunk_records(t, ops, incl):
        kpos = {}
        for idx, (p, k) in enumerate(ks):
            kpos.setdefault(k, []).append((p, idx))
        wit = []
        for idx, (p, b) in enumerate(bs):
            k = kill_key(t, b)
            if total.get(k) != 1 or k not in kpos:
                continue
            q, kidx = kpos[k][0]
            if q > p and (idx >= LB if which == "births" else kidx >= LK):
                wit.append(b)
        out.append((len(bs), len(ks), wit))
    return out


# ---------------------------------------------------------------- 3: the MV token hash
def mv_hash_overflow(n_dc, n_ops=2100, born_twice=False):
    """An MV key of three chunks whose assigns override three distinct tokens each: the previous
    op's token (its only kill) and two that were born in an earlier chunk or never: token
    j = i - 1030 when j % 20 == 9 (a survivor of an earlier chunk; those with j % 20 == 19 stay
    alive), else tokens never born.  One assign in ten (i % 10 == 0)
    overrides nothing, so token i - 1 survives it.  A full chunk kills about 2700 distinct tokens:
    more than the 2048 slots of the LDS token hash, so hash_kill fails for several hundred of them
    and those kills go to the global records.  Values repeat (i * 7919 % 1000).
    born_twice: op 2000 assigns token 100 again -- the key is outside the closed form, stays
    AM_NGRP_NONE, and a fresh read goes through k_big_chunk.  Without it the key is grouped and
    only a read over a cached base with pairs takes k_big_chunk."""
    effs = []
    for i in range(n_ops):
        ovr = []
        if i % 10 != 0:
            ovr.append(TOK + i - 1)
            j = i - 1030
            if j >= 0 and j % 20 == 9:
                ovr.append(TOK + j)
            else:
                ovr.append(NEVER + 2 * i)
            ovr.append(NEVER + 2 * i + 1)
        tok = TOK + 100 if born_twice and i == 2000 else TOK + i
        effs.append(("assign", (i * 7919) % 1000, tok, ovr))
    return stamp(MV, effs, n_dc)


def mv_hash_failures(ops, incl):
    """Per chunk: (distinct killed tokens, [kills (pos, tok) that find no slot in HPROBES probes],
    [births of the chunk whose single kill is one of those]) -- hash_kill in op order."""
    total = kill_counts(MV, ops, incl)
    out = []
    for bs, ks in chunk_records(MV, ops, incl):
        table, failed = {}, []
        for p, (tok, _) in ks:
            h = tok_slot(tok)
            for pr in range(HPROBES):
                sl = (h + pr) & (LK - 1)
                if table.setdefault(sl, tok) == tok:
                    break
            else:
                failed.append((p, tok))
        lost = dict((tok, p) for p, tok in failed)
        wit = [b for p, b in bs if total.get((b[1], 0)) == 1 and lost.get(b[1], -1) > p]
        out.append((len({k for _, k in ks}), failed, wit))
    return out


# ---------------------------------------------------------------- 4: the grouped mode's hash sets
GSET_OPS = 8192
GSET_CHUNK = 3        # the chunk that holds the window's births
GSET_KILLED = 80      # of them, overridden later in the same chunk
GSET_LATER = 20       # and overridden in chunk GSET_CHUNK + 2


def gset_window(n_groups):
    """(first start slot, the group ids < n_groups whose start slot lies in the 32 slots from it):
    the window of 32 consecutive start slots that holds most ids.  An id probes 32 slots from its
    start, so all of them compete for 32 + 31 = 63 slots."""
    per = [[] for _ in range(GH)]
    for g in range(n_groups):
        per[gslot(g)].append(g)
    best = max(range(GH), key=lambda s: sum(len(per[(s + k) % GH]) for k in range(GPROBES)))
    return best, sorted(g for k in range(GPROBES) for g in per[(best + k) % GH])


def mv_gset_overflow(n_dc):
    """A grouped MV key (8192 ops, distinct values 0 .. 8191, no token twice: group id = the
    value's rank = the value) whose chunk 3 cannot place its group ids in the LDS hash sets
    (am_big.hip grouped_records -> gset_insert):
      * the chunk's first m ops assign the m (about 127) values of gset_window(8192) and override
        nothing: m births that compete for 63 slots, so at least m - 63 inserts fail and their
        bits are ORed straight into the read's born bitmap;
      * its next 80 ops override one of those tokens each (and the previous op's): 80 kills for
        the same 63 slots of the kill set;
      * 20 ops of chunk 5 override 20 more of them; the rest (m - 100) survive.
    Every other op continues an override chain that breaks at i % 100 == 0 (a survivor)."""
    n = GSET_OPS
    _, win = gset_window(n)
    m = len(win)
    c0 = GSET_CHUNK * CHUNK
    inwin = set(win)
    rest = [v for v in range(n) if v not in inwin]
    random.Random(4).shuffle(rest)
    rest = iter(rest)
    effs = []
    for i in range(n):
        k = i - c0
        if 0 <= k < m:
            effs.append(("assign", win[k], TOK + i, []))
            continue
        ovr = [TOK + i - 1] if i % 100 != 0 and i > 0 and k != m else []
        if m <= k < m + GSET_KILLED:
            ovr.append(TOK + c0 + (k - m))
        k5 = i - (GSET_CHUNK + 2) * CHUNK
        if 0 <= k5 < GSET_LATER:
            ovr.append(TOK + c0 + GSET_KILLED + k5)
        effs.append(("assign", next(rest), TOK + i, ovr))
    return stamp(MV, effs, n_dc)


def gset_failures(ops, incl):
    """Per chunk: (births that find no slot, kills that find no slot) of the two group-id hash
    sets, inserting in op order; group id = value (mv_gset_overflow's values are their ranks)."""
    group = {op.effect[2]: op.effect[1] for op in ops}  # token -> group id
    out = []
    for bs, ks in chunk_records(MV, ops, incl):
        fails = []
        for ids in ([b[0] for _, b in bs], [group[k[0]] for _, k in ks if k[0] in group]):
            table, f = {}, 0
            for g in ids:
                s0 = gslot(g)
                for pr in range(GPROBES):
                    if table.setdefault((s0 + pr) & (GH - 1), g) == g:
                        break
                else:
                    f += 1
            fails.append(f)
        out.append(tuple(fails))
    return out


# ---------------------------------------------------------------- 5: survivors against SCAP
MANY_OPS = 4200


def _keep(n_ops, weight, target, tail):
    """The ops whose births stay alive: the last `tail` ops (nothing follows to kill them), then
    ops j with j % 4 != 0 from the oldest on until their births number `target` exactly."""
    keep = set(range(n_ops - tail, n_ops))
    have = sum(weight(j) for j in keep)
    for j in range(n_ops - tail):
        if have == target:
            break
        if j % 4 != 0 and have + weight(j) <= target:
            keep.add(j)
            have += weight(j)
    assert have == target, (have, target)
    return keep


def aw_many_survivors(n, n_dc, n_ops=MANY_OPS):
    """An AW key past AM_SETS_BIG_OPS with exactly n surviving pairs at its newest clock.  Op i adds
    token 2i to element i % 5, and when i % 7 == 0 token 2i + 1 with it (two in one effect); it
    removes op i - 5's tokens (the same element) unless that op is kept (_keep).  Each of the five
    elements so holds hundreds of live tokens born in different ops and two in one op, which fixes
    the output order: newest birth first, the effect's token order, base tokens last."""
    def weight(j):
        return 2 if j % 7 == 0 else 1

    keep = _keep(n_ops, weight, n, 5)
    effs = []
    for i in range(n_ops):
        adds = [(i % 5, TOK + 2 * i)] + ([(i % 5, TOK + 2 * i + 1)] if i % 7 == 0 else [])
        j = i - 5
        rms = []
        if j >= 0 and j not in keep:
            rms = [(j % 5, TOK + 2 * j)] + ([(j % 5, TOK + 2 * j + 1)] if j % 7 == 0 else [])
        effs.append(_aw_effect(adds, rms))
    return stamp(AW, effs, n_dc)


def mv_many_survivors(n, n_dc, n_ops=MANY_OPS):
    """An MV key past AM_SETS_BIG_OPS with exactly n surviving (value, token) pairs at its newest
    clock: op i assigns value i % 50 under token i (equal values under many tokens: the (value,
    token) order has ties on the value) and overrides op i - 1's token unless that op is kept.
    No token is born twice: a fresh read is grouped; over a cached base with pairs it goes through
    k_big_chunk and the sort of k_big_finish."""
    keep = _keep(n_ops, lambda j: 1, n, 1)
    effs = [("assign", i % 50, TOK + i, [TOK + i - 1] if i > 0 and i - 1 not in keep else []) for i in range(n_ops)]
    return stamp(MV, effs, n_dc)


# ---------------------------------------------------------------- 6: sums on the int64 edges
def edge_positions(n_ops):
    """Where edge amounts are planted: the first and the last op and either side of every 256-op
    boundary (every 1024-op boundary is one)."""
    pos = {0, n_ops - 1}
    for b in range(256, n_ops, 256):
        pos |= {b - 1, b}
    return sorted(pos)


def plant_positions(n_ops, k, turn=0):
    """k distinct op positions, ascending: spread over edge_positions (rotated by `turn`, so that
    the keys of one list share the boundaries out) when those are enough, else evenly over the key."""
    pos = edge_positions(n_ops)
    if len(pos) < k:
        pos = list(range(n_ops))
        turn = 0
    pos = pos[turn % len(pos):] + pos[:turn % len(pos)]
    at = [pos[0]] if k == 1 else [pos[round(j * (len(pos) - 1) / (k - 1))] for j in range(k)]
    assert len(set(at)) == k, (n_ops, k)
    return sorted(at)


def _climb(n_ops):
    """Amounts that climb by INT64_MAX steps (past 2^65 when the key has room for five) and come
    back to 7."""
    k = max(1, min(5, (n_ops - 1) // 2))
    return [INT64_MAX] * k + [-INT64_MAX] * k + [7]


# name -> (parts, wanted status at the newest clock): the parts' exact sum is the edge
def edge_sums(n_ops):
    return {
        "max_ok": ([1 << 62, (1 << 62) - 1], "ok"),                      # INT64_MAX
        "max_ovf": ([1 << 62, 1 << 62], "overflow"),                     # INT64_MAX + 1
        "min_ok": ([-(1 << 62), -(1 << 62)], "ok"),                      # INT64_MIN
        "min_ovf": ([-(1 << 62), -(1 << 62) - 1], "overflow"),           # INT64_MIN - 1
        "p64": ([INT64_MAX, INT64_MAX, 2], "overflow"),                  # 2^64: low word 0, high word 1
        "m64": ([INT64_MIN, INT64_MIN], "overflow"),                     # -2^64: low word 0, high word -1
        "climb": (_climb(n_ops), "ok"),                                  # ... and back to 7
    }


def pn_edge_keys(n_ops, n_dc, seed=0):
    """[{name, ops, base, want, total}]: PN keys of n_ops ops whose sum is an edge of edge_sums,
    its parts planted at edge_positions and the rest small amounts (+-1000) that sum to zero; and
    two keys read over a base value: INT64_MAX with ops summing to -5, INT64_MIN with ops summing to
    +5 (want holds for the read over the base; base None = a fresh read)."""
    rng = random.Random(600 + seed + n_ops)
    cases = [(nm, parts, want, None) for nm, (parts, want) in edge_sums(n_ops).items()]
    cases += [("base_max", [-5], "ok", INT64_MAX), ("base_min", [5], "ok", INT64_MIN)]
    out = []
    for ci, (nm, parts, want, base) in enumerate(cases):
        amounts = [rng.randint(-1000, 1000) for _ in range(n_ops)]
        assert len(parts) <= n_ops, (nm, n_ops)
        at = plant_positions(n_ops, len(parts), ci)
        for p in at:
            amounts[p] = 0
        free = [p for p in range(n_ops) if p not in set(at)]
        if free:  # the filler sums to zero
            amounts[free[-1]] -= sum(amounts)
        for p, v in zip(at, parts):
            amounts[p] = v
        total = sum(amounts) + (base or 0)
        assert total == sum(parts) + (base or 0)
        assert (want == "ok") == (INT64_MIN <= total <= INT64_MAX)
        out.append(dict(name=nm, ops=stamp(PN, amounts, n_dc), base=base, want=want, total=total))
    return out


def _bc_effect(n_dc, slot, v):
    """One (slot, amount) entry as an effect: P[f][f] an increment, P[f][t] a transfer, D[i] a
    decrement (am_block.h bc_slot)."""
    if slot >= n_dc * n_dc:
        return ("decrement", v, slot - n_dc * n_dc)
    f, t = divmod(slot, n_dc)
    return ("increment", v, f) if f == t else ("transfer", v, t, f)


def bc_slot_of(n_dc, eff):
    if eff[0] == "decrement":
        return n_dc * n_dc + eff[2]
    if eff[0] == "increment":
        return eff[2] * n_dc + eff[2]
    return eff[3] * n_dc + eff[2]


def bc_edge_keys(n_ops, n_dc, seed=0):
    """[{name, ops, base, want, slot, total}]: bounded-counter keys of n_ops ops with one slot on an
    edge and every other slot small (amounts 1 .. 50 on random other slots).  The slot rotates over
    P[0][1] (P[0][0] at one DC), the last P slot P[n_dc-1][n_dc-1] and the last D slot; the oracle
    takes an amount as int64, so parts may be negative.
      edge_sums           each of its sums, parts at edge_positions
      neg                 a slot summing to -3 from +-INT64_MAX and +-2^62 parts
      defer / nodefer     one amount of exactly 2^56 (the row tier defers the read) / 2^56 - 1
      flush               2^62 at ops n/8, 3n/8, 5n/8, 7n/8: four different chunks when the key is in
                          the big tier, each chunk's sum fits 64 bits, the carry to 2^64 happens only
                          at the flush into the read's global slots
      base_max{,_ovf}     a base snapshot with the slot at INT64_MAX - 10, ops adding 10 (11)
      base_neg{,_ovf}     a base snapshot with the slot at INT64_MIN + 3, ops adding -3 (-4)
    want / total hold for the read at the newest clock over the base (None: fresh)."""
    rng = random.Random(700 + seed + n_ops + 31 * n_dc)
    np_ = n_dc * n_dc
    slots = [min(1, n_dc - 1), np_ - 1, np_ + n_dc - 1]
    cases = [(nm, parts, want, None, None) for nm, (parts, want) in edge_sums(n_ops).items()]
    cases.append(("neg", [INT64_MAX, -INT64_MAX, 1 << 62, -(1 << 62) - 3], "ok", None, None))
    cases.append(("defer", [DEFER, 5], "ok", None, None))
    cases.append(("nodefer", [DEFER - 1, 5], "ok", None, None))
    eighths = [min(n_ops - 1, (2 * j + 1) * n_ops // 8) for j in range(4)]
    if len(set(eighths)) == 4:
        cases.append(("flush", [1 << 62] * 4, "overflow", None, eighths))
    cases += [("base_max", [4, 6], "ok", INT64_MAX - 10, None), ("base_max_ovf", [5, 6], "overflow", INT64_MAX - 10, None),
              ("base_neg", [-1, -2], "ok", INT64_MIN + 3, None), ("base_neg_ovf", [-2, -2], "overflow", INT64_MIN + 3, None)]
    out = []
    for ci, (nm, parts, want, base, at) in enumerate(cases):
        if len(parts) > n_ops:
            continue
        slot = slots[ci % 3]
        others = [s for s in range(np_ + n_dc) if s != slot]
        effs = [_bc_effect(n_dc, rng.choice(others), rng.randint(1, 50)) for _ in range(n_ops)]
        if at is None:
            at = plant_positions(n_ops, len(parts), ci)
        for p, v in zip(at, parts):
            effs[p] = _bc_effect(n_dc, slot, v)
        total = sum(parts) + (base or 0)
        assert (want == "ok") == (INT64_MIN <= total <= INT64_MAX)
        # a base snapshot: the slot and one small other entry, as the ABI's value (P dict, D dict)
        bval = None
        if base is not None:
            pd, dd = {}, {}
            for s, v in ((slot, base), (others[0], 9)):
                if s < np_:
                    pd[divmod(s, n_dc)] = v
                else:
                    dd[s - np_] = v
            bval = (pd, dd)
        out.append(dict(name=nm, ops=stamp(BC, effs, n_dc), base=bval, want=want, slot=slot, total=total))
    return out


def bc_slot_sum(n_dc, ops, incl, slot, base=0):
    """The exact (Python integer) sum of one slot over the included ops."""
    return base + sum(op.effect[1] for p, op in enumerate(ops) if incl[p] and bc_slot_of(n_dc, op.effect) == slot)
