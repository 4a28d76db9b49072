"""Host side of tests/test_gpu_split_after_apply.py: a store ingested in place, as a host model.

A log of 40 keys in three states -- as am_store_reserve lays it out, after a round of appends (A)
and after a round of GC prunes with some appends (B), both through am_store_apply -- with, per
state, the merged ops and their op ids as op_insert_gc/3 and prune_ops/2 leave them, and the
store's slot offsets from the room rule of antidote_amd/csrc/am_gc.hip slack_cap (they never move:
every apply must fit).  The rows (ROWS) put a key where the split fresh read's inclusion pass
(csrc/am_group_split.h k_grp_incl) cuts it differently after the apply: segment, tile and bitmap
word counts that change in place, lag bases that move, keys that become routed or unrouted, an
escaped quad written in place, a key pruned to empty, untouched keys behind freed slots.  The
checks here need no GPU (tests/test_split_after_apply_cpu.py runs them on the model; the GPU
module runs them again on the log the store gives back)."""
import dataclasses
import random

import numpy as np

from antidote_amd import abi
from antidote_amd.oplog import HostLog, Op
from tests import randlog
from tests.test_gpu_incl_compact import LAGMAX, SEG, T0, TILE, segment_lists, steer, times
from tests.test_gpu_incl_deferred import FAR, LAG_ONLY, plant
from tests.test_gpu_lagcadence import view_counts

CASES = [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3), (abi.AM_AWSET, 1), (abi.AM_AWSET, 5)]
COUNTS = [0, 1, 63, 64, 65, 129]   # entries of key a's list under the steered clocks
QUAD = [2, 3]                      # and two more: a list inside one lane's four ops
N_KEYS = 40
BIG_MIN_OPS = 1024                 # AM_BIG_MIN_OPS (include/antidote_mat.h): an MV key of more ops is the big tier's
# row -> (size, us between ops, timeline); the size is a position from t0 = slot offset & ~31 for
# the rows of POSITIONED, else an op count
ROWS = {"a": (1000, 1000, "asc"), "b": (250, 100, "asc"), "c": (2040, 30, "asc"), "d": (1100, 100, "asc"),
        "e": (600, 120, "asc"), "f": (300, 1000, "asc"), "g": (300, 1000, "asc"), "h": (300, 200, "asc"),
        "i": (400, 150, "asc"), "j": (300, 1000, "asc"), "k": (500, 200, "shuffled"), "l": (200, 300, "asc"),
        "m": (1020, 100, "asc"), "o": (4200, 10, "asc")}
POSITIONED = "abcde"
N_KINDS = [(300, 1000, "asc"), (280, 100, "inter"), (310, 10, "shuffled"), (290, 100, "asc"), (300, 300, "inter")]
# key index -> row; every other index holds a filler of 70 .. 74 ops.  n: the untouched keys (batch
# slots 0, 31, 32, and behind d and e); h sits in the second wave batch, among clean reads; 30 is a
# filler that grows to its room in round A and is pruned in round B, in front of slot 31
ORDER = {0: "n", 1: "a", 3: "b", 4: "c", 6: "d", 7: "n", 9: "e", 10: "n", 11: "f", 12: "g", 14: "i", 15: "j",
         16: "k", 17: "l", 18: "m", 19: "o", 31: "n", 32: "n", 33: "h"}
GROWN = 30
ESC_ROWS = "fghij"                 # rows that need a second DC (escapes, routing)
APPEND_A = {"a": 24, "b": 7, "c": 9, "f": 1, "h": 48, "j": 12, "m": 10, "o": 20}
APPEND_B = {"a": 1, "c": 5, "d": 3}
PRUNE_B = {"d": 150, "g": 10, "i": 150}  # the oldest ops go (e: its older two thirds; k, l, GROWN: below)
I_ESCAPED = 60                     # of key i's first 150 ops


def cap_of(n):
    """slack_cap: a key of n ops gets room for a quarter more, four at least."""
    return n + max(n // 4, 4)


def slot_offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum([cap_of(int(n)) for n in lens])
    return off


def row_of(ki, t, n_dc):
    r = ORDER.get(ki)
    if r is not None and ((n_dc == 1 and r in ESC_ROWS) or (r == "m" and t != abi.AM_MVREG)):
        return None
    return r


def layout(t, n_dc):
    """[(row or None, ops, step, timeline)] per key: op counts chosen from the slot offsets."""
    out, off, nth = [], 0, 0
    for ki in range(N_KEYS):
        r = row_of(ki, t, n_dc)
        if r is None:
            n, step, kind = 70 + ki % 5, 1000, "asc"
        elif r == "n":
            n, step, kind = N_KINDS[nth % len(N_KINDS)]
            nth += 1
        else:
            n, step, kind = ROWS[r]
            if r in POSITIONED:
                n -= off % 32
        out.append((r, n, step, kind))
        off += cap_of(n)
    return out


# ---------------------------------------------------------------- ops
def _stamp(ops, tl):
    for op, (ct, dc, back) in zip(ops, tl):
        op.commit_dc, op.commit_time = dc, ct
        op.snap = {d: ct - back[d] for d in back}


def later(rng, ops, m, n_dc, step):
    """Commit times and entries of m ops behind the key's newest, as times() makes them."""
    quiet = n_dc - 1 if n_dc > 1 else None
    committers = [d for d in range(n_dc) if d != quiet]
    last = max(op.commit_time for op in ops)
    return [(last + (j + 1) * step + rng.randrange(step), rng.choice(committers),
             {d: rng.randint(1, 9000) for d in range(n_dc)}) for j in range(m)]


def mv_live(ops):
    live = []
    for op in ops:
        e = op.effect
        ovr = e[1] if e[0] == "reset" else e[3]
        live = [x for x in live if x not in ovr] + ([] if e[0] == "reset" else [e[2]])
    return live


def new_ops(rng, t, n_dc, ops, m, step, book):
    """m ops appended to a key whose ops are `ops`.  AW: adds of one fresh token of a fresh element
    observing nothing, every fifth op a remove of one such live token; MV: assigns overriding
    exactly one live token -- two records an op at most, the record room of a free slot."""
    out = []
    for ct, dc, back in later(rng, ops, m, n_dc, step):
        book["n"] = book.get("n", 0) + 1
        tok = book["tok0"] + book["n"]
        if t == abi.AM_AWSET:
            mine = book.setdefault("live", [])
            if mine and book["n"] % 5 == 0:
                e, old = mine.pop(0)
                eff = [(e, [], [old])]
            else:
                eff = [(1000 + book["n"], [tok], [])]
                mine.append((1000 + book["n"], tok))
        else:
            live = mv_live(ops + out)
            eff = ("assign", book["n"], tok, live[-1:])
        out.append(Op(t, dc, ct, {d: ct - back[d] for d in back}, eff))
    return out


def survives(op, thr):
    """prune_ops/2 with the same threshold on every DC: an entry above it keeps the op."""
    return op.commit_time > thr or any(x > thr for d, x in op.snap.items() if d != op.commit_dc)


class Model:
    """states[s] = (ops per key, op ids per key); rounds[s - 1] = (touched keys, new ops per touched
    key, prune threshold per key or None) leads from state s - 1 to state s."""

    def __init__(self, t, n_dc):
        rng = random.Random(9900 + 10 * t + n_dc)
        self.t, self.n_dc, self.lay = t, n_dc, layout(t, n_dc)
        self.idx = {r: [k for k, l in enumerate(self.lay) if l[0] == r] for r in list(ROWS) + ["n", None]}
        self.key = {r: ks[0] for r, ks in self.idx.items() if ks and r not in ("n", None)}
        quiet = n_dc - 1
        keys = []
        for ki, (r, n, step, kind) in enumerate(self.lay):
            ops = randlog.rand_key_ops(rng, t, n_dc, n)
            _stamp(ops, times(rng, n, n_dc, step, kind))
            if r == "g":  # op 2 alone sets the quiet DC's base (1); op 200 lies 65536 above it
                for i, op in enumerate(ops):
                    back = op.commit_time - op.snap[quiet]
                    op.snap[quiet] = op.commit_time - (1 if i == 2 else 1 + LAGMAX + 1 if i == 200 else max(back, 2))
            if r == "i":
                for i in range(0, 150, 5):
                    plant(ops, i, n_dc, LAG_ONLY[i % len(LAG_ONLY)], rng)
                    plant(ops, i + 2, n_dc, LAG_ONLY[(i + 1) % len(LAG_ONLY)], rng)
            keys.append(ops)
        self.slot_off = slot_offsets([len(o) for o in keys])
        self.states = [(keys, [list(range(1, len(o) + 1)) for o in keys])]
        self.rounds = []
        self.books = [{"tok0": (1 << 40) + (k << 20)} for k in range(N_KEYS)]
        fill = self.idx[None]
        self._round(rng, {self.key[r]: m for r, m in APPEND_A.items() if r in self.key}
                    | {GROWN: 12, fill[0]: 1, fill[3]: 3}, {})
        old = self.states[1][0]
        prune = {self.key[r]: old[self.key[r]][m - 1].commit_time for r, m in PRUNE_B.items() if r in self.key}
        e, k, l = self.key["e"], self.key["k"], self.key["l"]
        prune[e] = old[e][2 * len(old[e]) // 3 - 1].commit_time
        prune[GROWN] = old[GROWN][2 * len(old[GROWN]) // 3 - 1].commit_time
        prune[k] = sorted(op.commit_time for op in old[k])[2 * len(old[k]) // 5]  # keeps ops all over the key
        prune[l] = max(op.commit_time for op in old[l]) + 1000
        self._round(rng, {self.key[r]: m for r, m in APPEND_B.items()} | {fill[1]: 2, fill[3]: 1}, prune)

    def _round(self, rng, appends, prune):
        ops0, ids0 = self.states[-1]
        s = len(self.states)
        touched = sorted(set(appends) | set(prune))
        ops1, ids1, new = [list(o) for o in ops0], [list(i) for i in ids0], []
        for k in touched:
            r, step = self.lay[k][0], self.lay[k][2]
            ctr = ids0[k][-1] if ids0[k] else 0  # OpCounter: ids are never reused (no key here is empty before a round)
            if k in prune:
                keep = [j for j, op in enumerate(ops0[k]) if survives(op, prune[k])]
                ops1[k], ids1[k] = [ops0[k][j] for j in keep], [ids0[k][j] for j in keep]
            add = new_ops(rng, self.t, self.n_dc, ops0[k], appends.get(k, 0), step, self.books[k])
            merged = ops1[k] + add
            n0 = len(ops1[k])
            if r == "f":  # an entry of the quiet DC with lag 0: below the key's base there (1)
                add[0].snap[self.n_dc - 1] = add[0].commit_time
            if r == "h":  # every appended op a lag-only escape: more than an eighth of the merged key
                for j in range(n0, len(merged)):
                    plant(merged, j, self.n_dc, LAG_ONLY[j % len(LAG_ONLY)], rng)
            if r == "j" and s == 1:  # a lag-only and a packed escape in one lane's four slots
                q = -(-(int(self.slot_off[k]) + n0 + 4) // 4) * 4 - int(self.slot_off[k])
                assert n0 < q and q + 2 < len(merged) - 2
                plant(merged, q, self.n_dc, LAG_ONLY[0], rng)
                plant(merged, q + 2, self.n_dc, FAR, rng)
                self.j_quad = q
            ops1[k] = merged
            ids1[k] += list(range(ctr + 1, ctr + 1 + len(add)))
            new.append(add)
            assert len(merged) + 1 <= cap_of(len(self.states[0][0][k])), (k, r, "outgrows its room")
        thr = {k: prune[k] for k in touched if k in prune}
        self.rounds.append((touched, new, thr))
        self.states.append((ops1, ids1))

    # ---- what the tests hand to the store and read back
    def host_log(self, s, ids=False):
        ops, idl = self.states[s]
        if ids:
            ops = [[dataclasses.replace(op, op_id=i) for op, i in zip(o, il)] for o, il in zip(ops, idl)]
        return HostLog(self.n_dc, ops, key_types=[self.t] * N_KEYS)

    def apply_args(self, s):
        """(touched, new-op log, prune arrays or None) of the round that leads to state s."""
        touched, new, thr = self.rounds[s - 1]
        prune = None
        if thr:
            mask = np.zeros(N_KEYS, np.uint8)
            tv = np.zeros((self.n_dc, N_KEYS), np.uint64)
            tp = np.zeros(N_KEYS, np.uint32)
            for k, x in thr.items():
                mask[k], tv[:, k], tp[k] = 1, x, (1 << self.n_dc) - 1
            prune = (mask, tv, tp)
        return touched, HostLog(self.n_dc, new, key_types=[self.t] * len(touched)), prune

    def lens(self, s):
        return [len(o) for o in self.states[s][0]]


_MODELS = {}


def model(t, n_dc):
    """The model of a case, built once and never changed."""
    if (t, n_dc) not in _MODELS:
        _MODELS[t, n_dc] = Model(t, n_dc)
    return _MODELS[t, n_dc]


# ---------------------------------------------------------------- the checks, on any log of a state
def read_clocks(m, s, log):
    """[(clock, presence mask or None, kind)] of the batches read in state s.  log: the state's ops
    as a dense log (the model's, or the store's own)."""
    n_dc, a = m.n_dc, m.key["a"]
    ops = [op for o in m.states[s][0] for op in o]
    byct = sorted(op.commit_time for op in ops)
    # key a's oldest segment holds the ops the steering sweeps: its only one, until round B
    seg = len(segment_lists(log, a, [T0] * n_dc, None, m.slot_off)) - 1
    found = steer(log, a, COUNTS + QUAD, m.slot_off, seg)
    assert sorted(found) == sorted(COUNTS + QUAD), found
    clocks = [([found[c]] * n_dc, None, "steered") for c in COUNTS + QUAD]
    clocks += [([T0 - 200_000] * n_dc, None, "below"), ([byct[-1] + 1000] * n_dc, None, "above"),
               ([byct[len(byct) // 2]] * n_dc, None, "mid"), ([byct[len(byct) * 3 // 4]] * n_dc, None, "mid"),
               ([T0 + 55_000] * n_dc, None, "mid")]  # inside every key
    if n_dc > 1:
        clocks.append(([T0 + 55_000] * n_dc, ((1 << n_dc) - 1) & ~2, "lacks"))
    return clocks


def coverage(m, s, log, clocks):
    """What the batches' lists look like in state s, by the host rule over the store's slots."""
    so, lens = m.slot_off, m.lens(s)
    a, c = m.key["a"], m.key["c"]
    cov = dict(whole_seg=False, tile_edge=False, seg_edge=False, one_quad=False, mid_window=True)
    if s >= 1:
        cov["seg_edge_c"] = False
    if s == 2:
        cov.update(seg_edge_a=False, before_freed=False)
    sizes, a_sizes = set(), set()
    for clock, pres, kind in clocks:
        for k in range(N_KEYS):
            segs = segment_lists(log, k, clock, pres, so)
            assert pres is None or all(len(w) == 0 for w in segs)
            for j, w in enumerate(segs):
                sizes.add(len(w))
                if k == a and kind == "steered":
                    a_sizes.add(len(w))
                cov["whole_seg"] |= len(w) == SEG
                if len(w) == 0:
                    continue
                cov["tile_edge"] |= len(set(w // TILE)) > 1
                cov["one_quad"] |= 1 < len(w) <= 4 and len(set(w // 4)) == 1
                if s == 2 and j == 0 and lens[k] < m.lens(1)[k]:  # the newest segment of a key that shrank
                    t0 = int(so[k]) & ~31
                    end = int(so[k]) + lens[k] - t0 - (len(segs) - 1) * SEG  # key_end, from the segment's start
                    cov["before_freed"] |= bool(((w >= end - 32) & (w < end)).any())
            edge = sum(1 for w in segs if len(w)) > 1
            cov["seg_edge"] |= edge
            if k == c and s >= 1:
                cov["seg_edge_c"] |= edge
            if k == a and s == 2:
                cov["seg_edge_a"] |= edge
            if kind == "mid" and m.lay[k][0] is not None and lens[k]:
                cov["mid_window"] &= any(len(w) for w in segs)
    cov["sizes"] = set(COUNTS) <= a_sizes and set(COUNTS) <= sizes
    return cov


def check_layout(m, s, log):
    """The rows are where the table puts them (positions from t0 = slot offset & ~31)."""
    so, lens = m.slot_off, m.lens(s)
    assert len(lens) == N_KEYS and [int(x) for x in np.diff(np.asarray(log.key_off).astype(np.int64))] == lens
    pos = {r: int(so[k]) % 32 + lens[k] for r, k in m.key.items()}
    cap = [int(so[k + 1] - so[k]) for k in range(N_KEYS)]
    assert all(lens[k] + 1 <= cap[k] for k in range(N_KEYS))
    want = {"a": (1000, 1024, 1025), "b": (250, 257, 257), "c": (2040, 2049, 2054)}
    for r, w in want.items():
        assert pos[r] == w[s], (r, pos[r])
    assert (pos["d"] == 1100) if s < 2 else (pos["d"] < SEG and lens[m.key["d"]] > 900), pos["d"]
    e0 = m.lens(0)[m.key["e"]]
    assert (pos["e"] == 600) if s < 2 else (e0 // 3 <= lens[m.key["e"]] <= e0 // 3 + 2), pos["e"]
    assert lens[m.key["o"]] == (4200, 4220, 4220)[s] and lens[m.key["l"]] == (200, 200, 0)[s]
    assert (lens[GROWN] == (70, 82)[s] if s < 2 else 26 <= lens[GROWN] <= 30) and cap[GROWN] == 87
    if "m" in m.key:
        assert lens[m.key["m"]] == (1020, 1030, 1030)[s] and 1020 <= BIG_MIN_OPS < 1030
    # the untouched keys: batch slots 0, 31 and 32, and behind d and e, their t0 inside the neighbour's room
    ns = m.idx["n"]
    assert ns == [0, m.key["d"] + 1, m.key["e"] + 1, 31, 32] and all(lens[k] == m.lens(0)[k] for k in ns)
    assert all(int(so[k]) % 32 for k in ns[1:])
    if s == 2:  # k's survivors are not consecutive: the store needs the explicit op id column
        ids = m.states[2][1][m.key["k"]]
        assert len(ids) > 100 and any(b - a > 1 for a, b in zip(ids, ids[1:]))


def check_view(m, s, log):
    """The view statistics of state s by the definition, with the flips the rows are there for."""
    stats, routed, lag_only = view_counts(log)
    ko = np.asarray(log.key_off).astype(np.int64)
    per = [int(lag_only[ko[k]:ko[k + 1]].sum()) for k in range(N_KEYS)]
    if m.n_dc == 1:
        assert stats["routed_keys"] == 0 and stats["lag_only_esc_ops"] == 0 and stats["pk_esc_ops"] == 0, stats
        return stats
    f, g, h, i, j = (m.key[r] for r in ESC_ROWS)
    assert bool(routed[h]) == (s >= 1) and bool(routed[i]) == (s < 2), (s, routed[h], routed[i])
    assert stats["routed_keys"] == (1, 2, 1)[s], stats
    assert per[f] == (0, 1, 1)[s] and per[g] == (1, 1, 0)[s], (s, per[f], per[g])
    assert per[h] == (0, APPEND_A["h"], APPEND_A["h"])[s] and per[i] == (I_ESCAPED, I_ESCAPED, 0)[s], (per[h], per[i])
    assert per[j] == (0, 1, 1)[s] and stats["pk_esc_ops"] == (0, 1, 1)[s], (per[j], stats)
    assert sum(per) == per[f] + per[g] + per[h] + per[i] + per[j]
    return stats


def check_state(m, s, log):
    """Every host-side condition of state s on `log`; returns (clocks, view statistics)."""
    check_layout(m, s, log)
    stats = check_view(m, s, log)
    clocks = read_clocks(m, s, log)
    cov = coverage(m, s, log, clocks)
    assert all(cov.values()), (s, cov)
    return clocks, stats
