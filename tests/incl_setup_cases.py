"""Host logs and clocks for the tests of the inclusion pass's lane-parallel set-up (csrc/am_group_split.h:
lane j of a wave batch computes read j's thresholds, lag bases and window limits into its LDS slot).
Every case is one or two batches of 32 reads; what can go wrong is the slot, so neighbouring reads
differ in everything a slot holds: the key's time base K, its lag base on every DC (some negative),
its length and where its ops lie under the clock.  Shared by tests/test_gpu_incl_setup.py (the device
against the oracle) and tests/test_incl_setup_cpu.py (the same inputs checked on the host alone)."""
import random

import numpy as np

from antidote_amd import abi
from antidote_amd.oplog import HostLog
from tests import randlog
from tests.test_gpu_incl_compact import host_view, segment_lists
from tests.test_gpu_incl_deferred import FAR, LAG_ONLY, plant

T0 = 1_700_000_000_000_000
SEG, LAGMAX = 1024, 0xFFFF
LATE = 1 << 33  # us after its key's first op: the op's packed entries lie 2^32 and more above K


def key_ops(rng, t, n_dc, n, start, step, ki):
    """n ops from T0 + start, step us apart.  The key commits on two DCs (which, by ki) and the
    others only trail: DC d's entries lie shift(ki, d) + 1 .. 9000 us behind the commit time, the
    shift between -20 and +20 ms -- so every key has its own lag base on every DC, negative where
    the entries run ahead of the commit times."""
    ops = randlog.rand_key_ops(rng, t, n_dc, n)
    committers = sorted({ki % n_dc, (ki + 1 + ki // n_dc) % n_dc})
    shift = [rng.randrange(-20_000, 20_001) for _ in range(n_dc)]
    for i, op in enumerate(ops):
        ct = T0 + start + i * step + rng.randrange(max(step, 1))
        op.commit_dc, op.commit_time = rng.choice(committers), ct
        op.snap = {d: ct - (shift[d] + rng.randint(1, 9000)) for d in range(n_dc)}
    return ops


def build(t, n_dc, spec, seed, other=None):
    """spec: per key (n_ops, start us, step us, kind).  Kinds: plain; other (a key of the type
    `other`: a read of type t gets an error status); routed (lag-only escapes on a quarter of the
    ops); lagesc (a lag-only escape mid-key); faresc (the newest op escaped from the packed view);
    late (the newest op 2^33 us after the first: escaped, its entries K + 2^32 and more)."""
    rng = random.Random(seed)
    keys, types, off = [], [], 0
    for ki, (n, start, step, kind) in enumerate(spec):
        kt = other if kind == "other" else t
        if (off + n) % 32 == 0 and ki + 1 < len(spec):  # no key but the first starts 32-aligned: neighbours share bitmap words
            assert n not in (1025, 2300), "a key of a set length ends 32-aligned: change the filler"
            n += 1
        ops = key_ops(rng, kt, n_dc, n, start, step, ki)
        if kind == "routed":
            for i in range(0, n, 4):
                plant(ops, i, n_dc, LAG_ONLY[0], rng)
        elif kind == "lagesc":
            plant(ops, n // 2, n_dc, LAG_ONLY[ki % len(LAG_ONLY)], rng)
        elif kind == "faresc":
            plant(ops, n - 1, n_dc, FAR, rng)
        elif kind == "late":
            op = ops[-1]
            op.commit_time = ops[0].commit_time + LATE
            op.snap = {d: op.commit_time - 5 - d for d in range(n_dc)}
        keys.append(ops)
        types.append(kt)
        off += n
    return keys, HostLog(n_dc, keys, key_types=types)


def key_bases(log):
    """The keys' time bases K (am_pk_base: 2^30 us under the first op's lowest recent entry)."""
    n = log.n_ops
    ct = log.commit_time[:n].astype(np.int64)
    dc = (log.op_meta[:n] & 0x1F).astype(np.int64)
    X = log.snap_vc[:, :n].astype(np.int64).copy()
    X[dc, np.arange(n)] = ct
    out = []
    for k in range(log.n_keys):
        a = int(log.key_off[k])
        lo, floor = int(ct[a]), max(int(ct[a]) - 0x7FFFFFFF, 0)
        for d in range(log.n_dc):
            if d != dc[a] and floor <= X[d, a] < lo:
                lo = int(X[d, a])
        out.append(lo - 0x40000000 if lo > 0x40000000 else 0)
    return out


def span(keys, sel=None):
    cts = [op.commit_time for k, ops in enumerate(keys) if sel is None or k in sel for op in ops]
    return min(cts), max(cts) + 30_000  # (past every entry: they run at most 20 ms ahead of the commit times)


# ---------------------------------------------------------------- the cases
def mixed_spec(n_keys=44):
    """Neighbouring keys start 4.099 ms apart (every K differs) and overlap in time: one clock
    lies in the middle of most of them.  Lengths past the lane tier; a few of several tiles."""
    lens = [70, 97, 131, 75, 300, 83, 111, 67]
    spec = [(lens[i % 8], 4099 * i, 1000, "plain") for i in range(n_keys)]
    spec[6] = (1100, 4099 * 6, 100, "plain")
    spec[33] = (600, 4099 * 33, 250, "plain")
    return spec


def mixed_clocks(keys, n_dc):
    lo, hi = span(keys)
    mids = [[T0 + x] * n_dc for x in (45_000, 90_000, 150_000, 210_000)]
    skew = [T0 + 120_000 + 7_000 * ((3 * d) % n_dc) for d in range(n_dc)]  # another time on every DC
    return [(c, None) for c in mids + [skew]]


def edge_clocks(keys, log, n_dc):
    """Over the mixed batch: a clock below some keys' K (on every DC, and on one DC alone); a
    clock that lacks a DC; above every op; below every op but above every K."""
    lo, hi = span(keys)
    ks = sorted(key_bases(log))
    kmid = ks[len(ks) // 2] - 1
    assert ks[0] <= kmid < ks[-1] and ks[-1] < lo
    one = [hi] * n_dc
    one[n_dc // 2] = kmid
    full = (1 << n_dc) - 1
    return [([kmid] * n_dc, None), (one, None), ([T0 + 90_000] * n_dc, full & ~2), ([hi] * n_dc, None),
            ([lo - 25_000] * n_dc, None)]


def sparse_spec():
    """69 reads: two batches of 32 and a partial one of 5.  Slots 0, 31 and 32 eligible; between
    them short keys (the lane tier's), a key over the wave tier's op limit, a routed key and a key
    of another type (an error status), so the eligible slots of a batch are not contiguous."""
    spec = []
    for i in range(69):
        kind, n, step = "plain", [70, 97, 131, 75, 83][i % 5], 1000
        if i in (0, 31, 32):
            n = 130
        elif i % 4 == 1:
            n = 20
        elif i in (6, 38):
            n, step = 8300, 20
        elif i in (10, 46):
            n, kind = 80, "routed"
        elif i in (14, 66):
            kind = "other"
        spec.append((n, 1013 * i, step, kind))
    return spec


def segment_spec():
    """A key of 1,025 ops first in the log (32-aligned: its newest segment is one op) and one of
    2,300 ops (three segments), their ops 100 us apart so that the window spans segment edges,
    next to 40-op keys and filler."""
    spec = [(1025, 0, 100, "plain")]
    for i in range(1, 40):
        spec.append((40 if i % 3 == 1 else 70 + i % 7, 2003 * i, 1000, "plain"))
    spec[5] = (2300, 2003 * 5, 100, "plain")
    return spec


def segment_clocks(keys, n_dc):
    out = []
    for k in (0, 5):
        ct = sorted(op.commit_time for op in keys[k])
        out += [[ct[len(ct) * q // 100]] * n_dc for q in (30, 47, 60, 92)]
        out.append([ct[1024 if k == 5 else 2] + 3] * n_dc)
    return [(c, None) for c in out]


def escape_spec():
    spec = [([70, 97, 131, 75, 83][i % 5], 3001 * i, 1000, "plain") for i in range(40)]
    spec[3] = (97, 3001 * 3, 1000, "lagesc")
    spec[7] = (83, 3001 * 7, 1000, "late")
    spec[11] = (131, 3001 * 11, 1000, "faresc")
    spec[31] = (75, 3001 * 31, 1000, "late")
    return spec


def escape_clocks(keys, n_dc):
    lo, hi = span(keys)  # hi: past the late ops too
    return [([hi] * n_dc, None), ([T0 + 100_000] * n_dc, None), ([T0 + 60_000] * n_dc, None)]


# ---------------------------------------------------------------- what the reads meet, by the host rule
def coverage(log, clocks, sel=None):
    """Over the reads of keys `sel` under the clocks: how many have a non-empty window list, how
    many a list of more than one round of 64 in a segment, how many a bound raised by a sure-in op
    before the rounds (the segment holds an op at or under cin and window ops), and how many carry
    a bound into an older segment that has window ops."""
    nd = log.n_dc
    ct, lbs, first = host_view(log)
    got = dict(listed=0, second_round=0, sure_raised=0, carried=0)
    for clock, pres in clocks:
        for k in (range(log.n_keys) if sel is None else sel):
            segs = segment_lists(log, k, clock, pres)
            got["listed"] += any(len(w) for w in segs)
            got["second_round"] += any(len(w) > 64 for w in segs)
            if pres is not None and pres != (1 << nd) - 1:
                continue
            cin = min(int(clock[d]) + int(lbs[k][d]) for d in range(nd))
            a, b = int(log.key_off[k]), int(log.key_off[k + 1])
            t0, raised, carried, seen_sure = a & ~31, False, False, False
            for i, s in enumerate(range(t0 + (b - 1 - t0) // SEG * SEG, t0 - 1, -SEG)):
                c = ct[max(s, a):min(s + SEG, b)]
                sure = bool((c <= cin).any())
                raised |= sure and len(segs[i]) > 0
                carried |= seen_sure and len(segs[i]) > 0
                seen_sure |= sure
            got["sure_raised"] += raised
            got["carried"] += carried
    return got


CASES = {
    # name: (spec, other type?, clocks)
    "mixed": (mixed_spec, False, lambda keys, log, nd: mixed_clocks(keys, nd)),
    "edges": (mixed_spec, False, edge_clocks),
    "sparse": (sparse_spec, True, lambda keys, log, nd: [([span(keys)[1]] * nd, None), ([T0 + 60_000] * nd, None)]),
    "segments": (segment_spec, False, lambda keys, log, nd: segment_clocks(keys, nd)),
    "escapes": (escape_spec, False, lambda keys, log, nd: escape_clocks(keys, nd)),
}
_LOGS = {}


def case(name, t, n_dc):
    """(keys, log, clocks) of a case, built once per (name, type, D) and never changed."""
    if (name, t, n_dc) not in _LOGS:
        spec, other, clocks = CASES[name]
        ot = (abi.AM_MVREG if t == abi.AM_AWSET else abi.AM_AWSET) if other else None
        keys, log = build(t, n_dc, spec(), 9900 + 10 * t + n_dc + len(name), ot)
        _LOGS[name, t, n_dc] = (keys, log, clocks(keys, log, n_dc))
    return _LOGS[name, t, n_dc]


PLAIN = {"mixed": None, "edges": None, "segments": None,
         "sparse": [i for i, s in enumerate(sparse_spec()) if s[3] == "plain" and 64 < s[0] <= 8192],
         "escapes": [i for i, s in enumerate(escape_spec()) if s[3] == "plain"]}
