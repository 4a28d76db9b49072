"""The lag instantiation of the split fresh read's inclusion pass (csrc/am_group_split.h
k_grp_incl<.., LAG = true>) classifies a 1024-op segment from its commit words, appends the ops the
commit word leaves undecided to a list and evaluates the list in rounds of 64, one op per lane.
Small hand-made logs put the list where that can go wrong: 0, 1, 63, 64, 65, 128 and 129 entries
and every op of a segment; keys of one tile, of one segment to the op and of two, of more than 64
bitmap words and of more than 16 tiles; window ops in one lane's quad, one per lane, across a tile
edge and across a segment edge; escaped ops among the window ops of a quad; reads at batch slots 0,
31 and 32 and a routed key beside them; every clock width and both types, and the runtime-width
instantiation.  Every batch is read three ways (test_gpu_inclwindow.three_ways): the lag view, the
same log with lag_ct nulled and the C oracle, every column and the pairs bit-equal.  The list sizes
are those of the rule replicated on the host log (the segment-wide bound that needs no load, which
is all the kernel knows of a read's newest segment), so a log that misses a size fails."""
import random

import numpy as np
import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostLog
from tests import randlog
from tests.test_gpu_incl_deferred import FAR, LAG_ONLY, plant
from tests.test_gpu_inclwindow import three_ways

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000
TILE, SEG, LAGMAX = 256, 1024, 0xFFFF
COUNTS = [0, 1, 3, 63, 64, 65, 128, 129]  # list entries: no round, one lane's ops, full rounds to the entry, several
FILL = 70                              # ops of the keys that only fill batch slots
# (ops, us between ops, timeline) of the keys that matter, by batch slot; every other slot < N_KEYS
# holds a FILL-op key.  Slot 0: the key the entry counts are steered on (one segment).
SPEC = {0: (1000, 1000, "asc"), 1: (65, 1000, "asc"), 2: (255, 100, "shuffled"), 3: (256, 10, "asc"),
        4: (257, 1000, "inter"), 5: (1023, 100, "asc"), 6: (1024, 10, "shuffled"), 7: (1025, 100, "inter"),
        8: (1100, 1000, "asc"), 9: (1100, 100, "asc"), 10: (2180, 1000, "asc"), 11: (4200, 100, "asc"),
        12: (1024, 100, "asc"), 13: (600, 0, "perlane"), 14: (2200, 10, "asc"),
        31: (1024, 100, "shuffled"), 32: (1100, 1000, "inter"), 33: (257, 10, "asc")}
ROUTED, ESCAPED = 30, (8, 31)  # a packed-routed key beside slot 31; keys with escapes among window ops
N_KEYS = 36


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


# ---------------------------------------------------------------- logs
def times(rng, n, n_dc, step, kind):
    """(commit_time, commit_dc, {dc: commit_time - entry}) of n ops in log order, step us apart:
    asc / shuffled / inter as test_gpu_inclwindow.timeline (the second timeline 40 ms ahead).
    perlane: every fourth op on a timeline of 300 us steps, the others a second earlier -- a clock
    on the late timeline leaves one window op per lane.  With more than one DC the last DC never
    commits and holds lags 0 and 65535 above its base, and one entry of DC 0 lies ahead of its
    commit time (a negative lag base)."""
    quiet = n_dc - 1 if n_dc > 1 else None
    committers = [d for d in range(n_dc) if d != quiet]
    out = []
    for i in range(n):
        dc = rng.choice(committers)
        if kind == "perlane":
            ct = T0 + (1_000_000 + i * 300 if i % 4 == 0 else i * 50) + rng.randrange(40)
        elif kind == "inter":
            dc = committers[i % 2 % len(committers)]
            ct = T0 + (i // 2) * 2 * step + (i % 2) * 40_000 + rng.randrange(step)
        else:
            ct = T0 + i * step + rng.randrange(step)
        out.append((ct, dc, {d: rng.randint(1, 9000) for d in range(n_dc)}))
    if n_dc > 1:
        i0, i1, i2 = rng.sample(range(n), 3)
        out[i0][2][quiet] = 1
        out[i1][2][quiet] = 1 + LAGMAX
        if out[i2][1] == 0 and len(committers) > 1:
            out[i2] = (out[i2][0], committers[1], out[i2][2])
        if out[i2][1] != 0:
            out[i2][2][0] = -500
    if kind == "shuffled":
        rng.shuffle(out)
    return out


def make_log(rng, t, n_dc):
    keys, off = [], 0
    for ki in range(N_KEYS):
        n, step, kind = SPEC.get(ki, (FILL + ki % 5, 1000, "asc"))
        assert ki == 0 or off % 32, "a key starts 32-aligned: change FILL"
        ops = randlog.rand_key_ops(rng, t, n_dc, n)
        for op, (ct, dc, back) in zip(ops, times(rng, n, n_dc, step, kind)):
            op.commit_dc, op.commit_time = dc, ct
            op.snap = {d: ct - back[d] for d in range(n_dc)}
        if n_dc > 1 and ki in ESCAPED:  # a lag-only and a packed escape in one quad, clean ops between
            q = 4 * ((off + n // 2) // 4 + 1) - off  # the first op of a lane's four
            plant(ops, q, n_dc, LAG_ONLY[ki % len(LAG_ONLY)], rng)
            plant(ops, q + 2, n_dc, FAR, rng)
        if n_dc > 1 and ki == ROUTED:  # lag-only escapes on more than 1 / 8 of the ops
            for i in range(0, len(ops), 4):
                plant(ops, i, n_dc, LAG_ONLY[0], rng)
        keys.append(ops)
        off += len(ops)
    return keys, HostLog(n_dc, keys, key_types=[t] * len(keys))


# ---------------------------------------------------------------- the rule, on the host log
_VIEW = {}


def host_view(log, slot_off=None):
    """(commit times, per-key lag bases, each key's first slot) of the host log, the first two
    computed once.  slot_off: the store's slot offsets where its keys have room for appends
    (a log ingested in place); by default the dense key_off, a store the log was just built into."""
    if id(log) not in _VIEW:
        n = log.n_ops
        ct = log.commit_time[:n].astype(np.int64)
        dc = (log.op_meta[:n] & 0x1F).astype(np.int64)
        X = log.snap_vc[:, :n].astype(np.int64).copy()
        X[dc, np.arange(n)] = ct
        ko = log.key_off.astype(np.int64)
        lbs = [(ct[ko[k]:ko[k + 1]][None, :] - X[:, ko[k]:ko[k + 1]]).min(axis=1) if ko[k + 1] > ko[k]
               else np.zeros(log.n_dc, np.int64) for k in range(log.n_keys)]  # (a key pruned to empty)
        _VIEW[id(log)] = (log, ct, lbs)
    first = log.key_off if slot_off is None else slot_off
    return _VIEW[id(log)][1:] + (np.asarray(first).astype(np.int64),)


def segment_lists(log, k, clock, pres=None, slot_off=None):
    """Key k under the clock: per segment (1024 ops, 32-aligned from the key's start), newest first,
    the positions from the segment's start of its window ops when cmax comes from the bound without
    loads over that segment and the newer ones.  Escaped ops are not told apart here (the keys
    the sizes are asserted on have none).  slot_off: as host_view's -- the segments are cut from
    the key's first slot in the store, not from its offset in the dense log."""
    nd = log.n_dc
    ct, lbs, first = host_view(log, slot_off)
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    lb = lbs[k]
    cin = min(int(clock[d]) + int(lb[d]) for d in range(nd))
    hi = cin + LAGMAX
    if pres is not None and pres != (1 << nd) - 1:
        cin, hi = -(1 << 62), -(1 << 62)
    sh = int(first[k]) - a  # the key's ops lie at log position + sh in the store
    a, b = a + sh, b + sh
    t0, cmax, out = a & ~31, -(1 << 62), []
    for s in range(t0 + (b - 1 - t0) // SEG * SEG, t0 - 1, -SEG):
        lo, c = max(s, a), ct[max(s, a) - sh:min(s + SEG, b) - sh]
        sure = c[c <= cin]
        if len(sure):
            cmax = max(cmax, int(sure.max()) - LAGMAX)
        out.append(np.nonzero((c > min(cin, cmax)) & (c <= hi))[0] + (lo - s))
    return out


def steer(log, k, want, slot_off=None, seg=0):
    """Clocks (one value for every DC) under which key k's list holds exactly the wanted sizes:
    the list of its newest segment, or of its seg-th newest."""
    found = {}
    for x in range(T0 - 70_000, T0 + 140_000, 50):
        n = len(segment_lists(log, k, [x] * log.n_dc, None, slot_off)[seg])
        if n in want and n not in found:
            found[n] = x
    return found


@pytest.fixture(scope="module")
def logs():
    cache = {}

    def get(t, n_dc):
        if (t, n_dc) not in cache:
            cache[t, n_dc] = make_log(random.Random(9700 + 10 * t + n_dc), t, n_dc)
        return cache[t, n_dc]
    return get


def read_clocks(keys, log, n_dc):
    """(clock, presence mask or None) of the batches read."""
    hi = max(op.commit_time for ops in keys for op in ops) + 10
    byct = sorted(op.commit_time for ops in keys for op in ops)
    q50, q75 = byct[len(byct) // 2], byct[len(byct) * 3 // 4]
    found = steer(log, 0, COUNTS)
    assert sorted(found) == COUNTS, found
    clocks = [([found[c]] * n_dc, None) for c in COUNTS]
    clocks += [([T0 - 200_000] * n_dc, None),             # below every op: count 0, base ignore
               ([hi] * n_dc, None),                       # above every op
               ([q50] * n_dc, None), ([q75] * n_dc, None),
               ([T0 + 50_000] * n_dc, None),              # inside every key
               ([T0 + 1_000_000 + 90_000] * n_dc, None)]  # on the late timeline of the per-lane key
    if n_dc > 1:
        clocks.append(([T0 + 50_000] * n_dc, ((1 << n_dc) - 1) & ~2))  # a clock that lacks a DC: nothing passes
    return clocks


def coverage(log, clocks):
    """What the batches' lists look like, by the host rule: every wanted size, a whole segment,
    a list across a tile edge and one across a segment edge, a list inside one lane's four ops
    and a list of one op per lane over at least a round."""
    ko = log.key_off.astype(np.int64)
    sizes = set()
    cov = dict(whole_seg=False, tile_edge=False, seg_edge=False, one_quad=False, per_lane=False)
    for clock, pres in clocks:
        for k in range(log.n_keys):
            segs = segment_lists(log, k, clock, pres)
            for w in segs:
                sizes.add(len(w))
                cov["whole_seg"] |= len(w) == SEG
                if len(w) == 0:
                    continue
                cov["tile_edge"] |= len(set(w // TILE)) > 1
                cov["one_quad"] |= 1 < len(w) <= 4 and len(set(w // 4)) == 1
                cov["per_lane"] |= len(w) >= 64 and len(set(w // 4)) == len(w)
            cov["seg_edge"] |= sum(1 for w in segs if len(w)) > 1
            assert pres is None or all(len(w) == 0 for w in segs)
    cov["sizes"] = set(COUNTS) <= sizes
    return cov


# n_dc 5: no template width, the runtime-width instantiation of D = 8
@pytest.mark.parametrize("t,n_dc", [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3), (abi.AM_MVREG, 3),
                                    (abi.AM_AWSET, 1), (abi.AM_MVREG, 1), (abi.AM_AWSET, 5)])
def test_gpu_incl_compact_three_ways(mat, logs, t, n_dc):
    keys, log = logs(t, n_dc)
    assert len(keys) == N_KEYS > 33 and all(int(o) % 32 for o in log.key_off[1:-1])
    ko = log.key_off.astype(np.int64)
    assert (int(ko[1]) + 31) // 32 * 32 <= SEG                      # slot 0: one segment
    assert max(np.diff(ko)) > 16 * TILE and int(ko[11]) // 32 + 64 < int(ko[12]) // 32
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        stats = st.view_stats()
        if n_dc > 1:
            assert stats["routed_keys"] == 1 and stats["lag_only_esc_ops"] >= 2 and stats["pk_esc_ops"] >= 2, stats
        else:
            assert stats["routed_keys"] == 0 and stats["lag_only_esc_ops"] == 0, stats
        dlog = st.device_log()
        assert dlog.lag_ct and not dlog.zone_vc
        clocks = read_clocks(keys, log, n_dc)
        cov = coverage(log, clocks)
        assert all(cov.values()), cov
        for clock, pres in clocks:
            three_ways(mat, dlog, log, keys, t, n_dc, clock, pres)
    finally:
        st.close()
