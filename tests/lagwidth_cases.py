"""Host logs, clocks and the host-side definitions for the tests of the per-key lag width (the store's
private column am_store_lag_width reads back, and the commit-word window k_grp_incl sizes by it:
csrc/am_inclwin.h, csrc/am_group_split.h).  Shared by tests/test_gpu_lagwidth.py (the device against
the definition and the oracle) and tests/test_lagwidth_cpu.py (the same inputs checked on the host:
the logs do put reads where a width can go wrong)."""
import random

import numpy as np

from antidote_amd import abi
from antidote_amd.oplog import HostLog
from tests import randlog
from tests.test_gpu_incl_deferred import FAR, LAG_ONLY, plant

T0 = 1_700_000_000_000_000
SEG, ESC, WMAX = 1024, 0xFFFFFFFF, 0xFFFF


# ---------------------------------------------------------------- the column, from its definition
def definition(log, lens=None):
    """The lag view of a host log in numpy, from include/antidote_mat.h: per key the time base K,
    the lag bases lb[d] (the smallest ct - X[d] over its packed ops), per op whether the view holds
    it, per key whether it is packed-routed, and the lag width: the largest (ct - X[d]) - lb[d] over
    the ops in the view and every DC; 0xFFFF for a routed key and a key with no op in the view.
    lens: the keys' op counts where the log has room behind them.  Returns a dict of arrays."""
    nd, n = log.n_dc, log.n_ops
    ko = np.asarray(log.key_off).astype(np.int64)
    ct = np.asarray(log.commit_time)[:n].astype(np.int64)
    dc = (np.asarray(log.op_meta)[:n] & 0x1F).astype(np.int64)
    bad = (np.asarray(log.op_meta)[:n] & 0x80) != 0
    X = np.asarray(log.snap_vc)[:, :n].astype(np.int64).copy()
    X[dc, np.arange(n)] = ct
    nk = log.n_keys
    out = dict(K=np.zeros(nk, np.int64), lb=np.zeros((nk, nd), np.int64), inview=np.zeros(n, bool),
               routed=np.zeros(nk, bool), width=np.full(nk, WMAX, np.int64), ct=ct, lag=np.zeros((nd, n), np.int64))
    for k in range(nk):
        a, b = int(ko[k]), int(ko[k + 1])
        if lens is not None:
            b = a + int(lens[k])
        if b <= a:
            continue
        lo, floor = int(ct[a]), max(int(ct[a]) - 0x7FFFFFFF, 0)
        for d in range(nd):
            if d != dc[a] and floor <= X[d, a] < lo:
                lo = int(X[d, a])
        base = lo - 0x40000000 if lo > 0x40000000 else 0
        out["K"][k] = base
        rel = X[:, a:b] - base
        esc = ((rel < 0) | (rel >= ESC)).any(axis=0) | bad[a:b]
        if esc.all():
            continue
        lag = ct[a:b][None, :] - X[:, a:b]
        lb = lag[:, ~esc].min(axis=1)
        out["lb"][k] = lb
        fit = bool(((lb > -(1 << 31)) & (lb < (1 << 31))).all())
        over = ((lag - lb[:, None] > WMAX) | (lag - lb[:, None] < 0)).any(axis=0) | (not fit)
        held = ~esc & ~over
        npk, nlo = int((~esc).sum()), int((over & ~esc).sum())
        out["routed"][k] = (not fit) or nlo * 8 > npk
        out["lag"][:, a:b] = lag - lb[:, None]
        if not out["routed"][k] and held.any():
            out["inview"][a:b] = held
            out["width"][k] = int((lag - lb[:, None])[:, held].max())
    return out


def window_lists(log, view, k, clock, width=None):
    """Key k (a dense host log: the store just built from it) under a clock that holds every DC: per
    segment of 1024 ops (32-aligned from the key's start), newest first, the log positions of its
    window ops -- the list the kernel builds, with the bound that needs no load over that segment
    and the newer ones.  width None: the key's own (view["width"]); else that value (0xFFFF: the
    window of a log whose widths the reader does not know)."""
    nd = log.n_dc
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    w = int(view["width"][k]) if width is None else int(width)
    K, lb = int(view["K"][k]), view["lb"][k]
    c = view["ct"] - K  # commit words
    cin = min(int(clock[d]) - K + int(lb[d]) for d in range(nd))
    if any(int(clock[d]) < K for d in range(nd)):
        cin = -(1 << 62)
    hi = cin + w
    t0, cmax, out = a & ~31, -(1 << 62), []
    for s in range(t0 + (b - 1 - t0) // SEG * SEG, t0 - 1, -SEG):
        p = np.arange(max(s, a), min(s + SEG, b))
        p = p[view["inview"][p]]
        sure = c[p][c[p] <= cin]
        if len(sure):
            cmax = max(cmax, int(sure.max()) - max(w, 1))
        out.append(p[(c[p] > min(cin, cmax)) & (c[p] <= hi)][::-1])
    return out


# ---------------------------------------------------------------- keys of a chosen width
def key_ops(rng, t, n_dc, n, start, step, width, ki, kind="plain"):
    """n ops from `start` (absolute us), step us apart, all committed at DC ki % n_dc; DC d's entry
    trails the commit time by shift(d) + r, r in [0, width] with both ends present on some DC: the
    key's lag bases are the shifts (0 at the committing DC) and its lag width is `width` exactly (0
    at one DC, where every lag is 0).  plain: jittered commit times, shifts of either sign.
    regular: ops exactly step apart and no negative shift, so cin is the clock's entry at the
    committing DC.  early: regular with every shift 0 and no entry below time 0."""
    ops = randlog.rand_key_ops(rng, t, n_dc, n)
    cdc = ki % n_dc
    lo = -3000 if kind == "plain" else 0
    shift = [0 if d == cdc or kind == "early" else rng.randrange(lo, 3001) for d in range(n_dc)]
    for i, op in enumerate(ops):
        ct = start + i * step + (rng.randrange(max(step, 1)) if kind == "plain" else 0)
        op.commit_dc, op.commit_time = cdc, ct
        top = min(width, ct) if kind == "early" else width
        op.snap = {d: ct - (shift[d] + (rng.randint(0, top) if top else 0)) for d in range(n_dc)}
    others = [d for d in range(n_dc) if d != cdc]
    if others and n >= 2 and width:
        i0, i1 = rng.sample(range(1, n), 2) if n > 2 else (0, 1)  # (an early key's op 0 lies below its width)
        for d in others:  # every DC attains its base; one DC the width
            ops[i0].snap[d] = ops[i0].commit_time - shift[d]
        ops[i1].snap[others[0]] = ops[i1].commit_time - (shift[others[0]] + width)
    return ops


def build(t, n_dc, spec, seed, other=None):
    """spec: per key (n_ops, start us after T0 or absolute when abs_, step, width, kind).  Kinds: plain;
    regular (no jitter: ops exactly step apart); other (a key of another type: an error status);
    routed (lag-only escapes on a quarter of the ops); lagesc (a lag-only escape mid-key); faresc
    (an op escaped from the packed view mid-key); early (absolute times from `start`, no T0: the
    key's time base is 0 and its commit words are its commit times)."""
    rng = random.Random(seed)
    keys, types, off = [], [], 0
    for ki, (n, start, step, width, kind) in enumerate(spec):
        kt = other if kind == "other" else t
        if n and (off + n) % 32 == 0 and ki + 1 < len(spec):  # neighbours share bitmap words
            n += 1
        begin = start if kind == "early" else T0 + start
        ops = key_ops(rng, kt, n_dc, n, begin, step, width, ki, kind if kind in ("regular", "early") else "plain") if n else []
        if n_dc > 1:
            if kind == "routed":
                for i in range(0, n, 4):
                    plant(ops, i, n_dc, LAG_ONLY[0], rng)
            elif kind == "lagesc":
                plant(ops, n // 2, n_dc, LAG_ONLY[ki % len(LAG_ONLY)], rng)
            elif kind == "faresc":
                plant(ops, n // 2, n_dc, FAR, rng)
        keys.append(ops)
        types.append(kt)
        off += n
    return keys, HostLog(n_dc, keys, key_types=types)


# ---------------------------------------------------------------- the cases
CYCLE = [0, 1, WMAX, 63, 8000, 0, WMAX, 1]  # neighbouring reads of a batch: another width each


def batch_spec():
    """40 reads (a batch of 32 and one of 8): widths 0, 1 and 0xFFFF side by side, every key past the
    lane tier and none but the first 32-aligned; a routed neighbour, a lag-only escape and an op
    escaped from the packed view among the window ops of narrow keys, and an empty key."""
    lens = [70, 97, 131, 75, 300, 83, 111, 67]
    spec = [(lens[i % 8], 997 * i, 400, CYCLE[i % 8], "plain") for i in range(40)]
    spec[4] = (80, 997 * 4, 400, 63, "routed")
    spec[9] = (97, 997 * 9, 400, 1, "lagesc")
    spec[12] = (300, 997 * 12, 100, 8000, "lagesc")
    spec[19] = (75, 997 * 19, 400, 63, "faresc")
    spec[22] = (0, 0, 1, 0, "plain")
    spec[37] = (97, 997 * 37, 400, 0, "faresc")
    return spec


def batch_clocks(keys, log, n_dc):
    return [[T0 + x] * n_dc for x in (15_000, 30_000, 42_000)] + \
           [[T0 + 25_000 + 900 * ((3 * d) % n_dc) for d in range(n_dc)], [T0 + 200_000] * n_dc, [T0 - 80_000] * n_dc]


LIST_WIDTHS = {0: 0, 1: 315, 2: 320, 3: 325, 4: 63, 5: 8000, 6: 8000}  # key -> width (keys 0..3: ops 10 us apart)


def lists_spec():
    """Regular keys (ops exactly 10 us apart, committed at one DC whose clock entry gives cin) of
    widths 0, 315, 320 and 325: under a clock at an op's commit time the window lists hold 1, 63,
    64 and 65 entries; under one far below the key none.  Key 4: ops 1 us apart, so that an op lies
    at cin + w and one at cin + w + 1; key 5 (20 us apart, width 8000): one at cin + w, none at
    cin + w + 1.  Key 6: an `early` key (time base 0) of width 8000
    whose first ops have the commit words 7999, 8000 and 8001: the bound of a sure-in op c' at
    c' - w = -1, 0 and 1.  Filler keys between them, of other widths."""
    spec = []
    for i in range(34):
        spec.append(([70, 97, 131, 75][i % 4], 3001 * i, 400, CYCLE[(i + 3) % 8], "plain"))
    for k in (0, 1, 2, 3):
        spec[k] = (400, 20_000 + 7 * k, 10, LIST_WIDTHS[k], "regular")
    spec[4] = (300, 20_000, 1, 63, "regular")
    spec[5] = (1000, 20_000, 20, 8000, "regular")
    spec[6] = (203, 7999, 1, 8000, "early")
    return spec


def lists_clocks(keys, log, n_dc):
    """Every clock holds one value on every DC.  For the regular keys: at the commit time of op 200
    (the list sizes above; the op at cin + w and the one at cin + w + 1 both exist where ops are 1 us
    apart), 1 us below it, and far below every op; for the early key its first three commit times."""
    out = []
    for k in (0, 1, 2, 3, 4, 5):
        ct = keys[k][200].commit_time
        out += [[ct] * n_dc, [ct - 1] * n_dc]
    out.append([T0 - 80_000] * n_dc)
    out += [[x] * n_dc for x in (7999, 8000, 8001)]
    return out


def segments_spec():
    """A key of 1,100 ops (two segments) and one of 4,200 (17 tiles, five segments) of a narrow
    width, ops 10 us apart: the window spans segment edges where the clock lies at one, and the
    bound without loads carries from a newer segment to the older ones."""
    spec = [(1100, 0, 10, 320, "regular")]
    for i in range(1, 36):
        spec.append((40 if i % 3 == 1 else 70 + i % 7, 2003 * i, 400, CYCLE[i % 8], "plain"))
    spec[5] = (4200, 2003 * 5, 10, 640, "regular")
    spec[9] = (1500, 2003 * 9, 10, 0, "regular")
    return spec


def segments_clocks(keys, log, n_dc):
    out = []
    for k, edges in ((0, (1023, 1024, 1040, 500)), (5, (1023, 2047, 2048, 3071, 4100, 3000)), (9, (1023, 1024, 700))):
        a = int(log.key_off[k])
        t0 = a & ~31
        for e in edges:  # ops at the segments' edges as the kernel cuts them (32-aligned from the key's start)
            i = min(max(t0 + e - a, 0), len(keys[k]) - 1)
            out.append([keys[k][i].commit_time] * n_dc)
    return out


def sparse_spec():
    """69 reads: two batches of 32 and one of 5.  Eligible slots of several widths between short
    keys (the lane tier's), keys over the wave tier's op limit, routed keys and keys of another
    type (an error status)."""
    spec = []
    for i in range(69):
        kind, n, step, w = "plain", [70, 97, 131, 75, 83][i % 5], 400, CYCLE[i % 8]
        if i in (0, 31, 32):
            n = 130
        elif i % 4 == 1:
            n = 20
        elif i in (6, 38):
            n, step = 8300, 5
        elif i in (10, 46):
            n, kind = 80, "routed"
        elif i in (14, 66):
            kind = "other"
        spec.append((n, 607 * i, step, w, kind))
    return spec


def sparse_clocks(keys, log, n_dc):
    return [[T0 + 30_000] * n_dc, [T0 + 300_000] * n_dc]


CASES = {"batch": (batch_spec, batch_clocks), "lists": (lists_spec, lists_clocks),
         "segments": (segments_spec, segments_clocks), "sparse": (sparse_spec, sparse_clocks)}
_LOGS = {}


def case(name, t, n_dc):
    """(keys, log, clocks, view) of a case, built once per (name, type, D) and never changed."""
    if (name, t, n_dc) not in _LOGS:
        spec, clocks = CASES[name]
        ot = abi.AM_MVREG if t == abi.AM_AWSET else abi.AM_AWSET
        keys, log = build(t, n_dc, spec(), 10_100 + 10 * t + n_dc + len(name), ot)
        _LOGS[name, t, n_dc] = (keys, log, clocks(keys, log, n_dc), definition(log))
    return _LOGS[name, t, n_dc]
