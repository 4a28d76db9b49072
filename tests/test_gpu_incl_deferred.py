"""The split fresh read's inclusion pass evaluates escaped ops after the loop over a wave batch's
32 reads, not inside it (csrc/am_group_split.h k_grp_incl, the deferred phase): a read with escapes
leaves its in-view partials in the batch's rows, its escape marks in a scratch row and its bit in
a mask, and the later phase ORs the included escaped ops into the bitmap and merges their
partials.  Hand-made keys put escapes where that can go wrong and the in-loop pass could not:
at batch slots 0, 15 and 31 between clean reads, in a batch where every read has them and one
where none has, in a partial last batch, on the first and last op of neighbouring keys (bitmap
words shared between reads), on every op of a read, on the ops that decide count 0 / > 0, the
first excluded op and a single DC's maximum, on an op Type:update/2 raises on, next to a routed
key, and in the late tiles of a key of more than 16 tiles (the walk path).  Every batch is read
three ways -- the lag view, the same device log with lag_ct nulled (the packed instantiation;
every column and the pairs bit-equal) and the C oracle.  The escapes are counted as they are
planted and the store's view statistics must equal those counts, so a log that planted none
fails."""
import random

import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostLog
from tests import randlog
from tests.test_gpu_inclwindow import packed_only, read_columns, three_ways
from tests.test_gpu_lagcadence import check_batch, view_counts

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000
MID = T0 + 100                 # the prefix clock: ~40 ops of every key (ops are 1 .. 4 us apart)
LAG_ONLY = [65536, 65537, 1 << 20]  # lags above the key's base that miss the lag view's 16 bits
FAR = 1 << 31                  # outside the packed window too: the escape row
N_KEYS = 100


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


# ---------------------------------------------------------------- the layout
def layout():
    """(n_ops, kind) per key = per read.  Reads 0 .. 31: escapes at slots 0, 15 and 31 only;
    32 .. 63: every read has escapes; 64 .. 95: none has; 96 .. 99: a partial batch with the
    routed key, the long key and a 40-op key."""
    cyc = ["edges", "all", "newest", "cut", "onedc", "both", "edges", "bad"]
    spec = []
    for i in range(N_KEYS):
        n = [65, 67, 70, 97, 131, 75, 300, 83][i % 8]
        kind = "clean"
        if i in (0, 31):
            kind = "edges"
        elif i == 15:
            n, kind = 1100, "both"
        elif 32 <= i < 64:
            kind = cyc[i % 8]
            if i == 40:
                n = 1024
        elif i == 96:
            n, kind = 80, "routed"
        elif i == 97:
            kind = "edges"
        elif i == 98:
            n, kind = 4400, "long"
        elif i == 99:
            n, kind = 40, "edges"
        spec.append([n, kind])
    off = 0
    for s in spec[:-1]:  # no key but the first starts 32-aligned: neighbours share bitmap words
        if (off + s[0]) % 32 == 0:
            s[0] += 1
        off += s[0]
    return [tuple(s) for s in spec]


def plant(ops, i, n_dc, val, rng):
    """Op i's entry on a DC it did not commit at: val us of lag above the key's base there."""
    op = ops[i]
    r = (op.commit_dc + 1 + rng.randrange(n_dc - 1)) % n_dc
    kmin = min(0 if o.commit_dc == r else o.commit_time - o.snap[r] for o in ops)
    op.snap[r] = op.commit_time - (kmin + val)
    return r


def make_log(rng, t, n_dc):
    """The keys, the log, and the planted counts {lag_only, pk_esc, routed}."""
    keys, want = [], {"lag_only": 0, "pk_esc": 0, "routed": 0}
    kinds = []
    for ki, (n, kind) in enumerate(layout()):
        ops = randlog.rand_key_ops(rng, t, n_dc, n, t0=T0)  # one time line for every key
        lag_only, far = [], []
        cut = next((i for i, o in enumerate(ops) if o.commit_time > MID), None)  # MID's first excluded op
        if kind == "edges":
            lag_only, far = [0], [n - 1]
        elif kind == "all":
            far = list(range(n))
        elif kind == "newest":
            far = [n - 1, n - 3]
            lag_only = [n - 2]
        elif kind == "cut":
            lag_only = [cut]
        elif kind == "onedc":
            far = [n - 1]
            for d in range(n_dc):  # the newest op: every entry but its commit time is old
                if d != ops[-1].commit_dc:
                    ops[-1].snap[d] = ops[0].commit_time
        elif kind == "both":
            lag_only = sorted({5, cut, n // 2 + 1})
            far = [i for i in (7, n // 2, n - 2) if i not in lag_only]
            assert len(far) >= 2
        elif kind == "bad":
            ops[-1].bad = True  # escaped from the packed view by its meta bit
            want["pk_esc"] += 1
            lag_only = [3]
        elif kind == "routed":
            lag_only = list(range(0, n, 4))  # more than 1 / 8 of the ops: the key is routed
            want["routed"] += 1
        elif kind == "long":
            lag_only = [0, 300, 4100, 4250, n - 1]  # tiles 16 and 17 have no mark bits
            far = [17, 4097, 4399 - 1]
        for j, i in enumerate(lag_only):
            plant(ops, i, n_dc, LAG_ONLY[(ki + j) % len(LAG_ONLY)], rng)
        for i in far:
            plant(ops, i, n_dc, FAR, rng)
        assert not set(lag_only) & set(far)
        want["lag_only"] += len(lag_only)
        want["pk_esc"] += len(far)
        keys.append(ops)
        kinds.append(kind)
    return keys, HostLog(n_dc, keys, key_types=[t] * len(keys)), want, kinds


def expect_view(st, log, want):
    """The store's view holds exactly the planted escapes (and the definition agrees)."""
    got = st.view_stats()
    assert got["lag_only_esc_ops"] == want["lag_only"] > 0, (got, want)
    assert got["pk_esc_ops"] == want["pk_esc"] > 0, (got, want)
    assert got["routed_keys"] == want["routed"] == 1, (got, want)
    assert got == view_counts(log)[0], got


@pytest.fixture(scope="module")
def logs():
    """The host logs, built once per (type, D) and never changed."""
    cache = {}

    def get(t, n_dc):
        if (t, n_dc) not in cache:
            cache[t, n_dc] = make_log(random.Random(9500 + 10 * t + n_dc), t, n_dc)
        return cache[t, n_dc]
    return get


@pytest.mark.parametrize("n_dc", [8, 3])
@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_gpu_incl_deferred_three_ways(mat, logs, t, n_dc):
    keys, log, want, kinds = logs(t, n_dc)
    assert len(keys) > 3 * 32 and len(keys) % 32  # several batches, the last one partial
    assert all(int(o) % 32 for o in log.key_off[1:-1])
    assert max(len(k) for k in keys) > 16 * 256  # the walk path
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        expect_view(st, log, want)
        dlog = st.device_log()
        assert dlog.lag_ct and not dlog.zone_vc
        hi = max(op.commit_time for ops in keys for op in ops) + 10
        # past every op (every escaped op included: count 0 -> > 0 for the all-escaped reads, the
        # single-DC maximum, the bad op's status); the prefix (the newest escapes excluded beside
        # in-view included ops; an escaped first excluded op); before every op (nothing passes)
        for clock in ([hi] * n_dc, [MID] * n_dc, [T0 - 5] * n_dc):
            three_ways(mat, dlog, log, keys, t, n_dc, clock)
        # the cases, on the device's own columns (the oracle agreed above)
        _, h = read_columns(mat, dlog, len(keys), n_dc, t, [hi] * n_dc, None, 512)
        _, m = read_columns(mat, dlog, len(keys), n_dc, t, [MID] * n_dc, None, 512)
        for ki, kind in enumerate(kinds):
            n = len(keys[ki])
            if kind == "bad":
                assert h["status"][ki] == abi.AM_ERR_UNEXPECTED_OPERATION and m["status"][ki] == 0, ki
                continue
            assert h["status"][ki] == 0 and m["status"][ki] == 0, (ki, kind)
            assert h["count"][ki] == n, (ki, kind, int(h["count"][ki]), n)
            if kind == "all":  # no in-view op at all: the merge alone flips these
                assert not h["last_ct_ignore"][ki] and h["is_new_ss"][ki], ki
                assert h["last_ct_pres"][ki] == (1 << n_dc) - 1, ki
            if kind == "onedc":  # the escaped newest op holds its own DC's maximum, and no other's
                op = keys[ki][-1]
                rest = keys[ki][:-1]
                for d in range(n_dc):
                    top = max(o.commit_time if o.commit_dc == d else o.snap[d] for o in rest)
                    if d == op.commit_dc:
                        assert int(h["last_ct"][d, ki]) == op.commit_time > top, (ki, d)
                    else:
                        assert int(h["last_ct"][d, ki]) == top > op.snap[d], (ki, d)
            if kind in ("newest", "cut"):  # MID: in-view ops included, every escaped op excluded
                cut = next(i for i, o in enumerate(keys[ki]) if o.commit_time > MID)
                assert 0 < m["count"][ki] == cut < n - 3, (ki, kind, int(m["count"][ki]), cut)
    finally:
        st.close()


@pytest.mark.parametrize("n_dc", [8, 3])
def test_gpu_incl_deferred_selections(mat, logs, n_dc):
    """Batches cut differently: only the reads with escapes (every slot of every batch has them),
    only the clean ones (no batch has any), and the partial batch's keys alone."""
    t = abi.AM_AWSET
    keys, log, want, kinds = logs(t, n_dc)
    st = mat.store(log)
    try:
        st.index(abi.AM_INDEX_NONE)
        expect_view(st, log, want)
        dlog = st.device_log()
        hi = max(op.commit_time for ops in keys for op in ops) + 10
        esc = [k for k, kind in enumerate(kinds) if kind != "clean"]
        clean = [k for k, kind in enumerate(kinds) if kind == "clean"]
        assert len(esc) > 32 and len(clean) > 32
        for clock in ([hi] * n_dc, [MID] * n_dc):
            for sel in (esc, clean, [96, 97, 98, 99]):
                check_batch(mat, dlog, log, keys, t, n_dc, clock, sel=sel)
                check_batch(mat, packed_only(dlog), log, keys, t, n_dc, clock, sel=sel)
    finally:
        st.close()
