"""Add-wins-set and MV-register reads over a cached base at every tier's base-merge limits, on the
hand-made keys of tests/basemerge.py (proven without a GPU by tests/test_basemerge_cpu.py).  Every
comparison is the full result tuple -- status, the value pairs in order, NewLastOp, LastOpCt,
IsNewSS, Count, flags -- against oracle/am_oracle.c, after the oracle alone has answered ok (or
the stated error) at the same capacity; the base of every read is the oracle's own earlier result.

Which tier a case reaches follows from the constants basemerge mirrors (KB = 120, VGB = 1024,
BCAP = 1024): the row, lane and workgroup kernels refuse base pairs (has_base_pairs), the wave tier
takes a base of at most KB pairs without a TxId (base_ok) and hands on a read with more than KB
new survivors, k_sets takes what fits BCAP births with the base, the big tier the rest.  The wave
tier also needs a grouped key: at most AM_GRP_MAX_REC = 2048 records, and an MV key of at most
AM_BIG_MIN_OPS = 1024 ops (basemerge.wave_tier_key; asserted per case in test_basemerge_cpu.py).

  case                         base / new      tier
  sizes nb <= 120, ns <= 120   nb / ns         wave tier, base_merge (by_birth: under 1024 groups);
                                               nb, ns in {63, 64, 65}: the lane split and the
                                               alive mask's word split; 119, 120: the lists' end
  sizes nb in 121, 128, 129    nb / 1          base_ok refuses -> k_sets
  sizes ns = 121               1, 120 / 121    base_merge returns false -> k_sets
  interleave, unborn           78, 71, 100     wave tier: rank search at lo = 0 / nb / between, AW
                                               ties, unborn groups (hinted_group / base_group)
  churn                        ~107 / ~97      wave tier, 1040 groups > VGB: by_birth off (L.grp)
  sizes 1024 / 1               1024 / 1        k_sets, 1025 births
  lds_edge sum-1024, base-1024 121, 1024       k_sets, its list exactly full
  lds_edge sum-1025, base-1025 121, 1025       k_sets overflows -> the big tier (am_big.hip)
  txid-5, txid-9               60 / 10         base_ok refuses a TxId read -> k_sets
  zone skip                    120 / 1, 120    wave tier over a 1100-op key (MV: 1000), blocks
                                               inside the base left out (AM_STAT_OPS_SKIPPED)
  through the cache            64 .. 121       wave tier with the pool tee and group hints, stale
                                               after in-place applies; k_sets + k_sc_copy (~0 hints)"""
import ctypes
import functools
import random

import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostBatch, HostLog, Read
from oracle import amo
from oracle import ref_materializer as R
from tests import basemerge as bm
from tests import randlog
from tests.basemerge import AW, MV

pytestmark = pytest.mark.gpu

CAPERR = ("error", abi.AM_ERR_CAPACITY)
WIDTHS = [1, 3, 5, 8, 13, 32]  # the exact templates 1, 3, 8, the runtime widths 5 and 13, OPL = 1 at 32


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def _diff(a, b):
    """A short account of where two results differ (a value may hold a thousand pairs)."""
    if a[0] != "ok" or b[0] != "ok":
        return (a if a[0] != "ok" else a[0], b if b[0] != "ok" else b[0])
    out = [(j, x, y) for j, (x, y) in enumerate(zip(a[2:], b[2:]), 2) if x != y]
    if a[1] != b[1]:
        va, vb = a[1], b[1]
        if isinstance(va, list) and isinstance(vb, list):
            first = next((j for j, (x, y) in enumerate(zip(va, vb)) if x != y), min(len(va), len(vb)))
            out.append(("value", len(va), len(vb), first, va[first:first + 2], vb[first:first + 2]))
        else:
            out.append(("value", va, vb))
    return out


def compare(mat, st, log, n_dc, reads, caps, names, tag, errors=()):
    """read_batch against the oracle, every read and every column; the oracle's own status is ok
    but for the reads listed in `errors`.  Returns the oracle's results."""
    got = mat.read_batch(st, reads, caps)
    ref = amo.materialize(log, HostBatch(n_dc, reads, caps))
    want = [ref.result(i) for i in range(len(reads))]
    not_ok = [(names[i], want[i]) for i in range(len(reads)) if (want[i][0] != "ok") != (i in errors)]
    assert not not_ok, (tag, not_ok[:5])
    bad = [(names[i], _diff(got.result(i), want[i])) for i in range(len(reads)) if got.result(i) != want[i]]
    assert not bad, (tag, len(bad), [b[0] for b in bad], bad[:3])
    return want


def filler(rng, t, n_dc, n):
    """A short random key on the cases' timeline and its fresh read near its end."""
    ops = randlog.rand_key_ops(rng, t, n_dc, n, t0=bm.T0)
    hi = ops[-1].commit_time if ops else bm.T0 + 20
    return ops, {d: hi - 3 + d % 3 for d in range(n_dc)}


# ---------------------------------------------------------------- a. sizes
def size_grid(n_dc):
    if n_dc in (13, 32):  # only the values 1, 64, 120, 121
        v = (1, 64, 120)
        return [(nb, ns) for nb in v for ns in v] + [(121, 1), (1, 121), (120, 121)]
    g = [(nb, ns) for nb in (1, 63, 64, 65, 119, 120) for ns in (0, 1, 63, 64, 65, 119, 120)]
    return g + [(121, 1), (128, 1), (129, 1), (1, 121), (120, 121)]


@functools.lru_cache(maxsize=None)
def sweep(t, n_dc):
    """One log: every sizes key of size_grid, interleave, unborn (explicit op ids, so every op of
    the log carries one), churn, and fillers of 3 .. 40 ops of all five types among them.
    -> (log, [(key, type, name, Read)]); the reads of the cases run over their bases."""
    rng = random.Random(100 * n_dc + t)
    cases = [bm.sizes(t, nb, ns, n_dc) for nb, ns in size_grid(n_dc)]
    cases += [bm.interleave(t, n_dc), bm.unborn(t, n_dc), bm.churn(t, n_dc)]
    keys, types, reads = [], [], []
    step = 6 if len(cases) >= 30 else 3  # all five types among the fillers
    for i, c in enumerate(cases):
        if i % step == 0:
            ft = randlog.TYPES[(i // step) % 5]
            ops, clock = filler(rng, ft, n_dc, rng.choice([3, 10, 25, 40]))
            reads.append((len(keys), ft, "filler-%d" % ft, Read(len(keys), ft, clock)))
            keys.append(ops)
            types.append(ft)
        reads.append((len(keys), t, c["name"], bm.read_of(c, len(keys), n_dc)))
        keys.append(c["ops"])
        types.append(t)
    return HostLog(n_dc, bm.with_ids(keys), key_types=types), reads


@pytest.mark.parametrize("n_dc", WIDTHS)
@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_base_sizes(mat, t, n_dc):
    """Every case once in a batch of its type alone (type_hint) and once inside the five-type
    batch (the planner's sub-streams), on the default store (zone index) and after dropping the
    index (AM_INDEX_NONE: cached reads take the lag view)."""
    log, reads = sweep(t, n_dc)
    st = mat.store(log)
    try:
        for level in ("default", abi.AM_INDEX_NONE):
            if level != "default":
                st.index(level)
            for mixed in (False, True):
                sel = [x for x in reads if mixed or x[1] == t]
                rd = [x[3] for x in sel]
                caps = randlog.caps_for(rd, n_dc, 256)
                compare(mat, st, log, n_dc, rd, caps, [x[2] for x in sel], (t, n_dc, level, "mixed" if mixed else "typed"))
    finally:
        st.close()


# ---------------------------------------------------------------- b. capacity
@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_base_capacity(mat, t):
    """The same key twice in one batch: with room exactly nout (ok, nout pairs) and with nout - 1
    (AM_ERR_CAPACITY), a neighbour key between them and after them staying exact.  (64, 64) and
    (120, 120): base_merge's own check; (121, 1): k_sets; (1024, 1): k_sets with 1025 births."""
    n_dc = 3
    cases = [bm.sizes(t, nb, ns, n_dc) for nb, ns in ((64, 64), (120, 120), (121, 1), (1024, 1))]
    side = bm.sizes(t, 30, 7, n_dc)
    log = HostLog(n_dc, [c["ops"] for c in cases] + [side["ops"]], key_types=[t] * 5)
    reads, caps, names, errors = [], [], [], set()
    for k, c in enumerate(cases):
        for room in (c["nout"], c["nout"] - 1):
            if room < c["nout"]:
                errors.add(len(reads))
            reads.append(bm.read_of(c, k, n_dc))
            caps.append(room)
            names.append("%s room %d" % (c["name"], room))
            reads.append(bm.read_of(side, 4, n_dc))
            caps.append(side["nout"])
            names.append("neighbour")
    st = mat.store(log)
    try:
        want = compare(mat, st, log, n_dc, reads, caps, names, (t, "capacity"), errors)
    finally:
        st.close()
    for i, r in enumerate(want):
        if i in errors:
            assert r == CAPERR, (names[i], r)
        else:
            assert len(r[1]) == caps[i], (names[i], len(r[1]))


# ---------------------------------------------------------------- c. the LDS-sort tier's edges
@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_base_lds_edges(mat, t):
    """basemerge.lds_edge (the birth list exactly full, one past it, the base alone at 1024 and at
    1025) and the TxId reads the wave tier refuses: TxId 5 re-applies two base ops (AW: their tokens
    twice), TxId 9 has no op in the key.  General reads at exactly the room the value needs."""
    n_dc = 3
    rng = random.Random(77 + t)
    cases = bm.lds_edge(t, n_dc) + [bm.txid_dup(t, n_dc), bm.txid_dup(t, n_dc, txid=9)]
    keys = [c["ops"] for c in cases]
    reads = [bm.read_of(c, k, n_dc) for k, c in enumerate(cases)]
    names = [c["name"] for c in cases]
    caps = [c["nout"] for c in cases]
    for n in (5, 40):  # neighbours with TxIds of their own, read fresh under TxId 5
        ops = randlog.rand_key_ops(rng, t, n_dc, n, txids=True, t0=bm.T0)
        reads.append(Read(len(keys), t, {d: ops[-1].commit_time - 4 for d in range(n_dc)}, 5))
        keys.append(ops)
        names.append("filler")
        caps.append(64)
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    st = mat.store(log)
    try:
        want = compare(mat, st, log, n_dc, reads, caps, names, (t, "lds"))
    finally:
        st.close()
    for c, r in zip(cases, want):
        assert len(r[1]) == c["nout"] and r[5] == c["count"], (c["name"], len(r[1]), r[5])


# ---------------------------------------------------------------- d. zone skip
def _skipped(mat):
    v = ctypes.c_uint64()
    abi.check(mat.L.am_ctx_stat(mat.ctx, abi.AM_STAT_OPS_SKIPPED, ctypes.byref(v), 1), "am_ctx_stat")
    return v.value


@pytest.mark.parametrize("ns", [1, 120])
@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_base_zone_skip(mat, t, ns):
    """Key 0 has 1100 ops (its 256-op blocks 0 .. 3 hold only its ops: exact) and a base of 120
    pairs taken after op 600: on the default store the merge runs with the blocks inside the base
    left out (the counter of tests/test_gpu_zones.py), and gives what the store without an index
    and the oracle give.  The MV key has 1000 ops: past AM_BIG_MIN_OPS = 1024 an MV key gets the
    chunked view, and its read over a base goes to k_sets, which streams every block."""
    n_dc = 3
    rng = random.Random(88 + t)
    n_ops = 1100 if t == AW else 1000
    big = bm.sizes(t, 120, ns, n_dc, base_ops=600, new_ops=n_ops - 600)
    assert big["n_base"] == 600 and big["n_read"] == n_ops and bm.wave_tier_key(t, big["ops"])
    side = [bm.sizes(t, 40, 9, n_dc), bm.interleave(t, n_dc)]
    keys = [big["ops"]] + [c["ops"] for c in side]
    reads = [bm.read_of(c, k, n_dc) for k, c in enumerate([big] + side)]
    names = ["zone-120-%d" % ns] + [c["name"] for c in side]
    ops, clock = filler(rng, t, n_dc, 30)
    reads.append(Read(len(keys), t, clock))
    keys.append(ops)
    names.append("filler")
    log = HostLog(n_dc, keys, key_types=[t] * len(keys))
    caps = [256] * len(reads)
    st = mat.store(log)
    try:
        _skipped(mat)
        indexed = compare(mat, st, log, n_dc, reads, caps, names, (t, ns, "indexed"))
        skipped = _skipped(mat)
        st.index(abi.AM_INDEX_NONE)
        plain = compare(mat, st, log, n_dc, reads, caps, names, (t, ns, "no index"))
        assert _skipped(mat) == 0
    finally:
        st.close()
    assert indexed == plain and len(indexed[0][1]) == big["nout"]
    assert skipped > 0, "no block inside the base was skipped"


# ---------------------------------------------------------------- e. hints through the snapshot cache
def _tuple(k, ops):
    return R.OpsTuple(k, len(ops), max(50, len(ops)), len(ops), [(i + 1, randlog.payload_term(op, key=k))
                                                                 for i, op in enumerate(ops)])


def _cache_round(cache, st, keys, types, clocks, tag):
    """One batch through the device cache and the oracle's internal_read/7: values, then the cache
    contents of every key (clocks, last op ids, values, newest first).  Returns the values."""
    reads = [Read(k, types[k], clocks[k]) for k in range(len(keys))]
    got = cache.read(reads, set_capacity=[256] * len(reads))
    vals = []
    for i, rd in enumerate(reads):
        ref = R.internal_read(rd.key, rd.type, dict(rd.clock), R.IGNORE, False, st)
        g = got.result(i)
        assert ref[0] == "ok" and g[0] == "ok", (tag, i, g[:1], ref[:1])
        v = randlog.canon_state(rd.type, ref[1])
        assert g[1] == v, (tag, i, _diff(("ok", g[1]), ("ok", v)))
        vals.append(v)
    for k in range(len(keys)):
        dev = cache.snapshots(k, types[k])
        lst, size = st.snapshot_cache[k]
        assert dev is not None and len(dev) == size == len(lst), (tag, k, len(dev or []), size)
        for (clock, snap), (dclock, dlo, dval) in zip(lst, dev):
            assert dict(clock) == dclock and snap.last_op_id == dlo, (tag, k)
            assert randlog.canon_state(types[k], snap.value) == dval, (tag, k, dlo)
    return vals


@pytest.mark.parametrize("t", [AW, MV])
def test_gpu_base_hints_through_cache(mat, t):
    """SnapshotCache over a reserve()d store against internal_read/7 over a VnodeState.
      round 1   reads after 160 ops store snapshots of 64, 120 and 121 pairs (and five smaller)
      round 2   8 ops later: served from those bases -- 64 and 120 by the wave tier, which tees the
                result into the pool with group hints; 121 by k_sets, copied by k_sc_copy with ~0
                hints.  The new ops replace four pairs, so 120 stays 120 and 121 stays 121
      rounds 3 .. 6   each appends six ops per key in place (am_store_apply): one adds an element /
                value below every existing one -- every group index of the key moves, the hints of
                the cached snapshots now name wrong groups -- and removes the pairs at positions 0,
                63, 64 and the last of the newest value; then every key is read at its newest clock
                (round 3 leaves the 121 key with 118 pairs, stored by k_sc_copy: from round 4 on the
                wave tier reads it over a base without hints)
      rounds 7, 8     no new ops, later clocks: every read is its newest snapshot, unchanged.
    Each key gains at least five ops per round up to 6, so every such read stores a snapshot, and
    every batch reserves 8 x 256 pool words beside them: the pool (4148 words) runs out by round 6 or
    7 and is compacted under the live snapshots; the last rounds read the moved words and hints."""
    n_dc = 3
    nbs = [64, 120, 121, 10, 30, 40, 100, 5]
    keys, types = [], [t] * len(nbs)
    for nb in nbs:
        kills = sorted({j for j in (1, 62, 65, nb - 2) if 0 <= j < nb})
        c = bm.sizes(t, nb, 4, n_dc, kills=kills, base_ops=160, new_ops=8)
        assert (c["n_base"], c["n_read"]) == (160, 168)
        keys.append(list(c["hist"][:168]))
    store0 = mat.store(HostLog(n_dc, keys, key_types=types))
    store = store0.reserve()
    store0.close()
    cache = mat.snapshot_cache(store, len(keys))
    st = R.VnodeState()
    for k, ops in enumerate(keys):
        st.ops_cache[k] = _tuple(k, ops)
    try:
        vals = _cache_round(cache, st, keys, types, [bm.clock_after(ops, 160, n_dc) for ops in keys], 1)
        assert [len(v) for v in vals] == nbs
        vals = _cache_round(cache, st, keys, types, [bm.clock_after(ops, 168, n_dc) for ops in keys], 2)
        assert [len(v) for v in vals][:3] == [66, 120, 121]
        for rnd in range(3, 7):
            new = []
            for k, v in enumerate(vals):
                dead = [v[j] for j in sorted({j for j in (0, 63, 64, len(v) - 1) if j < len(v)})]
                low, tok = 50 - rnd, bm.NEW + 5000 + rnd
                if t == AW:
                    main = sorted([(low, [tok], [])] + [(e, [], [x]) for e, x in dead])
                else:
                    main = ("assign", low, tok, [x for _, x in dead])
                new.append(bm.stamp(t, [main] + bm._pads(t, 5, 10000 + 100 * rnd), n_dc, first=len(keys[k])))
            applied, _ = store.apply(list(range(len(keys))), new_log=HostLog(n_dc, new, key_types=types))
            assert applied, "the appended ops fit the keys' room: applied in place"
            for k in range(len(keys)):
                keys[k] += new[k]
                st.ops_cache[k] = _tuple(k, keys[k])
            before = [len(v) for v in vals]
            vals = _cache_round(cache, st, keys, types, [bm.clock_after(ops, len(ops), n_dc) for ops in keys], rnd)
            assert all(v[0][0] == 50 - rnd for v in vals)  # the new pair sorts first
            assert [len(v) for v in vals] == [n + 1 - len({j for j in (0, 63, 64, n - 1) if j < n}) for n in before]
        assert len(vals[2]) < bm.KB  # the 121 key came down into the wave tier's range
        for rnd in (7, 8):
            top = [{d: ops[-1].commit_time + 10 * rnd + d for d in range(n_dc)} for ops in keys]
            assert _cache_round(cache, st, keys, types, top, rnd) == vals
    finally:
        cache.close()
        store.close()
