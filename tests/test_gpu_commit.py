"""Commit on the device: am_commit_build (a batch of committed transactions' effects -> the CSR op
log over the touched keys) against oplog.Commits.reference_log(), every column exact, and
am_vnode_commit_host (Vnode.commit) against am_vnode_insert_host (Vnode.insert) given the same ops
as a host log, on twin vnodes, and against the oracle's VnodeState (clocksi_vnode:commit/5 ->
update_materializer/3 -> op_insert_gc/3, src/clocksi_vnode.erl:499-531, 634-657,
src/materializer_vnode.erl:622-647).  Then the composition with am_update_objects_host (its effect
columns committed with no re-encoding), the reference's multi-DC / bounded-counter / transaction
suites with every delivery through Vnode.commit, and committers beside readers on one context."""
import ctypes
import random
import threading

import numpy as np
import pytest

from antidote_amd import abi
from antidote_amd.oplog import Commits, Effects, HostBatch, Read, Updates
from oracle import ref_materializer as R
from tests import dcsim, randlog
from tests.kat_util import load
from tests.test_gpu_vnode import _oracle_payload, _placeholder, compare_state

pytestmark = pytest.mark.gpu

PN, LWW, AW, MV, BC = abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER
TYPES = [PN, LWW, AW, MV, BC]


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


# ---------------------------------------------------------------- the builder
IN_COLS = ("dc", "commit_time", "snap_vc", "snap_pres", "txid", "eff_off", "key", "type", "eff_meta", "p0", "p1",
           "var_off", "var_data")


def key_bits_of(cm):
    k = int(cm.key[:cm.n_eff].max()) if cm.n_eff else 0
    return max(1, k.bit_length())


def build(mat, cm, key_bits=None, patch=None, pad=3):
    """am_commit_build over device copies of cm's columns (patch: column -> replacement array, or
    None to drop an optional column; n_* -> replacement count), outputs with spare capacity and a
    stride wider than the batch.  Returns (rc, bad, n_touched, downloaded columns or None)."""
    from antidote_amd.materializer import _DevBuf
    patch = dict(patch or {})
    s = cm.as_struct()
    bufs = []
    try:
        for c in IN_COLS:
            if not getattr(s, c) and c not in patch:
                continue
            a = patch[c] if c in patch else getattr(cm, c)
            if a is None:
                setattr(s, c, None)
                continue
            b = _DevBuf.of(mat, np.ascontiguousarray(a))
            bufs.append(b)
            setattr(s, c, b.ptr)
        for c in ("n_tx", "n_eff", "n_var"):
            if c in patch:
                setattr(s, c, patch[c])
        n, nv, nd = int(cm.n_eff), int(cm.n_var), cm.n_dc
        cap, capv = n + pad, nv + pad + 2
        o = abi.am_commit_log()
        o.cap_ops, o.cap_var, o.snap_stride = cap, capv, cap
        sizes = {"keys": 8 * cap, "key_off": 8 * (cap + 1), "key_type": cap, "key_flags": cap, "op_meta": cap,
                 "commit_time": 8 * cap, "snap_vc": 8 * cap * nd, "snap_pres": 4 * cap, "op_txid": 8 * cap,
                 "p0": 8 * cap, "p1": 8 * cap, "var_off": 8 * (cap + 1), "var_data": 8 * capv, "src": 4 * cap}
        ob = {}
        for c, nb in sizes.items():
            ob[c] = _DevBuf(mat, nb)
            bufs.append(ob[c])
            setattr(o, c, ob[c].ptr)
        log = abi.am_op_log()
        nt, bad = ctypes.c_uint64(99), ctypes.c_uint32(0)
        rc = mat.L.am_commit_build(mat.ctx, nd, ctypes.byref(s), key_bits or key_bits_of(cm), ctypes.byref(o),
                                   ctypes.byref(log), ctypes.byref(nt), ctypes.byref(bad))
        if rc != 0:
            return rc, bad.value, nt.value, None
        m = int(nt.value)
        assert (log.n_keys, log.n_ops, log.n_dc, log.snap_stride) == (m, n, nd, cap)
        assert bool(log.snap_pres) == cm.has_pres and bool(log.op_txid) == cm.has_txid
        assert log.key_off == o.key_off and log.var_data == o.var_data and log.p1 == o.p1

        def get(c, count, dt):
            a = np.zeros(max(count, 1), dt)
            ob[c].download(a)
            return a[:count]
        got = {"keys": get("keys", m, np.uint64), "key_off": get("key_off", m + 1, np.uint64),
               "key_type": get("key_type", m, np.uint8), "key_flags": get("key_flags", m, np.uint8),
               "op_meta": get("op_meta", n, np.uint8), "commit_time": get("commit_time", n, np.uint64),
               "snap_vc": get("snap_vc", cap * nd, np.uint64).reshape(nd, cap)[:, :n] if n else np.zeros((nd, 0), np.uint64),
               "snap_pres": get("snap_pres", n, np.uint32) if cm.has_pres else None,
               "op_txid": get("op_txid", n, np.uint64) if cm.has_txid else None,
               "p0": get("p0", n, np.uint64), "p1": get("p1", n, np.uint64),
               "var_off": get("var_off", n + 1, np.uint64), "src": get("src", n, np.uint32)}
        got["var_data"] = get("var_data", int(got["var_off"][n]) if n else 0, np.uint64)
        return rc, bad.value, m, got
    finally:
        for b in bufs:
            b.free()


def assert_built(mat, cm, **kw):
    rc, bad, m, got = build(mat, cm, **kw)
    assert rc == 0 and bad == 0, (rc, bad)
    ref = cm.reference_log()
    assert m == len(ref["keys"])
    for c, exp in ref.items():
        if exp is None:
            assert got[c] is None, c
        else:
            assert got[c].shape == exp.shape and np.array_equal(got[c], exp), (c, got[c], exp)
    return got


def batch_of(rng, n_eff, n_dc, n_keys, partial=False, txid=False, spread=977):
    """Transactions of 0-4 effects, n_eff in all, on sparse keys (key i -> i * spread + 5), every key
    of one type; set effects of 3-5 words between effects without words."""
    txs, left, t, state = [], n_eff, 0, {}
    while left:
        ne = min(left, rng.choice([0, 1, 1, 2, 3, 4]))
        effs = []
        for _ in range(ne):
            i = rng.randrange(n_keys)
            ty = TYPES[i % 5]
            effs.append((i * spread + 5, ty, randlog.rand_effect(rng, ty, n_dc, state.setdefault(i, {}))))
        snap = {d: 50 + t + d for d in range(n_dc) if not (partial and rng.random() < 0.4)}
        txs.append((rng.randrange(n_dc), 90 + 2 * t, snap, (7000 + t) if txid else None, effs))
        left -= ne
        t += 1
    return txs


@pytest.mark.parametrize("n_eff", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_builder_sizes(mat, n_eff):
    rng = random.Random(4000 + n_eff)
    cm = Commits(3, batch_of(rng, n_eff, 3, max(1, n_eff // 3), txid=n_eff % 2 == 0))
    assert cm.n_eff == n_eff
    assert_built(mat, cm)
    assert_built(mat, cm, key_bits=64, pad=0)


@pytest.mark.parametrize("n_dc,partial", [(1, False), (3, True), (8, False), (8, True), (16, True), (32, False), (32, True)])
def test_builder_dc_counts_and_partial_snapshots(mat, n_dc, partial):
    rng = random.Random(4100 + n_dc + partial)
    cm = Commits(n_dc, batch_of(rng, 150, n_dc, 20, partial=partial, txid=partial))
    assert cm.has_pres == partial
    assert_built(mat, cm)


def _pn(keys, dc=0, ct=10, nd=2):
    return (dc, ct, {d: 5 for d in range(nd)}, None, [(k, PN, i + 1) for i, k in enumerate(keys)])


def test_builder_key_orders_and_runs(mat):
    # keys given in descending order, one effect per transaction
    assert_built(mat, Commits(2, [_pn([k], ct=300 - k) for k in range(130, 0, -1)]))
    # one key taking all effects
    got = assert_built(mat, Commits(2, [_pn([77] * 3, ct=10 + t) for t in range(44)]))
    assert list(got["keys"]) == [77] and list(got["src"]) == list(range(132))
    # a key's run straddling a 64-op tile: ops 60..69 are key 2's
    got = assert_built(mat, Commits(2, [_pn([1] * 4, ct=t) for t in range(15)] + [_pn([2] * 5, ct=50), _pn([2] * 5, ct=51)]
                                    + [_pn([3] * 4, ct=60 + t) for t in range(20)]))
    assert list(got["key_off"]) == [0, 60, 70, 150]
    # two transactions on one key; one transaction twice on one key (two ops, in order)
    got = assert_built(mat, Commits(2, [_pn([9, 4], dc=0, ct=10), _pn([4, 9, 4], dc=1, ct=11)]))
    assert list(got["keys"]) == [4, 9] and list(got["src"]) == [1, 2, 4, 0, 3]
    assert list(got["op_meta"]) == [0, 1, 1, 0, 1] and list(got["p0"]) == [2, 1, 3, 1, 2]
    # transactions without effects at the start, in the middle and at the end
    got = assert_built(mat, Commits(2, [_pn([]), _pn([]), _pn([5, 6], ct=20), _pn([]), _pn([6], ct=21), _pn([]), _pn([])]))
    assert list(got["commit_time"]) == [20, 20, 21]
    # no transaction, and transactions without any effect
    for cm in (Commits(2, []), Commits(2, [_pn([]), _pn([])])):
        rc, bad, m, _ = build(mat, cm)
        assert (rc, bad, m) == (0, 0, 0)


def test_builder_variable_words(mat):
    """Effects without words between non-empty ones, effects of 3-5 words, and effects of 65, 257 and
    5000 words (an MV reset over a large state has the add-wins reset's shape: one flat run)."""
    big = lambda n, base: ("reset", list(range(base, base + n)))  # noqa: E731
    effs = [(1, PN, 1), (2, AW, [(7, [], [])]), (1, PN, 2), (1, PN, 3), (2, AW, [(7, [1], [])]), (2, AW, [(8, [2], [3])]),
            (3, MV, big(65, 100)), (1, PN, 4), (3, MV, big(257, 1000)), (4, BC, ("increment", 5, 1)),
            (3, MV, big(5000, 10 ** 4)), (2, AW, [(1, [4], []), (9, [], [5, 6])]), (1, PN, 5), (3, MV, ("assign", 1, 2, []))]
    txs = [(i % 2, 10 + i, {0: 1, 1: 2}, None, effs[i:i + 3]) for i in range(0, len(effs), 3)]
    cm = Commits(2, txs)
    got = assert_built(mat, cm)
    lens = np.diff(got["var_off"].astype(np.int64))
    assert {0, 3, 4, 5, 9, 65, 257, 5000} <= set(int(x) for x in lens)
    # the same effects many times over: tiles whose words begin and end inside long effects
    rng = random.Random(5)
    many = [(rng.randrange(2), 10 + i, {0: 1, 1: 2}, None, [rng.choice(effs) for _ in range(rng.randint(1, 4))])
            for i in range(120)]
    assert_built(mat, Commits(2, many))
    # var_off == NULL: no effect has words
    cm = Commits(2, [_pn([3, 1, 2], ct=10 + t) for t in range(30)])
    cm.has_var = False
    assert cm.as_struct().var_off is None
    got = assert_built(mat, cm)
    assert not got["var_off"].any() and got["var_data"].size == 0


def test_builder_mixed_types_flag_and_bad_effects(mat):
    cm = Commits(2, [(0, 10, {0: 1, 1: 1}, None, [(4, PN, 1), (4, PN, 2), (9, PN, 5), (6, AW, "bad")]),
                     (1, 11, {0: 2, 1: 2}, None, [(9, LWW, (3, 4)), (4, PN, 3), (6, AW, [(1, [2], [])])])])
    got = assert_built(mat, cm)
    assert list(got["keys"]) == [4, 6, 9] and list(got["key_flags"]) == [0, 0, abi.AM_KEY_MIXED_TYPES]
    assert list(got["key_type"]) == [PN, AW, PN] and int(got["op_meta"][3]) == abi.AM_META_BAD
    # a disagreement deep inside a long run
    txs = [_pn([2, 3], ct=t) for t in range(100)]
    txs[70] = (0, 70, {0: 5, 1: 5}, None, [(2, PN, 1), (3, LWW, (1, 1))])
    got = assert_built(mat, Commits(2, txs))
    assert list(got["key_flags"]) == [0, abi.AM_KEY_MIXED_TYPES]


def test_builder_rejects_invalid_batches(mat):
    rng = random.Random(77)
    cm = Commits(3, batch_of(rng, 200, 3, 30, partial=True))
    assert build(mat, cm)[0] == 0
    nt, n = cm.n_tx, cm.n_eff

    def bad_of(col, fn, **kw):
        a = getattr(cm, col).copy()
        fn(a)
        rc, bad, m, got = build(mat, cm, patch={col: a}, **kw)
        assert rc == abi.AM_ERR_INVALID and got is None and m == 0, (col, rc)
        return bad

    def set_(i, v):
        def f(a):
            a[i] = v
        return f
    assert bad_of("dc", set_(nt // 2, 3)) & abi.AM_COMMIT_BAD_DC
    assert bad_of("dc", set_(nt - 1, 255)) & abi.AM_COMMIT_BAD_DC
    t = next(t for t in range(1, nt) if cm.eff_off[t] > 0)
    assert bad_of("eff_off", set_(t, int(cm.eff_off[t]) + n)) & abi.AM_COMMIT_BAD_EFF_OFF      # decreasing after t
    assert bad_of("eff_off", set_(nt, n - 1)) & abi.AM_COMMIT_BAD_EFF_OFF                       # not ending at n_eff
    assert bad_of("eff_off", set_(0, 1)) & abi.AM_COMMIT_BAD_EFF_OFF                            # not starting at 0
    q = next(q for q in range(2, n) if cm.var_off[q - 1] > 0)
    assert bad_of("var_off", set_(q, 0)) & abi.AM_COMMIT_BAD_VAR_OFF                            # decreasing
    assert bad_of("var_off", set_(n, cm.n_var + 1)) & abi.AM_COMMIT_BAD_VAR_OFF                 # beyond n_var
    assert bad_of("type", set_(n // 2, 0)) & abi.AM_COMMIT_BAD_TYPE
    assert bad_of("type", set_(n - 1, 6)) & abi.AM_COMMIT_BAD_TYPE
    rc, bad, _, _ = build(mat, cm, key_bits=key_bits_of(cm) - 1)
    assert rc == abi.AM_ERR_INVALID and bad & abi.AM_COMMIT_BAD_KEY
    # 2^32 effects are refused on the host, before any column is read
    rc, _, _, _ = build(mat, cm, patch={"n_eff": 2 ** 32})
    assert rc == abi.AM_ERR_INVALID
    # and the batch still builds afterwards
    assert_built(mat, cm)


# ---------------------------------------------------------------- the vnode call
def store_cols(vn):
    d = vn.store().download()
    return {c: (None if a is None else (a if isinstance(a, bool) else np.array(a))) for c, a in d.items()}


def same_cols(a, b):
    assert a.keys() == b.keys()
    for c in a:
        x, y = a[c], b[c]
        if x is None or y is None or isinstance(x, bool):
            assert (x is None) == (y is None) and (x is None or x == y), c
        else:
            assert x.shape == y.shape and np.array_equal(x, y), c


def observe(vn, keys, types):
    return ([(vn.key_info(k), vn.op_ids(k), vn.snapshots(k, types[k])) for k in keys], vn.stats(), store_cols(vn))


def same_twins(a, b, keys, types):
    oa, ob = observe(a, keys, types), observe(b, keys, types)
    assert oa[0] == ob[0]
    assert oa[1] == ob[1], ("stats", oa[1], ob[1])
    same_cols(oa[2], ob[2])


class TxGen:
    """Transactions in the style of tests/test_gpu_vnode.KeyGen: one clock moving 2-4 per
    transaction, snapshot entries trailing it by a fixed lag, causally plausible effects per key."""

    def __init__(self, rng, ktype, n_dc):
        self.rng, self.ktype, self.n_dc, self.clock = rng, ktype, n_dc, 30
        self.state = {}

    def batch(self, quota):
        """quota: {key: ops}.  Transactions of 1-4 effects (a key may come twice in one) until every
        key got its ops."""
        left = dict(quota)
        txs = []
        while left:
            self.clock += self.rng.randint(2, 4)
            effs = []
            for _ in range(self.rng.randint(1, 4)):
                if not left:
                    break
                k = self.rng.choice(sorted(left))
                t = self.ktype[k]
                effs.append((k, t, randlog.rand_effect(self.rng, t, self.n_dc, self.state.setdefault(k, {}))))
                left[k] -= 1
                if not left[k]:
                    del left[k]
            snap = {d: max(0, self.clock - 20) for d in range(self.n_dc)}
            txs.append((self.rng.randrange(self.n_dc), self.clock, snap, None, effs))
        return txs


def commit_both(vc, vi, st, n_dc, txs, ktype, n_keys, dead=()):
    """The batch through Vnode.commit on vc, as a host log through Vnode.insert on vi, and through
    the oracle's op_insert_gc/3."""
    cm = Commits(n_dc, txs)
    by_key = cm.ops_by_key()
    for k in sorted(by_key):
        for op in by_key[k]:
            if k in dead or _placeholder(st, k):
                break
            R.op_insert_gc(k, _oracle_payload(op, k), st)
    vc.commit(cm)
    vi.insert([by_key.get(k, []) for k in range(n_keys)], ktype)


@pytest.mark.parametrize("seed", range(3))
def test_vnode_commit_equals_insert_random(mat, seed):
    rng = random.Random(9300 + seed)
    n_dc = [1, 3, 4][seed]
    n_keys = 20
    ktype = [TYPES[k % 5] for k in range(n_keys)]
    gen = TxGen(rng, ktype, n_dc)
    vc, vi = mat.vnode(n_dc, n_keys), mat.vnode(n_dc, n_keys)
    st = R.VnodeState()
    dcmap = {d: d for d in range(n_dc)}
    dead = set()
    try:
        for step in range(12):
            if step % 2 == 0:
                quota = {k: rng.choice([1, 5, 30, 49, 70]) for k in rng.sample(range(n_keys), 12) if k not in dead}
                commit_both(vc, vi, st, n_dc, gen.batch(quota), ktype, n_keys, dead)
            else:
                reads, sg = [], []
                for _ in range(30):
                    k = rng.randrange(n_keys)
                    if k in dead:
                        continue
                    c = gen.clock
                    q = rng.random()
                    at = c + 5 if q < 0.6 else (c - rng.randint(0, 40) if q < 0.9 else rng.randint(0, c))
                    reads.append(Read(k, ktype[k], {d: max(0, at + rng.randint(-2, 2)) for d in range(n_dc)}))
                    sg.append(rng.random() < 0.08)
                ga = vc.read(reads, should_gc=sg, set_capacity=[4096] * len(reads))
                gb = vi.read(reads, should_gc=sg, set_capacity=[4096] * len(reads))
                for i, rd in enumerate(reads):
                    assert ga.result(i) == gb.result(i), (step, i, rd)
                    if _placeholder(st, rd.key):
                        dead.add(rd.key)
                    if rd.key in dead:
                        continue
                    try:
                        ref = R.internal_read(rd.key, rd.type, dict(rd.clock), R.IGNORE, sg[i], st)
                    except R.LogColdPath:
                        ref = ("cold",)
                    g = ga.result(i)
                    if ref[0] == "cold":
                        assert g == ("error", abi.AM_ERR_COLD_PATH), (step, i, rd, g)
                    elif ref[0] == "error":
                        assert g[0] == "error", (step, i, rd, g, ref)
                    else:
                        assert g[0] == "ok" and g[1] == randlog.canon_state(rd.type, ref[1]), (step, i, rd, g, ref)
            for k in range(n_keys):
                if _placeholder(st, k):
                    dead.add(k)
            same_twins(vc, vi, range(n_keys), ktype)
            compare_state(vc, st, {k: k for k in range(n_keys) if k not in dead}, ktype, dcmap)
    finally:
        vc.close()
        vi.close()


def _flat(key, n, ct0, n_dc=2, per_tx=3, snap_at=5):
    """n PN increments on one key, per_tx per transaction, every snapshot at snap_at: a GC read at
    such a clock prunes nothing, so Length grows up to ListLen."""
    txs, q = [], 0
    while q < n:
        m = min(per_tx, n - q)
        txs.append((q % n_dc, ct0 + q, {d: snap_at for d in range(n_dc)}, None, [(key, PN, 1)] * m))
        q += m
    return txs


@pytest.mark.parametrize("n_ops", [49, 50, 51, 120])
def test_vnode_commit_one_batch_around_the_gc_trigger(mat, n_ops):
    """One batch on one fresh key: op 50 (and 100) runs the GC read before it goes in, so the built
    log is applied in slices."""
    ktype = [PN, PN, PN]
    vc, vi, st = mat.vnode(2, 3), mat.vnode(2, 3), R.VnodeState()
    try:
        txs = _flat(1, n_ops, 100) + [(0, 400, {0: 5, 1: 5}, None, [(2, PN, 7)])]
        commit_both(vc, vi, st, 2, txs, ktype, 3)
        same_twins(vc, vi, range(3), ktype)
        compare_state(vc, st, {k: k for k in range(3)}, ktype, {0: 0, 1: 1})
        assert vc.key_info(1)[2] == n_ops and vc.op_ids(1)[-1] == n_ops
        r = vc.read([Read(1, PN, {0: 1000, 1: 1000})]).result(0)
        assert r[0] == "ok" and r[1] == n_ops
    finally:
        vc.close()
        vi.close()


def test_vnode_commit_full_tuple_growth_rebuild_and_steady_state(mat):
    ktype = [PN] * 10
    vc, vi, st = mat.vnode(2, 4), mat.vnode(2, 4), R.VnodeState()
    dcmap = {0: 0, 1: 1}

    def step(txs, n_keys):
        commit_both(vc, vi, st, 2, txs, ktype[:n_keys], n_keys)
        same_twins(vc, vi, range(n_keys), ktype)
        compare_state(vc, st, {k: k for k in range(n_keys)}, ktype, dcmap)
    try:
        # a key at Length == ListLen: nothing is pruned at these snapshots, so the tuple fills up
        full = 0
        ct = 100
        for n in (49, 1, 20, 30, 1, 1, 45, 60):
            length, list_len, _ = vc.key_info(0)
            full += list_len > 0 and length >= list_len
            step(_flat(0, n, ct), 4)
            ct += n
        assert full >= 1
        # keys past the key space: it grows to the batch's largest key + 1
        step([(0, 900, {0: 5, 1: 5}, None, [(9, PN, 3), (2, PN, 1)]), (1, 901, {0: 5, 1: 5}, None, [(6, PN, 2)])], 10)
        assert vc.n_keys == 10 and vc.key_info(9) == (1, 50, 1)
        # a batch that forces the rebuild: 30 ops on a key that has only the default room
        before = vc.stats()
        step(_flat(7, 30, 1000), 10)
        assert vc.stats()[0] == before[0] + 1
        # steady state: small commits on keys with room never rebuild
        before = vc.stats()
        for i in range(12):
            step([(i % 2, 2000 + i, {0: 5, 1: 5}, None, [(7, PN, 1), (9, PN, 1)])], 10)
        assert vc.stats()[0] == before[0] and vc.stats()[1] > before[1]
        # a failing batch leaves every compared quantity as it was
        seen = observe(vc, range(10), ktype)
        for txs in ([(2, 3000, {0: 5, 1: 5}, None, [(1, PN, 1)])],                       # dc >= n_dc
                    [(0, 3000, {0: 5, 1: 5}, None, [(1, PN, 1), (40, 9, 1)])]):          # an unknown type, a new key
            cm = Commits(2, [(d, c, s, t, [(k, PN, e) for k, _, e in effs]) for d, c, s, t, effs in txs])
            cm.type[:cm.n_eff] = [ty for _, _, _, _, effs in txs for _, ty, _ in effs]
            with pytest.raises(abi.AmError, match="rc=-1"):
                vc.commit(cm)
            now = observe(vc, range(10), ktype)
            assert now[0] == seen[0] and now[1] == seen[1]
            same_cols(now[2], seen[2])
        same_twins(vc, vi, range(10), ktype)
    finally:
        vc.close()
        vi.close()


# ---------------------------------------------------------------- composition
def test_update_objects_effects_commit_unchanged(mat):
    """am_update_objects_host's effect columns go into a Commits with no re-encoding, are committed,
    and a following read returns what tests/dcsim.downstream + the oracle give."""
    n_dc = 2
    ktype = {0: PN, 1: AW, 2: MV, 3: BC}
    vn = mat.vnode(n_dc, 4)
    ora = dcsim.OracleBackend(1, ktype)
    base = np.array([0, 4], np.uint64)
    fresh = iter(range(10 ** 6, 2 * 10 ** 6))
    clock = 100
    steps = [[(0, "increment", 5), (1, "add", 3), (2, "assign", 8), (3, "increment", (40, 0))],
             [(1, "add_all", [3, 4, 9]), (3, "transfer", (15, 1, 0)), (0, "decrement", 2)],
             [(1, "remove", 3), (2, "assign", 9), (3, "decrement", (10, 1))],
             [(1, "remove_all", [4, 7]), (3, "increment", (1, 1)), (2, "assign", 1)]]
    try:
        for upds in steps:
            snap = {d: clock for d in range(n_dc)}
            clock += 10
            keys = [k for k, _, _ in upds]
            hb = HostBatch(n_dc, [Read(k, ktype[k], dict(snap)) for k in keys], [4096] * len(keys))
            b, _ = hb.structs()
            toks = []

            def token():
                toks.append(next(fresh))
                return toks[-1]
            ups = Updates([(i, ktype[k], (op, arg)) for i, (k, op, arg) in enumerate(upds)], token)
            eff = Effects(ups, 4096)
            parts = np.zeros(len(keys), np.uint32)
            u, e = ups.as_struct(), eff.as_struct()
            abi.check(mat.L.am_update_objects_host(vn.handle, 1, base.ctypes.data, parts.ctypes.data, ctypes.byref(b),
                                                   hb.o_set_off.ctypes.data, None, ctypes.byref(u), ctypes.byref(e),
                                                   eff.status.ctypes.data), "am_update_objects_host")
            assert not eff.status[:len(keys)].any()
            # the restatement's effects from the oracle's state, with the tokens the device took
            replay = iter(toks)
            items = []
            for i, (k, op, arg) in enumerate(upds):
                dc = arg[1] if ktype[k] == BC and op != "transfer" else 0
                a = arg[0] if ktype[k] == BC and op != "transfer" else arg
                want = dcsim.downstream(ktype[k], op, a, ora.read(0, k, snap), dc, lambda: next(replay))
                assert eff.effect(i) == want, (k, op, eff.effect(i), want)
                items.append((k, ktype[k], want, snap, 0, clock, None))
            ora.deliver(0, items)
            n = len(keys)
            cm = Commits.from_columns(n_dc, [(0, clock, snap, None, n)], keys, ups.type[:n], eff.eff_meta[:n], eff.p0[:n],
                                      eff.p1[:n], eff.var_off[:n + 1], eff.var_data[:int(eff.var_off[n])])
            vn.commit(cm)
            now = {d: clock for d in range(n_dc)}
            got = vn.read([Read(k, t, dict(now)) for k, t in ktype.items()], set_capacity=[4096] * 4)
            for i, (k, t) in enumerate(ktype.items()):
                r = got.result(i)
                assert r[0] == "ok" and r[1] == randlog.canon_state(t, ora.read(0, k, now)), (k, r)
    finally:
        vn.close()


class CommitBackend(dcsim.GpuBackend):
    """dcsim's GPU backend with every delivery -- a DC's own commits and the remote transactions
    under their origin DC -- through Vnode.commit: consecutive ops of one transaction are one row."""

    def deliver(self, dc, ops):
        txs = []
        for key, type_, eff, snap, origin, ct, txid in ops:
            k = self.kidx[key]
            lab = self._labels(dc, type_, eff)
            tid = self.txids[dc].intern_op(txid, origin, ct) if txid is not None else None
            head = (origin, ct, tuple(sorted(snap.items())), tid)
            if not txs or txs[-1][0] != head:
                txs.append((head, []))
            txs[-1][1].append((k, type_, lab))
        cm = Commits(self.n_dc, [(o, ct, dict(sn), tid, effs) for (o, ct, sn, tid), effs in txs])
        for k, ops_k in cm.ops_by_key().items():
            self.log[dc][k] += ops_k
        self.vn[dc].commit(cm)


SUITES = load("multidc_suites.json")["cases"] + load("txn_suites.json")["cases"]


@pytest.mark.parametrize("case", SUITES, ids=lambda c: c["name"])
def test_suites_through_commit(mat, case):
    made = []

    def factory(n_dc, keys):
        made.append(CommitBackend(n_dc, keys, mat))
        return made[-1]
    checks = dcsim.run_case(case, factory)
    assert checks and made
    for where, got, exp in checks:
        assert got == exp, where


def test_pb_client_suites_through_commit(mat):
    """The pb_client system-suite values (tests/golden/system_suites.json) with real Erlang terms
    through the codec, every transaction one Vnode.commit."""
    from tests import test_gpu_system_suites as S

    class CommitClient(S.Client):
        def commit(self, updates):
            snap = self.clock
            self.clock += 10
            effs = []
            for u in updates:
                eff, rl = self.codec.effect(self.t, self.downstream(u))
                if rl:
                    old, nw = self.codec.take_relabel()
                    self.vn.relabel(old, nw)
                effs.append((0, self.t, eff))
            self.vn.commit([(0, self.clock, {0: snap}, None, effs)])
            self.n += len(effs)
            return self.clock

    cases = [c for c in S.SUITES["cases"] if "txns" in c]
    assert cases
    for case in cases:
        t = S.TYPES[case["type"]]
        cl = CommitClient(mat, t)
        try:
            for txn in case["txns"]:
                cl.commit(txn)
            v = S._value(t, cl.state())
            exp = case["expect"]
            if "value" in exp:
                assert v == S._term(exp["value"]), (case["name"], v)
            if "length" in exp:
                assert len(v) == exp["length"] and all(S._term(x) in v for x in exp["contains"]), (case["name"], v)
        finally:
            cl.close()


# ---------------------------------------------------------------- threads
def test_committers_and_readers_share_a_context(mat):
    """Two committers on disjoint keys and four readers on one context: the run finishes and the
    final state equals the serial one."""
    n_dc, n_keys = 2, 8
    ktype = [PN, AW] * 4
    rng = random.Random(31)
    gens = [TxGen(random.Random(100 + i), ktype, n_dc) for i in range(2)]
    mine = [[0, 1, 2, 3], [4, 5, 6, 7]]
    batches = [[g.batch({k: rng.choice([3, 20, 55]) for k in ks}) for _ in range(6)] for g, ks in zip(gens, mine)]
    vt, vs = mat.vnode(n_dc, n_keys), mat.vnode(n_dc, n_keys)
    errors = []

    def committer(i):
        try:
            for txs in batches[i]:
                vt.commit(txs)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    stop = threading.Event()
    oks = [0] * 4

    def reader(i):
        r = random.Random(i)
        try:
            done = False
            while not done:   # at least one batch after the committers ended
                done = stop.is_set()
                ks = r.sample(range(n_keys), 3)
                at = r.randint(0, 400)  # any clock: one below every cached snapshot is the log's (cold path)
                hb = vt.read([Read(k, ktype[k], {d: at for d in range(n_dc)}) for k in ks], set_capacity=[4096] * 3)
                assert all(int(hb.status[j]) in (0, abi.AM_ERR_COLD_PATH) for j in range(3)), hb.status[:3]
                oks[i] += sum(int(hb.status[j]) == 0 for j in range(3))
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    try:
        ths = [threading.Thread(target=committer, args=(i,)) for i in range(2)]
        rds = [threading.Thread(target=reader, args=(i,)) for i in range(4)]
        for t in ths + rds:
            t.start()
        for t in ths:
            t.join()
        stop.set()
        for t in rds:
            t.join()
        assert not errors, errors
        assert sum(oks) > 0
        for i in range(2):
            for txs in batches[i]:
                vs.commit(txs)
        for k in range(n_keys):
            assert vt.key_info(k)[2] == vs.key_info(k)[2] and vt.op_ids(k)[-1:] == vs.op_ids(k)[-1:]
        now = {d: 10 ** 6 for d in range(n_dc)}
        reads = [Read(k, ktype[k], dict(now)) for k in range(n_keys)]
        a, b = vt.read(reads, set_capacity=[4096] * n_keys), vs.read(reads, set_capacity=[4096] * n_keys)
        for k in range(n_keys):
            assert a.result(k)[:2] == b.result(k)[:2], k
    finally:
        stop.set()
        vt.close()
        vs.close()
