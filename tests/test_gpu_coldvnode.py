"""A logged vnode (am_vnode_create_logged) against tests/coldlog.LoggedVnode: the oracle's
VnodeState whose internal_read/7 goes to the restated get_up_to_time/5 where the oracle alone
raises LogColdPath.  Random histories with late-delivered transactions (their GC reads go cold)
and readers at old clocks; after every step every read's value and status and the whole state
(tuple headers, op ids, snapshot dicts) are compared.  Then the small cases: a plain twin, insert
refused, and a cold read under read_objects, a write set and an update."""
import pytest

from antidote_amd import abi
from antidote_amd.oplog import Read
from oracle import ref_materializer as R
from tests import coldlog, randlog
from tests.test_gpu_vnode import compare_state

pytestmark = pytest.mark.gpu

AW, PN = abi.AM_AWSET, abi.AM_PN


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def expect_of(ref, type_):
    """An oracle internal_read result as the device renders it: ('ok', value) or ('error', status)."""
    if ref[0] == "ok":
        return ("ok", randlog.canon_state(type_, ref[1]))
    return ("error", abi.AM_ERR_UNEXPECTED_OPERATION)


@pytest.mark.parametrize("seed,n_dc", coldlog.HISTORY_SEEDS)
def test_gpu_logged_vnode_random_history(mat, monkeypatch, seed, n_dc):
    ktype, steps = coldlog.history(seed, n_dc)
    n_keys = coldlog.N_KEYS
    lv = coldlog.LoggedVnode().use(monkeypatch)
    vn = mat.vnode(n_dc, n_keys, logged=True)
    dcmap = {d: d for d in range(n_dc)}
    try:
        for s, step in enumerate(steps):
            if step[0] == "commit":
                for tx in step[1]:
                    lv.commit(tx)
                vn.commit(step[1])
                assert vn.log.size()[0] == len(lv.log)
            else:
                _, reads, sg = step
                got = vn.read([Read(k, t, dict(c)) for k, t, c in reads], should_gc=sg, set_capacity=[4096] * len(reads))
                for i, (k, t, c) in enumerate(reads):
                    ref = lv.read(k, t, c, sg[i])
                    if ref is None:  # the key left the comparison
                        continue
                    g = got.result(i)
                    assert g[:2] == expect_of(ref, t), (s, i, k, c, sg[i], g, ref)
            lv.mark_dead(n_keys)
            compare_state(vn, lv.st, {k: k for k in range(n_keys) if k not in lv.dead}, ktype, dcmap)
        print(seed, n_dc, "cold reads", lv.cold_reads, "with ShouldGC", lv.cold_should_gc, "cold GC reads",
              lv.cold_gc_reads, "left out", sorted(lv.dead))
        # the conditions tests/test_coldlog_cpu.py pre-checks on the CPU: nothing passes vacuously
        assert lv.cold_reads >= coldlog.MIN_COLD_READS
        assert lv.cold_gc_reads >= coldlog.MIN_COLD_GC_READS
        assert len(lv.dead) <= n_keys // 4
    finally:
        vn.close()


def test_gpu_logged_vnode_histories_held_cold_reads_with_should_gc(monkeypatch):
    """Over the seeds above at least 2 cold reads carried ShouldGC: the oracle's own count over the
    same histories (every such read was compared above), so the case holds whichever seeds ran."""
    from tests.test_coldlog_cpu import run_history_on_oracle
    total = sum(run_history_on_oracle(monkeypatch, seed, n_dc).cold_should_gc for seed, n_dc in coldlog.HISTORY_SEEDS)
    assert total >= coldlog.MIN_COLD_SHOULD_GC


# ---------------------------------------------------------------- small cases
KA, KP = 10, 11  # an add-wins set and a PN counter
OLD, AHEAD = {0: 1200, 1: 1200}, {0: 10 ** 4, 1: 10 ** 4}


def aged_history():
    """160 transactions, each adding one token to the set (replacing its element's) and 1 to the
    counter, snapshots monotone (no GC read goes cold): the GC reads at ids 50, 100 and 150 leave
    three cached snapshots and drop the initial {}, so a reader at OLD finds nothing cached."""
    live, txs = {}, []
    for i in range(160):
        ct = 1000 + 10 * i
        e = i % 4
        eff = [(e, [100 + i], list(live.get(e, [])))]
        live[e] = [100 + i]
        txs.append((i % 2, ct, {0: ct - 5, 1: ct - 5}, None, [(KA, AW, eff), (KP, PN, 1)]))
    return txs


def aged_oracle(monkeypatch):
    lv = coldlog.LoggedVnode().use(monkeypatch)
    for tx in aged_history():
        lv.commit(tx)
    return lv


def test_gpu_plain_vnode_and_logged_twin(mat, monkeypatch):
    """The same commits and reads: what the plain vnode answers the twin answers identically, and
    every AM_ERR_COLD_PATH of the plain one is the oracle's value on the twin."""
    lv = aged_oracle(monkeypatch)
    txs = [(d, ct, sn, tx, [(k - KA, t, e) for k, t, e in effs]) for d, ct, sn, tx, effs in aged_history()]
    plain, twin = mat.vnode(2, 2), mat.vnode(2, 2, logged=True)
    try:
        assert plain.log is None and twin.log.size() == (0, 0, 0)
        plain.commit(txs), twin.commit(txs)
        assert twin.log.size()[:2] == (160, 320)
        reads = [Read(0, AW, AHEAD), Read(1, PN, AHEAD), Read(0, AW, OLD), Read(1, PN, OLD), Read(1, PN, {0: 1500, 1: 1495})]
        a, b = plain.read(reads), twin.read(reads)
        cold = 0
        for i, rd in enumerate(reads):
            ref = lv.internal_read(rd.key + KA, rd.type, rd.clock, R.IGNORE, False)
            if a.result(i) == ("error", abi.AM_ERR_COLD_PATH):
                cold += 1
                assert b.result(i)[0] == "ok"
            else:
                assert a.result(i) == b.result(i), (i, a.result(i), b.result(i))
            assert b.result(i)[:2] == expect_of(ref, rd.type), (i, b.result(i), ref)
        assert cold == lv.cold_reads == 2
        assert b.result(3)[1] == 21 and len(b.result(2)[1]) == 4
        for k in range(2):  # a cold read without ShouldGC stores nothing
            assert plain.key_info(k) == twin.key_info(k) and plain.snapshots(k, [AW, PN][k]) == twin.snapshots(k, [AW, PN][k])
    finally:
        plain.close(), twin.close()


def test_gpu_logged_vnode_refuses_insert(mat):
    from antidote_amd.oplog import Op
    vn = mat.vnode(2, 2, logged=True)
    try:
        vn.commit([(0, 10, {0: 5, 1: 5}, None, [(0, PN, 1), (1, PN, 2)])])
        before = [vn.key_info(k) for k in range(2)]
        with pytest.raises(abi.AmError, match=f"rc={abi.AM_ERR_UNSUPPORTED}"):
            vn.insert([[Op(PN, 0, 20, {0: 15, 1: 15}, 1)], []], [PN, PN])
        assert [vn.key_info(k) for k in range(2)] == before and vn.log.size()[:2] == (1, 2)
        # an invalid commit batch leaves the log and the vnode as they were
        with pytest.raises(abi.AmError):
            vn.commit([(0, 30, {0: 25, 1: 25}, None, [(0, PN, 1)]), (2, 31, {0: 25, 1: 25}, None, [(1, PN, 1)])])
        assert [vn.key_info(k) for k in range(2)] == before and vn.log.size()[:2] == (1, 2)
    finally:
        vn.close()


@pytest.fixture(scope="module")
def aged_reader(mat):
    from antidote_amd.readbatch import PartitionedReader
    rd = PartitionedReader(mat, 2, 2, {KA: (AW, []), KP: (PN, [])}, logged=True)
    rd.commit(aged_history())
    yield rd
    rd.close()


def test_gpu_read_objects_serves_a_cold_read(aged_reader, monkeypatch):
    lv = aged_oracle(monkeypatch)
    got = aged_reader.read_objects([(KA, AW), (KP, PN)], OLD)
    want = [expect_of(lv.internal_read(k, t, OLD, R.IGNORE, False), t) for k, t in ((KA, AW), (KP, PN))]
    assert lv.cold_reads == 2
    assert [g[:2] for g in got] == want and want[1] == ("ok", 21) and len(want[0][1]) == 4


def test_gpu_read_objects_ws_folds_the_own_effect_into_a_cold_read(aged_reader, monkeypatch):
    lv = aged_oracle(monkeypatch)
    own = [(9, [999], [])]  # the reading transaction added element 9 itself
    got = aged_reader.read_objects([(KA, AW), (KP, PN)], OLD, write_set={KA: [own], KP: [5]})
    cold = lv.internal_read(KA, AW, OLD, R.IGNORE, False)[1]
    assert lv.cold_reads == 1
    assert got[0][:2] == ("ok", randlog.canon_state(AW, R.materialize_eager(AW, cold, [randlog.effect_term(AW, own)])))
    assert (9, 999) in got[0][1] and got[1][:2] == ("ok", 26)


def test_gpu_update_objects_generates_from_a_cold_read(aged_reader, monkeypatch):
    """An add-wins remove observes the cold value's tokens of its element."""
    lv = aged_oracle(monkeypatch)
    cold = randlog.canon_state(AW, lv.internal_read(KA, AW, OLD, R.IGNORE, False)[1])
    assert lv.cold_reads == 1
    toks = [tok for e, tok in cold if e == 2]
    assert toks
    effs, _, _ = aged_reader.update_objects([(KA, AW, ("remove", 2)), (KP, PN, ("increment", 3))], OLD)
    assert effs == [[(2, [], toks)], 3]
