"""The device log (am_plog) and the cold read served from it, against tests/coldlog.py: every
column PartitionLog.read returns -- status, value, NewLastOp, LastOpCt, IsNewSS, Count, flags --
equals R.materialize on the restated get_up_to_time response, canonicalised with
randlog.canon_state.  Chain lengths 0, 1, 16, 17, 64, 65 and 300 per key are the tier boundaries
of the temporary log (one 16-lane row, one wave, beyond one tile)."""
import random

import pytest

from antidote_amd import abi
from antidote_amd.oplog import Commits, Read
from tests import coldlog, randlog

pytestmark = pytest.mark.gpu

TYPES = [abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER]
LENS = [0, 1, 16, 17, 64, 65, 300]
CASES = coldlog.hand_cases()


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def check_reads(plog, log, reads, cap=4096, all_horizons=True):
    """reads: [(key, type, clock, txid, horizon)]; the device result of each against the helper."""
    hz = None
    if all_horizons or any(h is not None for *_, h in reads):
        hz = [len(log) if h is None else h for *_, h in reads]
    got = plog.read([Read(k, t, dict(c), tx) for k, t, c, tx, _ in reads], horizon=hz, set_capacity=[cap] * len(reads))
    for i, (k, t, c, tx, h) in enumerate(reads):
        want = coldlog.cold_result(log, k, t, c, tx, h)
        assert got.result(i) == want, (i, k, t, c, tx, h, got.result(i), want)
    return got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_plog_hand_cases(mat, case):
    _, n_dc, log, reads, expect = case
    plog = mat.partition_log(n_dc, 4, 8, 8)
    try:
        plog.append(log)
        got = check_reads(plog, log, reads, all_horizons=False)
        assert [got.result(i) for i in range(len(reads))] == expect
    finally:
        plog.close()


def rand_log(rng, n_dc, partial, txids, bad_rate=0.03):
    """A log in which key k (type TYPES[k % 5]) has exactly LENS[k // 5] effects: the key slots
    are shuffled and cut into transactions of 0-3 effects (so one transaction may touch a key
    twice); a tenth of the transactions are delivered late, their snapshots far behind."""
    slots = [k for k in range(5 * len(LENS)) for _ in range(LENS[k // 5])]
    rng.shuffle(slots)
    state, log, pos, t = {}, [], 0, 0
    while pos < len(slots):
        ne = rng.choice([0, 1, 1, 2, 3])
        effs = []
        for k in slots[pos:pos + ne]:
            ty = TYPES[k % 5]
            # (a tenth of the rate on the 300-op keys, so that some of their full reads have a value)
            rate = bad_rate if LENS[k // 5] < 300 else bad_rate / 10
            eff = "bad" if rng.random() < rate else randlog.rand_effect(rng, ty, n_dc, state.setdefault(k, {}))
            effs.append((k, ty, eff))
        pos += ne
        ct = 1000 + 3 * t
        late = rng.random() < 0.1
        dc = rng.randrange(n_dc)
        snap = {}
        for d in range(n_dc):
            if partial and d != dc and rng.random() < 0.25:
                continue
            snap[d] = max(0, ct - (rng.randint(300, 900) if late else rng.randint(1, 12)))
        if partial and rng.random() < 0.1:
            snap[rng.randrange(n_dc)] = 0
        log.append((dc, ct, snap, rng.randint(1, 5) if txids and rng.random() < 0.7 else None, effs))
        t += 1
    return log


def rand_reads(rng, log, n_dc, n, partial, txids):
    top = 1000 + 3 * len(log)
    reads = []
    for _ in range(n):
        k = rng.randrange(5 * len(LENS))
        q = rng.random()
        at = top + 5 if q < 0.3 else rng.randint(1000, top)
        clock = {d: max(0, at + rng.randint(-6, 6)) for d in range(n_dc) if not (partial and rng.random() < 0.2)}
        hz = None if rng.random() < 0.6 else rng.randint(0, len(log))
        reads.append((k, TYPES[k % 5], clock, rng.randint(1, 5) if txids and rng.random() < 0.5 else None, hz))
    return reads


@pytest.fixture(scope="module")
def log3(mat):
    """One random log at D = 3 (partial clocks, TxIds, bad effects) shared by the batch-size cases."""
    rng = random.Random(9401)
    log = rand_log(rng, 3, partial=True, txids=True)
    plog = mat.partition_log(3, 64, 64, 64)
    for i in range(0, len(log), 400):  # several batches: the columns grow, chains cross batches
        plog.append(log[i:i + 400])
    yield plog, log
    plog.close()


@pytest.mark.parametrize("n_dc", [1, 3, 8, 16, 32])
def test_gpu_plog_random_logs(mat, n_dc):
    """All five types, every chain length, partial clocks and TxId reads on two of the widths (both
    at 32, AM_MAX_DC: commit DC 31, presence bit 31), 3 % bad effects, late transactions; a mixed
    batch of 65 reads with horizons on some."""
    rng = random.Random(9300 + n_dc)
    partial, txids = n_dc in (3, 16, 32), n_dc in (3, 8, 32)
    log = rand_log(rng, n_dc, partial, txids)
    cm = Commits(n_dc, log)
    assert cm.n_var > 0 and any(len(e) > 1 for _, _, _, _, effs in log for _, t, e in effs
                                if t == abi.AM_AWSET and e != "bad")  # var_data is gathered
    plog = mat.partition_log(n_dc)
    try:
        plog.append(cm)
        assert plog.size() == (len(log), cm.n_eff, cm.n_var)
        reads = rand_reads(rng, log, n_dc, 65, partial, txids)
        check_reads(plog, log, reads, all_horizons=False)
        # every key once, far ahead of the log: the whole chain survives the filter
        ahead = {d: 10 ** 6 for d in range(n_dc)}
        check_reads(plog, log, [(k, TYPES[k % 5], ahead, None, None) for k in range(5 * len(LENS))], all_horizons=False)
    finally:
        plog.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_gpu_plog_batch_sizes(log3, n):
    plog, log = log3
    rng = random.Random(9500 + n)
    check_reads(plog, log, rand_reads(rng, log, 3, n, True, True))


@pytest.mark.parametrize("type_", TYPES)
def test_gpu_plog_one_type_batches(log3, type_):
    """A batch of one type takes the type's own chain of tiers (type_hint), every chain length."""
    plog, log = log3
    rng = random.Random(9600 + type_)
    reads = [r for r in rand_reads(rng, log, 3, 400, True, True) if r[1] == type_][:40]
    reads += [(k, type_, {0: 10 ** 6, 1: 10 ** 6, 2: 10 ** 6}, None, None) for k in range(5 * len(LENS)) if TYPES[k % 5] == type_]
    check_reads(plog, log, reads, all_horizons=False)


def test_gpu_plog_one_key_three_times(log3):
    """Two reads of one key at different clocks are two keys of the temporary log."""
    plog, log = log3
    k = 5 * LENS.index(65) + TYPES.index(abi.AM_AWSET)
    top = 1000 + 3 * len(log)
    full = lambda at: {0: at, 1: at, 2: at}  # noqa: E731
    check_reads(plog, log, [(k, abi.AM_AWSET, full(top), None, None), (k, abi.AM_AWSET, full(top), None, len(log) // 2),
                            (k, abi.AM_AWSET, full(1000 + top // 3), 2, None), (k, abi.AM_AWSET, full(top), None, 0)])


def test_gpu_plog_capacity_too_small(log3):
    plog, log = log3
    ahead = {0: 10 ** 6, 1: 10 ** 6, 2: 10 ** 6}
    # the longest add-wins key whose full read has a value (no bad effect inside) of two pairs or more
    for n in sorted(LENS, reverse=True):
        k = 5 * LENS.index(n) + TYPES.index(abi.AM_AWSET)
        want = coldlog.cold_result(log, k, abi.AM_AWSET, ahead)
        if want[0] == "ok" and len(want[1]) >= 2:
            break
    assert want[0] == "ok" and len(want[1]) >= 2
    got = plog.read([Read(k, abi.AM_AWSET, ahead), Read(k, abi.AM_AWSET, ahead)], set_capacity=[len(want[1]) - 1, 64])
    assert got.result(0) == ("error", abi.AM_ERR_CAPACITY)
    assert got.result(1) == want


def flat_index(log):
    """key -> [(global effect index, transaction index)] in log order."""
    out, q = {}, 0
    for t, (_, _, _, _, effs) in enumerate(log):
        for k, _, _ in effs:
            out.setdefault(k, []).append((q, t))
            q += 1
    return out


def test_gpu_plog_growth_accessors_and_invalid_batch(mat):
    """Capacities 4 / 8 / 8 and three batches of 7 transactions: every column and key_last grow at
    least twice; after each append key_ops of every key equals the Python log's chain, whole and
    under a horizon; a batch with a dc >= n_dc raises and changes nothing."""
    rng = random.Random(9700)
    n_dc, n_keys = 2, 40
    plog = mat.partition_log(n_dc, 4, 8, 8)
    log, state = [], {}
    try:
        assert plog.size() == (0, 0, 0) and plog.key_ops(3) == []
        for b in range(3):
            batch = []
            for t in range(7):
                effs = []
                for _ in range(rng.choice([0, 2, 3, 4])):
                    k = rng.choice([0, 1, 2, 5, 9 + 10 * b, rng.randrange(n_keys)])
                    effs.append((k, TYPES[k % 5], randlog.rand_effect(rng, TYPES[k % 5], n_dc, state.setdefault(k, {}))))
                ct = 100 + 10 * (7 * b + t)
                batch.append((rng.randrange(n_dc), ct, {0: ct - 3, 1: ct - 5}, None, effs))
            plog.append(batch)
            log += batch
            cm = Commits(n_dc, log)
            assert plog.size() == (len(log), cm.n_eff, cm.n_var)
            idx = flat_index(log)
            for k in range(n_keys + 2):
                assert plog.key_ops(k) == [q for q, _ in idx.get(k, [])], (b, k)
                hz = rng.randint(0, len(log))
                assert plog.key_ops(k, hz) == [q for q, t in idx.get(k, []) if t < hz], (b, k, hz)
        before = plog.size()
        with pytest.raises(abi.AmError):
            plog.append([(0, 500, {0: 1, 1: 1}, None, [(1, abi.AM_PN, 1)]), (n_dc, 501, {0: 1, 1: 1}, None, [(2, abi.AM_PN, 1)])])
        with pytest.raises(abi.AmError):
            plog.append([(n_dc, 502, {0: 1, 1: 1}, None, [])])
        assert plog.size() == before
        idx = flat_index(log)
        for k in range(n_keys + 2):
            assert plog.key_ops(k) == [q for q, _ in idx.get(k, [])], k
        # the grown log still reads right
        top = {0: 10 ** 4, 1: 10 ** 4}
        check_reads(plog, log, [(k, TYPES[k % 5], top, None, None) for k in range(n_keys)], all_horizons=False)
        check_reads(plog, log, [(k, TYPES[k % 5], {0: 150, 1: 150}, None, 9) for k in range(n_keys)])
    finally:
        plog.close()


def test_gpu_logged_vnode_relabel_reaches_the_log(mat):
    """Terms through the codec into a logged vnode; once the GC reads at ids 50, 100 and 150 have
    dropped the initial {} snapshot, a reader at an old clock is served from the log.  A forced
    relabel (terms interned between two stored ones until the label space there runs out) is
    applied with Vnode.relabel: the cold read, decoded through the codec, still gives the terms."""
    from antidote_amd.codec import Codec
    from tests.test_gpu_codec import KeyHist, _canon, _force_relabel
    rng = random.Random(9800)
    types = [abi.AM_AWSET, abi.AM_MVREG, abi.AM_LWW]
    codec = Codec()
    vn = mat.vnode(1, len(types), logged=True)
    hist = [KeyHist(rng, t) for t in types]
    old_state = None
    try:
        txs = []
        for i in range(160):
            ct = 1000 + 10 * i
            effs = []
            for k, t in enumerate(types):
                eff = hist[k].effect(ct)
                leff, rl = codec.effect(t, eff)
                assert not rl
                hist[k].apply(eff)
                effs.append((k, t, leff))
            txs.append((0, ct, {0: ct - 5}, None, effs))
            if ct == 1200:  # what a reader at {0: 1200} sees: transactions 0 .. 20
                old_state = [_canon(t, hist[k].state) for k, t in enumerate(types)]
        vn.commit(txs)
        at = {0: 1200}
        for k, t in enumerate(types):  # nothing cached at or below the old clock: the read is the log's
            snaps = vn.snapshots(k, t)
            assert len(snaps) == 3 and all(c[0] > 1200 for c, _, _ in snaps), (k, snaps)

        def cold():
            hb = vn.read([Read(k, t, at) for k, t in enumerate(types)], set_capacity=[4096] * len(types))
            return [hb.result(k) for k in range(len(types))]
        for k, r in enumerate(cold()):
            assert r[0] == "ok" and _canon(types[k], codec.value(types[k], r[1])) == old_state[k], (k, r)
        old, new = _force_relabel(codec)
        assert len(old) > 0
        vn.relabel(old, new)
        for k, r in enumerate(cold()):
            assert r[0] == "ok" and _canon(types[k], codec.value(types[k], r[1])) == old_state[k], (k, r, "after relabel")
    finally:
        vn.close()
        codec.close()
