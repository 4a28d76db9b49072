"""The device certifier (am_cert, materializer.Certifier) against tests/certsim.py: every status,
wait, key_info and min_prepared equal to what CertSim gives when it serves the same transactions one
at a time in batch order.  No tolerances.  "Tiny" means cap_keys 8 and cap_entries 8: a 16-slot
table, where collisions, tombstones and compaction happen within a few calls."""
import random
import threading

import pytest

from antidote_amd import abi
from antidote_amd.oplog import Finishes, Prepares
from tests import certcases, certsim
from tests.certsim import NO_UPDATES, OK, WRITE_CONFLICT, CertSim

pytestmark = pytest.mark.gpu

U64_MAX = certcases.U64_MAX


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def check_script(c, script, record=True, sim=None):
    """Every step on the device and on CertSim, compared as it goes; returns the CertSim."""
    sim = sim or CertSim(record)
    for i, step in enumerate(script):
        got, want = certcases.run_step(c, step), certcases.run_step(sim, step)
        assert got == want, (i, step[0], step[1:] if step[0] in ("info", "min") else "", got, want)
    return sim


def state(c, keys):
    return [c.key_info(k) for k in keys], c.size(), c.min_prepared()


def live_entries(sim):
    return sum(len(v) for v in sim.prepared.values())


def needs(script, record=True):
    """The largest number of live entries and of committed keys CertSim holds over the script."""
    sim, e, k = CertSim(record), 1, 1
    for s in script:
        certcases.run_step(sim, s)
        e, k = max(e, live_entries(sim)), max(k, len(sim.committed))
    return k, e


@pytest.mark.parametrize("case", certcases.golden_cases(), ids=[c["name"] for c in certcases.golden_cases()])
def test_gpu_cert_golden_suites(mat, case):
    c = mat.certifier(8, 8, case["record_commits"])
    try:
        assert certsim.replay(case, c.prepare, c.finish, c.read_ready) == []
        assert c.min_prepared() is None
        assert c.size()[1] == 0
    finally:
        c.close()
    c = mat.certifier(8, 8, case["record_commits"])  # again with the accessors against CertSim
    try:
        check_script(c, certcases.golden_script(case), case["record_commits"])
    finally:
        c.close()


@pytest.mark.parametrize("case", certcases.hand_cases(), ids=[c[0] for c in certcases.hand_cases()])
def test_gpu_cert_hand_cases(mat, case):
    _, record, script = case
    c = mat.certifier(8, 8, record)
    try:
        sim = check_script(c, script, record)
        assert c.size()[:2] == (len(sim.committed), live_entries(sim))
    finally:
        c.close()


def test_gpu_cert_hand_case_literals(mat):
    """The literal outcomes tests/test_certsim_cpu.py pins, on the device."""
    c = mat.certifier(8, 8)
    try:
        assert c.prepare([(1, 10, 50, False, [4]), (2, 10, 51, False, [4])]) == [OK, OK]
        assert c.finish([(1, 90, True, [4]), (2, 70, True, [4])]) == [OK, OK]
        assert c.key_info(4) == (70, [])
        assert c.prepare([(3, 80, 100, True, [4])]) == [OK]
        assert c.prepare([(4, 60, 101, True, [5, 4])]) == [WRITE_CONFLICT]
        assert c.prepare([(1, 10, 20, False, [3, 3, 7, 3]), (2, 10, 25, False, [3])]) == [OK, OK]
        assert c.key_info(3) == (0, [(1, 20), (2, 25)]) and c.key_info(7) == (0, [(1, 20)])
        assert c.read_ready([(3, 19), (3, 20), (3, 24), (7, 30), (5, 30), (3, 2001)], 1000) == [0, 10, 10, 10, 0, 2]
    finally:
        c.close()


def test_gpu_cert_batch_shapes(mat):
    c = mat.certifier(128, 256)
    try:
        sim = CertSim()
        one_key = [(100 + i, 10, 50 + i, i >= 3, [9]) for i in range(65)]  # crosses a wave; three stack, the rest conflict
        first = [(1000 + i, 10, 200 + i, True, [100 + i]) for i in range(64)]
        second = [(2000 + i, 10, 300 + i, True, [100 + i]) for i in range(64)]  # each key's second prepare: held
        script = [
            ("prepare", []), ("finish", []), ("read", [], 5), ("min",),
            ("prepare", [(1, 10, 20, True, [1])]), ("info", 1),
            ("prepare", [(2, 10, 21, True, [])]), ("prepare", [(3, 10, 22, False, [])]),
            ("prepare", [(4, 10, 23, True, []), (5, 10, 24, False, []), (6, 10, 25, True, [2]), (7, 10, 26, True, [])]),
            ("prepare", [(8, 10, 27, False, [5, 5, 5, 5])]), ("info", 5),
            ("prepare", one_key), ("info", 9), ("min",),
            ("prepare", first), ("prepare", second),
        ] + [("info", 100 + i) for i in range(64)] + [
            ("finish", [(t[0], 500 + i, i % 3 != 0, t[4]) for i, t in enumerate(one_key[:10])]), ("info", 9),
            ("finish", [(8, 600, True, [5, 5, 5, 5]), (8, 601, False, [5])]), ("info", 5), ("min",),
        ]
        check_script(c, script, sim=sim)
        side = CertSim()
        assert side.prepare(first) == [OK] * 64 and side.prepare(second) == [WRITE_CONFLICT] * 64  # all external
        assert c.size()[:2] == (len(sim.committed), live_entries(sim))
    finally:
        c.close()


@pytest.mark.parametrize("every", [0, 7], ids=["all_certify", "every_7th_stacks"])
def test_gpu_cert_chain_longer_than_any_group_of_rounds(mat, every, capsys):
    """Transaction i names keys {i, i + 1}: whether it conflicts depends on transaction i - 1, so
    the resolve loop needs about 300 dependent decisions, far more than one group of rounds.  On an
    MI355X the all-certify chain took 316 rounds and 8 readbacks (groups of 4, 8, 16, 32, then 64)."""
    n = 300
    txs = [(i + 1, 10, 100 + i, not (every and i % every == 0), [i, i + 1]) for i in range(n)]
    want = CertSim().prepare(txs)
    if not every:
        assert want == [OK if i % 2 == 0 else WRITE_CONFLICT for i in range(n)]
    c = mat.certifier(8, 1024)
    try:
        before = c.stats()
        got = c.prepare(txs)
        after = c.stats()
        with capsys.disabled():
            print(f"\n[cert chain every={every}] rounds {after['rounds'] - before['rounds']}, "
                  f"readbacks {after['readbacks'] - before['readbacks']}")
        assert got == want
        sim = CertSim()
        sim.prepare(txs)
        for k in range(n + 1):
            assert c.key_info(k) == sim.key_info(k), k
        # the fixed point, not a bounded number of rounds: a round decides one more link of a chain, and
        # the chain is the whole batch, or the 6 certifying transactions between two that stack
        assert after["rounds"] - before["rounds"] >= (6 if every else n - 1)
    finally:
        c.close()


def test_gpu_cert_edges_of_the_value_range(mat):
    m = U64_MAX
    c = mat.certifier(8, 8)
    try:
        script = [
            ("prepare", [(m, 0, m, True, [0, m]), (0, m, 0, False, [m])]), ("info", 0), ("info", m), ("min",),
            ("read", [(m, m), (m, 0), (0, m - 1), (0, m), (1, m)], m), ("read", [(0, m), (m, 1), (m, 0)], 0),
            ("prepare", [(5, m, 7, True, [0]), (0, 0, 9, False, [0, m])]), ("info", 0), ("info", m), ("min",),
            ("finish", [(m, m, True, [0, m])]), ("info", 0), ("info", m), ("min",),
            ("prepare", [(6, m, 8, True, [0]), (7, m - 1, 9, True, [m])]), ("info", 0), ("info", m),
            ("finish", [(0, 0, True, [m, 0])]), ("info", 0), ("info", m), ("min",),
            ("prepare", [(8, 0, 0, True, [0])]), ("info", 0), ("min",), ("read", [(0, 0)], 0),
        ]
        check_script(c, script)
    finally:
        c.close()


def test_gpu_cert_collisions_and_tombstones_in_a_tiny_table(mat):
    rng = random.Random(61)
    c = mat.certifier(8, 8)
    try:
        sim, inflight, txid = CertSim(), {}, 1
        for cycle in range(200):
            subset = rng.sample(range(6), rng.randint(1, 6))
            certify = rng.random() < 0.5
            if live_entries(sim) + len(subset) <= 8:  # what a certifier with cap_entries 8 must accept
                txs = [(txid, 10, 100 + cycle, certify, subset)]
                got, want = c.prepare(txs), sim.prepare(txs)
                assert got == want, (cycle, got, want)
                if want == [OK]:
                    inflight[txid] = subset
                txid += 1
            if inflight and (rng.random() < 0.6 or live_entries(sim) > 4):
                t = rng.choice(sorted(inflight))
                txs = [(t, 200 + cycle, rng.random() < 0.5, inflight.pop(t))]
                assert c.finish(txs) == sim.finish(txs), cycle
            for k in range(6):
                assert c.key_info(k) == sim.key_info(k), (cycle, k)
            assert c.min_prepared() == sim.min_prepared(), cycle
            assert c.size()[:2] == (len(sim.committed), live_entries(sim)), cycle
        assert c.stats()["compactions"] > 0  # far more removals than a 16-slot table has slots
        txs = [(t, 0, True, ks) for t, ks in inflight.items()]
        assert c.finish(txs) == sim.finish(txs)
        assert c.size()[1] == 0
        full = [(900 + i, 10, 900 + i, False, [i % 6]) for i in range(8)]  # 8 live entries at once
        assert c.prepare(full) == sim.prepare(full) == [OK] * 8
        assert c.size()[1] == 8
        for k in range(6):
            assert c.key_info(k) == sim.key_info(k)
    finally:
        c.close()


def rc_of(call, *args):
    with pytest.raises(abi.AmError) as e:
        call(*args)
    return e.value.rc


def test_gpu_cert_capacity(mat):
    c = mat.certifier(8, 8)
    keys = list(range(20, 32))
    try:
        sim = CertSim()
        fill = [(1 + i, 10, 50 + i, True, [20 + i]) for i in range(8)]
        assert c.prepare(fill) == sim.prepare(fill) == [OK] * 8
        before = state(c, keys)
        assert before[1] == (0, 8, 8, 8)
        # a ninth entry: one conflicting transaction and one that would add it
        assert rc_of(c.prepare, [(50, 10, 70, True, [20]), (51, 10, 71, True, [28])]) == abi.AM_ERR_CAPACITY
        assert state(c, keys) == before
        assert rc_of(c.prepare, [(52, 10, 72, False, [20, 21])]) == abi.AM_ERR_CAPACITY  # stacking needs room too
        assert state(c, keys) == before
        # a prepare that adds nothing still runs: a conflict, and an entry its TxId already holds
        again = [(60, 10, 73, True, [21]), (1, 10, 74, False, [20])]
        assert c.prepare(again) == sim.prepare(again) == [WRITE_CONFLICT, OK]
        assert state(c, keys) == before
        # eight committed keys, then a finish that needs a ninth
        done = [(1 + i, 100 + i, True, [20 + i]) for i in range(4)]
        assert c.finish(done) == sim.finish(done)
        more = [(70 + i, 500, 80 + i, True, [20 + i]) for i in range(4)]
        assert c.prepare(more) == sim.prepare(more) == [OK] * 4  # after a finish freed entries, the prepare succeeds
        done = [(5 + i, 110 + i, True, [24 + i]) for i in range(4)]
        assert c.finish(done) == sim.finish(done)
        before = state(c, keys)
        assert before[1] == (8, 4, 8, 8)
        ninth = [(70, 300, True, [20]), (71, 301, True, [21, 30])]  # overwrites, removals and one new key
        assert rc_of(c.finish, ninth) == abi.AM_ERR_CAPACITY
        assert state(c, keys) == before
        ok = [(70, 300, True, [20]), (71, 301, False, [21, 30])]  # the abort needs no key
        assert c.finish(ok) == sim.finish(ok)
        for k in keys:
            assert c.key_info(k) == sim.key_info(k), k
        assert c.size() == (8, 2, 8, 8) and c.min_prepared() == sim.min_prepared()
    finally:
        c.close()


def test_gpu_cert_reserve(mat):
    c = mat.certifier(8, 4)
    try:
        sim = CertSim()
        first = [(1, 10, 20, True, [3, 40]), (2, 10, 21, False, [3]), (3, 10, 22, True, [63])]
        assert c.prepare(first) == sim.prepare(first) == [OK] * 3
        fin = [(9, 15, True, [5]), (9, 16, True, [40])]
        assert c.finish(fin) == sim.finish(fin)
        assert c.size() == (2, 4, 8, 4)
        assert rc_of(c.prepare, [(4, 10, 23, True, [6])]) == abi.AM_ERR_CAPACITY
        before = [c.key_info(k) for k in range(64)]
        assert rc_of(c.reserve, 8, 3) == abi.AM_ERR_INVALID  # below the live entries
        assert rc_of(c.reserve, 1, 1024) == abi.AM_ERR_INVALID  # below the committed keys
        assert [c.key_info(k) for k in range(64)] == before and c.size() == (2, 4, 8, 4)
        c.reserve(64, 1024)
        assert c.size() == (2, 4, 64, 1024)
        assert [c.key_info(k) for k in range(64)] == before == [sim.key_info(k) for k in range(64)]
        assert c.min_prepared() == sim.min_prepared() == 20
        rng = random.Random(353)
        txs = [(i + 1, 100 - rng.randint(0, 60), 200 + i, rng.random() < 0.8, [rng.randrange(64) for _ in range(rng.randint(0, 5))])
               for i in range(128)]
        assert sum(len(t[4]) for t in txs) == 335
        assert c.prepare(txs) == sim.prepare(txs)
        for k in range(64):
            assert c.key_info(k) == sim.key_info(k), k
        assert c.size()[:2] == (2, live_entries(sim)) and c.min_prepared() == sim.min_prepared()
        fin = [(t[0], 400 + i, i % 2 == 0, t[4]) for i, t in enumerate(txs)]
        assert c.finish(fin) == sim.finish(fin)
        for k in range(64):
            assert c.key_info(k) == sim.key_info(k), k
        c.reserve(64, 8)  # back down to what is live
        assert [c.key_info(k) for k in range(64)] == [sim.key_info(k) for k in range(64)]
    finally:
        c.close()


@pytest.mark.parametrize("seed", range(20))
def test_gpu_cert_random_histories(mat, seed):
    """60 steps of prepares (1-128 transactions of 0-5 keys from 64 keys, 80 % certify), finishes of
    in-flight and never-prepared TxIds and read_ready batches; the certifier gets exactly the
    capacities CertSim's run of the history needs, so every entry CertSim holds must fit."""
    script = certcases.random_history(random.Random(7000 + seed), 60)
    record = seed % 5 != 4
    cap_keys, cap_entries = needs(script, record)
    c = mat.certifier(cap_keys, cap_entries, record)
    try:
        sim = check_script(c, script, record)
        assert c.size() == (len(sim.committed), live_entries(sim), cap_keys, cap_entries)
    finally:
        c.close()


def test_gpu_cert_invalid_batch_leaves_the_tables(mat):
    c = mat.certifier(8, 8)
    keys = list(range(8))
    try:
        sim = CertSim()
        first = [(1, 10, 20, True, [1, 2]), (2, 10, 21, True, [3])]
        assert c.prepare(first) == sim.prepare(first)
        fin = [(2, 30, True, [3])]
        assert c.finish(fin) == sim.finish(fin)
        before = state(c, keys)
        p = Prepares([(5, 10, 40, True, [4, 5]), (6, 10, 41, False, [6]), (7, 10, 42, True, [7, 0])])
        p.key_off[1], p.key_off[2] = 3, 2  # 0, 3, 2, 5: decreases
        assert rc_of(c.prepare, p) == abi.AM_ERR_INVALID
        assert state(c, keys) == before
        p = Prepares([(5, 10, 40, True, [4, 5])])
        p.key_off[0] = 1  # does not start at 0
        assert rc_of(c.prepare, p) == abi.AM_ERR_INVALID
        p = Prepares([(5, 10, 40, True, [4, 5])])
        p.key_off[1] = 1  # does not end at n_pairs
        assert rc_of(c.prepare, p) == abi.AM_ERR_INVALID
        f = Finishes([(1, 50, True, [1, 2]), (9, 51, True, [4]), (9, 52, True, [5])])
        f.key_off[1], f.key_off[2] = 3, 2
        assert rc_of(c.finish, f) == abi.AM_ERR_INVALID
        assert state(c, keys) == before
        for k in keys:
            assert c.key_info(k) == sim.key_info(k)
        ok = [(5, 10, 40, True, [4, 5])]
        assert c.prepare(ok) == sim.prepare(ok) == [OK]
    finally:
        c.close()


def test_gpu_cert_eight_threads_on_one_certifier(mat):
    """Each thread runs its own history over its own key range; the context lock serializes the calls,
    so every thread sees what CertSim gives for its history alone."""
    c = mat.certifier(8 * 32, 8 * 512)
    scripts = [certcases.random_history(random.Random(8100 + t), 25, n_keys=16, max_tx=24, info_every=0, key_base=1000 * t)
               for t in range(8)]
    sims, errors = [CertSim() for _ in range(8)], []

    def work(t):
        try:
            for i, step in enumerate(scripts[t]):
                got, want = certcases.run_step(c, step), certcases.run_step(sims[t], step)
                if got != want:
                    errors.append((t, i, got, want))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert errors == []
        for t in range(8):
            for k in range(1000 * t, 1000 * t + 18):
                assert c.key_info(k) == sims[t].key_info(k), (t, k)
        mins = [m for m in (s.min_prepared() for s in sims) if m is not None]
        assert c.min_prepared() == (min(mins) if mins else None)
        assert c.size()[:2] == (sum(len(s.committed) for s in sims), sum(live_entries(s) for s in sims))
    finally:
        c.close()
