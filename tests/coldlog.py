"""The log cold path restated for the tests: logging_vnode:get_up_to_time/5
(src/logging_vnode.erl:522-545, 586-591, 676-779) over a Python log, and a VnodeState whose
internal_read/7 takes it when the snapshot cache has nothing at or below the read clock
(src/materializer_vnode.erl:400-403, 415-419).  The reference holds no KAT for this path, so
this restatement pins the rule; oracle/ref_materializer.py is used as it is.

The log is a list of committed transactions in the order their commit records were appended, in
the shape oplog.Commits takes: (dc, commit_time, snap, txid, [(key, type, effect), ...]), the
string "bad" standing for an effect Type:update/2 raises on."""
from typing import Any, Dict, List, Optional, Sequence, Tuple

from antidote_amd.oplog import Op
from oracle import ref_materializer as R
from tests import randlog

Tx = Tuple[int, int, Dict[int, int], Optional[int], Sequence[Any]]
_GET_FROM_SNAPSHOT_CACHE = R.get_from_snapshot_cache  # the oracle's own, whatever is patched in later


def check_max_time(snapshot_time, max_ss) -> bool:
    """src/logging_vnode.erl:778-779."""
    return max_ss == R.UNDEFINED or R.vc_le(snapshot_time, max_ss)


def check_min_time(snapshot_time, min_ss) -> bool:
    """:775-776 (MinSnapshotTime is undefined on this path)."""
    return min_ss == R.UNDEFINED or R.vc_le(min_ss, snapshot_time)


def _payload(dc, ct, snap, txid, key, type_, eff) -> R.Payload:
    bad = isinstance(eff, str) and eff == "bad"
    return randlog.payload_term(Op(type_, dc, ct, dict(snap), None if bad else eff, txid, bad=bad), key=key)


def get_up_to_time(log: Sequence[Tx], key, type_, max_ss, horizon: Optional[int] = None) -> R.SnapshotGetResponse:
    """get_up_to_time(LogId, Partition, MaxSnapshotTime, Type, Key) over the first `horizon`
    transactions of the log: handle_command({get, ...}) -> get_ops_from_log -> filter_terms_for_key
    with Key = {key, Key}, MinSnapshotTime = undefined."""
    min_ss = R.UNDEFINED
    ops: Dict[int, list] = {}         # Ops: TxId -> its update records on Key (dict:append)
    committed: Dict[Any, list] = {}   # CommittedOpsDict: key -> [#clocksi_payload{}], oldest first
    for t, (dc, ct, snap, txid, effs) in enumerate(log[:len(log) if horizon is None else horizon]):
        for k, ty, eff in effs:       # handle_update: the update records of the transaction, in order
            if k == key:
                ops.setdefault(t, []).append((k, ty, eff))
        if t in ops:                  # handle_commit: the transaction's commit record
            for k, ty, eff in ops.pop(t):
                if check_min_time(snap, min_ss) and check_max_time(snap, max_ss):
                    committed.setdefault(k, []).append(_payload(dc, ct, snap, txid, k, ty, eff))
    # finish_op_load -> reverse_and_add_op_id(CommittedOps, 0, []): ids 0, 1, ... oldest first, the list
    # newest first
    lst: List[Tuple[int, R.Payload]] = []
    for i, p in enumerate(committed.get(key, [])):
        lst = [(i, p)] + lst
    return R.SnapshotGetResponse(ops_list=lst, number_of_ops=len(lst),
                                 materialized_snapshot=R.MatSnapshot(last_op_id=0, value=R.crdt_new(type_)),
                                 snapshot_time={}, is_newest_snapshot=False)


def cold_result(log, key, type_, clock, txid=None, horizon=None):
    """materialize/4 on the response, as the ABI renders a result: what PartitionLog.read returns."""
    from antidote_amd import abi
    resp = get_up_to_time(log, key, type_, dict(clock), horizon)
    R.MissingDcLog.count = 0
    try:
        r = R.materialize(type_, R.IGNORE if txid is None else txid, dict(clock), resp)
    except R.CorruptedOpsCache:
        return ("error", abi.AM_ERR_CORRUPTED_OPS_CACHE)
    if r[0] == "error":
        return ("error", abi.AM_ERR_UNEXPECTED_OPERATION)
    _, val, nlo, ct, newss, count = r
    flags = abi.AM_FLAG_MISSING_DC_LOGGED if R.MissingDcLog.count else 0
    return ("ok", randlog.canon_state(type_, val), nlo, None if ct == R.IGNORE else dict(ct), newss, count, flags)


class LoggedVnode:
    """An R.VnodeState plus the partition's log: internal_read/7 whose get_from_snapshot_cache/5
    goes to the log where the oracle raises LogColdPath.  use() patches
    R.get_from_snapshot_cache for the caller's duration (pytest's monkeypatch undoes it)."""

    def __init__(self):
        self.st = R.VnodeState()
        self.log: List[Tx] = []
        self.horizon: Optional[int] = None  # the transactions a read may see; None = the whole log
        self.last_cold = False
        self.dead = set()         # keys whose tuple holds prune_ops' placeholder (a reference crash)
        self.cold_reads = 0       # reader cold reads
        self.cold_should_gc = 0   # ... of them with ShouldGC
        self.cold_gc_reads = 0    # cold GC reads of commits
        self._orig = _GET_FROM_SNAPSHOT_CACHE

    def use(self, monkeypatch):
        monkeypatch.setattr(R, "get_from_snapshot_cache", self._get_from_snapshot_cache)
        return self

    def _get_from_snapshot_cache(self, txid, key, type_, min_ss_time, st):
        """src/materializer_vnode.erl:384-413 with the `undefined` branch (:400-403) taken."""
        try:
            return self._orig(txid, key, type_, min_ss_time, st)
        except R.LogColdPath:
            self.last_cold = True
            return get_up_to_time(self.log, key, type_, min_ss_time, self.horizon)

    def internal_read(self, key, type_, clock, txid, should_gc):
        self.last_cold = False
        self.horizon = None
        r = R.internal_read(key, type_, dict(clock), txid, should_gc, self.st)
        if self.last_cold:
            self.cold_reads += 1
            self.cold_should_gc += 1 if should_gc else 0
        return r

    def read(self, key, type_, clock, should_gc):
        """internal_read for a test's read batch: None once the key has left the comparison."""
        if placeholder(self.st, key):
            self.dead.add(key)
        if key in self.dead:
            return None
        return self.internal_read(key, type_, clock, R.IGNORE, should_gc)

    def mark_dead(self, n_keys):
        for k in range(n_keys):
            if placeholder(self.st, k):
                self.dead.add(k)

    def commit(self, tx: Tx):
        """append_commit, then update_materializer: op_insert_gc/3 per effect, whose GC read sees
        the log up to and including this transaction."""
        self.log.append(tx)
        dc, ct, snap, txid, effs = tx
        for k, ty, eff in effs:
            if placeholder(self.st, k):  # pruned empty by an earlier GC read: the key leaves the comparison
                self.dead.add(k)
            if k in self.dead:
                continue
            self.last_cold = False
            self.horizon = len(self.log)
            R.op_insert_gc(k, _payload(dc, ct, snap, txid, k, ty, eff), self.st)
            if self.last_cold:
                self.cold_gc_reads += 1
        self.horizon = None


def placeholder(st, k) -> bool:
    """prune_ops kept element(FIRST_OP+Len) -- a 0 -- when it pruned every op
    (src/materializer_vnode.erl:580-583); the reference's next read of the key crashes on it, so
    such keys leave the comparison (as in tests/test_gpu_vnode.py)."""
    t = st.ops_cache.get(k)
    return t is not None and t.element(2)[0] > 0 and t.element(R.FIRST_OP) == 0


# ---------------------------------------------------------------- random histories
# The generator of tests/test_gpu_coldvnode.py; tests/test_coldlog_cpu.py runs it against the helper
# alone and asserts the same conditions, so the seeds are chosen on the CPU.
HISTORY_SEEDS = [(9300, 1), (9301, 8), (9302, 4), (9303, 3)]  # (seed, n_dc)
N_KEYS = 20
MIN_COLD_READS, MIN_COLD_GC_READS, MIN_COLD_SHOULD_GC = 8, 1, 2  # per seed, per seed, over the seeds


def history(seed: int, n_dc: int):
    """[('commit', [Tx]) | ('read', [(key, type, clock)], [should_gc])]: seven commit batches of 40
    or 120 transactions on 1-4 keys each (1-2 effects per key), snapshots trailing the commit by
    1-20, 15 % of the transactions delivered late (every entry 300-1500 behind); after each a batch
    of 30 reads, clocks ahead, slightly behind or anywhere in the past, ShouldGC on about 10 % of
    the reads and about 30 % of the past ones."""
    import random
    from antidote_amd import abi
    types = [abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER]
    rng = random.Random(seed)
    ktype = [types[k % 5] for k in range(N_KEYS)]
    state: Dict[int, dict] = {}
    clock = 2000
    steps = []
    for b in range(7):
        txs = []
        for _ in range(rng.choice([40, 120])):
            clock += rng.randint(2, 4)
            late = rng.random() < 0.15
            snap = {d: max(0, clock - (rng.randint(300, 1500) if late else rng.randint(1, 20))) for d in range(n_dc)}
            effs = []
            for k in rng.sample(range(N_KEYS), rng.randint(1, 4)):
                for _ in range(rng.randint(1, 2)):
                    effs.append((k, ktype[k], randlog.rand_effect(rng, ktype[k], n_dc, state.setdefault(k, {}))))
            txs.append((rng.randrange(n_dc), clock, snap, None, effs))
        steps.append(("commit", txs))
        reads, sg = [], []
        for _ in range(30):
            k = rng.randrange(N_KEYS)
            q = rng.random()
            past = q >= 0.8
            at = clock + 5 if q < 0.5 else (clock - rng.randint(0, 40) if not past else rng.randint(0, clock))
            reads.append((k, ktype[k], {d: max(0, at + rng.randint(-2, 2)) for d in range(n_dc)}))
            sg.append(rng.random() < (0.3 if past else 0.1))
        steps.append(("read", reads, sg))
    return ktype, steps


# ---------------------------------------------------------------- hand-written cases
# (name, n_dc, log, [(key, type, clock, txid, horizon)], [expected result per read]) -- the
# expectations are written out by hand from the reference's rules; tests/test_coldlog_cpu.py holds
# the helper to them, tests/test_gpu_plog.py the device.
def hand_cases():
    from antidote_amd import abi
    PN, LWW, MISS = abi.AM_PN, abi.AM_LWW, abi.AM_FLAG_MISSING_DC_LOGGED
    both = {0: 20, 1: 20}
    return [
        # the middle transaction fails vectorclock:le(SnapshotTime, MaxSnapshotTime): it gets no id,
        # so the newest survivor's id is 1, not 2
        ("filtered_op_shifts_ids", 2,
         [(0, 10, {0: 5, 1: 5}, None, [(0, PN, 1)]),
          (0, 60, {0: 50, 1: 5}, None, [(0, PN, 2)]),
          (1, 12, {0: 7, 1: 7}, None, [(0, PN, 4)])],
         [(0, PN, both, None, None)],
         [("ok", 5, 1, {0: 10, 1: 12}, True, 2, 0)]),
        # id 0 passes the filter (snapshot 5 <= 20) but commits at 100: FirstHole = 0 - 1
        ("id0_not_included_gives_minus_one", 2,
         [(0, 100, {0: 5, 1: 5}, None, [(0, PN, 1)])],
         [(0, PN, both, None, None)],
         [("ok", 0, -1, {}, False, 0, 0)]),
        # snapshot_time[dc] = 50 > commit_time = 10: the inclusion test (on the commit-substituted
        # vector {0: 10, 1: 5}) would pass, the filter (on snapshot_time itself) drops the op
        ("snapshot_entry_above_commit_time", 2,
         [(0, 10, {0: 50, 1: 5}, None, [(0, PN, 1)])],
         [(0, PN, both, None, None)],
         [("ok", 0, 0, {}, False, 0, 0)]),
        # a DC missing from the read clock: a 0 snapshot entry passes le (missing = 0) and then
        # fails the inclusion test with the logger:error; a positive entry is filtered out
        ("dc_missing_from_read_clock", 2,
         [(0, 10, {0: 5, 1: 0}, None, [(0, PN, 1)]),
          (0, 11, {0: 5, 1: 3}, None, [(1, PN, 1)])],
         [(0, PN, {0: 20}, None, None), (1, PN, {0: 20}, None, None)],
         [("ok", 0, -1, {}, False, 0, MISS), ("ok", 0, 0, {}, False, 0, 0)]),
        # the LWW effect on a PN key is corrupted_ops_cache only for a read whose filter keeps it
        ("type_mismatch_among_filtered_ops", 2,
         [(0, 10, {0: 5, 1: 5}, None, [(0, PN, 3)]),
          (0, 60, {0: 50, 1: 50}, None, [(0, LWW, (7, 7))])],
         [(0, PN, both, None, None), (0, PN, {0: 100, 1: 100}, None, None)],
         [("ok", 3, 0, {0: 10, 1: 5}, True, 1, 0), ("error", abi.AM_ERR_CORRUPTED_OPS_CACHE)]),
        # no survivor: a key the log never saw, a key whose ops are all above the clock, horizon 0
        ("zero_survivors", 2,
         [(0, 10, {0: 50, 1: 50}, None, [(0, PN, 3)]),
          (0, 12, {0: 5, 1: 5}, None, [(1, LWW, (9, 4))])],
         [(7, PN, both, None, None), (0, PN, both, None, None), (1, LWW, both, None, 0), (1, LWW, both, None, None)],
         [("ok", 0, 0, {}, False, 0, 0), ("ok", 0, 0, {}, False, 0, 0), ("ok", (0, 0, True), 0, {}, False, 0, 0),
          ("ok", (9, 4, False), 0, {0: 12, 1: 5}, True, 1, 0)]),
        # two effects of one transaction on one key stay two ops in order; transactions without
        # effects count for the horizon; a horizon in the middle; the reader's own TxId
        ("one_transaction_twice_and_horizons", 2,
         [(0, 10, {0: 5, 1: 5}, 41, [(0, LWW, (3, 1)), (0, LWW, (3, 2)), (1, PN, 1)]),
          (0, 11, {0: 5, 1: 5}, None, []),
          (1, 12, {0: 6, 1: 6}, 42, [(0, LWW, (2, 9)), (1, PN, 10)]),
          (1, 40, {0: 6, 1: 6}, 43, [(1, PN, 100)])],
         [(0, LWW, both, None, None), (1, PN, both, None, 2), (1, PN, both, None, 3), (1, PN, both, 43, None),
          (1, PN, both, None, None)],
         [("ok", (3, 2, False), 2, {0: 10, 1: 12}, True, 3, 0), ("ok", 1, 0, {0: 10, 1: 5}, True, 1, 0),
          ("ok", 11, 1, {0: 10, 1: 12}, True, 2, 0), ("ok", 11, 1, {0: 10, 1: 12}, True, 2, 0),
          ("ok", 11, 1, {0: 10, 1: 12}, True, 2, 0)]),
    ]
