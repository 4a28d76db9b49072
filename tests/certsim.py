"""A sequential restatement of the partition's certification, over plain dicts: the checker a
device certifier (prepare, commit / abort clean-up and the read servers' probe in HBM) is tested
against, in the role tests/dcsim.py has for the materializer.  No device code uses it yet.

    clocksi_vnode:prepare/6, set_prepared/5, reset_prepared/5      src/clocksi_vnode.erl:450-497
    clocksi_vnode:commit/5, clean_and_notify/3, clean_prepared/3   :499-582
    certification_check/4, certification_with_check/4, check_prepared/3   :588-632
    get_min_prep/1                                                 :671-678
    clocksi_readitem_server:check_clock/4, check_prepared_list/3   src/clocksi_readitem_server.erl:236-264

One command at a time, as the vnode serves its mailbox.  committed_tx is a dict key -> time;
prepared_tx a dict key -> [(txid, time)] in the reference's order (set_prepared prepends, so the
newest entry is first; keydelete removes the first match), which key_info flattens to a list
sorted by (time, txid), the form a device accessor can return.  Times are the caller's: prepare_time stands for the NewPrepare
that dc_utilities:now_microsec() gives at :457.
"""
OK, WRITE_CONFLICT, NO_UPDATES = 0, 7, 8
SPIN_WAIT_MS = 10  # ?SPIN_WAIT, include/antidote.hrl:53


class CertSim:
    def __init__(self, record_commits: bool = True):
        self.record_commits = record_commits  # application:get_env(antidote, txn_cert), :508-514
        self.committed = {}
        self.prepared = {}

    # ---- certification_check/4 (:588-632)
    def _certify(self, start, certify, keys):
        if not certify:
            return True
        for k in keys:
            if k in self.committed and self.committed[k] > start:
                return False
            if self.prepared.get(k):  # check_prepared/3 ignores the TxId
                return False
        return True

    def prepare_one(self, txid, start, prepare_time, certify, keys):
        if not self._certify(start, certify, keys):
            return WRITE_CONFLICT
        if not keys:
            return NO_UPDATES
        for k in keys:  # set_prepared + reset_prepared: one entry per distinct key, prepended
            active = self.prepared.get(k, [])
            if any(t == txid for t, _ in active):
                continue
            self.prepared[k] = [(txid, prepare_time)] + active
        return OK

    def prepare(self, txs):
        """[(txid, start_time, prepare_time, certify, [key, ...])] -> statuses"""
        return [self.prepare_one(*t) for t in txs]

    def finish_one(self, txid, commit_time, committed, keys):
        if not keys:
            return NO_UPDATES
        if committed and self.record_commits:
            for k in keys:
                self.committed[k] = commit_time  # ets:insert overwrites: the last commit wins
        for k in keys:  # clean_prepared/3: lists:keydelete, then delete the row when it is empty
            active = self.prepared.get(k, [])
            for i, (t, _) in enumerate(active):
                if t == txid:
                    active = active[:i] + active[i + 1:]
                    break
            if active:
                self.prepared[k] = active
            else:
                self.prepared.pop(k, None)
        return OK

    def finish(self, txs):
        """[(txid, commit_time, committed, [key, ...])] -> statuses"""
        return [self.finish_one(*t) for t in txs]

    def read_ready_one(self, key, start, now):
        if start > now:  # check_clock/4
            return (start - now) // 1000 + 1
        for _, t in self.prepared.get(key, []):  # check_prepared_list/3
            if t <= start:
                return SPIN_WAIT_MS
        return 0

    def read_ready(self, reads, now):
        return [self.read_ready_one(k, s, now) for k, s in reads]

    def min_prepared(self):
        """The minimum prepare time in the table, None when it is empty (get_min_prep/1 answers from
        an orddict keyed by time, which equals this while in-flight prepare times are distinct)."""
        times = [t for lst in self.prepared.values() for _, t in lst]
        return min(times) if times else None

    def key_info(self, key):
        return self.committed.get(key, 0), sorted(self.prepared.get(key, []), key=lambda e: (e[1], e[0]))

    def key_list(self, key):
        """The key's entries in the reference's list order (newest first)."""
        return list(self.prepared.get(key, []))


STATUS_NAMES = {"ok": OK, "write_conflict": WRITE_CONFLICT, "no_updates": NO_UPDATES}


def replay(case, prepare, finish, read_ready):
    """Run one case of tests/golden/suite_certification.json through three callables shaped like
    CertSim's methods; returns [(step index, expected, got)] for the steps that disagree."""
    wrong = []
    for i, st in enumerate(case["steps"]):
        if st["op"] == "prepare":
            got = prepare([(t["txid"], t["start"], t["prepare"], t.get("certify", True), t["keys"]) for t in st["tx"]])
            exp = [STATUS_NAMES[s] for s in st["expect"]]
        elif st["op"] == "finish":
            got = finish([(t["txid"], t.get("commit_time", 0), t["committed"], t["keys"]) for t in st["tx"]])
            exp = [STATUS_NAMES[s] for s in st["expect"]]
        else:
            got = ["wait" if w else "ready" for w in read_ready([tuple(r) for r in st["reads"]], st["now"])]
            exp = st["expect"]
        if got != exp:
            wrong.append((i, exp, got))
    return wrong
