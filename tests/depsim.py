"""TEST INFRASTRUCTURE ONLY.  A sequential restatement of the reference's dependency buffer,
src/inter_dc_dep_vnode.erl:94-154, 187-238: one DepSim per partition, one command at a time.  It is the
contract of am_dep (antidote_amd/csrc/am_dep.hip) and of scripts/dep_cpu.cpp: a batched call leaves
the state, and returns the deliveries, that serving the batch one arrival at a time in batch order
through this class gives.

A transaction is (dc, timestamp, snapshot, ping, tag): #interdc_txn{dcid, timestamp, snapshot},
ping = (log_records == []), tag = the caller's handle, returned when the transaction is delivered
(logging_vnode:append_group + materializer_vnode:update, :146-152).

Decisions the reference leaves open:
  1. Queue order within a round.  process_all_queues/1 folds over dict:fetch_keys(Queues) (:98), the
     hash order of the DC ids, which the un-vendored runtime decides.  Here it is an explicit
     permutation `order` of the DC indices (None = ascending); a DC whose queue never received
     anything is skipped, as an absent dict key is.
  2. now.  get_partition_clock/1 reads dc_utilities:now_microsec() inside every try_store (:238);
     here the caller gives one `now` per handle() (the device takes one per batch).
  3. Publication.  update_clock/3 pushes the clock to meta_data_sender at most every
     ?VECTORCLOCK_UPDATE_PERIOD (:215-230); here `clock` is always current and the reader's timer
     decides when it is looked at.  Any clock a reader sees is one the vnode held after some call.
  4. Timestamp - 1 at timestamp 0 (:141) is -1 in Erlang and has no u64 form: a non-ping transaction
     with timestamp 0 is rejected (ValueError; AM_DEP_BAD_TIME on the device).
  5. An empty batch changes nothing: process_all_queues/1 runs only on an arrival (:159-161).

The quirk that follows from :97-103 and :141: an arrival into an empty queue d that fails raises
clock[d] to ts - 1 at d's turn in the round; queues visited before d in that round are not retried
(the round stored nothing), queues visited after d see the raise.  Delivery therefore depends on the
queue order, and "push the whole batch, then run to the fixed point" is not this contract.
"""
from __future__ import annotations

from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

from oracle.ref_materializer import vc_le

Txn = Tuple[int, int, Dict[int, int], bool, int]


class DepSim:
    def __init__(self, n_dc: int, own_dc: int, order: Optional[Sequence[int]] = None):
        self.n_dc, self.own_dc = n_dc, own_dc
        self.order = list(order) if order is not None else list(range(n_dc))
        assert sorted(self.order) == list(range(n_dc))
        self.clock: Dict[int, int] = {}          # vectorclock:new(), :89
        self.queues: Dict[int, deque] = {}       # dict:new(), :90
        self.drop_ping = False
        self.rounds = 0                          # process_all_queues/1 passes, for the tests
        self.first_try_failed = 0                # non-ping transactions whose first try_store failed
        self._tried: set = set()

    # handle_command({set_dependency_clock, Vector}), :156-157
    def set_dependency_clock(self, vc: Dict[int, int]):
        self.clock = dict(vc)

    # handle_command({drop_ping, DropPing}), :165-166
    def set_drop_ping(self, on: bool):
        self.drop_ping = bool(on)

    # handle_command({txn, Txn}), :159-161
    def handle(self, txn: Txn, now: int) -> List[int]:
        dc, ts, _snap, ping, _tag = txn
        if not ping and ts == 0:
            raise ValueError("timestamp 0 on a transaction that is not a ping")
        self.queues.setdefault(dc, deque()).append(txn)      # push_txn/2, :188-196
        out: List[int] = []
        while True:                                          # process_all_queues/1, :96-103
            self.rounds += 1
            stored = 0
            for d in self.order:                             # lists:foldl over the DCs that have a queue
                q = self.queues.get(d)
                if q is None:
                    continue
                while q and self._try_store(q[0], now, out):  # process_queue/2, :107-117
                    q.popleft()                              # pop_txn/2
                    stored += 1
            if stored == 0:
                return out

    def _try_store(self, txn: Txn, now: int, out: List[int]) -> bool:
        dc, ts, snap, ping, tag = txn
        if ping:                                             # :122-125
            if not self.drop_ping:
                self.clock[dc] = ts                          # update_clock/3 -> set_clock_of_dc, :208
            return True
        deps = dict(snap)
        deps[dc] = 0                                         # :131
        cur = dict(self.clock)
        cur[self.own_dc] = now                               # get_partition_clock/1, :236-238
        cur[dc] = 0                                          # :132
        first = id(txn) not in self._tried                   # (queued tuples are alive, so their ids are distinct)
        if vc_le(deps, cur):                                 # vectorclock:ge(CurrentClock, Dependencies), :135
            self._tried.discard(id(txn))
            out.append(tag)                                  # :146-152
            self.clock[dc] = ts                              # :153
            return True
        if first:
            self.first_try_failed += 1
            self._tried.add(id(txn))
        self.clock[dc] = ts - 1                              # :141
        return False

    def queued(self, dc: int) -> List[int]:
        return [t[4] for t in self.queues.get(dc, ())]

    def presence(self) -> int:
        return sum(1 << d for d in self.clock)

    def clock_row(self) -> List[int]:
        return [self.clock.get(d, 0) for d in range(self.n_dc)]
