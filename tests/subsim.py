"""TEST INFRASTRUCTURE ONLY.  A sequential restatement of the reference's subscriber buffer,
src/inter_dc_sub_buf.erl:57-162 behind src/inter_dc_sub_vnode.erl:84-94: one SubSim over n_part x n_dc
streams, one row at a time.  It is the contract of am_sub (antidote_amd/csrc/am_sub.hip) and of
scripts/sub_cpu.cpp: a batched call leaves the state, and returns the outputs, that serving the batch's
rows one at a time in batch order through this class gives.  Every comparison is exact.

A stream is #inter_dc_sub_buf{last_observed_opid, state_name, queue}: `last` (u64), `mode` (NORMAL |
BUFFERING) and a FIFO.  A row is (kind, part, dc, prev_opid, last_opid, timestamp, snapshot, ping, tag):
prev_opid = #interdc_txn.prev_log_opid#op_number.local, last_opid = inter_dc_txn:last_log_opid/1's local
(src/inter_dc_txn.erl:73-82), which for a ping (log_records == []) is prev_log_opid, so a ping's last_opid
column is ignored; timestamp, snapshot, ping and tag are carried untouched for the dependency buffer.
Kinds: TXN = {txn, Txn} (:77-80); RESP_TXN = one transaction of a {log_reader_resp, Txns} list, RESP_END
the list's end (:82-94) -- the response of a stream is the run RESP_TXN* RESP_END.

Decisions the reference leaves open:
  1. last_observed_opid = init (:58-76) asks the local log for the stream's last op id and retries while
     the log is down.  Here there is no init: a stream starts at 0, what get_op_id returns for an unknown
     stream (src/logging_vnode.erl:289-292, 995-1002), and set_last loads what request_op_id/3 returned
     after a restart; the retry loop is the caller's.
  2. query/3 returns ok | unknown_dc or throws (:117-129).  Here a set of reachable DCs (default: all)
     decides between the two branches, and only the gaps of reachable DCs are emitted: those are the
     requests the host must send.
  3. logging_enabled is read once, at construction (:48-54).
  4. last + 1 cannot wrap: a gap means prev_opid > last.
  5. A row the dependency buffer could never take -- timestamp 0 on a TXN or RESP_TXN row that is not a
     ping -- is refused at the door (ValueError; AM_SUB_BAD_TIME on the device, the batch invalid).  The
     reference's buffer does not look at timestamps; this keeps the chained call atomic.
  6. An empty batch changes nothing.

Quirks that follow from the text: after a response last becomes the queue head's prev_opid whatever the
response held (:84-88), so a short or empty response silently skips ops; response transactions are never
compared or de-duplicated (:83); a duplicate that arrives while buffering is dropped only when the queue
is released (:78-80, :138-140).
"""
from __future__ import annotations

from collections import deque
from typing import Dict, Iterable, List, Optional, Tuple

TXN, RESP_TXN, RESP_END = 0, 1, 2
NORMAL, BUFFERING = 0, 1

Row = Tuple[int, int, int, int, int, int, Dict[int, int], bool, int]


class Stream:
    def __init__(self):
        self.last, self.mode, self.queue = 0, NORMAL, deque()


class SubSim:
    def __init__(self, n_dc: int, n_part: int, logging_enabled: bool = True):
        self.n_dc, self.n_part, self.logging_enabled = n_dc, n_part, bool(logging_enabled)
        self.streams = {(p, d): Stream() for p in range(n_part) for d in range(n_dc)}
        self.reachable = set(range(n_dc))
        self.dropped = self.unexpected = self.delivered = 0
        self.released = 0            # deliveries triggered by RESP_END rows, for the tests

    def set_last(self, part: int, dc: int, opid: int):
        self.streams[(part, dc)].last = opid

    def set_reachable(self, dcs: Iterable[int]):
        self.reachable = set(dcs)

    def clear(self):
        for k in self.streams:
            self.streams[k] = Stream()

    def queued(self) -> int:
        return sum(len(s.queue) for s in self.streams.values())

    def handle(self, row: Row) -> Tuple[List[Row], Optional[Tuple[int, int, int, int]]]:
        """One row -> (the rows delivered, in order; the gap (part, dc, from, to) it triggered or None)."""
        kind, part, dc, _prev, _last, ts, _snap, ping, _tag = row
        if kind not in (TXN, RESP_TXN, RESP_END):
            raise ValueError("kind")
        if kind != RESP_END and ts == 0 and not ping:
            raise ValueError("timestamp 0 on a transaction that is not a ping")
        s = self.streams[(part, dc)]
        out: List[Row] = []
        gap = None
        if kind == TXN:                                   # :77-80
            s.queue.append(row)                           # push/2
            if s.mode == NORMAL:
                gap = self._process_queue(s, part, dc, out)
        elif kind == RESP_TXN:                            # lists:foreach(fun deliver/1, Txns), :83
            if s.mode == BUFFERING:
                out.append(row)
            else:
                self.unexpected += 1                      # "This case must not happen", :91-94
        else:
            if s.mode == BUFFERING:                       # :84-89
                if s.queue:
                    s.last = s.queue[0][3]
                gap = self._process_queue(s, part, dc, out)
                self.released += len(out)
            else:
                self.unexpected += 1
        self.delivered += len(out)
        return out, gap

    def _process_queue(self, s: Stream, part: int, dc: int, out: List[Row]):
        while True:                                       # :98-142
            if not s.queue:
                s.mode = NORMAL
                return None
            head = s.queue[0]
            prev = head[3]
            if prev == s.last or (prev > s.last and not self.logging_enabled):
                out.append(head)                          # deliver/1
                s.last = prev if head[7] else head[4]     # last_log_opid/1
                s.queue.popleft()
            elif prev < s.last:
                self.dropped += 1                         # "Dropping duplicate message"
                s.queue.popleft()
            elif dc in self.reachable:                    # query/3 = ok
                s.mode = BUFFERING
                return (part, dc, s.last + 1, prev)
            else:                                         # "will retry on next ping message"
                s.mode = NORMAL
                return None

    def stream(self, part: int, dc: int) -> Tuple[int, int, List[int]]:
        s = self.streams[(part, dc)]
        return s.last, s.mode, [r[8] for r in s.queue]
