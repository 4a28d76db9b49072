"""TEST INFRASTRUCTURE ONLY.  Cases for the subscriber buffer (tests/subsim.py is the contract): the hand
cases with their literal outputs, worked from src/inter_dc_sub_buf.erl by hand, a model of one SubSim
behind the device's interface, the random-history generators, and the text form scripts/sub_cpu.cpp
reads and prints.

A row is (kind, part, dc, prev_opid, last_opid, timestamp, snapshot, ping, tag).  A script is a list of
commands:
  ("process", [row, ...])
  ("set_last", part, dc, opid)
  ("set_reachable", [dc, ...])
  ("clear",)
"""
from __future__ import annotations

import random
from typing import Dict, List, Sequence

from tests.subsim import BUFFERING, NORMAL, RESP_END, RESP_TXN, TXN, SubSim

U64_MAX = 2 ** 64 - 1
H63 = 2 ** 63
N, B = NORMAL, BUFFERING
COUNTS = ("delivered", "gaps", "dropped", "unexpected", "queued")


def t(prev, last, tag, dc=1, ts=5, ping=False, part=0, snap=None, kind=TXN):
    return (kind, part, dc, prev, last, ts, dict(snap or {}), ping, tag)


def rt(prev, last, tag, dc=1, ts=5, part=0, snap=None):
    return t(prev, last, tag, dc, ts, False, part, snap, RESP_TXN)


def end(dc=1, part=0):
    return (RESP_END, part, dc, 0, 0, 0, {}, False, 0)


def ping(prev, tag, dc=1, part=0, garbage=0, ts=0):
    return (TXN, part, dc, prev, garbage, ts, {}, True, tag)


class Model:
    """One SubSim behind the device's interface: a batch is served one row at a time; an invalid batch
    changes nothing."""

    def __init__(self, n_dc: int, n_part: int, logging_enabled: bool = True):
        self.n_dc, self.n_part = n_dc, n_part
        self.sim = SubSim(n_dc, n_part, logging_enabled)
        self.rows = self.total_gaps = 0

    def process_rows(self, rows):
        """-> (per partition the delivered rows, the gaps, the counters)"""
        for r in rows:
            if r[0] not in (TXN, RESP_TXN, RESP_END) or r[1] >= self.n_part or r[2] >= self.n_dc or \
                    (r[0] != RESP_END and r[5] == 0 and not r[7]):
                raise ValueError("invalid batch")
        s = self.sim
        d0, u0 = s.dropped, s.unexpected
        out: List[list] = [[] for _ in range(self.n_part)]
        gaps = []
        for r in rows:
            got, gap = s.handle(r)
            for g in got:
                out[g[1]].append(g)
            if gap is not None:
                gaps.append(gap)
        self.rows += len(rows)
        self.total_gaps += len(gaps)
        cnt = dict(zip(COUNTS, (sum(len(o) for o in out), len(gaps), s.dropped - d0, s.unexpected - u0, s.queued())))
        return out, gaps, cnt

    def process(self, rows):
        out, gaps, cnt = self.process_rows(rows)
        return [[r[8] for r in o] for o in out], gaps, cnt

    def deliver_into(self, dep, rows, now: int):
        """dep: a depcases.Model.  What came out in order goes to the DepSims one at a time."""
        out, gaps, cnt = self.process_rows(rows)
        got = dep.deliver([(r[1], r[2], r[5], r[6], r[7], r[8]) for o in out for r in o], now)
        return got, gaps, cnt

    def set_last(self, part, dc, opid):
        self.sim.set_last(part, dc, opid)

    def set_reachable(self, dcs):
        self.sim.set_reachable(dcs)

    def clear(self):
        self.sim.clear()

    def stream(self, part, dc):
        return self.sim.stream(part, dc)

    def size(self):
        return (self.sim.queued(),)

    def state(self):
        return state_of(self, self.n_dc, self.n_part)


def state_of(target, n_dc: int, n_part: int):
    """{(part, dc): (last, mode, queued tags)} of the streams that are not new"""
    out = {}
    for p in range(n_part):
        for d in range(n_dc):
            s = tuple(target.stream(p, d))
            if s != (0, NORMAL, []):
                out[(p, d)] = s
    return out


def serve(target, script) -> list:
    """Runs a script through a Model or a materializer.SubBuffer: the outputs of every process."""
    out = []
    for cmd in script:
        if cmd[0] == "process":
            out.append(target.process(cmd[1]))
        elif cmd[0] == "set_last":
            target.set_last(cmd[1], cmd[2], cmd[3])
        elif cmd[0] == "set_reachable":
            target.set_reachable(cmd[1])
        elif cmd[0] == "clear":
            target.clear()
        else:
            raise ValueError(cmd[0])
    return out


def hand_cases():
    """[(name, n_dc, logging_enabled, steps, dropped, unexpected)].  A step is a control command of a
    script, or ("row", row, delivered tags, gap or None, (dc, last, mode, queued tags) afterwards).
    Everything runs on partition 0.  The literals are the reading of src/inter_dc_sub_buf.erl:57-142."""
    M = U64_MAX
    R = lambda row, tags, gap, st: ("row", row, tags, gap, st)  # noqa: E731
    return [
        ("in-order", 2, True, [
            R(t(0, 3, 1), [1], None, (1, 3, N, [])),
            R(t(3, 4, 2), [2], None, (1, 4, N, [])),
            R(t(4, 9, 3), [3], None, (1, 9, N, []))], 0, 0),
        ("duplicate", 2, True, [
            R(t(0, 3, 1), [1], None, (1, 3, N, [])),
            R(t(0, 3, 2), [], None, (1, 3, N, [])),
            R(t(3, 5, 3), [3], None, (1, 5, N, []))], 1, 0),
        # a hole emits (last + 1, prev) and buffers; rows that arrive while buffering wait, a duplicate
        # among them too; the full response is delivered uncompared, last := the head's prev
        ("hole-buffer-full-response", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 7, 2), [], (0, 1, 3, 5), (1, 2, B, [2])),
            R(t(7, 8, 3), [], None, (1, 2, B, [2, 3])),
            R(t(0, 2, 4), [], None, (1, 2, B, [2, 3, 4])),
            R(rt(2, 4, 10), [10], None, (1, 2, B, [2, 3, 4])),
            R(rt(4, 5, 11), [11], None, (1, 2, B, [2, 3, 4])),
            R(end(), [2, 3], None, (1, 8, N, []))], 1, 0),
        # ops 5 .. 9 are skipped silently
        ("short-response", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(9, 10, 2), [], (0, 1, 3, 9), (1, 2, B, [2])),
            R(rt(2, 4, 10), [10], None, (1, 2, B, [2])),
            R(end(), [2], None, (1, 10, N, []))], 0, 0),
        ("empty-response", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(9, 10, 2), [], (0, 1, 3, 9), (1, 2, B, [2])),
            R(end(), [2], None, (1, 10, N, []))], 0, 0),
        # response transactions are neither compared nor de-duplicated: the same one twice, and one
        # that is older than last
        ("response-not-compared", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 6, 2), [], (0, 1, 3, 5), (1, 2, B, [2])),
            R(rt(2, 5, 10), [10], None, (1, 2, B, [2])),
            R(rt(2, 5, 10), [10], None, (1, 2, B, [2])),
            R(rt(0, 1, 11), [11], None, (1, 2, B, [2])),
            R(end(), [2], None, (1, 6, N, []))], 0, 0),
        ("response-in-normal-mode", 2, True, [
            R(rt(0, 2, 10), [], None, (1, 0, N, [])),
            R(end(), [], None, (1, 0, N, [])),
            R(t(0, 2, 1), [1], None, (1, 2, N, []))], 0, 2),
        # a ping that equals last is delivered and leaves last at its prev: its last_opid column (999)
        # is ignored, or the next row would be a hole
        ("ping-equals-last", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(ping(2, 2, garbage=999), [2], None, (1, 2, N, [])),
            R(t(2, 3, 3), [3], None, (1, 3, N, []))], 0, 0),
        ("ping-reveals-hole", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(ping(6, 2, garbage=1), [], (0, 1, 3, 6), (1, 2, B, [2])),
            R(rt(2, 6, 10), [10], None, (1, 2, B, [2])),
            R(end(), [2], None, (1, 6, N, [])),
            R(t(6, 7, 3), [3], None, (1, 7, N, []))], 0, 0),
        ("second-hole-in-released-run", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 6, 2), [], (0, 1, 3, 5), (1, 2, B, [2])),
            R(t(6, 7, 3), [], None, (1, 2, B, [2, 3])),
            R(t(9, 10, 4), [], None, (1, 2, B, [2, 3, 4])),
            R(end(), [2, 3], (0, 1, 8, 9), (1, 7, B, [4])),
            R(end(), [4], None, (1, 10, N, []))], 0, 0),
        ("duplicate-in-released-run", 2, True, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 6, 2), [], (0, 1, 3, 5), (1, 2, B, [2])),
            R(t(5, 6, 3), [], None, (1, 2, B, [2, 3])),
            R(t(6, 8, 4), [], None, (1, 2, B, [2, 3, 4])),
            R(end(), [2, 4], None, (1, 8, N, []))], 1, 0),
        # DC 1 unreachable: the stream stays normal with its head kept, looks at it again on every
        # arrival, a response end is unexpected; reachable again, the next arrival emits the gap
        ("unreachable-dc", 2, True, [
            ("set_reachable", [0]),
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 6, 2), [], None, (1, 2, N, [2])),
            R(t(6, 7, 3), [], None, (1, 2, N, [2, 3])),
            R(end(), [], None, (1, 2, N, [2, 3])),
            ("set_reachable", [0, 1]),
            R(t(7, 8, 4), [], (0, 1, 3, 5), (1, 2, B, [2, 3, 4])),
            R(rt(2, 5, 10), [10], None, (1, 2, B, [2, 3, 4])),
            R(end(), [2, 3, 4], None, (1, 8, N, []))], 0, 1),
        ("logging-disabled", 2, False, [
            R(t(0, 2, 1), [1], None, (1, 2, N, [])),
            R(t(5, 6, 2), [2], None, (1, 6, N, [])),
            R(t(1, 3, 3), [], None, (1, 6, N, []))], 1, 0),
        ("set-last-after-restart", 2, True, [
            ("set_last", 0, 1, 100),
            R(t(100, 101, 1), [1], None, (1, 101, N, [])),
            R(t(50, 60, 2), [], None, (1, 101, N, [])),
            R(t(105, 106, 3), [], (0, 1, 102, 105), (1, 101, B, [3]))], 1, 0),
        ("op-ids-at-the-edges", 2, True, [
            R(t(0, H63, 1), [1], None, (1, H63, N, [])),
            R(t(H63, M, 2), [2], None, (1, M, N, [])),
            R(t(M - 1, M, 3), [], None, (1, M, N, [])),
            R(ping(M, 4, garbage=7), [4], None, (1, M, N, [])),
            ("set_last", 0, 0, H63),
            R(t(M, M, 5, dc=0), [], (0, 0, H63 + 1, M), (0, H63, B, [5])),
            R(rt(H63, M, 12, dc=0), [12], None, (0, H63, B, [5])),
            R(end(dc=0), [5], None, (0, M, N, []))], 1, 0),
    ]


def hand_script(steps):
    return [("process", [s[1]]) if s[0] == "row" else s for s in steps]


def hand_rows(steps):
    return [s[1] for s in steps if s[0] == "row"]


def random_rows(rng: random.Random, n_dc: int, n_part: int, length: int, tag0: int = 1):
    """Rows with no story behind them: small op ids so that equal, smaller and greater all occur, every
    kind, pings with garbage in last_opid."""
    out = []
    for i in range(length):
        p, d = rng.randrange(n_part), rng.randrange(n_dc)
        x = rng.random()
        if x < 0.15:
            out.append(end(d, p))
            continue
        prev = rng.randrange(6)
        if rng.random() < 0.15:
            out.append((TXN if x >= 0.3 else RESP_TXN, p, d, prev, rng.randrange(9), rng.randrange(3), {}, True, tag0 + i))
        else:
            out.append((TXN if x >= 0.3 else RESP_TXN, p, d, prev, prev + rng.randrange(3), 1 + rng.randrange(9),
                        {rng.randrange(n_dc): rng.randrange(5)}, False, tag0 + i))
    return out


def lossy_history(rng: random.Random, n_dc: int, n_part: int, length: int, p_loss=0.05, p_dup=0.05, p_ping=0.10,
                  logging_enabled=True, tag0: int = 1):
    """About `length` rows generated against a live SubSim, so that responses answer real gaps.  Every
    stream has a sender whose transactions take 1..3 op ids each; a message is lost with p_loss, sent
    twice (the copy at once, or an older message of the stream again) with p_dup, a ping with p_ping.  A
    gap the sim emits is answered 1..20 rows later by the sender's transactions with from <= last_opid <=
    to, then RESP_END; what is still owed at the end is answered there.
    -> (rows, the sim after them, messages sent)"""
    sim = SubSim(n_dc, n_part, logging_enabled)
    sent_last = {k: 0 for k in sim.streams}
    log: Dict[tuple, list] = {k: [] for k in sim.streams}
    due: Dict[int, list] = {}
    rows: List[tuple] = []
    sent = 0
    tag = tag0

    def emit(r):
        rows.append(r)
        _, gap = sim.handle(r)
        if gap is not None:
            due.setdefault(len(rows) + rng.randint(1, 20), []).append(gap)

    def answer(gap):
        p, d, lo, hi = gap
        for (kind, _, _, prev, last, ts, snap, pg, tg) in log[(p, d)]:
            if lo <= last <= hi:
                emit((RESP_TXN, p, d, prev, last, ts, snap, False, tg))
        emit(end(d, p))

    while len(rows) < length:
        for k in sorted(k for k in due if k <= len(rows)):
            for gap in due.pop(k):
                answer(gap)
        p, d = rng.randrange(n_part), rng.randrange(n_dc)
        prev = sent_last[(p, d)]
        ts = 1 + len(log[(p, d)])
        if rng.random() < p_ping:
            msg = (TXN, p, d, prev, rng.randrange(U64_MAX), ts, {}, True, tag)
        else:
            last = prev + rng.randint(1, 3)
            snap = {k: rng.randint(0, 3) for k in range(n_dc) if k != d and rng.random() < 0.3}
            msg = (TXN, p, d, prev, last, ts, snap, False, tag)
            sent_last[(p, d)] = last
            log[(p, d)].append(msg)
        tag += 1
        sent += 1
        if rng.random() < p_loss:
            continue
        emit(msg)
        if rng.random() < p_dup:
            old = log[(p, d)]
            emit(rng.choice(old) if old and rng.random() < 0.5 else msg)
    for k in sorted(due):
        for gap in due.pop(k):
            answer(gap)
    while due:  # a response may release a run with a second hole
        for k in sorted(due):
            for gap in due.pop(k):
                answer(gap)
    return rows, sim, sent


def split_calls(rows, sizes: Sequence[int]):
    """The rows as process commands of the given batch sizes (cycled)."""
    script, i, c = [], 0, 0
    while i < len(rows) or c < len(sizes):
        n = sizes[c % len(sizes)]
        script.append(("process", rows[i:i + n]))
        i += n
        c += 1
    return script


def tile_history(n: int, dup_at=None, hole_at=None):
    """n transactions buffered behind one hole on stream (0, 1), tags 100 .., then the empty response
    that releases them.  Entry dup_at repeats the one before it (entry 0: an op id below the hole);
    entry hole_at skips an op id."""
    rows = [t(0, 1, 1), t(5, 6, 2)]
    last = 6
    for i in range(n):
        if i == dup_at:
            rows.append(t(last - 1 if i else 3, last if i else 4, 100 + i))
            continue
        prev = last + (1 if i == hole_at else 0)
        rows.append(t(prev, prev + 1, 100 + i))
        last = prev + 1
    return rows, end()


# ---- the text form of scripts/sub_cpu.cpp ----
def history_text(script, n_dc: int, n_part: int, logging_enabled=True, dump=True) -> str:
    lines = ["C %d %d %d" % (n_dc, n_part, 1 if logging_enabled else 0)]
    for cmd in script:
        if cmd[0] == "process":
            toks = ["P", str(len(cmd[1]))]
            for kind, part, dc, prev, last, ts, snap, pg, tag in cmd[1]:
                toks += [str(kind), str(part), str(dc), str(prev), str(last), str(ts), "1" if pg else "0", str(tag)]
                toks += [str(snap.get(d, 0)) for d in range(n_dc)]
            lines.append(" ".join(toks))
        elif cmd[0] == "set_last":
            lines.append("L %d %d %d" % (cmd[1], cmd[2], cmd[3]))
        elif cmd[0] == "set_reachable":
            lines.append("R %d" % sum(1 << d for d in set(cmd[1])))
        elif cmd[0] == "clear":
            lines.append("Z")
    if dump:
        lines.append("X")
    return "\n".join(lines) + "\n"


def parse_cpu_output(text: str, n_part: int):
    """-> [per history (outputs of every P as process() returns them, the streams' state)]; a history
    ends at its X line."""
    hist, outs, state = [], [], {}
    dels = gaps = None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "D":
            dels = [[] for _ in range(n_part)]
            for i in range(int(w[1])):
                dels[int(w[2 + 2 * i])].append(int(w[3 + 2 * i]))
        elif w[0] == "G":
            gaps = [tuple(int(x) for x in w[2 + 4 * i:6 + 4 * i]) for i in range(int(w[1]))]
        elif w[0] == "N":
            outs.append((dels, gaps, dict(zip(COUNTS, (int(x) for x in w[1:6])))))
        elif w[0] == "E":
            outs.append(("invalid", int(w[1])))
        elif w[0] == "S":
            state[(int(w[1]), int(w[2]))] = (int(w[3]), int(w[4]), [int(x) for x in w[6:6 + int(w[5])]])
        elif w[0] == "X":
            hist.append((outs, state))
            outs, state = [], {}
    return hist


def expected(script, n_dc: int, n_part: int, logging_enabled=True):
    m = Model(n_dc, n_part, logging_enabled)
    return serve(m, script), m.state()
