"""TEST INFRASTRUCTURE ONLY.  Cases for the dependency buffer (tests/depsim.py is the contract): the hand
cases with their literal outputs, a random-history generator, a model of n_part DepSims that serves
scripts, and the text form scripts/dep_cpu.cpp reads and prints.

A script is a list of commands:
  ("deliver", [(part, dc, timestamp, snapshot, ping, tag), ...], now)
  ("set_clock", part, {dc: time})
  ("drop_ping", on)
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence

from tests.depsim import DepSim

U64_MAX = 2 ** 64 - 1
A, B = 1, 2


class Model:
    """n_part DepSims behind the device's interface: a batch is served one arrival at a time."""

    def __init__(self, n_dc: int, own_dc: int, n_part: int, order: Optional[Sequence[int]] = None):
        self.n_dc, self.own_dc, self.n_part = n_dc, own_dc, n_part
        self.sims = [DepSim(n_dc, own_dc, order) for _ in range(n_part)]
        self.nonping = self.delivered = 0

    def deliver(self, txs, now: int) -> List[List[int]]:
        out: List[List[int]] = [[] for _ in range(self.n_part)]
        for part, dc, ts, snap, ping, tag in txs:
            got = self.sims[part].handle((dc, ts, snap, bool(ping), tag), now)
            out[part] += got
            self.nonping += 0 if ping else 1
            self.delivered += len(got)
        return out

    def set_clock(self, part: int, vc: Dict[int, int]):
        self.sims[part].set_dependency_clock(vc)

    def set_drop_ping(self, on: bool):
        for s in self.sims:
            s.set_drop_ping(on)

    def clock(self, part: int) -> Dict[int, int]:
        return dict(self.sims[part].clock)

    def queue(self, part: int, dc: int) -> List[int]:
        return self.sims[part].queued(dc)

    def first_try_failed(self) -> int:
        return sum(s.first_try_failed for s in self.sims)

    def state(self):
        """(clocks [n_part], queues {(part, dc): tags} of the non-empty queues)"""
        return ([self.clock(p) for p in range(self.n_part)],
                {(p, d): self.queue(p, d) for p in range(self.n_part) for d in range(self.n_dc) if self.queue(p, d)})


def serve(target, script) -> list:
    """Runs a script through a Model or a materializer.DepBuffer: the deliveries of every deliver."""
    out = []
    for cmd in script:
        if cmd[0] == "deliver":
            out.append(target.deliver(cmd[1], cmd[2]))
        elif cmd[0] == "set_clock":
            target.set_clock(cmd[1], cmd[2])
        elif cmd[0] == "drop_ping":
            target.set_drop_ping(cmd[1])
        else:
            raise ValueError(cmd[0])
    return out


def state_of(target, n_dc: int, n_part: int):
    return ([target.clock(p) for p in range(n_part)],
            {(p, d): q for p in range(n_part) for d in range(n_dc) for q in [target.queue(p, d)] if q})


def txn(dc, ts, snap=None, tag=0, ping=False, part=0):
    return (part, dc, ts, dict(snap or {}), ping, tag)


def chain(links: int):
    """The ping-pong chain: a_i waits for b_(i-1), b_i for a_i, a_0 for DC 3.  (arrivals, the releasing
    ping, the delivery order)"""
    arr, want = [], []
    for i in range(links):
        arr.append(txn(1, 2 * i + 1, {2: 2 * i, 3: 1 if i == 0 else 0}, 1000 + i))
        arr.append(txn(2, 2 * i + 2, {1: 2 * i + 1}, 5000 + i))
        want += [1000 + i, 5000 + i]
    return arr, txn(3, 1, ping=True), want


def hand_cases():
    """[(name, n_dc, own_dc, order, [(arrival, now, delivered, clock after)])]: own DC 0; the literal
    outputs are the reading of src/inter_dc_dep_vnode.erl:94-154 that tests/depsim.py states."""
    rev = [3, 2, 1, 0]
    late = [txn(1, 5, {2: 9}, A), txn(2, 10, {3: 50}, B), txn(3, 7, ping=True)]
    mirr = [txn(2, 5, {1: 9}, A), txn(1, 10, {3: 50}, B)]
    arr, ping, want = chain(6)
    return [
        ("late-bump", 4, 0, None, [(late[0], 100, [], {1: 4}), (late[1], 100, [], {1: 4, 2: 9}),
                                   (late[2], 100, [A], {1: 5, 2: 9, 3: 7})]),
        ("late-bump-mirrored", 4, 0, None, [(mirr[0], 100, [], {2: 4}), (mirr[1], 100, [A], {2: 5, 1: 9})]),
        ("late-bump-reversed", 4, 0, rev, [(late[0], 100, [], {1: 4}), (late[1], 100, [A], {1: 5, 2: 9}),
                                           (late[2], 100, [], {1: 5, 2: 9, 3: 7})]),
        ("late-bump-mirrored-reversed", 4, 0, rev, [(mirr[0], 100, [], {2: 4}), (mirr[1], 100, [], {2: 4, 1: 9})]),
        ("chain", 4, 0, None, [(t, 100, [], {1: 0, 2: 1} if i else {1: 0}) for i, t in enumerate(arr)] +
         [(ping, 100, want, {1: 11, 2: 12, 3: 1})]),
        ("own-dc", 4, 0, None, [(txn(1, 5, {0: 101}, A), 100, [], {1: 4}), (txn(1, 6, ping=True), 101, [A], {1: 6})]),
    ]


def hand_script(steps):
    return [("deliver", [t], now) for t, now, _, _ in steps]


def random_history(rng: random.Random, n_dc: int, n_part: int, length: int, own_dc: int = 0, p_ping: float = 0.05,
                   p_held: float = 0.7, now: int = 10 ** 9, non_monotone: bool = False, tag0: int = 1, order=None, low_bias: bool = False,
                   ahead: Optional[int] = None):
    """length arrivals over n_part partitions, generated against a live DepSim per partition so that
    the generator knows each partition's clock.  Every DC is an origin (the own DC too), its
    timestamps go up by 1..2 per arrival.  A transaction of DC d is *held* with probability p_held when
    a higher DC k exists: its snapshot names a time 1..2 past DC k's newest timestamp and past every earlier
    wait on DC k, which DC k's queue reaches a few arrivals later.  Waiting only on higher DCs keeps the waits-for relation acyclic, so with the flush pings at
    the end every transaction can be delivered.  The other snapshot entries name times the clock has
    already reached.  ahead bounds how far past DC k's newest timestamp a wait may reach.  low_bias draws the lower DCs, the ones that can be held, more often.  non_monotone lets timestamps go down along a queue (nothing is promised about
    delivery then)."""
    sims = [DepSim(n_dc, own_dc, order) for _ in range(n_part)]
    latest = [[0] * n_dc for _ in range(n_part)]
    hold = [[0] * n_dc for _ in range(n_part)]   # the latest time any held transaction waits for, per DC
    out = []
    for i in range(length):
        p = rng.randrange(n_part)
        d = min(rng.randrange(n_dc), rng.randrange(n_dc)) if low_bias else rng.randrange(n_dc)
        sim = sims[p]
        latest[p][d] += rng.randint(1, 2)
        ts = latest[p][d]
        if non_monotone and rng.random() < 0.3:
            ts = max(1, ts - rng.randint(1, 5))
        if rng.random() < p_ping:
            t = (p, d, ts, {}, True, tag0 + i)
        else:
            snap = {}
            for k in range(n_dc):
                if k != d and k != own_dc and sim.clock.get(k, 0) and rng.random() < 0.5:
                    snap[k] = rng.randint(0, sim.clock[k])
            if d + 1 < n_dc and rng.random() < p_held:
                k = rng.randrange(d + 1, n_dc)
                if k != own_dc:
                    need = max(sim.clock.get(k, 0), latest[p][k], hold[p][k]) + rng.randint(1, 2)
                    if ahead is not None:
                        need = min(need, max(sim.clock.get(k, 0), latest[p][k]) + ahead)
                    hold[p][k] = snap[k] = need
            if rng.random() < 0.2:
                snap[d] = rng.randint(0, U64_MAX)  # the origin's entry is irrelevant, whatever it holds
            t = (p, d, ts, snap, False, tag0 + i)
        out.append(t)
        sim.handle(t[1:], now)
    return out


def flush_pings(n_dc: int, n_part: int, own_dc: int, ts: int, tag0: int):
    """Pings with a late timestamp for every (partition, DC), the highest DC first and the whole set
    twice: they release what the tail of a history still holds."""
    out = []
    for r in range(2):
        for p in range(n_part):
            for d in reversed(range(n_dc)):
                out.append((p, d, ts + r, {}, True, tag0 + len(out)))
    return out


def split_calls(arrivals, sizes: Sequence[int], now0: int, now_step: int = 1000):
    """The arrivals as deliver commands of the given batch sizes (cycled), now advancing."""
    script, i, c = [], 0, 0
    while i < len(arrivals) or c < len(sizes):
        n = sizes[c % len(sizes)]
        script.append(("deliver", arrivals[i:i + n], now0 + c * now_step))
        i += n
        c += 1
    return script


# ---- the text form of scripts/dep_cpu.cpp ----
def history_text(script, n_dc: int, own_dc: int, n_part: int, order=None, dump=True) -> str:
    o = list(order) if order is not None else list(range(n_dc))
    lines = ["C %d %d %d %s" % (n_dc, own_dc, n_part, " ".join(map(str, o)))]
    for cmd in script:
        if cmd[0] == "deliver":
            toks = ["D", str(cmd[2]), str(len(cmd[1]))]
            for part, dc, ts, snap, ping, tag in cmd[1]:
                toks += [str(part), str(dc), str(ts), "1" if ping else "0", str(tag)]
                toks += [str(snap.get(d, 0)) for d in range(n_dc)]
            lines.append(" ".join(toks))
        elif cmd[0] == "set_clock":
            pres = sum(1 << d for d in cmd[2])
            lines.append("S %d %d %s" % (cmd[1], pres, " ".join(str(cmd[2].get(d, 0)) for d in range(n_dc))))
        elif cmd[0] == "drop_ping":
            lines.append("P %d" % (1 if cmd[1] else 0))
    if dump:
        lines.append("X")
    return "\n".join(lines) + "\n"


def parse_cpu_output(text: str, n_dc: int, n_part: int):
    """-> [per history (deliveries of every D, clocks, queues)]; a history ends at its X line."""
    hist, dels, clocks, queues = [], [], [None] * n_part, {}
    for line in text.splitlines():
        t = line.split()
        if t[0] == "D":
            out = [[] for _ in range(n_part)]
            for i in range(int(t[1])):
                out[int(t[2 + 2 * i])].append(int(t[3 + 2 * i]))
            dels.append(out)
        elif t[0] == "K":
            pres = int(t[2])
            clocks[int(t[1])] = {d: int(t[3 + d]) for d in range(n_dc) if (pres >> d) & 1}
        elif t[0] == "Q":
            queues[(int(t[1]), int(t[2]))] = [int(x) for x in t[4:4 + int(t[3])]]
        elif t[0] == "X":
            hist.append((dels, clocks, queues))
            dels, clocks, queues = [], [None] * n_part, {}
    return hist


def expected(script, n_dc: int, own_dc: int, n_part: int, order=None):
    m = Model(n_dc, own_dc, n_part, order)
    dels = serve(m, script)
    clocks, queues = m.state()
    return dels, clocks, queues


def conditioned_history(n_dc: int, n_part: int, length: int, sizes: Sequence[int], seed0: int = 0, own_dc: int = 0):
    """A random history, cut into calls and ended by the flush pings, whose run through DepSim meets the
    conditions the device tests state on their inputs: at least a third of the non-ping transactions
    fail their first try_store and at least 90 % are delivered by the end.  The generator's parameters
    are searched on DepSim's run alone.  With one DC no transaction can fail (Dependencies is all
    zeros once the origin's entry is cleared), so there the first condition is that none fails.
    -> (script, the Model after it)"""
    for p_held, ahead in ((0.9, None), (0.9, 4), (0.9, 2), (0.7, None), (1.0, 3), (1.0, None), (0.5, None)):
        for low_bias in (False, True):
            for seed in range(seed0, seed0 + 4):
                rng = random.Random(seed * 7919 + n_dc * 131 + n_part)
                arr = random_history(rng, n_dc, n_part, length, own_dc, p_held=p_held, low_bias=low_bias, ahead=ahead)
                script = split_calls(arr + flush_pings(n_dc, n_part, own_dc, 10 ** 6, 10 ** 6), sizes, 10 ** 9)
                m = Model(n_dc, own_dc, n_part)
                serve(m, script)
                fails = m.first_try_failed() * 3 >= m.nonping if n_dc > 1 else m.first_try_failed() == 0
                if fails and m.delivered * 10 >= m.nonping * 9:
                    return script, m
    raise AssertionError("no generator parameters meet the conditions for n_dc=%d n_part=%d" % (n_dc, n_part))
