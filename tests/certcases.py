"""Certification histories shared by the CPU twin's test and the device tests: the hand cases of
tests/test_certsim_cpu.py as scripts, a random history generator, a runner over anything shaped like
CertSim, and the text form scripts/cert_cpu.cpp reads.  A script is a list of steps
    ("prepare", txs) | ("finish", txs) | ("read", reads, now) | ("min",) | ("info", key)
and its outcome the list of what each step returns; CertSim's outcome is the expected one."""
import json
import os

from tests.certsim import CertSim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "suite_certification.json")
U64_MAX = 2 ** 64 - 1


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def golden_script(case):
    """A golden case's steps as a script (its expectations are checked by certsim.replay)."""
    out = []
    for st in case["steps"]:
        if st["op"] == "prepare":
            out.append(("prepare", [(t["txid"], t["start"], t["prepare"], t.get("certify", True), t["keys"]) for t in st["tx"]]))
        elif st["op"] == "finish":
            out.append(("finish", [(t["txid"], t.get("commit_time", 0), t["committed"], t["keys"]) for t in st["tx"]]))
        else:
            out.append(("read", [tuple(r) for r in st["reads"]], st["now"]))
    keys = sorted({k for s in out if s[0] != "read" for t in s[1] for k in t[-1]})
    return out + [("info", k) for k in keys] + [("min",)]


def hand_cases():
    """(name, record_commits, script): tests/test_certsim_cpu.py's cases, an accessor step at each of
    its assertion points."""
    return [
        ("last_commit_wins", True, [
            ("prepare", [(1, 10, 50, False, [4]), (2, 10, 51, False, [4])]), ("info", 4), ("min",),
            ("finish", [(1, 90, True, [4]), (2, 70, True, [4])]), ("info", 4), ("min",),
            ("prepare", [(3, 80, 100, True, [4])]), ("info", 4), ("min",),
            ("prepare", [(4, 60, 101, True, [5, 4])]), ("info", 4), ("info", 5), ("min",)]),
        ("abort_holding_nothing", True, [
            ("finish", [(9, 0, False, [1, 2])]), ("info", 1), ("info", 2), ("min",)]),
        ("abort_leaves_another_owner", True, [
            ("prepare", [(1, 10, 20, True, [7, 8]), (2, 11, 21, True, [8, 9])]), ("info", 7), ("info", 8), ("info", 9), ("min",),
            ("finish", [(2, 0, False, [8, 9])]), ("info", 8), ("info", 9), ("min",),
            ("finish", [(1, 30, True, [7, 8])]), ("info", 7), ("info", 8), ("min",)]),
        ("empty_write_sets", True, [
            ("prepare", [(1, 10, 20, True, []), (2, 10, 21, False, [])]), ("min",),
            ("finish", [(1, 30, True, []), (2, 0, False, [])]), ("min",), ("info", 0)]),
        ("record_commits_off", False, [
            ("prepare", [(1, 10, 20, True, [3])]), ("info", 3), ("min",),
            ("finish", [(1, 99, True, [3])]), ("info", 3), ("min",),
            ("prepare", [(2, 5, 30, True, [3])]), ("info", 3), ("min",)]),
        ("repeated_key", True, [
            ("prepare", [(1, 10, 20, False, [3, 3, 4, 3]), (2, 10, 25, False, [3])]), ("info", 3), ("info", 4), ("min",),
            ("read", [(3, 19), (3, 20), (3, 24), (4, 30), (5, 30), (3, 2001)], 1000)]),
    ]


def run_step(c, step):
    """One step against c (a CertSim or anything with its methods)."""
    op = step[0]
    if op == "prepare":
        return c.prepare(step[1])
    if op == "finish":
        return c.finish(step[1])
    if op == "read":
        return c.read_ready(step[1], step[2])
    if op == "min":
        return c.min_prepared()
    ct, es = c.key_info(step[1])
    return (ct, [tuple(e) for e in es])


def run(script, c):
    return [run_step(c, s) for s in script]


def expected(script, record_commits=True):
    return run(script, CertSim(record_commits))


def random_history(rng, steps, n_keys=64, max_tx=128, max_keys=5, certify=0.8, info_every=10, record_commits=True,
                   key_base=0):
    """A script of `steps` random steps over keys key_base..key_base+n_keys-1, generated beside a CertSim so that
    finishes can name transactions in flight: prepares of 1..max_tx transactions with 0..max_keys keys
    (keys may repeat inside a write set; a twentieth of the transactions reuse a TxId in flight or one
    of the same batch), finishes of in-flight and of never-prepared TxIds, read_ready batches; every
    info_every steps (0: never) the key_info of every key and min_prepared."""
    sim = CertSim(record_commits)
    script, inflight, next_txid, now = [], {}, 1, 1000
    for i in range(steps):
        now += rng.randint(1, 40)
        r = rng.random()
        if r < 0.45 or not inflight:
            txs = []
            for _ in range(rng.randint(1, max_tx)):
                keys = [key_base + rng.randrange(n_keys) for _ in range(rng.randint(0, max_keys))]
                if rng.random() < 0.05 and (inflight or txs):
                    txid = rng.choice(list(inflight) + [t[0] for t in txs])
                else:
                    txid, next_txid = next_txid, next_txid + 1
                txs.append((txid, now - rng.randint(0, 60), now + len(txs), rng.random() < certify, keys))
            st = sim.prepare(txs)
            for t, s in zip(txs, st):
                if s == 0:
                    inflight.setdefault(t[0], set()).update(t[4])
            script.append(("prepare", txs))
        elif r < 0.85:
            txs = []
            for _ in range(rng.randint(1, max_tx)):
                q = rng.random()
                if q < 0.8 and inflight:
                    txid = rng.choice(list(inflight))
                    keys = sorted(inflight.pop(txid))
                    if rng.random() < 0.1:
                        keys = keys + keys[:1]  # a repeated pair: one entry to remove, two removers
                elif q < 0.9:
                    txid, next_txid = next_txid, next_txid + 1  # never prepared
                    keys = [key_base + rng.randrange(n_keys) for _ in range(rng.randint(0, max_keys))]
                else:
                    txid, keys = next_txid, []
                    next_txid += 1
                txs.append((txid, now + rng.randint(0, 30), rng.random() < 0.7, keys))
            sim.finish(txs)
            script.append(("finish", txs))
        else:
            reads = [(key_base + rng.randrange(n_keys + 2), now + rng.randint(-80, 20) + (5000 if rng.random() < 0.05 else 0))
                     for _ in range(rng.randint(1, max_tx))]
            script.append(("read", reads, now))
        if info_every and (i + 1) % info_every == 0:
            script += [("info", key_base + k) for k in range(n_keys)] + [("min",)]
    return script


def history_text(script, record_commits=True):
    """The script as scripts/cert_cpu.cpp reads it."""
    out = ["C %d" % (1 if record_commits else 0)]
    for s in script:
        if s[0] == "prepare":
            out.append("P %d" % len(s[1]))
            out += ["%d %d %d %d %d %s" % (x, st, pt, 1 if c else 0, len(ks), " ".join(map(str, ks))) for x, st, pt, c, ks in s[1]]
        elif s[0] == "finish":
            out.append("F %d" % len(s[1]))
            out += ["%d %d %d %d %s" % (x, ct, 1 if c else 0, len(ks), " ".join(map(str, ks))) for x, ct, c, ks in s[1]]
        elif s[0] == "read":
            out.append("R %d %d %s" % (len(s[1]), s[2], " ".join("%d %d" % (k, t) for k, t in s[1])))
        elif s[0] == "min":
            out.append("M")
        else:
            out.append("I %d" % s[1])
    return "\n".join(out) + "\n"


def parse_cpu_output(text):
    """cert_cpu's lines back as run()'s outcome (the closing T line dropped)."""
    out = []
    for line in text.splitlines():
        tok = line.split()
        if tok[0] in "PFR":
            out.append([int(x) for x in tok[1:]])
        elif tok[0] == "M":
            out.append(None if tok[1] == "none" else int(tok[1]))
        elif tok[0] == "I":
            n = int(tok[2])
            out.append((int(tok[1]), [(int(tok[3 + 2 * i]), int(tok[4 + 2 * i])) for i in range(n)]))
    return out
