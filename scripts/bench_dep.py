"""Bench of the dependency buffer (am_dep_deliver) against scripts/dep_cpu.cpp, not on the driver line.

Points: n_part in {64, 1024} x n_dc in {3, 8} x batch in {16 Ki, 256 Ki, 1 Mi} arrivals, 5 % pings, two
histories:
  in_order  every dependency is met on arrival (a snapshot names timestamps already delivered)
  held      10 % of the transactions wait for a timestamp that a higher DC's queue of the same partition
            delivers 1-64 arrivals later; the other entries name timestamps of higher DCs that have arrived
Per point one JSON line: median ms per am_dep_deliver on device columns plus a stream synchronize,
arrivals/s, the share delivered, status readbacks per call (must be 1), dep_cpu's ms on the same
history and the ratio.  There is no bar.

  python scripts/bench_dep.py [--points small] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from antidote_amd import abi  # noqa: E402
from antidote_amd.materializer import Materializer  # noqa: E402


def history(kind, n_part, n_dc, n, seed):
    """Columns of n arrivals; own DC 0 is not an origin; a queue's timestamps are 1, 2, ..."""
    rng = random.Random(seed)
    part, dc, ts = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    snap, ping = np.zeros((n, n_dc), np.uint64), np.zeros(n, np.uint8)
    seq = [[0] * n_dc for _ in range(n_part)]
    pending = [[0] * n_dc for _ in range(n_part)]
    forced = {}
    for i in range(n):
        f = forced.pop(i, None)
        p, d = f if f else (rng.randrange(n_part), rng.randrange(1, n_dc))
        if f:
            pending[p][d] -= 1
        seq[p][d] += 1
        part[i], dc[i], ts[i] = p, d, seq[p][d]
        if not f and rng.random() < 0.05:
            ping[i] = 1
            continue
        row = seq[p]
        for k in range(1, n_dc):
            if k != d and (kind == "in_order" or k > d):  # held: waits point at higher DCs only, so none is circular
                snap[i, k] = row[k] if kind == "in_order" else rng.randint(0, row[k])
        if kind == "held" and not f and d + 1 < n_dc and rng.random() < 0.10:
            k, at = rng.randrange(d + 1, n_dc), i + rng.randint(1, 64)
            while at in forced:
                at += 1
            if at < n:
                pending[p][k] += 1
                snap[i, k] = seq[p][k] + pending[p][k]
                forced[at] = (p, k)
    return part, dc, ts, snap, ping


def cpu_ms(exe, n_part, n_dc, cols):
    part, dc, ts, snap, ping = cols
    n = len(part)
    body = np.concatenate([part[:, None].astype(np.uint64), dc[:, None].astype(np.uint64), ts[:, None], ping[:, None].astype(np.uint64),
                           np.arange(n, dtype=np.uint64)[:, None], snap], axis=1)
    with tempfile.TemporaryFile("w+") as f:
        f.write("C %d 0 %d %s\nD 1000000000 %d\n" % (n_dc, n_part, " ".join(map(str, range(n_dc))), n))
        np.savetxt(f, body, fmt="%d")
        f.seek(0)
        out = subprocess.run([exe, "--quiet"], stdin=f, capture_output=True, text=True, check=True).stdout
    return float(out.split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="all", choices=["all", "small"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "dep_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "dep_cpu.cpp"), "-o", exe], check=True)
    mat = Materializer(0)
    L = mat.L
    batches = [16 << 10] if a.points == "small" else [16 << 10, 256 << 10, 1 << 20]
    for n_part in (64, 1024):
        for n_dc in (3, 8):
            for n in batches:
                for kind in ("in_order", "held"):
                    cols = history(kind, n_part, n_dc, n, 11)
                    part, dc, ts, snap, ping = cols
                    tag = np.arange(n, dtype=np.uint64)
                    dev = [mat.device_array(x) for x in (part, dc, ts, snap, ping, tag)]
                    off, out = mat.device_array(np.zeros(n_part + 1, np.uint64)), mat.device_array(np.zeros(n, np.uint64))
                    s = abi.am_dep_txns()
                    s.n_tx = n
                    s.part, s.dc, s.timestamp, s.snap_vc, s.ping, s.tag = [d.ptr for d in dev]
                    times, share, rb = [], 0.0, 0
                    b = mat.dep_buffer(n_dc, 0, n_part, n)
                    for rep in range(a.reps + 1):  # the first call is the warm-up: it grows the buffer's scratch
                        b.clear()
                        r0 = b.readbacks()
                        nd, bad = ctypes.c_uint64(), ctypes.c_uint32()
                        mat.sync()
                        t0 = time.perf_counter()
                        abi.check(L.am_dep_deliver(b.handle, ctypes.byref(s), 10 ** 9, n, off.ptr, out.ptr, ctypes.byref(nd),
                                                   ctypes.byref(bad)), "am_dep_deliver")
                        mat.sync()
                        times.append((time.perf_counter() - t0) * 1e3)
                        share, rb = nd.value / max(1, n - int(ping.sum())), b.readbacks() - r0
                    b.close()
                    for d in dev + [off, out]:
                        d.free()
                    ms = statistics.median(times[1:])
                    c = cpu_ms(exe, n_part, n_dc, cols)
                    print(json.dumps({"bench": "dep", "history": kind, "n_part": n_part, "n_dc": n_dc, "batch": n,
                                      "ms": round(ms, 3), "arrivals_per_s": round(n / ms * 1e3), "delivered_share": round(share, 4),
                                      "readbacks_per_call": rb, "cpu_ms": round(c, 3), "cpu_over_gpu": round(c / ms, 3)}), flush=True)
    mat.close()


if __name__ == "__main__":
    main()
