"""Bench of the subscriber buffer (am_sub_process) against scripts/sub_cpu.cpp, not on the driver line.

Points: n_part in {64, 1024} x n_dc in {3, 8} x batch in {16 Ki, 256 Ki, 1 Mi} rows, 10 % pings, three
histories:
  in_order  every message follows on the one before it
  lossy     1 % of the transactions are lost; the hole shows at the stream's next message (or, while the
            stream is buffering, when its queue is released) and is answered 1-64 rows later by the lost
            transactions and a RESP_END
  dups      5 % of the messages arrive twice
Per point one JSON line: median ms per am_sub_process on device columns plus a stream synchronize,
rows/s, the counters, status readbacks per call (must be 1), sub_cpu's ms on the same columns and the
ratio.  Then, per shape and batch on the lossy history, am_sub_deliver (chained: the delivered columns
stay in HBM) against am_sub_process_host followed by am_dep_deliver_host (unchained: they cross the
host twice).  There is no bar.

  python scripts/bench_sub.py [--points small] [--reps 5]
"""
import argparse
import ctypes
import json
import os
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
from antidote_amd.oplog import SubRows  # noqa: E402

TXN, RESP_TXN, RESP_END = abi.AM_SUB_TXN, abi.AM_SUB_RESP_TXN, abi.AM_SUB_RESP_END


def history(kind, n_part, n_dc, n, seed):
    """-> SubRows of n rows.  A stream's transactions take one op id each; tags number the rows."""
    rng = np.random.default_rng(seed)
    ns = n_part * n_dc
    stream = rng.integers(0, ns, n)
    is_ping = rng.random(n) < 0.10
    order = np.argsort(stream, kind="stable")
    st_sorted = stream[order]
    first = np.r_[True, st_sorted[1:] != st_sorted[:-1]]
    start = np.flatnonzero(first)
    cs = np.cumsum(~is_ping[order]) - (~is_ping[order])            # transactions before each message, whole array
    base = np.repeat(cs[start], np.diff(np.r_[start, n]))
    prev = np.zeros(n, np.uint64)
    prev[order] = (cs - base).astype(np.uint64)                    # ... of its own stream
    last = prev + (~is_ping).astype(np.uint64)
    kindc = np.zeros(n, np.uint8)
    pos = np.arange(n, dtype=np.float64)                           # where a row goes: after base message pos
    keep = np.ones(n, bool)
    extra = []                                                     # (pos, kind, stream, prev, last)
    if kind == "dups":
        twice = np.flatnonzero(rng.random(n) < 0.05)
        extra = [(float(i), TXN, int(stream[i]), int(prev[i]), int(last[i]), bool(is_ping[i])) for i in twice]
    elif kind == "lossy":
        lost = (rng.random(n) < 0.01) & ~is_ping
        keep = ~lost
        lost_sorted = lost[order]
        bounds = np.r_[start, n]
        for si in np.flatnonzero(np.add.reduceat(lost_sorted.astype(np.int64), start) > 0):
            lo, hi = bounds[si], bounds[si + 1]
            g, ls = order[lo:hi], lost_sorted[lo:hi]
            idx = np.flatnonzero(ls)
            until, j = -1.0, 0
            while j < len(idx):
                a = b = idx[j]
                while j + 1 < len(idx) and idx[j + 1] == b + 1:
                    j, b = j + 1, b + 1
                j += 1
                if b + 1 >= len(g):
                    break                                          # lost at the tail: nothing reveals it
                until = max(float(g[b + 1]), until) + int(rng.integers(1, 65))
                s = int(stream[g[a]])
                for m in range(a, b + 1):
                    extra.append((until, RESP_TXN, s, int(prev[g[m]]), int(last[g[m]]), False))
                extra.append((until, RESP_END, s, 0, 0, False))
    if extra:
        e = np.array([(x[0], x[1], x[2], x[3], x[4], x[5]) for x in extra], dtype=np.float64)
        pos = np.r_[pos[keep], e[:, 0] + 0.5]
        kindc = np.r_[kindc[keep], e[:, 1].astype(np.uint8)]
        stream = np.r_[stream[keep], e[:, 2].astype(np.int64)]
        prev = np.r_[prev[keep], np.array([x[3] for x in extra], np.uint64)]
        last = np.r_[last[keep], np.array([x[4] for x in extra], np.uint64)]
        is_ping = np.r_[is_ping[keep], e[:, 5] != 0]
        o = np.argsort(pos, kind="stable")[:n]
        kindc, stream, prev, last, is_ping = kindc[o], stream[o], prev[o], last[o], is_ping[o]
    m = len(kindc)
    return SubRows.from_columns(n_dc, kindc, stream // n_dc, stream % n_dc, prev, last, np.ones(m, np.uint64),
                                np.zeros((m, n_dc), np.uint64), is_ping, np.arange(m, dtype=np.uint64))


def cpu_ms(exe, n_part, b):
    with tempfile.NamedTemporaryFile("wb", suffix=".cols") as f:
        np.asarray([b.n_dc, n_part, 1, b.n_rows], np.uint64).tofile(f)
        for col in (b.kind, b.part, b.dc, b.prev_opid, b.last_opid, b.timestamp, b.snap_vc, b.ping, b.tag):
            col[:b.n_rows].tofile(f)
        f.flush()
        out = subprocess.run([exe, "--quiet", "--columns", f.name], capture_output=True, text=True, check=True).stdout
    return float(out.split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="all", choices=["all", "small"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "sub_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "sub_cpu.cpp"), "-o", exe], check=True)
    mat = Materializer(0)
    L = mat.L
    batches = [16 << 10] if a.points == "small" else [16 << 10, 256 << 10, 1 << 20]
    for n_part in (64, 1024):
        for n_dc in (3, 8):
            for n in batches:
                for kind in ("in_order", "lossy", "dups"):
                    b = history(kind, n_part, n_dc, n, 11)
                    n = b.n_rows
                    cols = (b.kind, b.part, b.dc, b.prev_opid, b.last_opid, b.timestamp, b.snap_vc, b.ping, b.tag)
                    dev = [mat.device_array(x) for x in cols]
                    s = abi.am_sub_rows()
                    s.n_rows = n
                    s.kind, s.part, s.dc, s.prev_opid, s.last_opid, s.timestamp, s.snap_vc, s.ping, s.tag = [d.ptr for d in dev]
                    outs = [mat.device_array(np.zeros(n, dt)) for dt in (np.uint32, np.uint8, np.uint64, np.uint8, np.uint64)]
                    osnap, off = mat.device_array(np.zeros((n, n_dc), np.uint64)), mat.device_array(np.zeros(n_part + 1, np.uint64))
                    o = abi.am_dep_txns()
                    o.part, o.dc, o.timestamp, o.ping, o.tag, o.snap_vc = [d.ptr for d in outs] + [osnap.ptr]
                    gd = [mat.device_array(np.zeros(n, dt)) for dt in (np.uint32, np.uint8, np.uint64, np.uint64)]
                    g = abi.am_sub_gaps()
                    g.part, g.dc, g.from_, g.to = [d.ptr for d in gd]
                    sub = mat.sub_buffer(n_dc, n_part, n)
                    cnt, times, rb = np.zeros(5, np.uint64), [], 0
                    for rep in range(a.reps + 1):  # the first call is the warm-up: it grows the buffer's scratch
                        sub.clear()
                        r0 = sub.stats()["readbacks"]
                        bad = ctypes.c_uint32()
                        mat.sync()
                        t0 = time.perf_counter()
                        abi.check(L.am_sub_process(sub.handle, ctypes.byref(s), n, off.ptr, ctypes.byref(o), n, ctypes.byref(g),
                                                   cnt.ctypes.data, ctypes.byref(bad)), "am_sub_process")
                        mat.sync()
                        times.append((time.perf_counter() - t0) * 1e3)
                        rb = sub.stats()["readbacks"] - r0
                    ms = statistics.median(times[1:])
                    c = cpu_ms(exe, n_part, b)
                    rec = {"bench": "sub", "history": kind, "n_part": n_part, "n_dc": n_dc, "batch": n, "ms": round(ms, 3),
                           "rows_per_s": round(n / ms * 1e3), "readbacks_per_call": rb, "cpu_ms": round(c, 3),
                           "cpu_over_gpu": round(c / ms, 3)}
                    rec.update(dict(zip(abi.SUB_COUNTS, (int(x) for x in cnt))))
                    print(json.dumps(rec), flush=True)
                    if kind == "lossy":
                        # chained against unchained, host columns in and the delivered tags out in both
                        dep = mat.dep_buffer(n_dc, 0, n_part, n)
                        hoff, htag = np.zeros(n_part + 1, np.uint64), np.zeros(n, np.uint64)
                        gh = [np.zeros(n, dt) for dt in (np.uint32, np.uint8, np.uint64, np.uint64)]
                        hg = abi.am_sub_gaps()
                        hg.part, hg.dc, hg.from_, hg.to = [x.ctypes.data for x in gh]
                        hs = b.as_struct()
                        hcols = [np.zeros(n, dt) for dt in (np.uint32, np.uint8, np.uint64, np.uint8, np.uint64)]
                        hsnap = np.zeros((n, n_dc), np.uint64)
                        ho = abi.am_dep_txns()
                        ho.part, ho.dc, ho.timestamp, ho.ping, ho.tag, ho.snap_vc = [x.ctypes.data for x in hcols] + [hsnap.ctypes.data]
                        res = {}
                        for mode in ("chained", "unchained"):
                            times, nd = [], ctypes.c_uint64()
                            for rep in range(a.reps + 1):
                                sub.clear(), dep.clear()
                                bad = ctypes.c_uint32()
                                mat.sync()
                                t0 = time.perf_counter()
                                if mode == "chained":
                                    abi.check(L.am_sub_deliver_host(sub.handle, dep.handle, ctypes.byref(hs), 10 ** 9, n, hoff.ctypes.data,
                                                                    htag.ctypes.data, ctypes.byref(nd), n, ctypes.byref(hg),
                                                                    cnt.ctypes.data, ctypes.byref(bad)), "am_sub_deliver_host")
                                else:
                                    abi.check(L.am_sub_process_host(sub.handle, ctypes.byref(hs), n, hoff.ctypes.data, ctypes.byref(ho), n,
                                                                    ctypes.byref(hg), cnt.ctypes.data, ctypes.byref(bad)),
                                              "am_sub_process_host")
                                    ho.n_tx = int(cnt[0])
                                    abi.check(L.am_dep_deliver_host(dep.handle, ctypes.byref(ho), 10 ** 9, n, hoff.ctypes.data,
                                                                    htag.ctypes.data, ctypes.byref(nd), ctypes.byref(bad)),
                                              "am_dep_deliver_host")
                                mat.sync()
                                times.append((time.perf_counter() - t0) * 1e3)
                            res[mode] = (statistics.median(times[1:]), int(nd.value))
                        dep.close()
                        assert res["chained"][1] == res["unchained"][1]
                        print(json.dumps({"bench": "sub_deliver", "history": kind, "n_part": n_part, "n_dc": n_dc, "batch": n,
                                          "chained_ms": round(res["chained"][0], 3), "unchained_ms": round(res["unchained"][0], 3),
                                          "unchained_over_chained": round(res["unchained"][0] / res["chained"][0], 3),
                                          "dep_delivered": res["chained"][1]}), flush=True)
                    sub.close()
                    for d in dev + outs + [osnap, off] + gd:
                        d.free()
    mat.close()


if __name__ == "__main__":
    main()
