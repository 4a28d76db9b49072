"""Certification on the device against the single-threaded CPU restatement (am_cert vs cert_cpu).

Per point -- batches of --tx transactions (default 1 Ki, 16 Ki, 256 Ki) x 4 keys, every transaction
certifying, keys drawn over 16 Mi keys uniformly or Zipf s = 1.1 (C5's popularity; ranks scattered
over the key space by an odd multiplier) -- one certifier gets --warmup + --steps rounds of
  prepare   am_cert_prepare on device columns, then a stream synchronize
  finish    am_cert_finish of the same transactions, committed where the prepare answered AM_OK,
            aborted where it answered a conflict
(wall clock around the C calls; the columns are uploaded before, the statuses read back between the
two).  Reported: the medians, transactions/s over prepare + finish, the share of AM_OK, the resolve
rounds and status-block readbacks per round of the bench (am_cert_stats), the compactions, and
cert_cpu (scripts/cert_cpu.cpp, built with g++ -O2 here) on the same history: its milliseconds per
batch, parsing excluded, and the ratio.  One JSON line per point.  There is no bar: nothing comparable
existed before."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from antidote_amd import abi  # noqa: E402
from antidote_amd.materializer import Materializer, _DevBuf  # noqa: E402
from antidote_amd.oplog import Finishes, Prepares  # noqa: E402

KEYS_PER_TX, KEY_SPACE, ZIPF_S = 4, 1 << 24, 1.1


def draw_keys(rng, n, dist):
    if dist == "uniform":
        return rng.integers(0, KEY_SPACE, n, dtype=np.uint64)
    out = np.empty(0, np.uint64)
    while len(out) < n:  # ranks past the key space are drawn again
        r = rng.zipf(ZIPF_S, 2 * (n - len(out)) + 16)
        out = np.concatenate([out, r[(r >= 1) & (r <= KEY_SPACE)].astype(np.uint64)])
    return ((out[:n] - np.uint64(1)) * np.uint64(0x9E3779B1)) % np.uint64(KEY_SPACE)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def on_device(mat, batch, cols):
    s, bufs = batch.as_struct(), []
    for c in cols:
        bufs.append(_DevBuf.of(mat, np.ascontiguousarray(getattr(batch, c))))
        setattr(s, c, bufs[-1].ptr)
    return s, bufs


def point(mat, cpu_exe, n_tx, dist, steps, warmup, seed):
    rng = np.random.default_rng(seed)
    n_pairs, total = n_tx * KEYS_PER_TX, warmup + steps
    cert = mat.certifier(min(KEY_SPACE, total * n_pairs), n_pairs)
    t_prep, t_fin, ok_share = [], [], []
    hist = tempfile.NamedTemporaryFile("w", suffix=".hist", delete=False)
    hist.write("C 1\n")
    key_off = np.arange(n_tx + 1, dtype=np.uint64) * np.uint64(KEYS_PER_TX)
    try:
        clock, txid0 = 1_000_000, 1
        base = cert.stats()
        for it in range(total):
            if it == warmup:
                base = cert.stats()
            keys = draw_keys(rng, n_pairs, dist)
            txid = np.arange(txid0, txid0 + n_tx, dtype=np.uint64)
            txid0 += n_tx
            start = np.full(n_tx, clock, np.uint64)
            ptime = np.uint64(clock + 10) + np.arange(n_tx, dtype=np.uint64)
            ctime = ptime + np.uint64(5)
            clock += n_tx + 100
            p = Prepares.from_columns(txid, start, ptime, np.ones(n_tx, np.uint8), key_off, keys)
            ps, pb = on_device(mat, p, ("txid", "start_time", "prepare_time", "certify", "key_off", "key"))
            st_dev, st = _DevBuf(mat, 4 * n_tx), np.zeros(n_tx, np.int32)

            def prepare():
                abi.check(mat.L.am_cert_prepare(cert.handle, ctypes.byref(ps), st_dev.ptr), "am_cert_prepare")
                mat.sync()
            a = timed(prepare)
            st_dev.download(st)
            ok = st == 0
            assert ((st == 0) | (st == abi.AM_ERR_WRITE_CONFLICT)).all()
            f = Finishes.from_columns(txid, ctime, ok.astype(np.uint8), key_off, keys)
            fs, fb = on_device(mat, f, ("txid", "commit_time", "committed", "key_off", "key"))

            def finish():
                abi.check(mat.L.am_cert_finish(cert.handle, ctypes.byref(fs), st_dev.ptr), "am_cert_finish")
                mat.sync()
            b = timed(finish)
            for x in pb + fb + [st_dev]:
                x.free()
            if it >= warmup:
                t_prep.append(a), t_fin.append(b), ok_share.append(float(ok.mean()))
            for name, t0, t1, flag in (("P", start, ptime, np.ones(n_tx, np.uint8)), ("F", ctime, None, ok.astype(np.uint8))):
                cols = [txid, t0] + ([t1] if t1 is not None else []) + [flag, np.full(n_tx, KEYS_PER_TX, np.uint64)]
                rows = np.column_stack([c.astype(np.uint64) for c in cols] + [keys.reshape(n_tx, KEYS_PER_TX)])
                hist.write("%s %d\n" % (name, n_tx))
                np.savetxt(hist, rows, fmt="%d")
        assert cert.size()[1] == 0  # every prepared entry was finished
        stats = cert.stats()
        hist.close()
        with open(hist.name) as fh:
            out = subprocess.run([cpu_exe, "--quiet"], stdin=fh, capture_output=True, text=True, check=True).stdout
        cpu_ms = float(out.split()[1]) / total
    finally:
        cert.close()
        hist.close()
        os.unlink(hist.name)
    med = statistics.median
    dev_ms = med(t_prep) + med(t_fin)
    print(json.dumps({
        "tx": n_tx, "keys_per_tx": KEYS_PER_TX, "dist": dist, "steps": steps,
        "prepare_ms": round(med(t_prep), 3), "prepare_min_max": [round(min(t_prep), 3), round(max(t_prep), 3)],
        "finish_ms": round(med(t_fin), 3), "finish_min_max": [round(min(t_fin), 3), round(max(t_fin), 3)],
        "tx_per_s": round(n_tx / dev_ms * 1e3), "ok_share": round(med(ok_share), 4),
        "rounds_per_prepare": round((stats["rounds"] - base["rounds"]) / steps, 2),
        "readbacks_per_prepare_finish": round((stats["readbacks"] - base["readbacks"]) / steps, 2),
        "compactions": stats["compactions"] - base["compactions"],
        "cpu_ms": round(cpu_ms, 3), "cpu_tx_per_s": round(n_tx / cpu_ms * 1e3), "cpu_over_device": round(cpu_ms / dev_ms, 2),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tx", type=int, nargs="*", default=[1 << 10, 1 << 14, 1 << 18])
    ap.add_argument("--dist", nargs="*", default=["uniform", "zipf"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        cpu_exe = os.path.join(d, "cert_cpu")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                        os.path.join(HERE, "cert_cpu.cpp"), "-o", cpu_exe], check=True)
        mat = Materializer(0)
        for n_tx in a.tx:
            for dist in a.dist:
                point(mat, cpu_exe, n_tx, dist, a.steps, a.warmup, 31 * n_tx + len(dist))
        mat.close()


if __name__ == "__main__":
    main()
