"""Commit on the device against the host-log path (am_vnode_commit_host vs am_vnode_insert_host).

Twin vnodes of --keys keys (default 2^16 and 2^20) in one process get the same batches of --tx
transactions (default 64 and 1024) x 4 effects on uniformly random keys (add-wins-set adds, D = 8):
  commit   the C call am_vnode_commit_host on a prebuilt am_commits
  insert   the C call am_vnode_insert_host over the same ops as a prebuilt host log, CSR over every
           key of the vnode (the parent path; the yardstick)
Runs are interleaved (commit, insert, commit, ...): --warmup batches, then --steps timed ones
(wall clock around the C call); median and min-max per point.  The Python encoding of each
(oplog.Commits, oplog.HostLog over all keys) is timed separately.  `builder` is am_commit_build
alone on device copies of the last batch (median of --steps calls, wall clock with its one
readback), and builder_share its part of the commit call's median.  One JSON line per point; the
script exits 1 when a commit median is above the insert median at some point."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from antidote_amd import abi  # noqa: E402
from antidote_amd.materializer import Materializer, _DevBuf  # noqa: E402
from antidote_amd.oplog import Commits, HostLog  # noqa: E402

AW, N_DC, EFFS = abi.AM_AWSET, 8, 4


def batch(rng, n_tx, n_keys, clock, token):
    """n_tx transactions of 4 add-wins adds ({Elem, [Token], []}) on uniformly random keys."""
    txs = []
    for t in range(n_tx):
        ct = clock + 3 * t
        effs = [(int(rng.integers(n_keys)), AW, [(int(rng.integers(64)), [token + EFFS * t + j], [])]) for j in range(EFFS)]
        txs.append((int(rng.integers(N_DC)), ct, {d: ct - 20 for d in range(N_DC)}, None, effs))
    return txs


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def builder_ms(mat, cm, steps):
    s = cm.as_struct()
    bufs = []
    for c in ("dc", "commit_time", "snap_vc", "eff_off", "key", "type", "eff_meta", "p0", "p1", "var_off", "var_data"):
        bufs.append(_DevBuf.of(mat, np.ascontiguousarray(getattr(cm, c))))
        setattr(s, c, bufs[-1].ptr)
    n, nv = cm.n_eff, cm.n_var
    o = abi.am_commit_log()
    o.cap_ops, o.cap_var, o.snap_stride = n, nv, n
    for c, nb in {"keys": 8 * n, "key_off": 8 * (n + 1), "key_type": n, "key_flags": n, "op_meta": n, "commit_time": 8 * n,
                  "snap_vc": 8 * n * N_DC, "snap_pres": 4 * n, "op_txid": 8 * n, "p0": 8 * n, "p1": 8 * n,
                  "var_off": 8 * (n + 1), "var_data": 8 * nv + 8, "src": 4 * n}.items():
        bufs.append(_DevBuf(mat, nb))
        setattr(o, c, bufs[-1].ptr)
    log, nt = abi.am_op_log(), ctypes.c_uint64()
    bits = max(1, int(cm.key[:n].max()).bit_length())
    call = lambda: abi.check(mat.L.am_commit_build(mat.ctx, N_DC, ctypes.byref(s), bits, ctypes.byref(o),  # noqa: E731
                                                   ctypes.byref(log), ctypes.byref(nt), None), "am_commit_build")
    for _ in range(3):
        call()
    ms = [timed(call) for _ in range(steps)]
    for b in bufs:
        b.free()
    return statistics.median(ms)


def point(mat, n_keys, n_tx, steps, warmup, seed):
    rng = np.random.default_rng(seed)
    vc, vi = mat.vnode(N_DC, n_keys), mat.vnode(N_DC, n_keys)
    ktype = [AW] * n_keys
    t_commit, t_insert, enc_c, enc_i = [], [], [], []
    clock, token = 1000, 1 << 32
    cm = None
    try:
        for it in range(warmup + steps):
            txs = batch(rng, n_tx, n_keys, clock, token)
            clock += 3 * n_tx + 5
            token += EFFS * n_tx
            t0 = time.perf_counter()
            cm = Commits(N_DC, txs)
            cs = cm.as_struct()
            e_c = (time.perf_counter() - t0) * 1e3
            by_key = cm.ops_by_key()
            t0 = time.perf_counter()
            hl = HostLog(N_DC, [by_key.get(k, ()) for k in range(n_keys)], key_types=ktype)
            hs = hl.as_struct()
            e_i = (time.perf_counter() - t0) * 1e3
            a = timed(lambda: abi.check(mat.L.am_vnode_commit_host(vc.handle, ctypes.byref(cs)), "am_vnode_commit_host"))
            b = timed(lambda: abi.check(mat.L.am_vnode_insert_host(vi.handle, ctypes.byref(hs)), "am_vnode_insert_host"))
            if it >= warmup:
                t_commit.append(a), t_insert.append(b), enc_c.append(e_c), enc_i.append(e_i)
        assert vc.stats() == vi.stats(), (vc.stats(), vi.stats())
        bld = builder_ms(mat, cm, steps)
    finally:
        vc.close()
        vi.close()
    med = statistics.median
    out = {"keys": n_keys, "tx": n_tx, "effects": n_tx * EFFS, "steps": steps,
           "commit_ms": round(med(t_commit), 3), "commit_min_max": [round(min(t_commit), 3), round(max(t_commit), 3)],
           "insert_ms": round(med(t_insert), 3), "insert_min_max": [round(min(t_insert), 3), round(max(t_insert), 3)],
           "speedup": round(med(t_insert) / med(t_commit), 2),
           "encode_commits_ms": round(med(enc_c), 3), "encode_hostlog_ms": round(med(enc_i), 3),
           "builder_ms": round(bld, 3), "builder_share": round(bld / med(t_commit), 3)}
    print(json.dumps(out), flush=True)
    return med(t_commit) <= med(t_insert)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, nargs="*", default=[1 << 16, 1 << 20])
    ap.add_argument("--tx", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    mat = Materializer(0)
    ok = True
    for nk in a.keys:
        for nt in a.tx:
            ok = point(mat, nk, nt, a.steps, a.warmup, 17 * nk + nt) and ok
    mat.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
