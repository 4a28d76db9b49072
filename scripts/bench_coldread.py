"""Cold reads from the device log against warm reads, the log's size, and the commit's cost.

One process, one logged vnode of --keys add-wins-set keys (default 2^16) at D = 8:
  cold_vs_warm  read keys with 16 and 256 logged effects each; once four ShouldGC reads have left
                three cached snapshots above them (the initial {} dropped), a batch of 64 / 4096
                reads at the clock below those snapshots is served from the log
                (am_vnode_read_host, every logged effect of the key a survivor).  Beside it the
                same keys read warm: a clock above the newest cached snapshot, served from the ops
                cache -- the parent commit's path, the yardstick.  Both times and their ratio.
  log_size      the same cold batches after the log is padded to --pad effects (default 2^22 and
                2^24; the read keys' own effects already make it 2^20) on other keys
                (PartitionLog.append on the vnode's log: the ops cache is not involved); the ratio to
                the unpadded time.
  commit        am_vnode_commit_host on a logged and a plain twin vnode (the plain one is the
                parent's path), 64 and 1024 transactions x 4 effects; both times and the ratio.
Runs are interleaved (cold, warm, cold, ...; logged, plain, ...): --warmup, then --steps timed calls,
wall clock around the C call; median and min-max; one JSON line per point.  No result gates."""
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
from antidote_amd.materializer import Materializer  # noqa: E402
from antidote_amd.oplog import Commits, HostBatch, Read  # noqa: E402

AW, N_DC, TX_EFFS = abi.AM_AWSET, 8, 16
U64 = np.uint64
CAP = [64]  # set pairs per read: every add keeps its token (nothing is removed), so a value holds one per effect


def adds(keys, clock, token, per_tx=TX_EFFS):
    """One add-wins add ({Elem, [Token], []}) per entry of `keys` (numpy), per_tx effects per
    transaction, as a Commits built from columns; returns (Commits, the clock after)."""
    n = len(keys)
    nt = (n + per_tx - 1) // per_tx
    txs = []
    for t in range(nt):
        ct = clock + 3 * t
        txs.append((t % N_DC, ct, {d: ct - 2 for d in range(N_DC)}, None, min(per_tx, n - t * per_tx)))
    var = np.zeros((n, 4), U64)  # [elem, 1 add token, 0 remove tokens, token]
    var[:, 0] = np.arange(n, dtype=U64) % 64
    var[:, 1] = 1
    var[:, 3] = token + np.arange(n, dtype=U64)
    cm = Commits.from_columns(N_DC, txs, keys.astype(U64), np.full(n, AW, np.uint8), np.zeros(n, np.uint8),
                              np.zeros(n, U64), np.zeros(n, U64), np.arange(n + 1, dtype=U64) * 4, var.reshape(-1))
    return cm, clock + 3 * nt + 5


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return round(statistics.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)]


def read_call(vn, keys, at):
    hb = HostBatch(N_DC, [Read(int(k), AW, {d: at for d in range(N_DC)}) for k in keys], [CAP[0]] * len(keys))
    b, r = hb.structs()
    return hb, lambda: abi.check(vn.mat.L.am_vnode_read_host(vn.handle, ctypes.byref(b), None, ctypes.byref(r)),
                                 "am_vnode_read_host")


def cold_and_warm(vn, keys, t_cold, t_warm, steps, warmup):
    hc, cold = read_call(vn, keys, t_cold)
    hw, warm = read_call(vn, keys, t_warm)
    tc, tw = [], []
    for it in range(warmup + steps):
        a, b = timed(cold), timed(warm)
        if it >= warmup:
            tc.append(a), tw.append(b)
    assert all(int(s) == 0 for s in hc.status[:len(keys)]) and all(int(s) == 0 for s in hw.status[:len(keys)])
    return tc, tw, int(hc.count[:len(keys)].min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 16)
    ap.add_argument("--read-keys", type=int, default=4096)
    ap.add_argument("--effects", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--reads", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--pad", type=int, nargs="*", default=[1 << 22, 1 << 24])
    ap.add_argument("--tx", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    mat = Materializer(0)
    rk = a.read_keys
    CAP[0] = max(a.effects) + 16
    vn = mat.vnode(N_DC, a.keys, logged=True)
    clock, token = 1000, 1 << 32
    groups = {}  # effects per key -> (its keys, the cold clock)
    for g, e in enumerate(a.effects):  # group g: keys [g * rk, (g + 1) * rk) with e logged effects each
        keys = np.arange(g * rk, (g + 1) * rk)
        for _ in range(e):
            cm, clock = adds(keys, clock, token)
            token += rk
            vn.commit(cm)
        groups[e] = (keys, clock)
    all_keys = np.arange(len(a.effects) * rk)
    for _ in range(4):  # four ShouldGC reads, an op between them: three cached snapshots above the cold clock
        cm, clock = adds(all_keys, clock, token)
        token += len(all_keys)
        vn.commit(cm)
        hb = HostBatch(N_DC, [Read(int(k), AW, {d: clock for d in range(N_DC)}) for k in all_keys], [CAP[0]] * len(all_keys))
        b, r = hb.structs()
        sg = np.ones(len(all_keys), np.uint8)
        abi.check(mat.L.am_vnode_read_host(vn.handle, ctypes.byref(b), sg.ctypes.data, ctypes.byref(r)), "am_vnode_read_host")
    t_warm = clock + 10
    base = {}
    for pad in [0] + sorted(a.pad):
        n_eff = vn.log.size()[1]
        while pad and n_eff < pad:  # padding on keys no read names, straight into the log
            m = min(1 << 20, pad - n_eff)
            cm, clock = adds(np.random.default_rng(n_eff).integers(len(all_keys), a.keys, m), clock, token, 1024)
            token += m
            vn.log.append(cm)
            n_eff += m
        for e, (keys, t_cold) in groups.items():
            for n in a.reads:
                tc, tw, survivors = cold_and_warm(vn, keys[:n], t_cold, t_warm, a.steps, a.warmup)
                (cms, cmm), (wms, wmm) = stats(tc), stats(tw)
                out = {"bench": "log_size" if pad else "cold_vs_warm", "effects_per_key": e, "reads": n,
                       "log_effects": n_eff, "min_survivors": survivors, "steps": a.steps,
                       "cold_ms": cms, "cold_min_max": cmm, "warm_ms": wms, "warm_min_max": wmm,
                       "cold_over_warm": round(cms / wms, 2)}
                if pad:
                    out["cold_over_unpadded"] = round(cms / base[(e, n)], 2)
                else:
                    base[(e, n)] = cms
                print(json.dumps(out), flush=True)
    vn.close()
    for nt in a.tx:  # the commit's cost with and without the log
        rng = np.random.default_rng(nt)
        lg, pl = mat.vnode(N_DC, a.keys, logged=True), mat.vnode(N_DC, a.keys)
        tl, tp = [], []
        clock = 1000
        for it in range(a.warmup + a.steps):
            cm, clock = adds(rng.integers(0, a.keys, nt * 4), clock, token, 4)
            token += nt * 4
            cs = cm.as_struct()
            x = timed(lambda: abi.check(mat.L.am_vnode_commit_host(lg.handle, ctypes.byref(cs)), "am_vnode_commit_host"))
            y = timed(lambda: abi.check(mat.L.am_vnode_commit_host(pl.handle, ctypes.byref(cs)), "am_vnode_commit_host"))
            if it >= a.warmup:
                tl.append(x), tp.append(y)
        (lms, lmm), (pms, pmm) = stats(tl), stats(tp)
        print(json.dumps({"bench": "commit", "tx": nt, "effects": nt * 4, "steps": a.steps,
                          "logged_ms": lms, "logged_min_max": lmm, "plain_ms": pms, "plain_min_max": pmm,
                          "logged_over_plain": round(lms / pms, 2)}), flush=True)
        lg.close(), pl.close()
    mat.close()


if __name__ == "__main__":
    main()
