#!/usr/bin/env python3
"""CPU replay of the inclusion pass's commit-word window (antidote_amd/csrc/am_inclwin.h, the schedule of
k_grp_incl<.., LAG = true>) on the first keys of the benchmark's C3 population, with the format's 16-bit
lag range and with each key's own lag width.  Needs the built library (the generator), no GPU.
   python scripts/lagwidth_replay.py [n_keys=512] [config=c3]
Per read (mean over the keys; min-max in brackets): the key's largest lag, the window list's entries,
the rounds of 64 walked and those that load lags, the ops whose lags are gathered, and the 128-byte
lag lines (64 ops of one DC) those ops touch per DC."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from antidote_amd import synth  # noqa: E402

SEG, WAVE, ESC = 1024, 64, 0xFFFFFFFF


def key_view(log, k):
    """(absolute positions, commit words, lags [n][nd], lag bases) of key k's ops, all in the view
    (a key with an op outside it is skipped: None)."""
    nd = log.n_dc
    a, b = int(log.key_off[k]), int(log.key_off[k + 1])
    ct = log.commit_time[a:b].astype(np.int64)
    dc = (log.op_meta[a:b] & 0x1F).astype(np.int64)
    X = log.snap_vc[:, a:b].astype(np.int64).copy()
    X[dc, np.arange(b - a)] = ct
    lo, floor = int(ct[0]), max(int(ct[0]) - 0x7FFFFFFF, 0)
    for d in range(nd):
        if d != dc[0] and floor <= X[d, 0] < lo:
            lo = int(X[d, 0])
    K = lo - 0x40000000 if lo > 0x40000000 else 0
    lag = ct[None, :] - X
    lb = lag.min(axis=1)
    lag = (lag - lb[:, None]).T
    if ((X - K < 0) | (X - K >= ESC)).any() or (lag > 0xFFFF).any():
        return None
    return np.arange(a, b), ct - K, lag, lb, K


def replay(pos, c, lag, lb, thr, w):
    """One read: (list entries, rounds walked, rounds that load, ops loaded, lag lines per DC, included)."""
    cin = int((thr + lb).min())
    hi, cmax = cin + w, -(1 << 62)
    x = c[:, None] - lb[None, :] - lag
    nl = walked = loading = loaded = 0
    lines, inc = set(), 0
    t0 = int(pos[0]) & ~31
    nseg = (int(pos[-1]) - t0) // SEG + 1
    for sg in range(nseg - 1, -1, -1):
        m = (pos >= t0 + sg * SEG) & (pos < t0 + (sg + 1) * SEG)
        idx = np.nonzero(m)[0]
        sure = c[idx][c[idx] <= cin]
        if len(sure):
            cmax = max(cmax, int(sure.max()) - max(w, 1))
        lim = min(cin, cmax)
        inc += int((c[idx] <= lim).sum())
        lst = idx[(c[idx] > lim) & (c[idx] <= hi)][::-1]
        nl += len(lst)
        mx = np.zeros(len(lb), np.int64)
        for r0 in range(0, len(lst), WAVE):
            e = lst[r0:r0 + WAVE]
            walked += 1
            need = c[e] > min(cin, cmax) if r0 else np.ones(len(e), bool)
            inc += int((~need).sum())
            if not need.any():
                continue
            loading += 1
            loaded += int(need.sum())
            lines |= {int(p) // 64 for p in pos[e[need]]}
            ok = need & (x[e] <= thr[None, :]).all(axis=1)
            inc += int(ok.sum())
            if ok.any():
                mx = np.maximum(mx, x[e][ok].max(axis=0))
                cmax = max(cmax, int((mx + lb).min()))
    return nl, walked, loading, loaded, len(lines), inc


def main():
    n_keys = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    cfg = dict(bench.CONFIGS[sys.argv[2] if len(sys.argv) > 2 else "c3"])
    p = bench.synth_params(cfg)
    log = synth.host_log(p, 0, n_keys)
    clock = np.asarray(synth.read_clock(p, bench.Q), np.int64)
    rows = {"format": [], "key": []}
    widths, skipped = [], 0
    for k in range(n_keys):
        v = key_view(log, k)
        if v is None:
            skipped += 1
            continue
        pos, c, lag, lb, K = v
        thr = np.clip(clock - K, 0, ESC - 1)
        w = int(lag.max())
        widths.append(w)
        a, b = replay(pos, c, lag, lb, thr, 0xFFFF), replay(pos, c, lag, lb, thr, w)
        assert a[5] == b[5] == int((c[:, None] - lb[None, :] - lag <= thr[None, :]).all(axis=1).sum())
        rows["format"].append(a[:5])
        rows["key"].append(b[:5])
    print(f"{len(widths)} keys ({skipped} skipped: an op outside the lag view), D = {log.n_dc}, "
          f"largest lag of the key: mean {np.mean(widths):.0f} (max {max(widths)}) us")
    names = ["window list entries", "rounds walked", "rounds that load lags", "ops whose lags are gathered",
             "128-byte lag lines per DC"]
    for i, name in enumerate(names):
        f, o = np.array(rows["format"])[:, i], np.array(rows["key"])[:, i]
        print(f"{name:30s} 0xFFFF: {f.mean():7.1f} ({f.min()}-{f.max()})   key's width: {o.mean():7.1f} ({o.min()}-{o.max()})")


if __name__ == "__main__":
    main()
