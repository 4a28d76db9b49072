"""Read-your-writes fold (am_materialize_eager) on snapshots of a synthetic add-wins store.

The store's keys are read once with am_materialize (host batch); from the downloaded values one
write set per read is built on the host -- one effect that adds an element with a fresh token and
removes an observed one (all tokens of the value's first element) -- and am_materialize_eager
folds them on the device: value batch, write set and outputs resident in HBM, timed with
am_timer_* (median of 20 calls after 3 warm-ups).  Prints one JSON line: ms per call and the
algorithmic traffic (input pairs + output pairs) x 16 B / time against the 8 TB/s HBM peak."""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from antidote_amd import abi, synth  # noqa: E402
from antidote_amd.materializer import Materializer  # noqa: E402
from antidote_amd.oplog import Read, WriteSet  # noqa: E402

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 17)
    ap.add_argument("--ops", type=int, default=64)
    ap.add_argument("--universe", type=int, default=64)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n_dc, n = 3, args.keys
    mat = Materializer(0)
    L = mat.L
    p = synth.params(n, n_dc, abi.AM_AWSET, ops_per_key=args.ops, universe=args.universe)
    store = mat.synth_store(p)
    clock = dict(enumerate(synth.read_clock(p, 1.0)))
    hb = mat.read_batch(store, [Read(k, abi.AM_AWSET, clock) for k in range(n)], [args.cap] * n)
    store.close()
    assert (hb.status[:n] == 0).all(), "a snapshot read failed (raise --cap)"
    # one write set per read: add a new element, remove an observed one
    off, ln = hb.o_set_off, hb.o_set_len
    entries, pairs_in, pairs_out = [], 0, 0
    for i in range(n):
        o, m = int(off[i]), int(ln[i])
        eff = [(args.universe + 1 + (i % 7), [(1 << 40) + i], [])]
        if m:
            a, b = hb.o_set_a[o:o + m], hb.o_set_b[o:o + m]
            e0 = int(a[0])
            rm = b[a == a[0]].tolist()
            eff = [(e0, [], rm)] + eff
            pairs_out -= len(rm)
        entries.append((i, abi.AM_AWSET, [eff]))
        pairs_in += m
        pairs_out += m + 1
    ws = WriteSet(entries)
    dev = [mat.device_array(a) for a in (ws.row, ws.type, ws.eff_off, ws.eff_meta, ws.p0, ws.p1, ws.var_off, ws.var_data,
                                         hb.o_set_off, hb.o_set_len, hb.o_set_a, hb.o_set_b)]
    outs = [mat.device_array(np.zeros_like(a)) for a in (hb.o_set_len, hb.o_set_a, hb.o_set_b, hb.status)]
    w = abi.am_writeset()
    w.n_ws, w.n_eff, w.n_var = ws.n_ws, ws.n_eff, ws.n_var
    w.row, w.type, w.eff_off, w.eff_meta, w.p0, w.p1, w.var_off, w.var_data = (d.ptr for d in dev[:8])
    vin, vout = abi.am_values(), abi.am_values()
    vin.set_off, vin.set_len, vin.set_a, vin.set_b = (d.ptr for d in dev[8:])
    vout.set_off = dev[8].ptr  # the same capacities
    vout.set_len, vout.set_a, vout.set_b = outs[0].ptr, outs[1].ptr, outs[2].ptr

    def call():
        abi.check(L.am_materialize_eager(mat.ctx, n_dc, ctypes.byref(w), ctypes.byref(vin), None, ctypes.byref(vout),
                                         outs[3].ptr), "am_materialize_eager")

    for _ in range(args.warmup):
        call()
    mat.sync()
    times = []
    for _ in range(args.steps):
        ms = ctypes.c_float()
        abi.check(L.am_timer_start(mat.ctx), "am_timer_start")
        call()
        abi.check(L.am_timer_stop(mat.ctx, ctypes.byref(ms)), "am_timer_stop")
        times.append(ms.value)
    st, sl = np.zeros_like(hb.status), np.zeros_like(hb.o_set_len)
    outs[3].download(st)
    outs[0].download(sl)
    assert (st[:n] == 0).all() and int(sl[:n].sum()) == pairs_out, "the fold failed"
    ms = float(np.median(times))
    nbytes = (pairs_in + pairs_out) * 16
    print(json.dumps({"metric": "materialize_eager ms per call", "value": ms, "unit": "ms", "entries": n,
                      "pairs_in": pairs_in, "pairs_out": pairs_out, "alg_bytes": nbytes,
                      "alg_TBps": nbytes / (ms * 1e-3) / 1e12, "frac_of_8TBps": nbytes / (ms * 1e-3) / PEAK,
                      "ms_min": float(min(times)), "ms_max": float(max(times)),
                      "config": {"workload": f"add-wins set, {n} keys x {args.ops} ops, D={n_dc}, universe "
                                             f"{args.universe}, read at q=1; write set per read: one effect, "
                                             f"1 add + the removal of an observed element",
                                 "steps": args.steps, "warmup": args.warmup}}))
    for d in dev + outs:
        d.free()
    mat.close()


if __name__ == "__main__":
    main()
