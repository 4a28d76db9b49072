"""Downstream generation on the device (am_generate_downstream, am_update_objects_host).

A value batch of add-wins sets (--rows sets of --pairs (elem, token) pairs, four tokens per
element) is built on the host and kept in HBM with the updates and the effect columns.  Timed with
am_timer_* (median of --steps calls after --warmup), one JSON line per case:
  remove        one `remove` of 4 present elements per row: binary searches, the base never streamed
  reset         an add-wins-set reset per row: the base streamed once
  mv_assign     an MV assign per row over the same pairs
  eager         am_materialize_eager of the `remove` effects (the device columns as the write set)
                over the same values: that kernel streams the same base once
  single_remove / single_reset   one update against one set of 2^16 pairs; the script fails if the
                remove takes longer than the reset (the base would be being streamed)
  update_objects / read_objects_ws   am_update_objects_host against am_read_objects_ws_host of the
                same batch over a vnode (wall clock): the second copies every state to the host.
                d2h_bytes is computed from the columns each call copies back (update_objects: per
                update 16 effect words and 45 B of eff_off, eff_meta, p0, p1, var_off, avail and
                status, plus n_var and the two closing offsets), not measured
Each line carries the bytes the case must move: 16 B per streamed pair plus the words written for
reset / assign; for remove the searched lines (two searches of ceil(log2 pairs) 64-byte probes per
element, an upper bound) plus the words written."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from antidote_amd import abi  # noqa: E402
from antidote_amd.materializer import Materializer  # noqa: E402
from antidote_amd.oplog import Effects, HostBatch, Op, Read, Updates  # noqa: E402

AW, MV = abi.AM_AWSET, abi.AM_MVREG
TOK_PER_ELEM = 4


class Dev:
    """Device copies of host arrays, freed together."""

    def __init__(self, mat):
        self.mat, self.bufs = mat, []

    def put(self, arr):
        self.bufs.append(self.mat.device_array(np.ascontiguousarray(arr)))
        return self.bufs[-1]

    def free(self):
        for b in self.bufs:
            b.free()


def values(rows, pairs, rng):
    set_off = np.arange(rows + 1, dtype=np.uint64) * np.uint64(pairs)
    set_len = np.full(rows, pairs, np.uint32)
    a = np.tile(np.arange(pairs, dtype=np.uint64) // TOK_PER_ELEM * 3 + 10, rows)
    b = rng.integers(1, 1 << 40, rows * pairs, dtype=np.uint64)
    return set_off, set_len, a, b


class Case:
    def __init__(self, mat, dev, dv, n_dc, entries, var_cap):
        self.mat, self.n_dc, self.dv = mat, n_dc, dv
        fresh = iter(range(1 << 41, 1 << 42))
        self.ups = Updates(entries, lambda: next(fresh))
        n = self.ups.n_up
        u = self.u = abi.am_updates()
        u.n_up, u.n_var = n, self.ups.n_var
        u.row, u.type, u.op, u.a0, u.a1, u.var_off, u.var_data = (dev.put(x).ptr for x in (
            self.ups.row, self.ups.type, self.ups.op, self.ups.a0, self.ups.a1, self.ups.var_off, self.ups.var_data))
        self.host = Effects(self.ups, 0)
        e = self.e = abi.am_effects()
        e.var_cap = var_cap
        self.d_eo, self.d_em, self.d_p0, self.d_p1, self.d_vo = (dev.put(x) for x in (
            self.host.eff_off, self.host.eff_meta, self.host.p0, self.host.p1, self.host.var_off))
        self.d_vd, self.d_nv = dev.put(np.zeros(max(var_cap, 1), np.uint64)), dev.put(self.host.n_var)
        self.d_st = dev.put(self.host.status)
        e.eff_off, e.eff_meta, e.p0, e.p1, e.var_off = (x.ptr for x in (self.d_eo, self.d_em, self.d_p0, self.d_p1, self.d_vo))
        e.var_data, e.n_var = self.d_vd.ptr, self.d_nv.ptr

    def call(self):
        abi.check(self.mat.L.am_generate_downstream(self.mat.ctx, self.n_dc, ctypes.byref(self.u), ctypes.byref(self.dv),
                                                    None, ctypes.byref(self.e), self.d_st.ptr), "am_generate_downstream")

    def check(self):
        self.d_st.download(self.host.status)
        self.d_nv.download(self.host.n_var)
        assert (self.host.status[:self.ups.n_up] == 0).all() and int(self.host.n_var[0]) <= self.e.var_cap
        return int(self.host.n_var[0])


def timed(mat, call, steps, warmup):
    for _ in range(warmup):
        call()
    mat.sync()
    times = []
    for _ in range(steps):
        ms = ctypes.c_float()
        abi.check(mat.L.am_timer_start(mat.ctx), "am_timer_start")
        call()
        abi.check(mat.L.am_timer_stop(mat.ctx, ctypes.byref(ms)), "am_timer_stop")
        times.append(ms.value)
    return float(np.median(times)), float(min(times)), float(max(times))


def line(name, t, nbytes, **kw):
    ms, lo, hi = t
    print(json.dumps(dict({"metric": f"downstream {name} ms per call", "value": ms, "unit": "ms", "ms_min": lo,
                           "ms_max": hi, "must_move_bytes": int(nbytes),
                           "must_move_TBps": nbytes / (ms * 1e-3) / 1e12 if ms else 0.0}, **kw)), flush=True)


def remove_bytes(n_elems, pairs, words):
    return n_elems * 2 * math.ceil(math.log2(max(pairs, 2))) * 64 + words * 8


def device_cases(mat, args):
    rng = np.random.default_rng(7)
    rows, pairs, n_dc = args.rows, args.pairs, 3
    so, sl, a, b = values(rows, pairs, rng)
    dev = Dev(mat)
    dv = abi.am_values()
    d_so, d_sl = dev.put(so), dev.put(sl)
    dv.set_off, dv.set_len, dv.set_a, dv.set_b = d_so.ptr, d_sl.ptr, dev.put(a).ptr, dev.put(b).ptr
    n_elem = pairs // TOK_PER_ELEM
    pick = lambda i: [10 + 3 * int(x) for x in rng.choice(n_elem, 4, replace=False)]  # noqa: E731
    cfg = {"rows": rows, "pairs_per_row": pairs, "steps": args.steps, "warmup": args.warmup}
    try:
        rm = Case(mat, dev, dv, n_dc, [(i, AW, ("remove_all", pick(i))) for i in range(rows)], rows * 4 * (3 + TOK_PER_ELEM))
        t = timed(mat, rm.call, args.steps, args.warmup)
        w = rm.check()
        line("remove (4 elements per update)", t, remove_bytes(4 * rows, pairs, w), updates=rows, words_out=w, config=cfg)
        for name, typ, upd in (("reset", AW, ("reset",)), ("mv_assign", MV, ("assign", 5))):
            c = Case(mat, dev, dv, n_dc, [(i, typ, upd) for i in range(rows)], rows * (pairs + 3 * n_elem))
            t = timed(mat, c.call, args.steps, args.warmup)
            w = c.check()
            line(name, t, rows * pairs * 16 + w * 8, updates=rows, pairs_streamed=rows * pairs, words_out=w, config=cfg)
        # am_materialize_eager over the same values, the remove effects as its write set
        rm.call()
        ws = abi.am_writeset()
        ws.n_ws = ws.n_eff = rows
        ws.n_var = rm.e.var_cap
        ws.row, ws.type = rm.u.row, rm.u.type
        ws.eff_off, ws.eff_meta, ws.p0, ws.p1, ws.var_off, ws.var_data = (rm.e.eff_off, rm.e.eff_meta, rm.e.p0, rm.e.p1,
                                                                          rm.e.var_off, rm.e.var_data)
        vout = abi.am_values()
        vout.set_off, vout.set_len = d_so.ptr, dev.put(np.zeros(rows, np.uint32)).ptr
        vout.set_a, vout.set_b = dev.put(np.zeros(rows * pairs, np.uint64)).ptr, dev.put(np.zeros(rows * pairs, np.uint64)).ptr
        d_est = dev.put(np.zeros(rows, np.int32))

        def eager():
            abi.check(mat.L.am_materialize_eager(mat.ctx, n_dc, ctypes.byref(ws), ctypes.byref(dv), None, ctypes.byref(vout),
                                                 d_est.ptr), "am_materialize_eager")
        t = timed(mat, eager, args.steps, args.warmup)
        est = np.ones(rows, np.int32)
        d_est.download(est)
        assert (est == 0).all(), "the eager fold failed"
        out_pairs = rows * (pairs - 4 * TOK_PER_ELEM)
        line("eager (am_materialize_eager, same values, the remove effects)", t, (rows * pairs + out_pairs) * 16,
             entries=rows, config=cfg)
    finally:
        dev.free()


def single_check(mat, args):
    """A remove of 4 elements must not take longer than a reset against one set of 2^16 pairs."""
    rng = np.random.default_rng(11)
    pairs = 1 << 16
    so, sl, a, b = values(1, pairs, rng)
    dev = Dev(mat)
    dv = abi.am_values()
    dv.set_off, dv.set_len, dv.set_a, dv.set_b = (dev.put(x).ptr for x in (so, sl, a, b))
    try:
        elems = [10, 10 + 3 * 5000, 10 + 3 * 11111, 10 + 3 * (pairs // TOK_PER_ELEM - 1)]
        rm = Case(mat, dev, dv, 1, [(0, AW, ("remove_all", elems))], 64)
        rs = Case(mat, dev, dv, 1, [(0, AW, ("reset",))], 2 * pairs)
        t_rm = timed(mat, rm.call, 50, 5)
        t_rs = timed(mat, rs.call, 50, 5)
        w_rm, w_rs = rm.check(), rs.check()
        line("single_remove (4 elements, one set of 2^16 pairs)", t_rm, remove_bytes(4, pairs, w_rm), words_out=w_rm)
        line("single_reset (one set of 2^16 pairs)", t_rs, pairs * 16 + w_rs * 8, words_out=w_rs)
        assert t_rm[0] <= t_rs[0], f"remove {t_rm[0]} ms > reset {t_rs[0]} ms: the base is being streamed"
    finally:
        dev.free()


def objects_case(mat, args):
    from antidote_amd.readbatch import PartitionedReader
    n_dc, keys, elems = 3, args.keys, args.key_elems
    objects = {}
    for k in range(keys):   # one committed add_all per key: `elems` elements, one token each
        eff = [(10 + 3 * e, [(k << 20) + e + 1], []) for e in range(elems)]
        objects[k] = (AW, [Op(type=AW, commit_dc=0, commit_time=100, snap={d: 50 for d in range(n_dc)}, effect=eff)])
    rd = PartitionedReader(mat, 4, n_dc, objects)
    try:
        clock = {d: 1000 for d in range(n_dc)}
        cap = 2 * elems
        rng = np.random.default_rng(3)
        parts = np.zeros(keys, np.uint32)
        reads = []
        for k in range(keys):
            parts[k], local = rd.where[k]
            reads.append(Read(local, AW, dict(clock)))
        ups = Updates([(k, AW, ("remove_all", [10 + 3 * int(x) for x in rng.choice(elems, 4, replace=False)]))
                       for k in range(keys)])
        eff = Effects(ups, keys * 4 * 4)
        u, e = ups.as_struct(), eff.as_struct()

        hb = HostBatch(n_dc, reads, [cap] * keys)   # both calls reuse these host buffers
        b, r = hb.structs()

        def update_objects():
            abi.check(mat.L.am_update_objects_host(rd.vnode.handle, rd.n_partitions, rd.part_key_base.ctypes.data,
                                                   parts.ctypes.data, ctypes.byref(b), hb.o_set_off.ctypes.data, None,
                                                   ctypes.byref(u), ctypes.byref(e), eff.status.ctypes.data),
                      "am_update_objects_host")

        def read_ws():
            abi.check(mat.L.am_read_objects_ws_host(rd.vnode.handle, rd.n_partitions, rd.part_key_base.ctypes.data,
                                                    parts.ctypes.data, ctypes.byref(b), None, ctypes.byref(r)),
                      "am_read_objects_ws_host")
        out = {}
        for name, fn in (("update_objects", update_objects), ("read_objects_ws", read_ws)):
            for _ in range(2):
                fn()
            ts = []
            for _ in range(10):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name] = (float(np.median(ts)), float(min(ts)), float(max(ts)))
        assert (eff.status[:keys] == 0).all() and int(eff.n_var[0]) == keys * 4 * 4
        read_ws()
        assert (hb.status[:keys] == 0).all() and (hb.o_set_len[:keys] == elems).all()
        cfg = {"keys": keys, "pairs_per_key": elems, "set_capacity": cap, "clock": "wall", "steps": 10, "warmup": 2}
        line("update_objects (am_update_objects_host, a remove of 4 per key)", out["update_objects"],
             keys * 16 * 8 + keys * 45 + 24, d2h_bytes=keys * (16 * 8 + 45) + 24, config=cfg)
        line("read_objects_ws (am_read_objects_ws_host, the states copied back)", out["read_objects_ws"],
             keys * cap * 16, d2h_bytes=keys * cap * 16, config=cfg)
    finally:
        rd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--keys", type=int, default=512)
    ap.add_argument("--key-elems", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    mat = Materializer(0)
    try:
        device_cases(mat, args)
        single_check(mat, args)
        objects_case(mat, args)
    finally:
        mat.close()


if __name__ == "__main__":
    main()
