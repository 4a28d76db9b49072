"""Read-your-writes through the read path: am_read_objects_ws_host / _submit over three
partitions equal the oracle's internal_read/7 followed by materialize_eager/3 per request
(apply_tx_updates_to_snapshot/4, src/clocksi_interactive_coord.erl:883-894), an empty write set
changes nothing, and the reference's system suites run with a transaction's own writes folded by
Materializer.materialize_eager instead of the TxId trick of dcsim.GpuBackend.staged."""
import ctypes
import random

import numpy as np
import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostBatch, Read, WriteSet
from oracle import ref_materializer as R
from tests import dcsim, randlog
from tests.kat_util import load
from tests.test_gpu_vnode import KeyGen, _placeholder

pytestmark = pytest.mark.gpu

AW, MV = abi.AM_AWSET, abi.AM_MVREG
COLS = ("status", "new_last_op", "last_ct", "last_ct_pres", "last_ct_ignore", "is_new_ss", "count", "flags", "v0", "v1",
        "vflag", "o_set_len", "o_set_a", "o_set_b")


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def _objects(rng, n_keys, n_dc):
    keys = rng.sample(range(-5000, 5000), n_keys)
    objects = {}
    for key in keys:
        t = rng.choice(randlog.TYPES)
        objects[key] = (t, KeyGen(rng, t, n_dc, 10).ops(rng.choice([0, 1, 6, 40, 100])))
    return keys, objects


def _own_effects(rng, t, ops, n_dc, fresh):
    """A transaction's effects on a key: fresh tokens, removes / overrides of tokens the key's
    log holds (some live in the snapshot, some not)."""
    out = []
    for _ in range(rng.choice([1, 1, 2, 4])):
        if t == AW:
            seen = {}
            for op in ops:
                for e, add, _ in op.effect:
                    seen.setdefault(e, []).extend(add)
            ents = []
            for e in sorted(rng.sample(range(8), rng.randint(1, 2))):
                fresh[0] += 1
                rm = rng.sample(seen.get(e, []), min(len(seen.get(e, [])), rng.randint(0, 6)))
                ents.append((e, [fresh[0]] if rng.random() < 0.7 else [], rm))
            out.append(ents)
        elif t == MV:
            toks = [op.effect[2] for op in ops if op.effect[0] == "assign"]
            own = [e[2] for e in out]  # the transaction's earlier assigns to the key
            fresh[0] += 1
            ovr = toks[len(toks) - min(len(toks), rng.randint(0, 8)):] + (own if rng.random() < 0.7 else [])
            out.append(("assign", rng.randint(0, 4), fresh[0], ovr))
        else:
            out.append(randlog.rand_effect(rng, t, n_dc, {}))
    return out


def _raw(rd, mat, req, clock, ws_struct, use_ws_call):
    """am_read_objects_host, or am_read_objects_ws_host with the given write set (None = NULL)."""
    parts = np.zeros(max(len(req), 1), np.uint32)
    reads = []
    for i, (key, t) in enumerate(req):
        parts[i], local = rd.where[key]
        reads.append(Read(local, t, dict(clock)))
    hb = HostBatch(rd.n_dc, reads, [4096] * len(reads))
    b, r = hb.structs()
    if use_ws_call:
        abi.check(mat.L.am_read_objects_ws_host(rd.vnode.handle, rd.n_partitions, rd.part_key_base.ctypes.data,
                                                parts.ctypes.data, ctypes.byref(b),
                                                ctypes.byref(ws_struct) if ws_struct is not None else None,
                                                ctypes.byref(r)), "am_read_objects_ws_host")
    else:
        abi.check(mat.L.am_read_objects_host(rd.vnode.handle, rd.n_partitions, rd.part_key_base.ctypes.data,
                                             parts.ctypes.data, ctypes.byref(b), ctypes.byref(r)), "am_read_objects_host")
    return hb


def test_gpu_read_objects_ws_equals_read_then_eager(mat):
    from antidote_amd.readbatch import PartitionedReader
    rng = random.Random(717)
    n_dc, n_part = 3, 3
    keys, objects = _objects(rng, 60, n_dc)
    st = R.VnodeState()
    dead = set()
    for key in keys:
        for op in objects[key][1]:
            if _placeholder(st, key):
                dead.add(key)
                break
            R.op_insert_gc(key, randlog.payload_term(op, key=key), st)
    plain = PartitionedReader(mat, n_part, n_dc, objects)   # the snapshot reads, for the other columns
    rd = PartitionedReader(mat, n_part, n_dc, objects)
    fresh = [10 ** 7]
    try:
        assert {rd.partition_of(k) for k in keys} == set(range(n_part))
        hi = max(op.commit_time for _, ops in objects.values() for op in ops)
        applied = 0
        for rnd in range(4):
            clock = {d: rng.randint(hi // 2, hi + 10) for d in range(n_dc)}
            req = [(k, objects[k][0]) for k in rng.choices(keys, k=40)]   # keys requested twice and more
            assert len({k for k, _ in req}) < len(req)
            wkeys = rng.sample(sorted({k for k, _ in req}), 12)
            write_set = {k: _own_effects(rng, objects[k][0], objects[k][1], n_dc, fresh) for k in wkeys}
            snap = plain.read_objects(req, clock)
            if rnd % 2 == 0:   # am_read_objects_ws_submit + am_ticket_wait
                got = rd.read_objects(req, clock, write_set=write_set)
            else:              # am_read_objects_ws_host
                ws = WriteSet([(i, t, write_set[k]) for i, (k, t) in enumerate(req) if k in write_set])
                hb = _raw(rd, mat, req, clock, ws.as_struct(), True)
                got = [hb.result(i) for i in range(len(req))]
            for (key, t), g, s in zip(req, got, snap):
                if _placeholder(st, key):
                    dead.add(key)
                if key in dead:
                    continue
                try:
                    ref = R.internal_read(key, t, dict(clock), R.IGNORE, False, st)
                except R.LogColdPath:
                    assert g == s == ("error", abi.AM_ERR_COLD_PATH), (key, g, s)
                    continue
                assert s[0] == "ok" and s[1] == randlog.canon_state(t, ref[1]), (key, s, ref)
                if key not in write_set:
                    assert g == s, (key, g, s)
                    continue
                eager = R.materialize_eager(t, ref[1], [randlog.effect_term(t, e) for e in write_set[key]])
                assert g[0] == "ok" and g[1] == randlog.canon_state(t, eager), (key, t, write_set[key], g, s)
                assert g[2:] == s[2:], "every other column stays the snapshot read's"
                applied += 1
        assert applied > 20
    finally:
        rd.close()
        plain.close()


def test_gpu_read_objects_ws_empty_write_set_is_the_plain_read(mat):
    from antidote_amd.readbatch import PartitionedReader
    rng = random.Random(818)
    n_dc, n_part = 3, 3
    keys, objects = _objects(rng, 40, n_dc)
    rds = [PartitionedReader(mat, n_part, n_dc, objects) for _ in range(3)]
    try:
        hi = max(op.commit_time for _, ops in objects.values() for op in ops)
        for _ in range(2):
            clock = {d: rng.randint(hi // 2, hi + 10) for d in range(n_dc)}
            req = [(k, objects[k][0]) for k in rng.choices(keys, k=50)]
            empty = WriteSet([])
            hbs = [_raw(rds[0], mat, req, clock, None, False), _raw(rds[1], mat, req, clock, None, True),
                   _raw(rds[2], mat, req, clock, empty.as_struct(), True)]
            for c in COLS:
                for hb in hbs[1:]:
                    assert getattr(hbs[0], c).tobytes() == getattr(hb, c).tobytes(), c
    finally:
        for rd in rds:
            rd.close()


# ---- the reference's system suites with staged reads through materialize_eager ----
class EagerBackend(dcsim.GpuBackend):
    def staged(self, dc, key, clock, txid, effects, base):
        """apply_tx_updates_to_snapshot/4: the snapshot read, then the transaction's own
        writes folded by am_materialize_eager (no TxId, no scratch log)."""
        t = self.keys[key]
        labs = [self._labels(dc, t, e) for e in effects]  # may relabel: intern before reading the base
        base_lab = self._read_labels(dc, key, clock)
        hb = self.mat.materialize_eager(self.n_dc, [(t, base_lab, labs)], [4096])
        assert int(hb.status[0]) == 0, int(hb.status[0])
        return self._terms(dc, t, hb.value(0))


SUITES = load("multidc_suites.json")["cases"] + load("txn_suites.json")["cases"]


@pytest.mark.parametrize("case", SUITES, ids=lambda c: c["name"])
def test_gpu_suites_staged_reads_through_materialize_eager(mat, case):
    from tests.test_gpu_multidc import _Tee

    class Tee(_Tee):
        def __init__(self, n_dc, keys, m):
            self.g = EagerBackend(n_dc, keys, m)
            self.o = dcsim.OracleBackend(n_dc, keys)
            self.n = 0

    tees = []

    def factory(n_dc, keys):
        tees.append(Tee(n_dc, keys, mat))
        return tees[-1]

    checks = dcsim.run_case(case, factory)
    assert checks and tees[0].n > 0
    for where, got, exp in checks:
        assert got == exp, where
