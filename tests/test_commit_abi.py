"""CPU checks of the device-commit boundary: include/antidote_mat.h declares am_commit_build and
am_vnode_commit_host, the library exports them, am_commits / am_commit_log have the header's layout,
the ABI version is still 15, the calls reject missing arguments before touching a device, the host
encoder (oplog.Commits) round-trips encode_effect, and Commits.reference_log() -- the expected value
of the GPU tests -- equals a HostLog built from the same ops grouped per key."""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np

from antidote_amd import abi
from antidote_amd.oplog import Commits, HostLog, decode_effect, encode_effect
from tests import randlog
from tests.test_abi import HDR, ROOT, declared_functions

CM_FNS = ["am_commit_build", "am_vnode_commit_host"]
TYPES = [abi.AM_PN, abi.AM_LWW, abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER]


def test_header_declares_and_library_exports_the_commit_calls():
    fns = declared_functions()
    L = abi.lib()
    names = {n for n, _, _ in abi.SIGNATURES}
    for fn in CM_FNS:
        assert fn in fns, fn
        assert fn in names, fn
        assert hasattr(L, fn), fn
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_commits_and_commit_log_layout_and_codes_match_header():
    cm_f = [f for f, _ in abi.am_commits._fields_]
    lg_f = [f for f, _ in abi.am_commit_log._fields_]
    offs_c = ", ".join(f"offsetof(am_commits, {f})" for f in cm_f)
    offs_l = ", ".join(f"offsetof(am_commit_log, {f})" for f in lg_f)
    codes = ["AM_COMMIT_BAD_DC", "AM_COMMIT_BAD_EFF_OFF", "AM_COMMIT_BAD_VAR_OFF", "AM_COMMIT_BAD_TYPE",
             "AM_COMMIT_BAD_KEY", "AM_KEY_MIXED_TYPES", "AM_META_BAD"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 size_t u[] = {%s}; size_t e[] = {%s}; long c[] = {%s};
 printf("%%zu %%zu\n", sizeof(am_commits), sizeof(am_commit_log));
 for (size_t i = 0; i < sizeof u / sizeof *u; ++i) printf("%%zu ", u[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof e / sizeof *e; ++i) printf("%%zu ", e[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof c / sizeof *c; ++i) printf("%%ld ", c[i]);
 printf("\n");
 return 0;}
''' % (offs_c, offs_l, ", ".join(f"(long){c}" for c in codes))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert list(map(int, lines[0].split())) == [ctypes.sizeof(abi.am_commits), ctypes.sizeof(abi.am_commit_log)]
    assert list(map(int, lines[1].split())) == [getattr(abi.am_commits, f).offset for f in cm_f]
    assert list(map(int, lines[2].split())) == [getattr(abi.am_commit_log, f).offset for f in lg_f]
    assert list(map(int, lines[3].split())) == [getattr(abi, c) for c in codes]


def test_commit_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    cm, out, log = abi.am_commits(), abi.am_commit_log(), abi.am_op_log()
    nt, bad = ctypes.c_uint64(), ctypes.c_uint32()
    assert L.am_commit_build(None, 1, None, 64, None, None, None, None) == abi.AM_ERR_INVALID
    assert L.am_commit_build(None, 1, ctypes.byref(cm), 64, ctypes.byref(out), ctypes.byref(log), ctypes.byref(nt),
                             ctypes.byref(bad)) == abi.AM_ERR_INVALID
    assert L.am_vnode_commit_host(None, None) == abi.AM_ERR_INVALID
    assert L.am_vnode_commit_host(None, ctypes.byref(cm)) == abi.AM_ERR_INVALID


def rand_batch(rng, n_dc, n_keys, n_tx, partial=False, txid=False, max_eff=4):
    """A random batch in Commits' input shape: every key keeps one type, each key's effects come
    from one causally plausible stream (randlog.rand_effect)."""
    state = {}
    txs = []
    for t in range(n_tx):
        effs = []
        for _ in range(rng.choice([0, 1, 1, 2, max_eff])):
            k = rng.randrange(n_keys)
            ty = TYPES[k % 5]
            eff = "bad" if rng.random() < 0.03 else randlog.rand_effect(rng, ty, n_dc, state.setdefault(k, {}))
            effs.append((k, ty, eff))
        snap = {d: 100 + t + d for d in range(n_dc) if not (partial and rng.random() < 0.3)}
        txs.append((rng.randrange(n_dc), 200 + 3 * t, snap, (1000 + t) if txid and rng.random() < 0.8 else None, effs))
    return txs


def test_commits_round_trips_encode_effect():
    rng = random.Random(11)
    txs = rand_batch(rng, 3, 7, 40, partial=True, txid=True)
    cm = Commits(3, txs)
    s = cm.as_struct()
    assert (s.n_tx, s.n_eff, s.n_var) == (40, cm.n_eff, cm.n_var) and s.eff_off and s.key and s.var_off
    assert len(cm.eff_off) == 41 and len(cm.var_off) == cm.n_eff + 1 and int(cm.var_off[-1]) == cm.n_var
    q = 0
    for t, (dc, ct, snap, txid, effs) in enumerate(txs):
        assert int(cm.dc[t]) == dc and int(cm.commit_time[t]) == ct
        assert {d: int(cm.snap_vc[t, d]) for d in range(3) if (int(cm.snap_pres[t]) >> d) & 1} == snap
        assert int(cm.txid[t]) == (txid or 0)
        assert int(cm.eff_off[t + 1]) - int(cm.eff_off[t]) == len(effs)
        for k, ty, eff in effs:
            meta, p0, p1, words = cm.effect(q)
            assert (int(cm.key[q]), int(cm.type[q])) == (k, ty)
            if eff == "bad":
                assert meta == abi.AM_META_BAD and words == []
            else:
                kind, a, b, w = encode_effect(ty, eff)
                assert (meta, p0, p1, words) == (abi.make_meta(0, kind), a & (2 ** 64 - 1), b & (2 ** 64 - 1), w)
                assert encode_effect(ty, decode_effect(ty, meta, p0, p1, words)) == (kind, a, b, w)
            q += 1
    assert q == cm.n_eff
    empty = Commits(2, [])
    assert (empty.n_tx, empty.n_eff) == (0, 0) and empty.reference_log()["keys"].size == 0


def test_reference_log_equals_hostlog_of_the_ops_grouped_per_key():
    """A few hundred random batches: the builder's expected output is the HostLog of the same ops
    grouped per key in commit order (what Vnode.insert uploads for the batch)."""
    rng = random.Random(12)
    for it in range(300):
        n_dc = rng.choice([1, 2, 3, 8])
        txs = rand_batch(rng, n_dc, rng.choice([1, 3, 17]), rng.randint(1, 25), partial=it % 3 == 0, txid=it % 2 == 0)
        cm = Commits(n_dc, txs)
        ref = cm.reference_log()
        by_key = cm.ops_by_key()
        keys = sorted(by_key)
        assert list(ref["keys"]) == keys
        n = cm.n_eff
        assert sorted(ref["src"]) == list(range(n))
        if not keys:
            continue
        log = HostLog(n_dc, [by_key[k] for k in keys])
        assert np.array_equal(ref["key_off"], log.key_off)
        assert np.array_equal(ref["key_type"], log.key_type[:len(keys)])
        assert np.array_equal(ref["key_flags"], log.key_flags[:len(keys)])
        for c in ("op_meta", "commit_time", "p0", "p1"):
            assert np.array_equal(ref[c], getattr(log, c)[:n]), c
        assert np.array_equal(ref["snap_vc"], log.snap_vc[:, :n])
        assert (ref["snap_pres"] is None) == (log.snap_pres is None)
        if ref["snap_pres"] is not None:
            assert np.array_equal(ref["snap_pres"], log.snap_pres[:n])
        assert (ref["op_txid"] is None) == (log.op_txid is None)
        if ref["op_txid"] is not None:
            assert np.array_equal(ref["op_txid"], log.op_txid[:n])
        assert np.array_equal(ref["var_off"], log.var_off)
        assert np.array_equal(ref["var_data"], log.var_data[:log.n_var])
        # src names the batch effect of every op; a key's ops keep (transaction, effect) order
        for i in range(len(keys)):
            run = [int(x) for x in ref["src"][int(ref["key_off"][i]):int(ref["key_off"][i + 1])]]
            assert run == sorted(run) and all(int(cm.key[q]) == keys[i] for q in run)


def test_reference_log_marks_mixed_types_and_keeps_one_transactions_order():
    cm = Commits(2, [(0, 10, {0: 1, 1: 1}, None, [(4, abi.AM_PN, 1), (4, abi.AM_PN, 2), (9, abi.AM_PN, 5)]),
                     (1, 11, {0: 2, 1: 2}, None, [(9, abi.AM_LWW, (3, 4)), (4, abi.AM_PN, 3)])])
    ref = cm.reference_log()
    assert list(ref["keys"]) == [4, 9] and list(ref["key_off"]) == [0, 3, 5]
    assert list(ref["src"]) == [0, 1, 4, 2, 3] and list(ref["p0"][:3]) == [1, 2, 3]
    assert list(ref["key_type"]) == [abi.AM_PN, abi.AM_PN] and list(ref["key_flags"]) == [0, abi.AM_KEY_MIXED_TYPES]
    assert list(ref["op_meta"]) == [0, 0, 1, 0, 1] and list(ref["commit_time"]) == [10, 10, 11, 10, 11]
