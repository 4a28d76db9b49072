"""CPU checks of the certifier's boundary: include/antidote_mat.h declares the am_cert calls and the
library exports them, am_prepares / am_finishes have the header's layout, the two new statuses are 7
and 8, the ABI version is still 15, every call rejects missing arguments before it touches a device,
and the host encoders (oplog.Prepares / Finishes) round-trip CertSim's tuples."""
import ctypes
import os
import subprocess
import tempfile

from antidote_amd import abi
from antidote_amd.oplog import Finishes, Prepares
from tests import certsim
from tests.test_abi import HDR, ROOT, declared_functions

CERT_FNS = ["am_cert_create", "am_cert_destroy", "am_cert_reserve", "am_cert_prepare", "am_cert_prepare_host",
            "am_cert_finish", "am_cert_finish_host", "am_cert_read_ready", "am_cert_read_ready_host",
            "am_cert_min_prepared", "am_cert_key_info", "am_cert_size", "am_cert_stats"]
U64_MAX = 2 ** 64 - 1


def test_header_declares_and_library_exports_the_cert_calls():
    fns = declared_functions()
    L = abi.lib()
    names = {n for n, _, _ in abi.SIGNATURES}
    for fn in CERT_FNS:
        assert fn in fns, fn
        assert fn in names, fn
        assert hasattr(L, fn), fn
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_prepares_and_finishes_layout_and_codes_match_header():
    pr_f = [f for f, _ in abi.am_prepares._fields_]
    fi_f = [f for f, _ in abi.am_finishes._fields_]
    offs_p = ", ".join(f"offsetof(am_prepares, {f})" for f in pr_f)
    offs_f = ", ".join(f"offsetof(am_finishes, {f})" for f in fi_f)
    codes = ["AM_ERR_WRITE_CONFLICT", "AM_ERR_NO_UPDATES", "AM_CERT_SPIN_WAIT_MS", "AM_ERR_CAPACITY", "AM_ERR_INVALID"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 size_t u[] = {%s}; size_t e[] = {%s}; long c[] = {%s};
 printf("%%zu %%zu\n", sizeof(am_prepares), sizeof(am_finishes));
 for (size_t i = 0; i < sizeof u / sizeof *u; ++i) printf("%%zu ", u[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof e / sizeof *e; ++i) printf("%%zu ", e[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof c / sizeof *c; ++i) printf("%%ld ", c[i]);
 printf("\n");
 return 0;}
''' % (offs_p, offs_f, ", ".join(f"(long){c}" for c in codes))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert list(map(int, lines[0].split())) == [ctypes.sizeof(abi.am_prepares), ctypes.sizeof(abi.am_finishes)]
    assert list(map(int, lines[1].split())) == [getattr(abi.am_prepares, f).offset for f in pr_f]
    assert list(map(int, lines[2].split())) == [getattr(abi.am_finishes, f).offset for f in fi_f]
    assert list(map(int, lines[3].split())) == [getattr(abi, c) for c in codes]


def test_status_values_are_the_checkers():
    assert (abi.AM_ERR_WRITE_CONFLICT, abi.AM_ERR_NO_UPDATES) == (7, 8)
    assert (abi.AM_OK, abi.AM_ERR_WRITE_CONFLICT, abi.AM_ERR_NO_UPDATES) == (certsim.OK, certsim.WRITE_CONFLICT,
                                                                            certsim.NO_UPDATES)
    assert abi.AM_CERT_SPIN_WAIT_MS == certsim.SPIN_WAIT_MS


def test_cert_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    out, u, i = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    pr, fi = abi.am_prepares(), abi.am_finishes()
    st = (ctypes.c_int32 * 4)()
    inv = abi.AM_ERR_INVALID
    assert L.am_cert_create(None, 8, 8, 1, ctypes.byref(out)) == inv and not out.value
    assert L.am_cert_create(None, 8, 8, 1, None) == inv
    assert L.am_cert_destroy(None) == abi.AM_OK  # as every destroy of the library: nothing to do
    assert L.am_cert_reserve(None, 8, 8) == inv
    for fn in (L.am_cert_prepare, L.am_cert_prepare_host):
        assert fn(None, ctypes.byref(pr), st) == inv
        assert fn(None, None, None) == inv
    for fn in (L.am_cert_finish, L.am_cert_finish_host):
        assert fn(None, ctypes.byref(fi), st) == inv
        assert fn(None, None, None) == inv
    for fn in (L.am_cert_read_ready, L.am_cert_read_ready_host):
        assert fn(None, 1, st, st, 0, st) == inv
        assert fn(None, 0, None, None, 0, None) == inv
    assert L.am_cert_min_prepared(None, ctypes.byref(u), ctypes.byref(i)) == inv
    assert L.am_cert_key_info(None, 0, ctypes.byref(u), 0, None, None, ctypes.byref(u)) == inv
    assert L.am_cert_size(None, None, None, None, None) == inv
    assert L.am_cert_stats(None, None, None, None) == inv


def test_prepares_round_trips_its_input():
    txs = [(7, 10, 20, True, [3, 4]), (U64_MAX, 0, U64_MAX, False, []), (0, U64_MAX, 0, True, [5, 5, 5, 5]),
           (9, 1, 2, False, [0, U64_MAX])]
    p = Prepares(txs)
    assert p.transactions() == txs
    s = p.as_struct()
    assert (s.n_tx, s.n_pairs) == (4, 8) and s.txid and s.start_time and s.prepare_time and s.certify and s.key_off and s.key
    assert list(p.key_off) == [0, 2, 2, 6, 8] and list(p.key[:8]) == [3, 4, 5, 5, 5, 5, 0, U64_MAX]
    assert list(p.certify) == [1, 0, 1, 0]
    empty = Prepares([])
    assert (empty.n_tx, empty.n_pairs) == (0, 0) and list(empty.key_off) == [0] and empty.transactions() == []
    assert empty.as_struct().n_tx == 0
    q = Prepares.from_columns(p.txid, p.start_time, p.prepare_time, p.certify, p.key_off, p.key[:8])
    assert q.transactions() == txs and (q.n_tx, q.n_pairs) == (4, 8)
    only_empty = Prepares([(1, 2, 3, True, [])])
    assert (only_empty.n_tx, only_empty.n_pairs) == (1, 0) and list(only_empty.key_off) == [0, 0]
    assert only_empty.transactions() == [(1, 2, 3, True, [])]


def test_finishes_round_trips_its_input():
    txs = [(7, 30, True, [3, 4]), (U64_MAX, U64_MAX, False, []), (0, 0, True, [5, 5, 5, 5])]
    f = Finishes(txs)
    assert f.transactions() == txs
    s = f.as_struct()
    assert (s.n_tx, s.n_pairs) == (3, 6) and s.txid and s.commit_time and s.committed and s.key_off and s.key
    assert list(f.key_off) == [0, 2, 2, 6] and list(f.committed) == [1, 0, 1]
    assert Finishes.from_columns(f.txid, f.commit_time, f.committed, f.key_off, f.key[:6]).transactions() == txs
    empty = Finishes([])
    assert (empty.n_tx, empty.n_pairs) == (0, 0) and list(empty.key_off) == [0] and empty.transactions() == []
    only_empty = Finishes([(1, 2, False, [])])
    assert only_empty.transactions() == [(1, 2, False, [])] and list(only_empty.key_off) == [0, 0]
