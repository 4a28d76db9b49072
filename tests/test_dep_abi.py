"""CPU checks of the dependency buffer's boundary: include/antidote_mat.h declares the am_dep calls and
the library exports them with abi.py's prototypes, am_dep_txns has the header's layout, the AM_DEP_BAD_*
values agree, the ABI version is still 15, every call rejects missing arguments before it touches a
device, and the host encoder (oplog.DepTxns) round-trips its tuples."""
import ctypes
import os
import subprocess
import tempfile

from antidote_amd import abi
from antidote_amd.oplog import DepTxns
from tests.test_abi import HDR, ROOT, declared_functions

DEP_FNS = ["am_dep_create", "am_dep_destroy", "am_dep_reserve", "am_dep_set_clock", "am_dep_set_drop_ping", "am_dep_clear",
           "am_dep_deliver", "am_dep_deliver_host", "am_dep_clocks", "am_dep_clock_host", "am_dep_queue", "am_dep_size",
           "am_dep_stats"]
U64_MAX = 2 ** 64 - 1


def test_header_declares_and_library_exports_the_dep_calls():
    fns = declared_functions()
    L = abi.lib()
    sigs = {n: (r, a) for n, r, a in abi.SIGNATURES}
    for fn in DEP_FNS:
        assert fn in fns, fn
        assert fn in sigs, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes == sigs[fn][1] and getattr(L, fn).restype is sigs[fn][0]
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_argument_counts_match_the_header():
    hdr = open(HDR).read()
    sigs = {n: a for n, _, a in abi.SIGNATURES}
    for fn in DEP_FNS:
        i = hdr.index("int " + fn + "(")
        args = hdr[i:hdr.index(");", i)].split("(", 1)[1]
        assert len(args.split(",")) == len(sigs[fn]), fn


def test_dep_txns_layout_and_bad_bits_match_header():
    fields = [f for f, _ in abi.am_dep_txns._fields_]
    offs = ", ".join(f"offsetof(am_dep_txns, {f})" for f in fields)
    codes = ["AM_DEP_BAD_PART", "AM_DEP_BAD_DC", "AM_DEP_BAD_TIME"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 size_t u[] = {%s}; long c[] = {%s};
 printf("%%zu\n", sizeof(am_dep_txns));
 for (size_t i = 0; i < sizeof u / sizeof *u; ++i) printf("%%zu ", u[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof c / sizeof *c; ++i) printf("%%ld ", c[i]);
 printf("\n");
 return 0;}
''' % (offs, ", ".join(f"(long){c}" for c in codes))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == ctypes.sizeof(abi.am_dep_txns)
    assert list(map(int, lines[1].split())) == [getattr(abi.am_dep_txns, f).offset for f in fields]
    assert list(map(int, lines[2].split())) == [getattr(abi, c) for c in codes] == [1, 2, 4]


def test_dep_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    out, u, w = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
    tx = abi.am_dep_txns()
    buf = (ctypes.c_uint64 * 4)()
    inv = abi.AM_ERR_INVALID
    assert L.am_dep_create(None, 3, 0, 1, 8, None, ctypes.byref(out)) == inv and not out.value
    assert L.am_dep_destroy(None) == abi.AM_OK  # as every destroy of the library: nothing to do
    assert L.am_dep_reserve(None, 8) == inv
    assert L.am_dep_set_clock(None, 0, buf, 0) == inv
    assert L.am_dep_set_drop_ping(None, 1) == inv
    assert L.am_dep_clear(None) == inv
    for fn in (L.am_dep_deliver, L.am_dep_deliver_host):
        assert fn(None, ctypes.byref(tx), 0, 4, buf, buf, ctypes.byref(u), ctypes.byref(w)) == inv
        assert fn(None, None, 0, 0, None, None, None, None) == inv
    assert L.am_dep_clocks(None, ctypes.byref(out), ctypes.byref(out)) == inv
    assert L.am_dep_clock_host(None, 0, buf, ctypes.byref(w)) == inv
    assert L.am_dep_queue(None, 0, 0, 4, buf, ctypes.byref(u)) == inv
    assert L.am_dep_size(None, None, None) == inv
    assert L.am_dep_stats(None, None) == inv


def test_dep_txns_round_trips_its_input():
    txs = [(0, 1, 5, {2: 9}, False, 7), (3, 0, U64_MAX, {0: U64_MAX, 1: 1}, False, U64_MAX), (2 ** 32 - 1, 31, 0, {}, True, 0)]
    b = DepTxns(32, txs)
    assert b.transactions() == txs
    s = b.as_struct()
    assert s.n_tx == 3 and s.part and s.dc and s.timestamp and s.snap_vc and s.ping and s.tag
    assert b.snap_vc.shape == (3, 32) and int(b.snap_vc[0, 2]) == 9 and list(b.ping) == [0, 0, 1]
    q = DepTxns.from_columns(32, b.part, b.dc, b.timestamp, b.snap_vc, b.ping, b.tag)
    assert q.transactions() == txs
    empty = DepTxns(3, [])
    assert empty.n_tx == 0 and empty.transactions() == [] and empty.as_struct().n_tx == 0
