"""CPU checks of the subscriber buffer's boundary: include/antidote_mat.h declares the am_sub calls and
the library exports them with abi.py's prototypes, am_sub_rows and am_sub_gaps have the header's layout,
the AM_SUB_* values agree, the ABI version is still 15, every call rejects missing arguments before it
touches a device, and the host encoder (oplog.SubRows) round-trips its tuples."""
import ctypes
import os
import subprocess
import tempfile

from antidote_amd import abi
from antidote_amd.oplog import SubRows
from tests.test_abi import HDR, ROOT, declared_functions

SUB_FNS = ["am_sub_create", "am_sub_destroy", "am_sub_reserve", "am_sub_clear", "am_sub_set_last", "am_sub_set_reachable",
           "am_sub_process", "am_sub_process_host", "am_sub_deliver", "am_sub_deliver_host", "am_sub_stream", "am_sub_size",
           "am_sub_stats"]
U64_MAX = 2 ** 64 - 1


def test_header_declares_and_library_exports_the_sub_calls():
    fns = declared_functions()
    L = abi.lib()
    sigs = {n: (r, a) for n, r, a in abi.SIGNATURES}
    for fn in SUB_FNS:
        assert fn in fns, fn
        assert fn in sigs, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes == sigs[fn][1] and getattr(L, fn).restype is sigs[fn][0]
    assert sorted(f for f in fns if f.startswith("am_sub_")) == sorted(SUB_FNS)
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_argument_counts_match_the_header():
    hdr = open(HDR).read()
    sigs = {n: a for n, _, a in abi.SIGNATURES}
    for fn in SUB_FNS:
        i = hdr.index("int " + fn + "(")
        args = hdr[i:hdr.index(");", i)].split("(", 1)[1]
        assert len(args.split(",")) == len(sigs[fn]), fn


def test_sub_structs_layout_and_constants_match_header():
    rows = [f for f, _ in abi.am_sub_rows._fields_]
    gaps = [("from" if f == "from_" else f) for f, _ in abi.am_sub_gaps._fields_]
    offs = ", ".join([f"offsetof(am_sub_rows, {f})" for f in rows] + [f"offsetof(am_sub_gaps, {f})" for f in gaps])
    codes = ["AM_SUB_TXN", "AM_SUB_RESP_TXN", "AM_SUB_RESP_END", "AM_SUB_BAD_PART", "AM_SUB_BAD_DC", "AM_SUB_BAD_TIME",
             "AM_SUB_BAD_KIND", "AM_SUB_NORMAL", "AM_SUB_BUFFERING"]
    order = ["AM_SUB_N_DELIVERED", "AM_SUB_N_GAPS", "AM_SUB_N_DROPPED", "AM_SUB_N_UNEXPECTED", "AM_SUB_N_QUEUED"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 size_t u[] = {%s}; long c[] = {%s};
 printf("%%zu %%zu\n", sizeof(am_sub_rows), sizeof(am_sub_gaps));
 for (size_t i = 0; i < sizeof u / sizeof *u; ++i) printf("%%zu ", u[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof c / sizeof *c; ++i) printf("%%ld ", c[i]);
 printf("\n");
 return 0;}
''' % (offs, ", ".join(f"(long){c}" for c in codes + order))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert list(map(int, lines[0].split())) == [ctypes.sizeof(abi.am_sub_rows), ctypes.sizeof(abi.am_sub_gaps)]
    assert list(map(int, lines[1].split())) == [getattr(abi.am_sub_rows, f).offset for f in rows] + \
        [getattr(abi.am_sub_gaps, f).offset for f, _ in abi.am_sub_gaps._fields_]
    vals = list(map(int, lines[2].split()))
    assert vals[:9] == [getattr(abi, c) for c in codes] == [0, 1, 2, 1, 2, 4, 8, 0, 1]
    assert vals[9:] == [0, 1, 2, 3, 4] and abi.SUB_COUNTS == ("delivered", "gaps", "dropped", "unexpected", "queued")
    # the bits a row shares with am_dep keep am_dep's values
    assert (abi.AM_SUB_BAD_PART, abi.AM_SUB_BAD_DC, abi.AM_SUB_BAD_TIME) == (abi.AM_DEP_BAD_PART, abi.AM_DEP_BAD_DC, abi.AM_DEP_BAD_TIME)


def test_sub_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    out, u, w = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
    rows, cols, gaps = abi.am_sub_rows(), abi.am_dep_txns(), abi.am_sub_gaps()
    buf = (ctypes.c_uint64 * 8)()
    inv = abi.AM_ERR_INVALID
    assert L.am_sub_create(None, 3, 1, 8, 1, ctypes.byref(out)) == inv and not out.value
    assert L.am_sub_destroy(None) == abi.AM_OK  # as every destroy of the library: nothing to do
    assert L.am_sub_reserve(None, 8) == inv
    assert L.am_sub_clear(None) == inv
    assert L.am_sub_set_last(None, 0, 0, 1) == inv
    assert L.am_sub_set_reachable(None, 1) == inv
    for fn in (L.am_sub_process, L.am_sub_process_host):
        assert fn(None, ctypes.byref(rows), 4, buf, ctypes.byref(cols), 4, ctypes.byref(gaps), buf, ctypes.byref(w)) == inv
        assert fn(None, None, 0, None, None, 0, None, None, None) == inv
    for fn in (L.am_sub_deliver, L.am_sub_deliver_host):
        assert fn(None, None, ctypes.byref(rows), 0, 4, buf, buf, ctypes.byref(u), 4, ctypes.byref(gaps), buf, ctypes.byref(w)) == inv
        assert fn(None, None, None, 0, 0, None, None, None, 0, None, None, None) == inv
    assert L.am_sub_stream(None, 0, 0, ctypes.byref(u), ctypes.byref(w), 4, buf, ctypes.byref(u)) == inv
    assert L.am_sub_size(None, None, None) == inv
    assert L.am_sub_stats(None, None) == inv


def test_sub_rows_round_trips_its_input():
    rows = [(abi.AM_SUB_TXN, 0, 1, 5, 9, 7, {2: 9}, False, 7),
            (abi.AM_SUB_RESP_TXN, 3, 0, 2 ** 63, U64_MAX, U64_MAX, {0: U64_MAX, 1: 1}, False, U64_MAX),
            (abi.AM_SUB_RESP_END, 2 ** 32 - 1, 31, 0, 0, 0, {}, False, 0),
            (abi.AM_SUB_TXN, 1, 2, 4, 12345, 0, {}, True, 3)]
    b = SubRows(32, rows)
    assert b.rows() == rows
    s = b.as_struct()
    assert s.n_rows == 4 and all(getattr(s, f) for f, _ in abi.am_sub_rows._fields_)
    assert b.snap_vc.shape == (4, 32) and int(b.snap_vc[0, 2]) == 9 and list(b.ping) == [0, 0, 0, 1] and list(b.kind) == [0, 1, 2, 0]
    q = SubRows.from_columns(32, b.kind, b.part, b.dc, b.prev_opid, b.last_opid, b.timestamp, b.snap_vc, b.ping, b.tag)
    assert q.rows() == rows
    empty = SubRows(3, [])
    assert empty.n_rows == 0 and empty.rows() == [] and empty.as_struct().n_rows == 0
