"""CPU checks of the read-your-writes boundary (ABI 15): include/antidote_mat.h declares
am_materialize_eager / _host and am_read_objects_ws_host / _submit, the library exports them,
am_writeset has the header's layout, and the host encoder of a write set (oplog.WriteSet)
writes exactly what encode_effect gives."""
import ctypes
import os
import subprocess
import tempfile

from antidote_amd import abi
from antidote_amd.oplog import WriteSet, encode_effect
from tests.test_abi import HDR, ROOT, declared_functions

EAGER_FNS = ["am_materialize_eager", "am_materialize_eager_host", "am_read_objects_ws_host",
             "am_read_objects_ws_submit"]


def test_header_declares_and_library_exports_the_eager_calls():
    fns = declared_functions()
    L = abi.lib()
    names = {n for n, _, _ in abi.SIGNATURES}
    for fn in EAGER_FNS:
        assert fn in fns, fn
        assert fn in names, fn
        assert hasattr(L, fn), fn
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_writeset_layout_and_limits_match_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 printf("%zu\n", sizeof(am_writeset));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(am_writeset, n_ws), offsetof(am_writeset, n_eff),
        offsetof(am_writeset, n_var), offsetof(am_writeset, row), offsetof(am_writeset, type),
        offsetof(am_writeset, eff_off), offsetof(am_writeset, eff_meta), offsetof(am_writeset, p0),
        offsetof(am_writeset, p1), offsetof(am_writeset, var_off), offsetof(am_writeset, var_data));
 printf("%u %u %u %u %u %u %u\n", AM_EAGER_MAX_BIRTHS, AM_EAGER_MAX_KILLS, AM_EAGER_MAX_EFFECTS, AM_EAGER_TILE_WAVE,
        AM_EAGER_TILE_WG, AM_EAGER_SMALL_WORDS, AM_EAGER_SMALL_SLOTS);
 return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    W = abi.am_writeset
    assert int(lines[0]) == ctypes.sizeof(W)
    assert list(map(int, lines[1].split())) == [getattr(W, f).offset for f, _ in W._fields_]
    assert list(map(int, lines[2].split())) == [abi.AM_EAGER_MAX_BIRTHS, abi.AM_EAGER_MAX_KILLS,
                                                abi.AM_EAGER_MAX_EFFECTS, abi.AM_EAGER_TILE_WAVE,
                                                abi.AM_EAGER_TILE_WG, abi.AM_EAGER_SMALL_WORDS,
                                                abi.AM_EAGER_SMALL_SLOTS]
    # at least the LDS tier's lists (am_sets.hip BCAP / KCAP)
    assert abi.AM_EAGER_MAX_BIRTHS >= 1024 and abi.AM_EAGER_MAX_KILLS >= 2048


def test_eager_calls_reject_a_missing_context_without_a_gpu():
    L = abi.lib()
    ws, vin, vout = abi.am_writeset(), abi.am_values(), abi.am_values()
    st = (ctypes.c_int32 * 1)()
    for fn in (L.am_materialize_eager, L.am_materialize_eager_host):
        assert fn(None, 1, None, None, None, None, None) == abi.AM_ERR_INVALID
        assert fn(None, 1, ctypes.byref(ws), ctypes.byref(vin), None, ctypes.byref(vout), st) == abi.AM_ERR_INVALID
    assert L.am_read_objects_ws_host(None, 1, None, None, None, None, None) == abi.AM_ERR_INVALID
    t = ctypes.c_void_p()
    assert L.am_read_objects_ws_submit(None, 1, None, None, None, None, None, ctypes.byref(t)) == abi.AM_ERR_INVALID


def test_writeset_encoder_round_trips_encode_effect():
    entries = [
        (4, abi.AM_PN, [5, -3, -(1 << 63)]),
        (0, abi.AM_LWW, [(7, 2), (7, 9)]),
        (9, abi.AM_AWSET, [[(1, [101, 102], [7]), (5, [], [8, 9])], [], [(2, [103], [])]]),
        (2, abi.AM_MVREG, [("assign", 3, 501, [400, 401]), ("reset", [501]), "bad"]),
        (7, abi.AM_BCOUNTER, [("increment", 4, 1), ("decrement", 0, 2), ("transfer", 3, 0, 2)]),
        (1, abi.AM_PN, []),
    ]
    ws = WriteSet(entries)
    s = ws.as_struct()
    assert (s.n_ws, s.n_eff, s.n_var) == (6, sum(len(e) for _, _, e in entries), ws.n_var)
    assert list(ws.row) == [4, 0, 9, 2, 7, 1] and list(ws.type) == [t for _, t, _ in entries]
    assert list(ws.eff_off) == [0, 3, 5, 8, 11, 14, 14]
    assert len(ws.var_off) == ws.n_eff + 1 and int(ws.var_off[-1]) == ws.n_var
    for i, (_, t, effs) in enumerate(entries):
        for j, eff in enumerate(effs):
            meta, p0, p1, words = ws.effect(i, j)
            if eff == "bad":
                assert meta & abi.AM_META_BAD and words == []
                continue
            kind, a, b, w = encode_effect(t, eff)
            assert meta == abi.make_meta(0, kind, False)
            assert (p0, p1, words) == (a & (2**64 - 1), b & (2**64 - 1), w)
    # an empty write set still has every column
    e = WriteSet([])
    es = e.as_struct()
    assert es.n_ws == 0 and es.n_eff == 0 and list(e.eff_off) == [0] and es.row and es.var_off
