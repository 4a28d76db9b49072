"""CPU checks of the downstream-generation boundary: include/antidote_mat.h declares
am_generate_downstream / _host and am_update_objects_host / _submit, the library exports them,
am_updates / am_effects have the header's layout, AM_ERR_NO_PERMISSIONS is 6 on both sides, the
calls reject missing arguments before touching a device, and the host encoder / decoder pair
(oplog.Updates, oplog.Effects) sorts set elements and round-trips encode_effect."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from antidote_amd import abi
from antidote_amd.oplog import Effects, Updates, WriteSet, decode_effect, encode_effect
from tests.test_abi import HDR, ROOT, declared_functions

DS_FNS = ["am_generate_downstream", "am_generate_downstream_host", "am_update_objects_host",
          "am_update_objects_submit"]


def test_header_declares_and_library_exports_the_downstream_calls():
    fns = declared_functions()
    L = abi.lib()
    names = {n for n, _, _ in abi.SIGNATURES}
    for fn in DS_FNS:
        assert fn in fns, fn
        assert fn in names, fn
        assert hasattr(L, fn), fn
    assert L.am_abi_version() == 15
    assert "#define AM_ABI_VERSION 15" in open(HDR).read()


def test_updates_and_effects_layout_and_codes_match_header():
    up_f = [f for f, _ in abi.am_updates._fields_]
    ef_f = [f for f, _ in abi.am_effects._fields_]
    offs_u = ", ".join(f"offsetof(am_updates, {f})" for f in up_f)
    offs_e = ", ".join(f"offsetof(am_effects, {f})" for f in ef_f)
    codes = ["AM_UP_PN_INCREMENT", "AM_UP_PN_DECREMENT", "AM_UP_LWW_ASSIGN", "AM_UP_AW_ADD", "AM_UP_AW_REMOVE",
             "AM_UP_AW_RESET", "AM_UP_MV_ASSIGN", "AM_UP_MV_RESET", "AM_UP_BC_INCREMENT", "AM_UP_BC_DECREMENT",
             "AM_UP_BC_TRANSFER", "AM_DS_TILE_WG", "AM_ERR_NO_PERMISSIONS"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "antidote_mat.h"
int main(void){
 size_t u[] = {%s}; size_t e[] = {%s}; long c[] = {%s};
 printf("%%zu %%zu\n", sizeof(am_updates), sizeof(am_effects));
 for (size_t i = 0; i < sizeof u / sizeof *u; ++i) printf("%%zu ", u[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof e / sizeof *e; ++i) printf("%%zu ", e[i]);
 printf("\n");
 for (size_t i = 0; i < sizeof c / sizeof *c; ++i) printf("%%ld ", c[i]);
 printf("\n");
 return 0;}
''' % (offs_u, offs_e, ", ".join(f"(long){c}" for c in codes))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert list(map(int, lines[0].split())) == [ctypes.sizeof(abi.am_updates), ctypes.sizeof(abi.am_effects)]
    assert list(map(int, lines[1].split())) == [getattr(abi.am_updates, f).offset for f in up_f]
    assert list(map(int, lines[2].split())) == [getattr(abi.am_effects, f).offset for f in ef_f]
    assert list(map(int, lines[3].split())) == [getattr(abi, c) for c in codes]
    assert abi.AM_ERR_NO_PERMISSIONS == 6
    assert re.search(r"AM_ERR_NO_PERMISSIONS\s*=\s*6\s*,", open(HDR).read())


def test_downstream_calls_reject_missing_arguments_without_a_gpu():
    L = abi.lib()
    up, vin, eff, b = abi.am_updates(), abi.am_values(), abi.am_effects(), abi.am_read_batch()
    st = (ctypes.c_int32 * 1)()
    for fn in (L.am_generate_downstream, L.am_generate_downstream_host):
        assert fn(None, 1, None, None, None, None, None) == abi.AM_ERR_INVALID
        assert fn(None, 1, ctypes.byref(up), ctypes.byref(vin), None, ctypes.byref(eff), st) == abi.AM_ERR_INVALID
    base = (ctypes.c_uint64 * 2)(0, 1)
    assert L.am_update_objects_host(None, 1, None, None, None, None, None, None, None, None) == abi.AM_ERR_INVALID
    assert L.am_update_objects_host(None, 1, base, None, ctypes.byref(b), None, None, ctypes.byref(up), ctypes.byref(eff),
                                    st) == abi.AM_ERR_INVALID
    t = ctypes.c_void_p()
    assert L.am_update_objects_submit(None, 1, None, None, None, None, None, None, None, None,
                                      ctypes.byref(t)) == abi.AM_ERR_INVALID
    assert L.am_update_objects_submit(None, 1, base, None, ctypes.byref(b), None, None, ctypes.byref(up),
                                      ctypes.byref(eff), st, ctypes.byref(t)) == abi.AM_ERR_INVALID
    assert not t.value


def test_updates_encoder_sorts_and_dedupes_set_elements():
    fresh = iter(range(900, 1000))
    ups = Updates([
        (3, abi.AM_AWSET, ("add_all", [9, 2, 9, 5, 2])),
        (0, abi.AM_AWSET, ("remove_all", [7, 7, 1, 2 ** 64 - 1, 1])),
        (5, abi.AM_AWSET, ("add", 4)),
        (6, abi.AM_AWSET, ("remove", 4)),
        (7, abi.AM_AWSET, ("reset",)),
        (1, abi.AM_MVREG, ("assign", 77)),
        (2, abi.AM_MVREG, ("reset",)),
        (4, abi.AM_PN, ("decrement", 5)),
        (8, abi.AM_LWW, ("assign", 123456, 9)),
        (9, abi.AM_BCOUNTER, ("increment", (-4, 2))),
        (10, abi.AM_BCOUNTER, ("transfer", (3, 1, 2))),
    ], tokens=lambda: next(fresh))
    s = ups.as_struct()
    assert (s.n_up, s.n_var) == (11, ups.n_var) and len(ups.var_off) == 12 and int(ups.var_off[-1]) == ups.n_var
    w = lambda i: [int(x) for x in ups.var_data[int(ups.var_off[i]):int(ups.var_off[i + 1])]]  # noqa: E731
    assert w(0) == [2, 900, 5, 901, 9, 902] and ups.tokens[0] == [900, 901, 902]
    assert w(1) == [1, 7, 2 ** 64 - 1]
    assert w(2) == [4, 903] and w(3) == [4] and w(4) == []
    assert list(ups.op) == [abi.AM_UP_AW_ADD, abi.AM_UP_AW_REMOVE, abi.AM_UP_AW_ADD, abi.AM_UP_AW_REMOVE,
                            abi.AM_UP_AW_RESET, abi.AM_UP_MV_ASSIGN, abi.AM_UP_MV_RESET, abi.AM_UP_PN_DECREMENT,
                            abi.AM_UP_LWW_ASSIGN, abi.AM_UP_BC_INCREMENT, abi.AM_UP_BC_TRANSFER]
    assert (int(ups.a0[5]), int(ups.a1[5])) == (77, 904) and ups.tokens[5] == [904]
    assert int(ups.a0[7]) == 5 and (int(ups.a0[8]), int(ups.a1[8])) == (123456, 9)
    assert int(ups.a0[9]) == 2 ** 64 - 4 and int(ups.a1[9]) == 2
    assert int(ups.a0[10]) == 3 and int(ups.a1[10]) == 2 | (1 << 8)
    assert list(ups.row) == [3, 0, 5, 6, 7, 1, 2, 4, 8, 9, 10]


def test_effects_as_writeset_round_trips_encode_effect():
    """One effect of every type and op, written into am_effects' columns as the device writes
    them, decodes to the shape encode_effect takes and leaves as the write set WriteSet encodes."""
    cases = [
        (abi.AM_PN, ("increment", 5), 5),
        (abi.AM_PN, ("decrement", 5), -5),
        (abi.AM_LWW, ("assign", 1234, 8), (1234, 8)),
        (abi.AM_AWSET, ("raw", abi.AM_UP_AW_ADD, 0, 0, [2, 50, 7, 51]), [(2, [50], [11, 12]), (7, [51], [])]),
        (abi.AM_AWSET, ("remove_all", [2, 7]), [(2, [], [11, 12]), (7, [], [])]),
        (abi.AM_AWSET, ("reset",), [(2, [], [11, 12]), (3, [], [13])]),
        (abi.AM_MVREG, ("raw", abi.AM_UP_MV_ASSIGN, 4, 60, []), ("assign", 4, 60, [21, 22])),
        (abi.AM_MVREG, ("reset",), ("reset", [21, 22])),
        (abi.AM_BCOUNTER, ("increment", (6, 1)), ("increment", 6, 1)),
        (abi.AM_BCOUNTER, ("decrement", (6, 2)), ("decrement", 6, 2)),
        (abi.AM_BCOUNTER, ("transfer", (6, 0, 2)), ("transfer", 6, 0, 2)),
    ]
    ups = Updates([(2 * i + 1, t, u) for i, (t, u, _) in enumerate(cases)])
    eff = Effects(ups, 64)
    var = []
    for i, (t, _, e) in enumerate(cases):
        kind, p0, p1, words = encode_effect(t, e)
        eff.eff_meta[i], eff.p0[i], eff.p1[i] = abi.make_meta(0, kind), p0 & (2 ** 64 - 1), p1 & (2 ** 64 - 1)
        eff.eff_off[i + 1] = i + 1
        var += words
        eff.var_off[i + 1] = len(var)
        assert decode_effect(t, abi.make_meta(0, kind), p0, p1, words) == e
    eff.var_data[:len(var)] = var
    eff.n_var[0] = len(var)
    eff.status[:] = 0
    assert eff.effects() == [e for _, _, e in cases]
    ws = eff.as_writeset()
    ref = WriteSet([(2 * i + 1, t, [e]) for i, (t, _, e) in enumerate(cases)])
    assert (ws.n_ws, ws.n_eff, ws.n_var) == (ref.n_ws, ref.n_eff, ref.n_var)
    for c in ("row", "type", "eff_off", "eff_meta", "p0", "p1", "var_off"):
        assert np.array_equal(getattr(ws, c), getattr(ref, c)), c
    assert np.array_equal(ws.var_data[:ws.n_var], ref.var_data[:ref.n_var])
    s = ws.as_struct()
    assert s.n_ws == len(cases) and s.row and s.var_off
    # a failed update leaves as an effect Type:update/2 raises on
    eff.status[3] = abi.AM_ERR_CAPACITY
    eff.eff_meta[3] = abi.AM_META_BAD
    assert eff.effect(3) == ("error", abi.AM_ERR_CAPACITY)
    assert eff.as_writeset().entries[3][2] == ["bad"]
