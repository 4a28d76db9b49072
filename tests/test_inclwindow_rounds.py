"""CPU replay of the schedule the lag instantiation of the inclusion pass walks a read in
(antidote_amd/csrc/am_group_split.h k_grp_incl, LAG): segments of 1024 ops, newest first; per
segment the bound that needs no load over the whole segment, then every op's class, then the
window ops newest first in rounds of 64, one op per lane, cmax raised from the lanes' maxima after
each round and the next round's entries classified again before they would load; the bound is
carried from a segment to the older ones.  The replay is numpy over the functions of am_inclwin.h
(a C shim loaded through ctypes) and is compared with the direct evaluation of all D entries:
inclusion bits and per-DC maxima, on random logs and at the edges of the rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, WAVE, LAGMAX, ESC, TMAX = 1024, 64, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFE

SHIM = r'''
#include "am_inclwin.h"
void iw_setup(am_inclwin *w, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never) { am_iw_setup(w, thr, lb, nd, never); }
uint32_t iw_lim(int64_t v) { return am_iw_lim(v); }
uint32_t iw_in_lim(const am_inclwin *w) { return am_iw_in_lim(w); }
void iw_raise(am_inclwin *w, int64_t c) { am_iw_raise(w, c); }
int64_t iw_cmax_sure(uint32_t c) { return am_iw_cmax_sure(c); }
int64_t iw_cmax_of32(uint32_t f, int32_t lbm) { return am_iw_cmax_of32(f, lbm); }
void iw_class32_n(const uint32_t *c, int n, uint32_t in_lim, uint32_t out_lim, int32_t *out) {
  for (int i = 0; i < n; ++i) out[i] = am_iw_class32(c[i], in_lim, out_lim);
}
/* per lane: the fold of its maxima m[lane][nd] */
void iw_fold32_n(const uint32_t *m, int lanes, const uint32_t *lb, uint32_t nd, int32_t lbm, uint32_t *out) {
  for (int l = 0; l < lanes; ++l) {
    uint32_t f = 0xFFFFFFFFu;
    for (uint32_t d = 0; d < nd; ++d) f = am_iw_fold32(f, m[l * nd + d], lb[d], lbm);
    out[l] = f;
  }
}
'''
ESCAPED, OUT, IN, WINDOW = 0, 1, 2, 3


class InclWin(ctypes.Structure):
    _fields_ = [("cin", ctypes.c_int64), ("hi", ctypes.c_int64), ("cmax", ctypes.c_int64)]


@pytest.fixture(scope="module")
def iw(tmp_path_factory):
    d = tmp_path_factory.mktemp("iwshim")
    src, so = str(d / "shim.c"), str(d / "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "antidote_amd", "csrc"), src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.iw_lim.restype, lib.iw_lim.argtypes = ctypes.c_uint32, [ctypes.c_int64]
    lib.iw_in_lim.restype = ctypes.c_uint32
    lib.iw_raise.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.iw_cmax_sure.restype, lib.iw_cmax_sure.argtypes = ctypes.c_int64, [ctypes.c_uint32]
    lib.iw_cmax_of32.restype, lib.iw_cmax_of32.argtypes = ctypes.c_int64, [ctypes.c_uint32, ctypes.c_int32]
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def direct(c, lag, lb, thr, never):
    """Every op by all its entries: (inclusion bits, per-DC maxima over the included ops)."""
    x = (c[:, None] - (lb[None, :] + lag)).astype(np.uint32)  # u32 arithmetic, as the kernels rebuild it
    inc = (c != ESC) & (x <= thr[None, :]).all(axis=1) & (not never)
    return inc, (x[inc].max(axis=0) if inc.any() else np.zeros(len(lb), np.uint32))


def replay(lib, c, lag, lb, thr, never, lead):
    """The schedule: (inclusion bits, per-DC maxima, lag rows loaded, rounds).  lead: slots of a
    neighbouring key in front of the read inside its first segment (the read's start is not aligned)."""
    n, nd = len(c), len(lb)
    w = InclWin()
    lib.iw_setup(ctypes.byref(w), ptr(thr), ptr(lb), ctypes.c_uint32(nd), int(never))
    cin_lim, out_lim = lib.iw_lim(w.cin), lib.iw_lim(w.hi)
    lbm = int(lb.astype(np.int32).min())
    bits, mxr = np.zeros(n, bool), np.zeros(nd, np.uint32)
    loaded = rounds = 0
    nseg = (lead + n + SEG - 1) // SEG
    for sg in range(nseg - 1, -1, -1):
        a, b = max(sg * SEG - lead, 0), min((sg + 1) * SEG - lead, n)
        cs = np.ascontiguousarray(c[a:b])
        # the bound without loads, over the whole segment, before any op is classified
        if lib.iw_in_lim(ctypes.byref(w)) < cin_lim:
            sure = cs[cs < cin_lim]
            if len(sure):
                lib.iw_raise(ctypes.byref(w), lib.iw_cmax_sure(int(sure.max())))
        cl = np.zeros(len(cs), np.int32)
        lib.iw_class32_n(ptr(cs), len(cs), lib.iw_in_lim(ctypes.byref(w)), out_lim, ptr(cl))
        bits[a:b] = cl == IN
        lst = a + np.nonzero(cl == WINDOW)[0][::-1]  # newest first
        mx = np.zeros((WAVE, nd), np.uint32)         # the lanes' maxima of this segment
        for r0 in range(0, len(lst), WAVE):
            ent = lst[r0:r0 + WAVE]
            ce = np.ascontiguousarray(c[ent])
            need = np.ones(len(ent), bool)
            if r0:  # classified again against the raised limit: IN takes no load and no maximum
                cl = np.zeros(len(ent), np.int32)
                lib.iw_class32_n(ptr(ce), len(ent), lib.iw_in_lim(ctypes.byref(w)), out_lim, ptr(cl))
                assert ((cl == IN) | (cl == WINDOW)).all()
                bits[ent[cl == IN]] = True
                need = cl == WINDOW
            if not need.any():
                continue
            rounds += 1
            loaded += int(need.sum())
            x = (ce[:, None] - (lb[None, :] + lag[ent])).astype(np.uint32)
            inc = need & (x <= thr[None, :]).all(axis=1)
            bits[ent[inc]] = True
            lanes = np.nonzero(inc)[0]
            mx[lanes] = np.maximum(mx[lanes], x[inc])
            if inc.any():
                f = np.zeros(WAVE, np.uint32)
                lib.iw_fold32_n(ptr(np.ascontiguousarray(mx)), WAVE, ptr(lb), ctypes.c_uint32(nd), lbm, ptr(f))
                lib.iw_raise(ctypes.byref(w), lib.iw_cmax_of32(int(f.max()), lbm))
        mxr = np.maximum(mxr, mx.max(axis=0))
    return bits, mxr, loaded, rounds


def check(lib, c, lag, lb, thr, never=False, lead=0):
    c, lag = np.asarray(c, np.uint32), np.asarray(lag, np.uint32).reshape(len(c), len(lb))
    lb, thr = np.asarray(lb, np.int64).astype(np.uint32), np.asarray(thr, np.uint32)  # lb: the int32 as stored
    x = c.astype(np.int64)[:, None] - lb.astype(np.int32).astype(np.int64)[None, :] - lag
    assert ((x >= 0) & (x <= TMAX))[c != ESC].all(), "not a log the view holds"
    want_bits, want_mx = direct(c, lag, lb, thr, never)
    bits, mx, loaded, rounds = replay(lib, c, lag, lb, thr, never, lead)
    live = c != ESC
    assert np.array_equal(bits[live], want_bits[live])
    assert not bits[~live].any()
    assert np.array_equal(mx, want_mx), (mx, want_mx)
    return int(want_bits.sum()), loaded, rounds


def timeline(rng, n, kind, step):
    """Commit times of n ops in log order: asc, shuffled, or two timelines 40 ms apart interleaved."""
    if kind == "inter":
        t = (np.arange(n) // 2) * 2 * step + (np.arange(n) % 2) * 40_000 + rng.integers(0, step, n)
    else:
        t = np.arange(n) * step + rng.integers(0, step, n)
    if kind == "shuffled":
        rng.shuffle(t)
    return t


@pytest.mark.parametrize("kind", ["asc", "shuffled", "inter"])
def test_rounds_schedule_random_logs(iw, kind):
    rng = np.random.default_rng(9800 + len(kind))
    seen = dict(loaded=0, rounds=0, inc=0, multi=0)
    for it in range(60):
        nd = int(rng.integers(1, 9))
        n = int(rng.choice([65, 255, 256, 257, 1023, 1024, 1025, 1100, 2180, 4200]))
        step = int(rng.choice([1000, 100, 10]))
        lb = rng.integers(-300_000, 300_000, nd)
        base = max(int(lb.max()), 0) + LAGMAX + int(rng.integers(0, 1000))
        c = base + timeline(rng, n, kind, step)
        k = rng.integers(0, 8, (n, nd))
        lag = np.where(k == 0, 0, np.where(k == 1, LAGMAX, rng.integers(0, LAGMAX + 1, (n, nd))))
        if it % 3 == 0:
            c = np.where(rng.integers(0, 64, n) == 0, ESC, c)
        clk = base + int(rng.integers(-80_000, n * step + 80_000))  # in commit-word units
        thr = np.clip(clk - lb - rng.integers(0, 2 * LAGMAX, nd), 0, TMAX)
        inc, loaded, rounds = check(iw, c, lag, lb, thr, never=it % 19 == 0, lead=int(rng.integers(0, 32)))
        seen["loaded"] += loaded
        seen["rounds"] += rounds
        seen["inc"] += inc
        seen["multi"] += rounds > 1
    assert seen["loaded"] > 1000 and seen["inc"] > 1000 and seen["multi"] >= 5, seen


def test_rounds_schedule_edges(iw):
    rng = np.random.default_rng(9811)
    n, nd = 1100, 3
    c = 200_000 + np.arange(n) * 100
    # lags 0 and 65535 on every op, a negative and a large lag base
    for lb in ([0, 7, -7], [-70_000, 70_000, 0], [100_000, -100_000, 5]):
        cc = c + max(lb) + LAGMAX
        for lagv in (0, LAGMAX):
            lag = np.full((n, nd), lagv)
            lag[::7, 1] = LAGMAX - lagv
            for clk in (cc[0] - 1, cc[n // 2], cc[-1] + 2 * LAGMAX):
                thr = np.clip(clk - np.asarray(lb) - lagv, 0, TMAX)
                check(iw, cc, lag, lb, thr, lead=5)
    lb = [0, 0, 0]
    cc, lag = c + LAGMAX, rng.integers(0, LAGMAX + 1, (n, nd))
    # never: nothing passes, nothing loads
    assert check(iw, cc, lag, lb, [int(cc[n // 2])] * nd, never=True) == (0, 0, 0)
    # an empty window: a clock below every op, and one so far above that the bound without loads
    # leaves only the newest ops (the list is not empty there: the op that gave the bound is on it)
    assert check(iw, cc, lag, lb, [int(cc[0]) - LAGMAX - 1] * nd) == (0, 0, 0)
    inc, loaded, _ = check(iw, c + 10 * LAGMAX, lag, lb, [TMAX] * nd)
    assert inc == n and 0 < loaded < n
    # a window equal to the whole key: 1100 ops inside 11 ms, the clock among them -- two segments,
    # every op on a list unless a round's maxima decide it first
    tight = 500_000 + np.arange(n) * 10
    inc, loaded, rounds = check(iw, tight, lag, lb, [int(tight[n // 2])] * nd, lead=31)
    assert 0 < inc < n and rounds > 2 and loaded > n // 2
