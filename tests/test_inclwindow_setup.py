"""CPU check of a read's set-up for the inclusion pass (am_iw_read_setup, antidote_amd/csrc/am_inclwin.h)
and of the window state kept as u32 limits (am_iw_lim_sure / am_iw_lim_of32 / am_iw_lim_raise).

The header is plain C: a host compiler builds it into a small shared library, which runs the same
code the kernel's lanes run.  Its thr / never / miss / lbm / cin_lim / out_lim are compared with a
direct evaluation of the definitions -- over a million random reads in numpy's 64-bit integers (exact:
unsigned compares, and differences taken only where they are not negative), and over every edge of the
rule, and a sample of the random reads, in Python integers.  The C side then checks, for every read
and for commit words around each limit, that the u32 limits classify as the int64 window does when
both take the same 0-6 raises, sure-in and maxima kinds mixed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMAX = 8
ESC = 0xFFFFFFFF
TMAX = 0xFFFFFFFE
LAGMAX = 0xFFFF
I32MAX, I32MIN = 2**31 - 1, -(2**31)

LIB = r'''
#include <stdlib.h>
#include "am_inclwin.h"
#define DMAX 8

/* out[5 i ..]: never, miss, lbm (the int32's bits), cin_lim, out_lim */
void setup_batch(long n, const uint64_t *S, const uint32_t *spres, const uint32_t *nd, const uint64_t *K,
                 const uint32_t *lb, int with_lb, uint32_t *thr, uint32_t *out) {
  for (long i = 0; i < n; ++i) {
    am_iw_read o;
    const uint32_t all = nd[i] >= 32 ? 0xFFFFFFFFu : (1u << nd[i]) - 1u;
    am_iw_read_setup(S + DMAX * i, spres[i], all, K[i], with_lb ? lb + DMAX * i : 0, nd[i], DMAX, thr + DMAX * i, &o);
    out[5 * i] = (uint32_t)o.never, out[5 * i + 1] = (uint32_t)o.miss, out[5 * i + 2] = (uint32_t)o.lbm;
    out[5 * i + 3] = o.cin_lim, out[5 * i + 4] = o.out_lim;
  }
}

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

/* For read i: the int64 window of am_iw_setup and the u32 limits of the set-up take the same raises;
 * after each, every commit word of a set around the limits must get the same class from both.
 * stat: 0 words checked, 1-3 classes OUT / IN / WINDOW met, 4 sure raises, 5 maxima raises,
 * 6 maxima raises whose am_iw_fold32 saturated, 7 reads with no raise.  Returns 0, or 1 + the first
 * read that differs. */
long class_check(long n, const uint32_t *thr, const uint32_t *lb, const uint32_t *nd, const uint32_t *out, long *stat) {
  for (long i = 0; i < n; ++i) {
    const uint32_t *t = thr + DMAX * i, *l = lb + DMAX * i;
    const int32_t lbm = (int32_t)out[5 * i + 2];
    const uint32_t cin_lim = out[5 * i + 3], out_lim = out[5 * i + 4];
    am_inclwin w;
    am_iw_setup(&w, t, l, nd[i], (int)out[5 * i]);
    if (am_iw_lim(w.cin) != cin_lim || am_iw_lim(w.hi) != out_lim) return 1 + i;
    uint32_t cmax_lim = 0;
    const int nr = (int)(rnd() % 7);
    if (!nr) ++stat[7];
    for (int r = 0; r <= nr; ++r) {
      if (r) { /* raise r of nr */
        const int k = (int)(rnd() % 4);
        if (k < 2) { /* a commit word, mostly a sure-in one */
          uint32_t c = (uint32_t)rnd();
          if (k == 0 && w.cin >= 0) {
            const uint64_t top = w.cin > 0xFFFFFFFEll ? 0xFFFFFFFEull : (uint64_t)w.cin;
            const uint64_t back = rnd() % 4 ? rnd() % 200000 : rnd();
            c = (uint32_t)(top - back % (top + 1));
          }
          if (c == AM_IW_ESC) c = 0xFFFFFFFEu;
          am_iw_raise(&w, am_iw_cmax_sure(c));
          cmax_lim = am_iw_lim_raise(cmax_lim, am_iw_lim_sure(c));
          ++stat[4];
        } else { /* running maxima: near the thresholds, or anywhere (k == 3: large, so that folds saturate) */
          uint32_t f = 0xFFFFFFFFu, m[DMAX] = {0};
          int sat = 0;
          for (uint32_t d = 0; d < nd[i]; ++d) {
            m[d] = k == 3 ? 0xFFFFFFFFu - (uint32_t)(rnd() % 3) * (uint32_t)(rnd() % 100000) : t[d] - (uint32_t)(rnd() % 70000 % (t[d] + 1ull));
            f = am_iw_fold32(f, m[d], l[d], lbm);
            sat |= (uint64_t)m[d] + (l[d] - (uint32_t)lbm) > 0xFFFFFFFFull;
          }
          /* the u32 fold is the int64 fold where no term saturates, and a smaller bound where one does */
          const int64_t exact = am_iw_cmax_of(m, l, nd[i]);
          if (am_iw_cmax_of32(f, lbm) > exact || (!sat && am_iw_cmax_of32(f, lbm) != exact)) return 1 + i;
          am_iw_raise(&w, am_iw_cmax_of32(f, lbm));
          cmax_lim = am_iw_lim_raise(cmax_lim, am_iw_lim_of32(f, lbm));
          ++stat[5], stat[6] += sat;
        }
      }
      const uint32_t in_lim = cin_lim < cmax_lim ? cin_lim : cmax_lim;
      if (in_lim != am_iw_in_lim(&w)) return 1 + i;
      const int64_t cs[] = {w.cin - 1, w.cin, w.cin + 1, w.hi - 1, w.hi, w.hi + 1, w.cmax - 1, w.cmax, w.cmax + 1,
                            (int64_t)cin_lim - 1, cin_lim, (int64_t)out_lim - 1, out_lim, (int64_t)cmax_lim - 1, cmax_lim,
                            (int64_t)cmax_lim + 1, 0, 1, 0xFFFE, 0xFFFF, 0x10000, 0xFFFFFFFDll, 0xFFFFFFFEll, 0xFFFFFFFFll,
                            (int64_t)(rnd() & 0xFFFFFFFFu)};
      for (unsigned ci = 0; ci < sizeof cs / sizeof *cs; ++ci) {
        if (cs[ci] < 0 || cs[ci] > 0xFFFFFFFFll) continue;
        const uint32_t c = (uint32_t)cs[ci];
        const int cl = am_iw_class(&w, c);
        if (cl != am_iw_class32(c, in_lim, out_lim)) return 1 + i;
        ++stat[0], ++stat[cl];
      }
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def lib():
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "iws.c")
        with open(c, "w") as f:
            f.write(LIB)
        so = os.path.join(d, "libiws.so")
        subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "antidote_amd", "csrc"), c, "-o", so], check=True)
        yield ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_setup(lib, S, spres, nd, K, lb, with_lb=True):
    n = len(K)
    S = np.ascontiguousarray(S, np.uint64)
    lb = np.ascontiguousarray(lb, np.uint32)
    thr = np.zeros((n, DMAX), np.uint32)
    out = np.zeros((n, 5), np.uint32)
    lib.setup_batch(ctypes.c_long(n), _p(S), _p(spres), _p(nd), _p(K), _p(lb), ctypes.c_int(with_lb), _p(thr), _p(out))
    return thr, out


def lim(v):
    return 0 if v < 0 else ESC if v >= TMAX else v + 1


def setup_py(S, spres, nd, K, lb):
    """One read in Python integers: (thr[DMAX], never, miss, lbm, cin_lim, out_lim); lb None: packed."""
    thr, never, miss = [], False, False
    for d in range(DMAX):
        if d >= nd:
            thr.append(ESC)
            continue
        present = (spres >> d) & 1
        s = S[d] if present else 0
        miss |= not present
        never |= s < K
        thr.append(0 if s < K else min(s - K, TMAX))
    never |= miss
    if lb is None:
        return thr, never, miss, None, None, None
    cin = -1 - LAGMAX if never or nd == 0 else min(thr[d] + lb[d] for d in range(nd))
    lbm = min(lb[:nd]) if nd else I32MAX
    return thr, never, miss, lbm, lim(cin), lim(cin + LAGMAX)


def setup_np(S, spres, nd, K, lb):
    """The same over arrays, in 64-bit integers."""
    n = len(K)
    d = np.arange(DMAX)[None, :]
    live = d < nd[:, None]
    present = ((spres[:, None] >> d.astype(np.uint32)) & 1).astype(bool)
    s = np.where(present, S, np.uint64(0))
    below = s < K[:, None]
    diff = np.where(below, np.uint64(0), s - np.where(below, np.uint64(0), K[:, None]))
    thr = np.where(live, np.minimum(diff, np.uint64(TMAX)), np.uint64(ESC))
    miss = (live & ~present).any(1)
    never = miss | (live & below).any(1)
    lbs = lb.astype(np.int32).astype(np.int64)
    big = np.int64(2**62)
    cin = np.where(live, thr.astype(np.int64) + lbs, big).min(1)
    cin = np.where(never, np.int64(-1 - LAGMAX), cin)
    lbm = np.where(live, lbs, np.int64(I32MAX)).min(1)

    def lim_np(v):
        return np.where(v < 0, 0, np.where(v >= TMAX, ESC, v + 1)).astype(np.uint32)
    assert n == len(cin)
    return thr.astype(np.uint32), never, miss, lbm.astype(np.int32), lim_np(cin), lim_np(cin + LAGMAX)


def random_reads(n, seed):
    g = np.random.default_rng(seed)
    nd = g.integers(1, DMAX + 1, n, dtype=np.uint32)
    kk = g.integers(0, 4, n)
    K = np.where(kk == 0, g.integers(0, 2**20, n, dtype=np.uint64),
                 np.where(kk == 1, g.integers(2**63, 2**64 - 2**34, n, dtype=np.uint64, endpoint=False),
                          g.integers(10**15, 2 * 10**15, n, dtype=np.uint64)))
    # S - K per DC: typical, below K, and around the clamp at AM_PK_ESC
    m = g.integers(0, 16, (n, DMAX))
    delta = g.integers(0, 2 * 10**9, (n, DMAX)).astype(np.int64)
    delta = np.where(m == 0, -g.integers(1, 10**6, (n, DMAX)), delta)
    delta = np.where(m == 1, ESC - 3 + g.integers(0, 6, (n, DMAX)), delta)
    delta = np.where(m == 2, g.integers(2**32, 2**33, (n, DMAX)), delta)
    delta = np.where(m == 3, g.integers(0, 200000, (n, DMAX)), delta)
    delta = np.where(m == 4, g.integers(0, 2**32, (n, DMAX)), delta)
    neg = delta < 0
    S = np.where(neg, K[:, None] - np.minimum((-delta).astype(np.uint64), K[:, None]), K[:, None] + np.abs(delta).astype(np.uint64))
    allm = (np.uint32(1) << nd) - np.uint32(1)
    drop = np.uint32(1) << g.integers(0, DMAX, n).astype(np.uint32)
    spres = np.where(g.integers(0, 12, n) == 0, allm & ~drop, allm).astype(np.uint32)
    spres |= np.where(g.integers(0, 2, n) == 0, np.uint32(0), ~allm)  # bits beyond the log's DCs change nothing
    lm = g.integers(0, 8, (n, DMAX))
    lb = g.integers(-300000, 300001, (n, DMAX)).astype(np.int64)
    lb = np.where(lm == 0, g.integers(-2 * 10**9, 2 * 10**9, (n, DMAX)), lb)
    lb = np.where(lm == 1, I32MAX - g.integers(0, 70000, (n, DMAX)), lb)
    lb = np.where(lm == 2, 0, lb)
    lb = np.where(lm == 3, I32MIN + g.integers(0, 70000, (n, DMAX)), lb)
    lb = np.where(lm == 4, -g.integers(0, 4 * 10**9 // 2, (n, DMAX)), lb)
    return S.astype(np.uint64), spres, nd, K.astype(np.uint64), lb.astype(np.int32).view(np.uint32)


def edge_reads():
    """Every edge of the rule: (S, spres, nd, K, lb) lists in Python integers."""
    out = []
    K0 = 1_700_000_000_000_000
    deltas = [-1, 0, 1, 65534, 65535, 65536, ESC - 2, ESC - 1, ESC, ESC + 1, 2**40]  # S[d] - K of one DC
    lbs = [I32MIN, I32MIN + 1, -2 * 10**9, -70000, -1, 0, 1, 70000, 2 * 10**9, I32MAX - 1, I32MAX]
    for nd in range(1, DMAX + 1):
        allm = (1 << nd) - 1
        for e in {0, nd - 1, nd // 2}:
            # S[d] < K for one DC (never); the clamp at AM_PK_ESC - 1, AM_PK_ESC and beyond
            for dl in deltas:
                for l in lbs:
                    S = [K0 + 5000 + d for d in range(DMAX)]
                    S[e] = K0 + dl
                    lb = [(l if d == e else 7 * d - 20) for d in range(DMAX)]
                    out.append((S, allm, nd, K0, lb))
            # a DC absent from the clock (miss), its entry whatever
            for junk in (0, K0 + 99):
                S = [K0 + 5000 + d for d in range(DMAX)]
                S[e] = junk
                out.append((S, allm & ~(1 << e), nd, K0, [3 - d for d in range(DMAX)]))
        # cin negative, at -1, at 0, around the lag span and above 2^32 - 2: thr + lb = t on DC 0
        for t in (-70000, -65537, -65536, -2, -1, 0, 1, 65534, 65535, 65536, ESC - 65537, ESC - 65536, ESC - 65535,
                  ESC - 3, ESC - 2, ESC - 1, ESC, ESC + 5, TMAX + I32MAX):
            for l in lbs:
                dl = t - l
                if not 0 <= dl <= TMAX:
                    continue
                S = [K0 + TMAX for d in range(DMAX)]  # the others' folds lie above t wherever lb allows
                S[0] = K0 + dl
                lb = [(l if d == 0 else I32MAX) for d in range(DMAX)]
                out.append((S, allm, nd, K0, lb))
        # pads (DMAX = 8): garbage beyond nd in the clock and in the lag bases changes nothing
        S = [K0 + 100 + d for d in range(nd)] + [0] * (DMAX - nd)
        out.append((S, allm | (0xFF & ~allm), nd, K0, [5] * nd + [I32MIN] * (DMAX - nd)))
        # K = 0 and K near 2^64
        out.append(([2**64 - 1] * DMAX, allm, nd, 0, [0] * DMAX))
        out.append(([2**64 - 1] * DMAX, allm, nd, 2**64 - 1, [-1] * DMAX))
        out.append(([2**64 - 2] * DMAX, allm, nd, 2**64 - 1, [1] * DMAX))
    return out


def as_arrays(reads):
    S = np.array([r[0] for r in reads], np.uint64)
    spres = np.array([r[1] for r in reads], np.uint32)
    nd = np.array([r[2] for r in reads], np.uint32)
    K = np.array([r[3] for r in reads], np.uint64)
    lb = np.array([r[4] for r in reads], np.int64).astype(np.int32).view(np.uint32)
    return S, spres, nd, K, lb


def check_py(reads_arrays, thr, out, idx, with_lb=True):
    S, spres, nd, K, lb = reads_arrays
    for i in idx:
        lbi = [int(x) for x in lb[i].view(np.int32)] if with_lb else None
        t, never, miss, lbm, cl, ol = setup_py([int(x) for x in S[i]], int(spres[i]), int(nd[i]), int(K[i]), lbi)
        got = [int(x) for x in out[i]]
        assert [int(x) for x in thr[i]] == t, i
        assert got[0] == int(never) and got[1] == int(miss), i
        if with_lb:
            assert got[2] == lbm & 0xFFFFFFFF and got[3] == cl and got[4] == ol, (i, got, lbm, cl, ol)


def check_classes(lib, thr, lb, nd, out):
    stat = (ctypes.c_long * 8)()
    rc = lib.class_check(ctypes.c_long(len(nd)), _p(thr), _p(lb), _p(nd), _p(out), stat)
    assert rc == 0, f"read {rc - 1}: the u32 limits and the int64 window disagree"
    return list(stat)


def test_setup_edges(lib):
    reads = edge_reads()
    arrs = as_arrays(reads)
    thr, out = run_setup(lib, *arrs)
    check_py(arrs, thr, out, range(len(reads)))
    # every edge is met: never by a DC below K, the clamp, miss, cin on both sides of 0 and of 2^32 - 2
    assert len(reads) >= 3000
    never, miss, cin_lim, out_lim = out[:, 0], out[:, 1], out[:, 3], out[:, 4]
    assert (never & ~miss).sum() >= 100 and miss.sum() >= 20
    assert (thr == TMAX).sum() >= 100 and (thr == 0).sum() >= 100
    assert (cin_lim == 0).sum() >= 100 and (cin_lim == 1).sum() >= 5 and (cin_lim == ESC).sum() >= 10
    assert ((out_lim > 0) & (cin_lim == 0) & (never == 0)).sum() >= 10  # cin < 0 <= hi
    # the packed instantiation's call (no lag bases): the same thr, never and miss
    thr_p, out_p = run_setup(lib, *arrs, with_lb=False)
    assert (thr_p == thr).all() and (out_p[:, :2] == out[:, :2]).all()
    check_py(arrs, thr_p, out_p, range(0, len(reads), 7), with_lb=False)
    stat = check_classes(lib, thr, arrs[4], arrs[2], out)
    assert min(stat[1:4]) >= 1000


def test_setup_random_reads(lib):
    n = 1_050_000
    arrs = random_reads(n, 20240611)
    S, spres, nd, K, lb = arrs
    thr, out = run_setup(lib, *arrs)
    e_thr, e_never, e_miss, e_lbm, e_cin, e_out = setup_np(S, spres, nd, K, lb)
    assert (thr == e_thr).all()
    assert (out[:, 0] == e_never).all() and (out[:, 1] == e_miss).all()
    assert (out[:, 2].view(np.int32) == e_lbm).all()
    assert (out[:, 3] == e_cin).all() and (out[:, 4] == e_out).all()
    check_py(arrs, thr, out, range(0, n, 53))  # the two direct evaluations agree as well
    # the inputs reach every branch in numbers
    assert e_never.sum() >= 50_000 and (~e_never).sum() >= 100_000 and e_miss.sum() >= 10_000
    assert ((e_cin > 0) & (e_cin < ESC)).sum() >= 100_000 and (e_cin == ESC).sum() >= 1000
    assert ((e_cin == 0) & ~e_never).sum() >= 1000
    stat = check_classes(lib, thr, lb, nd, out)
    # words checked; every class; both kinds of raise, saturated folds among them; reads without a raise
    assert stat[0] >= 20_000_000 and min(stat[1:4]) >= 500_000
    assert stat[4] >= 500_000 and stat[5] >= 500_000 and stat[6] >= 10_000 and stat[7] >= 50_000
