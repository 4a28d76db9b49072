"""CPU check of the commit-word window rule with a per-key lag width (antidote_amd/csrc/am_inclwin.h,
the *_w forms): hi = cin + w and the bound without loads of an op c' <= cin is c' - w (c' - 1 at
w = 0: the op that gives the bound stays in the window, whose ops alone are folded into the maxima),
where w is an upper bound of the lags of the key's ops the view holds.  A C program compares the width forms
with the direct evaluation of all D entries on random logs whose lags lie in [0, w], at every edge of
the rule and at the u32 limits, and at w = 0xFFFF with the functions without a width, bit for bit.
The rounds schedule of tests/test_inclwindow_rounds.py is then replayed with widths."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import test_inclwindow_rounds as rounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [0, 1, 63, 8000, 0xFFFE, 0xFFFF]
ESC, TMAX = 0xFFFFFFFF, 0xFFFFFFFE

PROG = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "am_inclwin.h"
#define DMAX 8
#define TMAX 0xFFFFFFFEu /* the largest threshold / entry (2^32 - 2) */

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static int64_t rr(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }
static long n_cls[4], n_checked, n_same, n_top, n_negraise;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); exit(1); } } while (0)
static const uint32_t WS[] = {0, 1, 63, 8000, 0xFFFE, 0xFFFF};
#define NW 6

typedef struct { uint32_t c; uint32_t lag[DMAX]; } op_t;
static uint32_t ent(const op_t *o, const uint32_t *lb, int d) { return o->c - (lb[d] + o->lag[d]); }
static int valid(const op_t *o, const uint32_t *lb, uint32_t nd, uint32_t w) { /* x_d in [0, 2^32 - 2], lag_d <= w */
  for (uint32_t d = 0; d < nd; ++d) {
    const int64_t x = (int64_t)o->c - (int32_t)lb[d] - (int64_t)o->lag[d];
    if (x < 0 || x > (int64_t)TMAX || o->lag[d] > w) return 0;
  }
  return o->c != AM_IW_ESC;
}

/* the running state in u32 limits, as the kernel keeps it, next to the int64 window */
typedef struct { am_inclwin w; uint32_t cin_lim, out_lim, cmax_lim; } st_t;
static void st_init(st_t *t, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never, uint32_t lw) {
  am_iw_setup_w(&t->w, thr, lb, nd, never, lw);
  t->cin_lim = am_iw_lim(t->w.cin), t->out_lim = am_iw_lim(t->w.hi), t->cmax_lim = 0;
}
static uint32_t st_in_lim(const st_t *t) { return t->cin_lim < t->cmax_lim ? t->cin_lim : t->cmax_lim; }
static void st_check(const st_t *t) { /* the u32 limits equal the int64 window under the same raises */
  CHECK(st_in_lim(t) == am_iw_in_lim(&t->w));
  CHECK(t->out_lim == am_iw_lim(t->w.hi));
}
static void st_raise_sure(st_t *t, uint32_t c, uint32_t lw) {
  CHECK(am_iw_lim_sure_w(c, lw) == am_iw_lim(am_iw_cmax_sure_w(c, lw)));
  if (c < (lw ? lw : 1u)) { ++n_negraise; CHECK(am_iw_cmax_sure_w(c, lw) < 0 && am_iw_lim_sure_w(c, lw) == 0); }
  am_iw_raise(&t->w, am_iw_cmax_sure_w(c, lw));
  t->cmax_lim = am_iw_lim_raise(t->cmax_lim, am_iw_lim_sure_w(c, lw));
  st_check(t);
}
static void st_raise_of(st_t *t, const uint32_t *m, const uint32_t *lb, uint32_t nd) {
  int32_t lbm = INT32_MAX;
  uint32_t f = 0xFFFFFFFFu;
  for (uint32_t d = 0; d < nd; ++d) lbm = (int32_t)lb[d] < lbm ? (int32_t)lb[d] : lbm;
  for (uint32_t d = 0; d < nd; ++d) f = am_iw_fold32(f, m[d], lb[d], lbm);
  am_iw_raise(&t->w, am_iw_cmax_of32(f, lbm)); /* (may saturate below am_iw_cmax_of: a smaller bound is safe) */
  t->cmax_lim = am_iw_lim_raise(t->cmax_lim, am_iw_lim_of32(f, lbm));
  st_check(t);
}

static void check_op(const st_t *t, const op_t *o, const uint32_t *thr, const uint32_t *lb, uint32_t nd, const uint32_t *M) {
  const int cl = am_iw_class(&t->w, o->c);
  CHECK(cl == am_iw_class32(o->c, st_in_lim(t), t->out_lim));
  int in = 1, below = 1;
  for (uint32_t d = 0; d < nd; ++d) in &= ent(o, lb, d) <= thr[d], below &= ent(o, lb, d) <= M[d];
  ++n_cls[cl], ++n_checked;
  if (cl == AM_IW_OUT) CHECK(!in);
  if (cl == AM_IW_IN) CHECK(in && below);
  CHECK(cl != AM_IW_ESCAPED);
}

static void check_read(const op_t *ops, int n, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never, uint32_t lw) {
  uint32_t mx0[DMAX] = {0}, mx1[DMAX] = {0};
  st_t t;
  st_init(&t, thr, lb, nd, never, lw);
  st_check(&t);
  if (never) CHECK(t.w.hi < 0 && t.out_lim == 0);
  for (int i = 0; i < n; ++i) {
    const op_t *o = &ops[i];
    if (o->c == AM_IW_ESC) { CHECK(am_iw_class(&t.w, o->c) == AM_IW_ESCAPED); continue; }
    int in = !never;
    for (uint32_t d = 0; d < nd; ++d) in &= ent(o, lb, d) <= thr[d];
    if (in) for (uint32_t d = 0; d < nd; ++d) mx0[d] = ent(o, lb, d) > mx0[d] ? ent(o, lb, d) : mx0[d];
    if (am_iw_sure_in(&t.w, o->c)) st_raise_sure(&t, o->c, lw);
    if (!never) check_op(&t, o, thr, lb, nd, mx1);
    const int cl = am_iw_class(&t.w, o->c);
    int in1 = cl == AM_IW_IN;
    if (cl == AM_IW_WINDOW) {
      in1 = 1;
      for (uint32_t d = 0; d < nd; ++d) in1 &= ent(o, lb, d) <= thr[d];
      if (in1) for (uint32_t d = 0; d < nd; ++d) mx1[d] = ent(o, lb, d) > mx1[d] ? ent(o, lb, d) : mx1[d];
      if (in1 && (i & 1)) st_raise_of(&t, mx1, lb, nd);
    }
    CHECK(in1 == in);
  }
  if (!never) for (uint32_t d = 0; d < nd; ++d) CHECK(mx0[d] == mx1[d]);
}

static void shuffle(op_t *o, int n) {
  for (int i = n - 1; i > 0; --i) { int j = (int)(rnd() % (uint64_t)(i + 1)); op_t x = o[i]; o[i] = o[j]; o[j] = x; }
}

static void random_reads(long n_reads, int n_ops) {
  op_t *ops = malloc(sizeof(op_t) * (size_t)n_ops);
  for (long r = 0; r < n_reads; ++r) {
    const uint32_t lw = WS[r % NW];
    const uint32_t nd = (uint32_t)rr(1, DMAX);
    uint32_t lb[DMAX] = {0}, thr[DMAX];
    const int wide = (int)(rnd() % 4) == 0;
    for (uint32_t d = 0; d < DMAX; ++d) lb[d] = d < nd ? (uint32_t)(int32_t)rr(wide ? -2000000000ll : -300000, wide ? 2000000000ll : 300000) : 0u;
    int64_t lbmax = -(1ll << 40), lbmin = 1ll << 40;
    for (uint32_t d = 0; d < nd; ++d) {
      lbmax = (int32_t)lb[d] > lbmax ? (int32_t)lb[d] : lbmax;
      lbmin = (int32_t)lb[d] < lbmin ? (int32_t)lb[d] : lbmin;
    }
    int64_t clo = lbmax + (int64_t)lw, chi = (int64_t)TMAX + lbmin;
    if (clo < 0) clo = 0;
    if (chi > (int64_t)TMAX) chi = TMAX;
    if (clo > chi) continue;
    /* the ops lie within a few widths of the clock, so that every class is met at every width */
    const int64_t room = 4 * (int64_t)lw + 40;
    const int64_t span = chi - clo < room ? chi - clo : room;
    const int64_t c0 = rr(clo, chi - span);
    const int64_t clk = rr(c0, c0 + span);
    for (uint32_t d = 0; d < DMAX; ++d) {
      int64_t t = clk - (int32_t)lb[d] - rr(0, 2 * (int64_t)lw + 4);
      if (rnd() % 16 == 0) t = TMAX;
      if (rnd() % 16 == 0) t = 0;
      thr[d] = d < nd ? (uint32_t)(t < 0 ? 0 : t > (int64_t)TMAX ? TMAX : t) : AM_IW_ESC;
    }
    for (int i = 0; i < n_ops; ++i) {
      ops[i].c = (uint32_t)(c0 + (span * i) / n_ops + rr(0, span / n_ops));
      if (ops[i].c > (uint64_t)chi) ops[i].c = (uint32_t)chi;
      for (uint32_t d = 0; d < DMAX; ++d) {
        const int k = (int)(rnd() % 8);
        ops[i].lag[d] = d >= nd ? 0u : k == 0 ? 0u : k == 1 ? lw : (uint32_t)rr(0, lw);
      }
      CHECK(valid(&ops[i], lb, nd, lw));
      if (rnd() % 64 == 0) ops[i].c = AM_IW_ESC;
    }
    const int order = (int)((r / NW) % 3); /* ascending, descending (newest first), shuffled */
    if (order == 1) for (int i = 0; i < n_ops / 2; ++i) { op_t x = ops[i]; ops[i] = ops[n_ops - 1 - i]; ops[n_ops - 1 - i] = x; }
    if (order == 2) shuffle(ops, n_ops);
    check_read(ops, n_ops, thr, lb, nd, r % 37 == 0, lw);
  }
  free(ops);
}

/* every edge of the rule, at every width */
static void edges(void) {
  static const int32_t LBS[] = {0, 7, -7, -70000, 70000, 2000000000, -2000000000};
  for (int wi = 0; wi < NW; ++wi)
    for (uint32_t nd = 1; nd <= DMAX; ++nd)
      for (unsigned a = 0; a < 7; ++a)
        for (unsigned b = 0; b < 7; ++b)
          for (int tk = 0; tk < 5; ++tk) {
            const uint32_t lw = WS[wi];
            uint32_t lb[DMAX] = {0}, thr[DMAX], M[DMAX];
            const uint32_t dm = (a + b + (unsigned)tk) % nd;
            for (uint32_t d = 0; d < DMAX; ++d) lb[d] = d >= nd ? 0u : (uint32_t)(d == 0 ? LBS[a] : LBS[b]);
            /* tk 2: cin + w at the top of the u32 range where the lag bases allow; tk 3: cin below w, or negative */
            const int64_t base = tk == 0 ? 3000000000ll : tk == 1 ? 200000 : tk == 2 ? (int64_t)TMAX : tk == 3 ? 100 : 2200000000ll;
            for (uint32_t d = 0; d < DMAX; ++d) {
              int64_t t = d == dm ? base : base + 1000 * (int64_t)(d + 1);
              if (tk == 3) t -= (int32_t)lb[d];
              thr[d] = d >= nd ? AM_IW_ESC : (uint32_t)(t < 0 ? 0 : t > (int64_t)TMAX ? TMAX : t);
            }
            st_t t;
            st_init(&t, thr, lb, nd, 0, lw);
            int64_t cin = INT64_MAX;
            for (uint32_t d = 0; d < nd; ++d) { const int64_t v = (int64_t)thr[d] + (int32_t)lb[d]; cin = v < cin ? v : cin; }
            CHECK(t.w.cin == cin && t.w.hi == cin + (int64_t)lw && t.w.cmax == -1);
            if (cin + (int64_t)lw >= (int64_t)TMAX) { ++n_top; CHECK(t.out_lim == 0xFFFFFFFFu); }
            uint32_t dmin = 0;
            for (uint32_t d = 0; d < nd; ++d) if ((int64_t)thr[d] + (int32_t)lb[d] == cin) { dmin = d; break; }
            for (int mk = 0; mk < 3; ++mk) {
              /* M: none yet / maxima a little under the thresholds / the sure-in bound of c = CIN */
              const uint32_t under = lw < 40000 ? lw / 2 : 40000;
              for (uint32_t d = 0; d < DMAX; ++d) M[d] = mk == 1 && d < nd ? (thr[d] > under ? thr[d] - under : 0) : 0;
              t.w.cmax = -1, t.cmax_lim = 0;
              if (mk == 1) st_raise_of(&t, M, lb, nd);
              if (mk == 2 && cin >= 0 && cin < (int64_t)AM_IW_ESC) {
                st_raise_sure(&t, (uint32_t)cin, lw);
                for (uint32_t d = 0; d < nd; ++d) { /* what that op's entries are at the least */
                  const int64_t x = cin - (int32_t)lb[d] - (int64_t)lw;
                  M[d] = (uint32_t)(x < 0 ? 0 : x);
                }
              }
              const int64_t hi = t.w.hi;
              const int64_t cs[] = {cin - 1, cin, cin + 1, hi - 1, hi, hi + 1, t.w.cmax - 1, t.w.cmax, t.w.cmax + 1, 0, (int64_t)TMAX};
              const uint32_t lags[] = {0, lw ? 1u : 0u, lw ? lw - 1 : 0u, lw};
              for (unsigned ci = 0; ci < sizeof cs / sizeof *cs; ++ci)
                for (unsigned l0 = 0; l0 < 4; ++l0)
                  for (unsigned l1 = 0; l1 < 4; ++l1) {
                    if (cs[ci] < 0 || cs[ci] > (int64_t)TMAX) continue;
                    op_t o;
                    o.c = (uint32_t)cs[ci];
                    for (uint32_t d = 0; d < DMAX; ++d) o.lag[d] = d >= nd ? 0u : d == dmin ? lags[l0] : lags[l1];
                    if (!valid(&o, lb, nd, lw)) continue;
                    check_op(&t, &o, thr, lb, nd, M);
                    const int cl = am_iw_class(&t.w, o.c);
                    if (cs[ci] > hi) CHECK(cl == AM_IW_OUT);
                    else if (cs[ci] <= cin && cs[ci] <= t.w.cmax) CHECK(cl == AM_IW_IN);
                    else CHECK(cl == AM_IW_WINDOW);
                    if (cin < 0) CHECK(cl != AM_IW_IN);
                    /* tight: lag 0 at c = cin + 1 is out on the DC attaining cin; lag w at c = cin + w is in on it */
                    if (cs[ci] == cin + 1 && o.lag[dmin] == 0) CHECK(ent(&o, lb, (int)dmin) > thr[dmin]);
                    if (cs[ci] == hi && o.lag[dmin] == lw) CHECK(ent(&o, lb, (int)dmin) <= thr[dmin]);
                  }
            }
            /* pad DCs take no part; never: nothing passes at any width */
            st_t t2;
            uint32_t lb2[DMAX], thr2[DMAX];
            memcpy(lb2, lb, sizeof lb), memcpy(thr2, thr, sizeof thr);
            for (uint32_t d = nd; d < DMAX; ++d) lb2[d] = 0x80000001u, thr2[d] = 0;
            st_init(&t2, thr2, lb2, nd, 0, lw);
            CHECK(t2.w.cin == cin && t2.w.hi == t.w.hi);
            st_init(&t2, thr, lb, nd, 1, lw);
            CHECK(t2.out_lim == 0 && t2.cin_lim == 0);
            CHECK(am_iw_class(&t2.w, 0) == AM_IW_OUT && am_iw_class(&t2.w, TMAX) == AM_IW_OUT);
            CHECK(am_iw_class(&t2.w, AM_IW_ESC) == AM_IW_ESCAPED && am_iw_class(&t.w, AM_IW_ESC) == AM_IW_ESCAPED);
          }
}

/* at w = 0xFFFF the width forms are the functions without a width, bit for bit; and the read's set-up
   (am_iw_read_setup_w) gives the limits of am_iw_setup_w over the thresholds it makes, at every width */
static void same_at_format_width(long n) {
  for (long r = 0; r < n; ++r) {
    const uint32_t nd = (uint32_t)rr(0, DMAX);
    uint32_t lb[DMAX] = {0}, thr[DMAX] = {0}, thr2[DMAX] = {0};
    uint64_t S[DMAX] = {0};
    const uint64_t K = rnd() % 3 == 0 ? 0 : (uint64_t)rr(0, 1ll << 50);
    for (uint32_t d = 0; d < DMAX; ++d) {
      lb[d] = (uint32_t)(int32_t)rr(-2000000000ll, 2000000000ll);
      const int k = (int)(rnd() % 8);
      S[d] = k == 0 ? (K ? K - 1 : 0) : k == 1 ? K + 0xFFFFFFFFull + (uint64_t)rr(0, 5) : K + (uint64_t)rr(0, 0xFFFFFFFEll);
    }
    const uint32_t allmask = nd >= 32 ? 0xFFFFFFFFu : (1u << nd) - 1u;
    const uint32_t spres = rnd() % 8 == 0 ? (uint32_t)rnd() & allmask : allmask;
    const int never = (int)(rnd() % 5 == 0);
    const uint32_t c = (uint32_t)(rnd() % 3 == 0 ? rr(0, 0x20000) : rr(0, TMAX));
    am_inclwin a, b;
    am_iw_setup(&a, thr, lb, 0, never), am_iw_setup_w(&b, thr, lb, 0, never, 0xFFFF);
    CHECK(!memcmp(&a, &b, sizeof a));
    for (uint32_t d = 0; d < DMAX; ++d) thr[d] = (uint32_t)rr(0, TMAX);
    am_iw_setup(&a, thr, lb, nd, never), am_iw_setup_w(&b, thr, lb, nd, never, 0xFFFF);
    CHECK(!memcmp(&a, &b, sizeof a));
    const int64_t fold = rnd() % 8 == 0 ? AM_IW_NOBOUND : rr(-3000000000ll, 6000000000ll);
    am_iw_init(&a, fold, never), am_iw_init_w(&b, fold, never, 0xFFFF);
    CHECK(!memcmp(&a, &b, sizeof a));
    CHECK(am_iw_cmax_sure(c) == am_iw_cmax_sure_w(c, 0xFFFF) && am_iw_lim_sure(c) == am_iw_lim_sure_w(c, 0xFFFF));
    am_iw_read ra, rb;
    memset(&ra, 0, sizeof ra), memset(&rb, 0, sizeof rb);
    am_iw_read_setup(S, spres, allmask, K, lb, nd, DMAX, thr, &ra);
    am_iw_read_setup_w(S, spres, allmask, K, lb, nd, DMAX, 0xFFFF, thr2, &rb);
    CHECK(!memcmp(&ra, &rb, sizeof ra) && !memcmp(thr, thr2, sizeof thr));
    const uint32_t lw = WS[r % NW];
    am_iw_read_setup_w(S, spres, allmask, K, lb, nd, DMAX, lw, thr2, &rb);
    CHECK(!memcmp(thr, thr2, sizeof thr) && rb.never == ra.never && rb.miss == ra.miss && rb.lbm == ra.lbm);
    CHECK(rb.cin_lim == ra.cin_lim); /* cin does not depend on the width */
    am_iw_setup_w(&b, thr2, lb, nd, rb.never, lw);
    if (nd) CHECK(rb.cin_lim == am_iw_lim(b.cin) && rb.out_lim == am_iw_lim(b.hi));
    else CHECK(rb.out_lim == 0 && rb.cin_lim == 0);
    ++n_same;
  }
}

int main(void) {
  edges();
  const long n_edge = n_checked;
  random_reads(24000, 160);
  same_at_format_width(200000);
  printf("edge_ops %ld random_ops %ld out %ld in %ld window %ld same %ld top %ld negraise %ld\n", n_edge,
         n_checked - n_edge, n_cls[AM_IW_OUT], n_cls[AM_IW_IN], n_cls[AM_IW_WINDOW], n_same, n_top, n_negraise);
  return 0;
}
'''


def test_width_rule_matches_direct_evaluation():
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "iww.c")
        with open(c, "w") as f:
            f.write(PROG)
        exe = os.path.join(d, "iww")
        subprocess.run(["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                        c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(zip(out.stdout.split()[0::2], map(int, out.stdout.split()[1::2])))
    assert f["random_ops"] >= 3_000_000 and f["edge_ops"] >= 100_000 and f["same"] == 200_000
    assert min(f["out"], f["in"], f["window"]) >= 100_000
    # cin + w at the top of the u32 range, and the raise c' - w at c' < w, were both met
    assert f["top"] >= 100 and f["negraise"] >= 100


# ---------------------------------------------------------------- the rounds schedule with widths
# The replay of tests/test_inclwindow_rounds.py calls iw_setup and iw_cmax_sure of its shim: this shim
# gives it the same names over the width forms, at the width set by iw_set_width.
SHIM = r'''
#include "am_inclwin.h"
static uint32_t g_w = 0xFFFF;
void iw_set_width(uint32_t w) { g_w = w; }
void iw_setup(am_inclwin *w, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never) { am_iw_setup_w(w, thr, lb, nd, never, g_w); }
uint32_t iw_lim(int64_t v) { return am_iw_lim(v); }
uint32_t iw_in_lim(const am_inclwin *w) { return am_iw_in_lim(w); }
void iw_raise(am_inclwin *w, int64_t c) { am_iw_raise(w, c); }
int64_t iw_cmax_sure(uint32_t c) { return am_iw_cmax_sure_w(c, g_w); }
int64_t iw_cmax_of32(uint32_t f, int32_t lbm) { return am_iw_cmax_of32(f, lbm); }
void iw_class32_n(const uint32_t *c, int n, uint32_t in_lim, uint32_t out_lim, int32_t *out) {
  for (int i = 0; i < n; ++i) out[i] = am_iw_class32(c[i], in_lim, out_lim);
}
void iw_fold32_n(const uint32_t *m, int lanes, const uint32_t *lb, uint32_t nd, int32_t lbm, uint32_t *out) {
  for (int l = 0; l < lanes; ++l) {
    uint32_t f = 0xFFFFFFFFu;
    for (uint32_t d = 0; d < nd; ++d) f = am_iw_fold32(f, m[l * nd + d], lb[d], lbm);
    out[l] = f;
  }
}
'''


@pytest.fixture(scope="module")
def iww(tmp_path_factory):
    d = tmp_path_factory.mktemp("iwwshim")
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
    lib.iw_set_width.argtypes = [ctypes.c_uint32]
    return lib


@pytest.mark.parametrize("kind", ["asc", "shuffled", "inter"])
def test_rounds_schedule_with_widths(iww, kind):
    """Random logs whose lags lie in [0, w], w the largest among them (the builder's exact width) or a
    looser bound: bits and maxima equal the direct evaluation in every visiting order, and the narrow
    window loads fewer lag rows than the 16-bit one on the same log."""
    rng = np.random.default_rng(9900 + len(kind))
    seen = dict(loaded=0, loaded16=0, inc=0, multi=0)
    for it in range(48):
        w = WIDTHS[it % len(WIDTHS)]
        nd = int(rng.integers(1, 9))
        n = int(rng.choice([65, 255, 256, 257, 1023, 1024, 1025, 1100, 2180]))
        step = int(rng.choice([100, 10, 1])) if w < 8000 else int(rng.choice([1000, 100, 10]))
        lb = rng.integers(-300_000, 300_000, nd)
        base = max(int(lb.max()), 0) + w + int(rng.integers(0, 1000))
        c = base + rounds.timeline(rng, n, kind, step)
        k = rng.integers(0, 8, (n, nd))
        lag = np.where(k == 0, 0, np.where(k == 1, w, rng.integers(0, w + 1, (n, nd))))
        if it % 3 == 0:
            c = np.where(rng.integers(0, 64, n) == 0, ESC, c)
        clk = base + int(rng.integers(-2 * w - 50, n * step + 2 * w + 50))
        thr = np.clip(clk - lb - rng.integers(0, 2 * w + 2, nd), 0, TMAX)
        lead = int(rng.integers(0, 32))
        use = w if it % 4 else min(0xFFFF, w + int(rng.integers(0, 500)))  # any upper bound is a safe width
        iww.iw_set_width(use)
        inc, loaded, nr = rounds.check(iww, c, lag, lb, thr, never=it % 19 == 0, lead=lead)
        iww.iw_set_width(0xFFFF)
        inc16, loaded16, _ = rounds.check(iww, c, lag, lb, thr, never=it % 19 == 0, lead=lead)
        assert inc == inc16 and loaded <= loaded16
        seen["loaded"] += loaded
        seen["loaded16"] += loaded16
        seen["inc"] += inc
        seen["multi"] += nr > 1
    assert seen["loaded"] > 500 and seen["inc"] > 1000 and seen["multi"] >= 3, seen
    assert seen["loaded"] < seen["loaded16"], seen


def test_rounds_schedule_width_edges(iww):
    n, nd = 1100, 3
    c = 200_000 + np.arange(n) * 10
    for w in WIDTHS:
        iww.iw_set_width(w)
        for lb in ([0, 7, -7], [-70_000, 70_000, 0]):
            cc = c + max(lb) + w
            for lagv in (0, w):  # every lag at the width, and at 0 with some at the width
                lag = np.full((n, nd), lagv)
                lag[::7, 1] = w - lagv
                for clk in (cc[0] - 1, cc[n // 2], cc[n // 2] + w, cc[n // 2] + w + 1, cc[-1] + 2 * w + 2):
                    thr = np.clip(clk - np.asarray(lb) - lagv, 0, TMAX)
                    rounds.check(iww, cc, lag, lb, thr, lead=5)
    # width 0: every lag is 0, so the commit word decides every op and nothing is listed
    iww.iw_set_width(0)
    inc, loaded, nr = rounds.check(iww, c, np.zeros((n, nd), int), [0, 0, 0], [int(c[n // 2])] * nd, lead=31)
    assert inc == n // 2 + 1 and loaded <= 1 and nr <= 1
    iww.iw_set_width(0xFFFF)
