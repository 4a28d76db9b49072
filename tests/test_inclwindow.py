"""CPU check of the commit-word window rule (antidote_amd/csrc/am_inclwin.h): a C program
classifies ops from their commit word alone and compares with the direct evaluation of all
D entries -- on random reads (any visiting order) and exhaustively at every edge of the rule."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
static long n_cls[4], n_checked;
#define CHECK(x) do { if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

typedef struct { uint32_t c; uint32_t lag[DMAX]; } op_t;

/* the entry as the kernels rebuild it: u32 arithmetic on the stored words */
static uint32_t ent(const op_t *o, const uint32_t *lb, int d) { return o->c - (lb[d] + o->lag[d]); }
static int valid(const op_t *o, const uint32_t *lb, uint32_t nd) { /* the view's contract: x_d in [0, 2^32 - 2] */
  for (uint32_t d = 0; d < nd; ++d) {
    const int64_t x = (int64_t)o->c - (int32_t)lb[d] - (int64_t)o->lag[d];
    if (x < 0 || x > (int64_t)TMAX) return 0;
  }
  return o->c != AM_IW_ESC;
}

/* one op against the rule: the per-op properties */
static void check_op(const am_inclwin *w, const op_t *o, const uint32_t *thr, const uint32_t *lb, uint32_t nd,
                     const uint32_t *M) {
  const int cl = am_iw_class(w, o->c);
  CHECK(cl == am_iw_class32(o->c, am_iw_in_lim(w), am_iw_lim(w->hi))); /* the u32 form the kernel uses */
  CHECK(am_iw_sure_in(w, o->c) == (o->c < am_iw_lim(w->cin)));
  int in = 1, below = 1;
  for (uint32_t d = 0; d < nd; ++d) in &= ent(o, lb, d) <= thr[d], below &= ent(o, lb, d) <= M[d];
  ++n_cls[cl], ++n_checked;
  if (cl == AM_IW_OUT) CHECK(!in);
  if (cl == AM_IW_IN) CHECK(in && below);
  CHECK(cl != AM_IW_ESCAPED);
}

/* a read over n ops in the given order: all ops evaluated vs window ops only */
static void check_read(const op_t *ops, int n, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never) {
  uint32_t mx0[DMAX] = {0}, mx1[DMAX] = {0};
  am_inclwin w;
  am_iw_setup(&w, thr, lb, nd, never);
  if (never) CHECK(w.hi < 0);
  for (int i = 0; i < n; ++i) {
    const op_t *o = &ops[i];
    if (o->c == AM_IW_ESC) { CHECK(am_iw_class(&w, o->c) == AM_IW_ESCAPED); continue; }
    int in = !never;
    for (uint32_t d = 0; d < nd; ++d) in &= ent(o, lb, d) <= thr[d];
    if (in) for (uint32_t d = 0; d < nd; ++d) mx0[d] = ent(o, lb, d) > mx0[d] ? ent(o, lb, d) : mx0[d];
    /* the windowed evaluation: the bound without loads first, then the class */
    if (am_iw_sure_in(&w, o->c)) am_iw_raise(&w, am_iw_cmax_sure(o->c));
    if (!never) check_op(&w, o, thr, lb, nd, mx1);
    const int cl = am_iw_class(&w, o->c);
    int in1 = cl == AM_IW_IN;
    if (cl == AM_IW_WINDOW) {
      in1 = 1;
      for (uint32_t d = 0; d < nd; ++d) in1 &= ent(o, lb, d) <= thr[d];
      if (in1) for (uint32_t d = 0; d < nd; ++d) mx1[d] = ent(o, lb, d) > mx1[d] ? ent(o, lb, d) : mx1[d];
      if (in1 && (i & 1)) am_iw_raise(&w, am_iw_cmax_of(mx1, lb, nd)); /* refreshed late at times: stale is safe */
    }
    CHECK(in1 == in);
  }
  /* the maxima over the window ops alone are those over all ops (an op that raised cmax by the
     bound without loads lies above that bound itself, so it or a newer op was evaluated) */
  for (int i = 0; i < n; ++i) {
    const op_t *o = &ops[i];
    if (o->c == AM_IW_ESC || never) continue;
    int in = 1;
    for (uint32_t d = 0; d < nd; ++d) in &= ent(o, lb, d) <= thr[d];
    if (in) for (uint32_t d = 0; d < nd; ++d) CHECK(ent(o, lb, d) <= mx1[d]);
  }
  if (!never) for (uint32_t d = 0; d < nd; ++d) CHECK(mx0[d] == mx1[d]);
}

static void shuffle(op_t *o, int n) {
  for (int i = n - 1; i > 0; --i) { int j = (int)(rnd() % (uint64_t)(i + 1)); op_t t = o[i]; o[i] = o[j]; o[j] = t; }
}

static void random_reads(long n_reads, int n_ops) {
  op_t *ops = malloc(sizeof(op_t) * (size_t)n_ops);
  for (long r = 0; r < n_reads; ++r) {
    const uint32_t nd = (uint32_t)rr(1, DMAX);
    uint32_t lb[DMAX] = {0}, thr[DMAX];
    const int wide = (int)(rnd() % 4) == 0;
    for (uint32_t d = 0; d < DMAX; ++d) lb[d] = d < nd ? (uint32_t)(int32_t)rr(wide ? -2000000000ll : -300000, wide ? 2000000000ll : 300000) : 0u;
    int64_t lbmax = -(1ll << 40), lbmin = 1ll << 40;
    for (uint32_t d = 0; d < nd; ++d) {
      lbmax = (int32_t)lb[d] > lbmax ? (int32_t)lb[d] : lbmax;
      lbmin = (int32_t)lb[d] < lbmin ? (int32_t)lb[d] : lbmin;
    }
    /* commit words of valid ops: c - lb_d - lag_d in [0, 2^32 - 2] for every lag */
    int64_t clo = lbmax + AM_IW_LAG_MAX, chi = (int64_t)TMAX + lbmin;
    if (clo < 0) clo = 0;
    if (chi > (int64_t)TMAX) chi = TMAX;
    if (clo > chi) { --r; continue; }
    const int64_t span = rr(1, 4) == 1 ? chi - clo : (chi - clo < 400000 ? chi - clo : 400000);
    const int64_t c0 = rr(clo, chi - span);
    const int64_t clk = rr(c0, c0 + span); /* the snapshot, in commit-word units */
    for (uint32_t d = 0; d < DMAX; ++d) {
      int64_t t = clk - (int32_t)lb[d] - rr(0, 2 * AM_IW_LAG_MAX);
      if (rnd() % 16 == 0) t = TMAX;
      if (rnd() % 16 == 0) t = 0;
      thr[d] = d < nd ? (uint32_t)(t < 0 ? 0 : t > (int64_t)TMAX ? TMAX : t) : AM_IW_ESC;
    }
    for (int i = 0; i < n_ops; ++i) {
      ops[i].c = (uint32_t)(c0 + (span * i) / n_ops + rr(0, span / n_ops));
      if (ops[i].c > (uint64_t)chi) ops[i].c = (uint32_t)chi;
      for (uint32_t d = 0; d < DMAX; ++d) {
        const int k = (int)(rnd() % 8);
        ops[i].lag[d] = d >= nd ? 0u : k == 0 ? 0u : k == 1 ? 0xFFFFu : (uint32_t)rr(0, 0xFFFF);
      }
      CHECK(valid(&ops[i], lb, nd));
      if (rnd() % 64 == 0) ops[i].c = AM_IW_ESC;
    }
    const int order = (int)(r % 3); /* ascending, descending (newest first), shuffled */
    if (order == 1) for (int i = 0; i < n_ops / 2; ++i) { op_t t = ops[i]; ops[i] = ops[n_ops - 1 - i]; ops[n_ops - 1 - i] = t; }
    if (order == 2) shuffle(ops, n_ops);
    check_read(ops, n_ops, thr, lb, nd, r % 37 == 0);
  }
  free(ops);
}

/* every edge of the rule, exhaustively over small choices */
static void edges(void) {
  static const int32_t LBS[] = {0, 7, -7, -70000, 70000, 2000000000, -2000000000};
  static const uint32_t LAGS[] = {0, 1, 0xFFFE, 0xFFFF};
  for (uint32_t nd = 1; nd <= DMAX; ++nd)
    for (unsigned a = 0; a < 7; ++a)
      for (unsigned b = 0; b < 7; ++b)
        for (int tk = 0; tk < 5; ++tk) {
          uint32_t lb[DMAX] = {0}, thr[DMAX], M[DMAX];
          /* DC 0 takes lb a, the others lb b; thresholds place the minimum on DC dm */
          const uint32_t dm = (a + b + (unsigned)tk) % nd;
          for (uint32_t d = 0; d < DMAX; ++d) lb[d] = d >= nd ? 0u : (uint32_t)(d == 0 ? LBS[a] : LBS[b]);
          const int64_t base = tk == 0 ? 3000000000ll : tk == 1 ? 200000 : tk == 2 ? (int64_t)TMAX : tk == 3 ? 100 : 2200000000ll;
          for (uint32_t d = 0; d < DMAX; ++d) {
            int64_t t = d == dm ? base : base + 1000 * (int64_t)(d + 1);
            if (tk == 3) t -= (int32_t)lb[d]; /* thr + lb small or negative: CIN < 0 where lb is below -100 */
            thr[d] = d >= nd ? AM_IW_ESC : (uint32_t)(t < 0 ? 0 : t > (int64_t)TMAX ? TMAX : t);
          }
          am_inclwin w;
          am_iw_setup(&w, thr, lb, nd, 0);
          int64_t cin = INT64_MAX;
          for (uint32_t d = 0; d < nd; ++d) { const int64_t v = (int64_t)thr[d] + (int32_t)lb[d]; cin = v < cin ? v : cin; }
          CHECK(w.cin == cin && w.hi == cin + 65535 && w.cmax == -1);
          uint32_t dmin = 0; /* the DC that attains CIN */
          for (uint32_t d = 0; d < nd; ++d) if ((int64_t)thr[d] + (int32_t)lb[d] == cin) { dmin = d; break; }
          for (int mk = 0; mk < 3; ++mk) {
            /* M: none yet / maxima a little under the thresholds / the sure-in bound of c = CIN */
            for (uint32_t d = 0; d < DMAX; ++d) M[d] = mk == 1 && d < nd ? (thr[d] > 40000 ? thr[d] - 40000 : 0) : 0;
            w.cmax = -1;
            if (mk == 1) am_iw_raise(&w, am_iw_cmax_of(M, lb, nd));
            if (mk == 2 && cin >= 0 && cin < (int64_t)AM_IW_ESC) {
              am_iw_raise(&w, am_iw_cmax_sure((uint32_t)cin));
              for (uint32_t d = 0; d < nd; ++d) { /* what that op's entries are at the least */
                const int64_t x = cin - (int32_t)lb[d] - 65535;
                M[d] = (uint32_t)(x < 0 ? 0 : x);
              }
            }
            const int64_t cs[] = {cin - 1, cin, cin + 1, w.hi - 1, w.hi, w.hi + 1, w.cmax - 1, w.cmax, w.cmax + 1, 0, (int64_t)TMAX};
            for (unsigned ci = 0; ci < sizeof cs / sizeof *cs; ++ci)
              for (unsigned l0 = 0; l0 < 4; ++l0)
                for (unsigned l1 = 0; l1 < 4; ++l1) {
                  if (cs[ci] < 0 || cs[ci] > (int64_t)TMAX) continue;
                  op_t o;
                  o.c = (uint32_t)cs[ci];
                  for (uint32_t d = 0; d < DMAX; ++d) o.lag[d] = d >= nd ? 0u : d == dmin ? LAGS[l0] : LAGS[l1];
                  if (!valid(&o, lb, nd)) continue;
                  check_op(&w, &o, thr, lb, nd, M);
                  const int cl = am_iw_class(&w, o.c);
                  if (cs[ci] > w.hi) CHECK(cl == AM_IW_OUT);
                  else if (cs[ci] <= cin && cs[ci] <= w.cmax) CHECK(cl == AM_IW_IN);
                  else CHECK(cl == AM_IW_WINDOW);
                  if (cin < 0) CHECK(cl != AM_IW_IN);
                  /* the bounds are tight: lag 0 at c = CIN + 1 is out, lag 0xFFFF at c = HI is in on that DC */
                  if (cs[ci] == cin + 1 && o.lag[dmin] == 0) CHECK(ent(&o, lb, (int)dmin) > thr[dmin]);
                  if (cs[ci] == w.hi && o.lag[dmin] == 0xFFFF) CHECK(ent(&o, lb, (int)dmin) <= thr[dmin]);
                }
          }
          /* pad DCs take no part: garbage in lb / thr beyond nd changes nothing */
          am_inclwin w2;
          uint32_t lb2[DMAX], thr2[DMAX];
          memcpy(lb2, lb, sizeof lb), memcpy(thr2, thr, sizeof thr);
          for (uint32_t d = nd; d < DMAX; ++d) lb2[d] = 0x80000001u, thr2[d] = 0;
          am_iw_setup(&w2, thr2, lb2, nd, 0);
          CHECK(w2.cin == cin);
          am_iw_setup(&w2, thr, lb, nd, 1);
          CHECK(am_iw_class(&w2, 0) == AM_IW_OUT && am_iw_class(&w2, TMAX) == AM_IW_OUT);
          CHECK(am_iw_class(&w2, AM_IW_ESC) == AM_IW_ESCAPED && am_iw_class(&w, AM_IW_ESC) == AM_IW_ESCAPED);
        }
}

int main(void) {
  edges();
  const long n_edge = n_checked;
  random_reads(20000, 192);
  printf("edge_ops %ld random_ops %ld out %ld in %ld window %ld\n", n_edge, n_checked - n_edge, n_cls[AM_IW_OUT],
         n_cls[AM_IW_IN], n_cls[AM_IW_WINDOW]);
  return 0;
}
'''


def test_window_rule_matches_direct_evaluation():
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "iw.c")
        with open(c, "w") as f:
            f.write(PROG)
        exe = os.path.join(d, "iw")
        subprocess.run(["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "antidote_amd", "csrc"),
                        c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(zip(out.stdout.split()[0::2], map(int, out.stdout.split()[1::2])))
    # a few million random ops, and every class met both at the edges and at random
    assert f["random_ops"] >= 3_000_000 and f["edge_ops"] >= 100_000
    assert min(f["out"], f["in"], f["window"]) >= 100_000
