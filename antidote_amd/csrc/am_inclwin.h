// am_inclwin.h -- the commit-word window of a snapshot read over the lag view (host and device;
// plain C, no HIP: tests/test_inclwindow.py builds it with a host compiler).
//
// An op the lag view holds (c = lag_ct[p] != AM_PK_ESC) has, per DC d < nd, the entry
//   x_d = c - lb_d - lag_d,   lb_d = key_lag[k][d] (int32),   lag_d in [0, 0xFFFF],
// and is included iff x_d <= thr_d for every d (PkRead::thr).  Since the lags are bounded, the
// 4-byte commit word decides most ops without them.  Per read, in int64:
//   cin  = min_d (thr_d + lb_d)   c <= cin: every x_d <= c - lb_d <= thr_d        -> included
//   hi   = cin + 0xFFFF           c >  hi : the DC attaining cin has x_d > thr_d  -> excluded
//   cmax = min_d (M_d + lb_d)     c <= cmax: every x_d <= M_d, so the op raises no LastOpCt
//                                 maximum that already stands at M_d or above
// M_d is any lower bound of the read's final maximum of DC d: the running maximum over included
// ops (0 before the first: entries are >= 0), or c' - lb_d - 0xFFFF of an op c' <= cin, which
// gives cmax >= c' - 0xFFFF without a lag load.  Only ops with min(cin, cmax) < c <= hi (the
// window) need their lags.  Exact in any visiting order; a stale, smaller cmax is always safe.
//
// 0xFFFF is the range of the lag's format.  Where a bound w of the key's own lags is known -- every
// lag_d of every op of the key the view holds is <= w <= 0xFFFF (the store's per-key lag width) -- the
// same argument holds with w in its place: hi = cin + w, and an op c' <= cin gives cmax >= c' - w
// (taken as c' - max(w, 1): see am_iw_cmax_sure_w).
// The *_w forms take the width; the others are the same functions at w = AM_IW_LAG_MAX, and any
// upper bound of the lags is a safe width.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AM_IW_HD __host__ __device__ __forceinline__
#else
#define AM_IW_HD static inline
#endif

#define AM_IW_LAG_MAX 0xFFFFll
#define AM_IW_ESC 0xFFFFFFFFu /* AM_PK_ESC: the lag view does not hold the op */

enum { AM_IW_ESCAPED = 0, AM_IW_OUT = 1, AM_IW_IN = 2, AM_IW_WINDOW = 3 };

typedef struct am_inclwin {
  int64_t cin;  /* c <= cin: included; negative: nothing is sure-in */
  int64_t hi;   /* c >  hi : excluded */
  int64_t cmax; /* c <= min(cin, cmax): included and below every maximum; -1: no bound yet */
} am_inclwin;

/* one DC's term of a minimum min_d (v_d + lb_d): v the threshold or the maximum, lb the key's
 * lag base (the int32 as stored, in u32).  Start from AM_IW_NOBOUND; DCs d >= nd take no part. */
#define AM_IW_NOBOUND INT64_MAX
AM_IW_HD int64_t am_iw_fold(int64_t acc, uint32_t v, uint32_t lb) {
  const int64_t t = (int64_t)v + (int64_t)(int32_t)lb;
  return t < acc ? t : acc;
}
/* cin_fold: am_iw_fold over the thresholds of the DCs d < nd.  never (PkRead::never): no op
 * passes and nothing needs lags. */
AM_IW_HD void am_iw_init_w(am_inclwin *w, int64_t cin_fold, int never, uint32_t lw) {
  const int64_t cin = (never || cin_fold == AM_IW_NOBOUND) ? -1 - (int64_t)lw : cin_fold;
  w->cin = cin, w->hi = cin + (int64_t)lw, w->cmax = -1;
}
AM_IW_HD void am_iw_init(am_inclwin *w, int64_t cin_fold, int never) {
  am_iw_init_w(w, cin_fold, never, (uint32_t)AM_IW_LAG_MAX);
}
AM_IW_HD void am_iw_setup_w(am_inclwin *w, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never,
                            uint32_t lw) {
  int64_t f = AM_IW_NOBOUND;
  for (uint32_t d = 0; d < nd; ++d) f = am_iw_fold(f, thr[d], lb[d]);
  am_iw_init_w(w, f, never, lw);
}
AM_IW_HD void am_iw_setup(am_inclwin *w, const uint32_t *thr, const uint32_t *lb, uint32_t nd, int never) {
  am_iw_setup_w(w, thr, lb, nd, never, (uint32_t)AM_IW_LAG_MAX);
}

/* the bound a set of running maxima m[] (over included ops; 0 where none yet) gives */
AM_IW_HD int64_t am_iw_cmax_of(const uint32_t *m, const uint32_t *lb, uint32_t nd) {
  int64_t f = AM_IW_NOBOUND;
  for (uint32_t d = 0; d < nd; ++d) f = am_iw_fold(f, m[d], lb[d]);
  return nd ? f : -1;
}
/* the bound an op with c <= cin gives without its lags (lw: the key's lag width): c - lw, and
 * below c itself -- the maxima are folded over the window ops alone, so the op that gives the bound
 * has to stay in the window (at lw = 0, where its entries ARE the maxima, the bound is c - 1) */
AM_IW_HD int64_t am_iw_cmax_sure_w(uint32_t c, uint32_t lw) { return (int64_t)c - (int64_t)(lw ? lw : 1u); }
AM_IW_HD int64_t am_iw_cmax_sure(uint32_t c) { return am_iw_cmax_sure_w(c, (uint32_t)AM_IW_LAG_MAX); }
AM_IW_HD void am_iw_raise(am_inclwin *w, int64_t cmax) { w->cmax = cmax > w->cmax ? cmax : w->cmax; }

/* The bound of running maxima in u32, for the rounds of the inclusion pass (one op per lane): one
 * DC's term of min_d (m_d + lb_d) - lbm, lbm the smallest lag base of the DCs d < nd, saturating
 * at 2^32 - 1 (a smaller bound is safe).  Start from 0xFFFFFFFF; the bound of the lanes' folds f is
 * am_iw_cmax_of32(max over the lanes of f, lbm): any lane's maxima bound the read's. */
AM_IW_HD uint32_t am_iw_fold32(uint32_t acc, uint32_t m, uint32_t lb, int32_t lbm) {
#if defined(__HIPCC__)
  const uint32_t t = __builtin_elementwise_add_sat(m, lb - (uint32_t)lbm);
#else
  const uint32_t s = m + (lb - (uint32_t)lbm), t = s < m ? 0xFFFFFFFFu : s;
#endif
  return t < acc ? t : acc;
}
AM_IW_HD int64_t am_iw_cmax_of32(uint32_t f, int32_t lbm) { return (int64_t)f + (int64_t)lbm; }

AM_IW_HD int am_iw_sure_in(const am_inclwin *w, uint32_t c) { return c != AM_IW_ESC && (int64_t)c <= w->cin; }
/* escape first: AM_PK_ESC lies above every hi */
AM_IW_HD int am_iw_class(const am_inclwin *w, uint32_t c) {
  if (c == AM_IW_ESC) return AM_IW_ESCAPED;
  if ((int64_t)c > w->hi) return AM_IW_OUT;
  if ((int64_t)c <= (w->cin < w->cmax ? w->cin : w->cmax)) return AM_IW_IN;
  return AM_IW_WINDOW;
}

/* The same classes from exclusive u32 limits, one compare each: for a commit word c <= 2^32 - 2,
 * c < am_iw_lim(v) iff c <= v.  in_lim = am_iw_lim(min(cin, cmax)), out_lim = am_iw_lim(hi);
 * AM_PK_ESC lies at or above every limit, so escape is still tested first. */
AM_IW_HD uint32_t am_iw_lim(int64_t v) { return v < 0 ? 0u : v >= 0xFFFFFFFEll ? 0xFFFFFFFFu : (uint32_t)v + 1u; }
AM_IW_HD uint32_t am_iw_in_lim(const am_inclwin *w) { return am_iw_lim(w->cin < w->cmax ? w->cin : w->cmax); }
AM_IW_HD int am_iw_class32(uint32_t c, uint32_t in_lim, uint32_t out_lim) {
  if (c == AM_IW_ESC) return AM_IW_ESCAPED;
  if (c >= out_lim) return AM_IW_OUT;
  return c < in_lim ? AM_IW_IN : AM_IW_WINDOW;
}
/* The running bound as a limit.  am_iw_lim is monotone, so am_iw_in_lim(w) == min(cin_lim, cmax_lim)
 * with cin_lim = am_iw_lim(cin) and cmax_lim = am_iw_lim(cmax): cmax_lim starts at 0 (cmax = -1) and
 * a raise is a u32 max with the limit of the new bound, which the two kinds of raise give in 32 bits:
 *   am_iw_lim_sure(c)      == am_iw_lim(am_iw_cmax_sure(c))       c <= 2^32 - 2 a sure-in commit word
 *                             (am_iw_lim_sure_w(c, lw) == am_iw_lim(am_iw_cmax_sure_w(c, lw)) likewise)
 *   am_iw_lim_of32(f, lbm) == am_iw_lim(am_iw_cmax_of32(f, lbm))  f the lanes' largest am_iw_fold32 */
/* (with m = max(lw, 1): c - m + 1 <= c <= 2^32 - 2, no carry and no saturation to apply) */
AM_IW_HD uint32_t am_iw_lim_sure_w(uint32_t c, uint32_t lw) {
  const uint32_t m = lw ? lw : 1u;
  return c >= m ? c - m + 1u : 0u;
}
AM_IW_HD uint32_t am_iw_lim_sure(uint32_t c) { return am_iw_lim_sure_w(c, (uint32_t)AM_IW_LAG_MAX); }
AM_IW_HD uint32_t am_iw_lim_of32(uint32_t f, int32_t lbm) {
  if (lbm >= 0) {
    const uint32_t s = f + (uint32_t)lbm;
    return (s < f || s >= 0xFFFFFFFEu) ? 0xFFFFFFFFu : s + 1u;
  }
  const uint32_t n = 0u - (uint32_t)lbm; /* |lbm|, 1 .. 2^31 */
  return f < n ? 0u : f - n + 1u;
}
AM_IW_HD uint32_t am_iw_lim_raise(uint32_t cmax_lim, uint32_t lim) { return lim > cmax_lim ? lim : cmax_lim; }

/* A read's set-up, from its clock and its key: what the inclusion pass needs of them before it meets
 * an op.  The clock is S[d] for the DCs d < nd in spres (all the log's DCs: allmask); K the key's
 * time base; lb the key's lag bases (null: the read streams the packed view, and only thr, never
 * and miss are set).  thr[d], d < dmax: the packed thresholds (PkRead::thr: min(S_d - K, 2^32 - 2),
 * 0 where S_d < K, AM_PK_ESC for the pad DCs d >= nd); never / miss as PkRead's. */
typedef struct am_iw_read {
  int never;        /* no op passes: a DC missing from the clock or below K */
  int miss;         /* a DC of the ops is not in the clock */
  int32_t lbm;      /* the smallest lag base of the DCs d < nd (am_iw_fold32) */
  uint32_t cin_lim; /* am_iw_lim(cin) */
  uint32_t out_lim; /* am_iw_lim(hi) */
} am_iw_read;
#if defined(__HIPCC__)
#define AM_IW_UNROLL _Pragma("unroll")
#else
#define AM_IW_UNROLL
#endif
AM_IW_HD uint32_t am_iw_thr(uint64_t s, uint64_t K) {
  return s < K ? 0u : (s - K >= (uint64_t)AM_IW_ESC ? AM_IW_ESC - 1u : (uint32_t)(s - K));
}
/* lw: the key's lag width (am_inclwin.h's opening comment); out_lim is the limit of cin + lw */
AM_IW_HD void am_iw_read_setup_w(const uint64_t *S, uint32_t spres, uint32_t allmask, uint64_t K, const uint32_t *lb,
                                 uint32_t nd, uint32_t dmax, uint32_t lw, uint32_t *thr, am_iw_read *o) {
  int64_t f = 0; /* am_iw_fold over the DCs d < nd, from DC 0's term (no 64-bit start value to hold) */
  int32_t lbm = INT32_MAX;
  const int miss = (allmask & ~spres) != 0;
  int never = miss;
  AM_IW_UNROLL
  for (uint32_t d = 0; d < dmax; ++d) {
    if (d >= nd) {
      thr[d] = AM_IW_ESC;
      continue;
    }
    const uint64_t s = ((spres >> d) & 1u) ? S[d] : 0u;
    never |= s < K;
    thr[d] = am_iw_thr(s, K);
    if (lb) {
      const int64_t t = (int64_t)thr[d] + (int64_t)(int32_t)lb[d];
      f = (d == 0 || t < f) ? t : f;
      lbm = (int32_t)lb[d] < lbm ? (int32_t)lb[d] : lbm;
    }
  }
  am_inclwin w;
  am_iw_init_w(&w, (lb && nd) ? f : AM_IW_NOBOUND, never, lw);
  o->never = never, o->miss = miss, o->lbm = lbm;
  o->cin_lim = am_iw_lim(w.cin), o->out_lim = am_iw_lim(w.hi);
}
AM_IW_HD void am_iw_read_setup(const uint64_t *S, uint32_t spres, uint32_t allmask, uint64_t K, const uint32_t *lb,
                               uint32_t nd, uint32_t dmax, uint32_t *thr, am_iw_read *o) {
  am_iw_read_setup_w(S, spres, allmask, K, lb, nd, dmax, (uint32_t)AM_IW_LAG_MAX, thr, o);
}
