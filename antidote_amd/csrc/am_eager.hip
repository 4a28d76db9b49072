// am_eager.hip -- materializer:materialize_eager/3 (src/materializer.erl:62-70) for a batch:
// a reading transaction's own effects folded into the snapshots it read
// (clocksi_vnode:read_data_item/5, src/clocksi_vnode.erl:99-107; the coordinator's
// apply_tx_updates_to_snapshot/4, src/clocksi_interactive_coord.erl:883-894).
//
// An eager fold has no clocks, no inclusion test and no op log: a base value of any size and a
// short effect list.  Its cost is one pass over the base value.
//   k_eager_lane     one lane per entry: the in_status pass-through, the PN sum and the LWW max;
//                    set / MV / bounded-counter entries are classified by write-set size and the
//                    large ones appended to a device list (no host readback)
//   k_eager_set<64>  one wavefront per small entry, four entries per 256-thread block, each with
//                    its own LDS slice (most transactions write a key once or twice)
//   k_eager_set<256> one workgroup per large entry of the list
// Set and MV entries use the closed form of am_sets.hip: every token an effect inserts is a BIRTH
// at the effect's position, every token it drops a KILL; the base pairs are births at position
// -1; a birth survives unless a kill of the same token (set: and element) comes at a strictly
// later position.  Only the write set lives in LDS:
//   1. the effects' births and kills are appended to LDS lists (am_block.h set_effects, the
//      store builder's validity rule), the kills sorted by (token, elem, position);
//   2. births with a later kill are dropped, the survivors sorted into output order (set: elem,
//      newest effect first, the effect's token order; MV: (value, token), equal pairs once);
//   3. the base value is streamed ONCE in coalesced tiles of set_a / set_b, one pair per lane: a
//      pair is kept iff no kill matches it (MV: and no surviving birth repeats it); its output
//      index is (surviving base pairs before it: wave ballots and prefix counts) + (births that
//      sort before it: a binary search j in the sorted births).  j never decreases along the
//      stream, so the lane whose pair raises it from j' to j tells births j' .. j-1 how many
//      surviving base pairs precede them;
//   4. birth i goes to (its rank i) + (that count).
// Nothing but the write set is sorted, and a base of any size works.
// A bounded counter is a keyed sum (orddict:update_counter): the n_dc * n_dc + n_dc slots as exact
// 128-bit LDS accumulators, seeded from the base pairs, compacted in slot order.
#include <vector>

#include "am_block.h"

using namespace amk;

namespace {

constexpr uint32_t UNSET = 0xFFFFFFFFu;
enum { CLS_NONE = 0, CLS_SCALAR = 1, CLS_SMALL = 2, CLS_BIG = 3 };

struct EagerArgs {
  am_writeset ws;
  am_values in;
  const int32_t *in_status;
  am_values out;
  int32_t *out_status;
  uint32_t nd;
};

template <int TPE>
struct Shape {
  static constexpr uint32_t NB = TPE == 64 ? AM_EAGER_SMALL_WORDS : AM_EAGER_MAX_BIRTHS;
  static constexpr uint32_t NK = TPE == 64 ? AM_EAGER_SMALL_WORDS : AM_EAGER_MAX_KILLS;
  // kills (a, b, p), births (a, b, p), the births' base counts, 16 counters
  static constexpr size_t BYTES = (size_t)NK * 20 + (size_t)NB * 24 + 16 * 4;
  static constexpr int PER_BLOCK = 256 / TPE;
};
static_assert((AM_EAGER_SMALL_WORDS & (AM_EAGER_SMALL_WORDS - 1)) == 0 && (AM_EAGER_MAX_BIRTHS & (AM_EAGER_MAX_BIRTHS - 1)) == 0 &&
                  (AM_EAGER_MAX_KILLS & (AM_EAGER_MAX_KILLS - 1)) == 0,
              "the LDS lists are sorted padded to a power of two");
static_assert(AM_EAGER_SMALL_SLOTS <= AM_EAGER_SMALL_WORDS && AM_MAX_DC * AM_MAX_DC + AM_MAX_DC <= AM_EAGER_MAX_KILLS,
              "the bounded-counter slots alias the kill lists");
static_assert(AM_EAGER_TILE_WAVE == 64 && AM_EAGER_TILE_WG == 256, "one base pair per lane per pass");

struct Lds {
  uint64_t *ka, *kb;  // kills: token, elem (MV: 0)
  uint64_t *ba, *bb;  // births: set (elem, token), MV (value, token)
  int32_t *kp;        // kill position (effect index)
  int32_t *bp;        // birth order: (n_eff - 1 - position) << 16 | index in the effect's add list
  uint32_t *bcnt;     // birth i: surviving base pairs that sort before it
  uint32_t *ctr;      // [0] kills [1] births [2] over the limits [3] bad effect [4] dead births
                      // [5] duplicate births [8..11] wave sums [12] emitted slots
  // bounded-counter slots (alias the kill lists)
  uint64_t *slo;
  int64_t *shi;
  uint32_t *spres;
};

template <int TPE>
__device__ __forceinline__ Lds carve(unsigned char *p) {
  constexpr uint32_t NB = Shape<TPE>::NB, NK = Shape<TPE>::NK;
  Lds s;
  s.ka = (uint64_t *)p;
  s.kb = s.ka + NK;
  s.ba = s.kb + NK;
  s.bb = s.ba + NB;
  s.kp = (int32_t *)(s.bb + NB);
  s.bp = s.kp + NK;
  s.bcnt = (uint32_t *)(s.bp + NB);
  s.ctr = s.bcnt + NB;
  s.slo = s.ka, s.shi = (int64_t *)s.kb, s.spres = (uint32_t *)s.kp;
  return s;
}

// the entry's threads meet: a workgroup barrier, or for one wavefront (whose lanes run in
// lockstep) an LDS fence the compiler may not move accesses across
template <int TPE>
__device__ __forceinline__ void gsync() {
  if constexpr (TPE == 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// ascending bitonic sort of n <= cap triples by (a, b, p), or BY_P by (a, p, b); padded with +inf
template <int TPE, bool BY_P>
__device__ void gsort(uint64_t *a, uint64_t *b, int32_t *p, uint32_t n, uint32_t cap, uint32_t t) {
  uint32_t N = 1;
  while (N < n) N <<= 1;
  if (N > cap) N = cap;
  for (uint32_t i = n + t; i < N; i += TPE) a[i] = ~0ull, b[i] = ~0ull, p[i] = POS_MAX;
  gsync<TPE>();
  for (uint32_t k = 2; k <= N; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < N; i += TPE) {
        const uint32_t x = i ^ j;
        if (x > i) {
          const bool up = (i & k) == 0;
          const uint64_t ai = a[i], ax = a[x], bi = b[i], bx = b[x];
          const int32_t pi = p[i], px = p[x];
          const bool lt = BY_P ? (ax != ai ? ax < ai : (px != pi ? px < pi : bx < bi)) : less3(ax, bx, px, ai, bi, pi);
          if (lt == up) a[i] = ax, a[x] = ai, b[i] = bx, b[x] = bi, p[i] = px, p[x] = pi;
        }
      }
      gsync<TPE>();
    }
  }
}

// An entry's class: CLS_SCALAR (PN / LWW), CLS_SMALL / CLS_BIG (set, MV, bounded counter, by
// write-set size), or CLS_NONE with its final status (pass-through or AM_ERR_INVALID).
__device__ __forceinline__ int eager_class(const EagerArgs &A, uint64_t i, uint64_t &e0, uint64_t &e1, int32_t &st) {
  const uint64_t row = A.ws.row[i];
  st = A.in_status ? A.in_status[row] : AM_OK;
  if (st != AM_OK) return CLS_NONE;
  st = AM_ERR_INVALID;
  const uint32_t type = A.ws.type[i];
  e0 = A.ws.eff_off[i], e1 = A.ws.eff_off[i + 1];
  if (e0 > e1 || e1 > A.ws.n_eff) return CLS_NONE;
  if (type == AM_PN) return A.out.v0 ? CLS_SCALAR : CLS_NONE;
  if (type == AM_LWW) return (A.out.v0 && A.out.v1 && A.out.vflag) ? CLS_SCALAR : CLS_NONE;
  if (type != AM_AWSET && type != AM_MVREG && type != AM_BCOUNTER) return CLS_NONE;
  if (!A.out.set_off || !A.out.set_len || !A.out.set_a || !A.out.set_b) return CLS_NONE;
  if (type == AM_BCOUNTER) return A.nd * A.nd + A.nd <= AM_EAGER_SMALL_SLOTS ? CLS_SMALL : CLS_BIG;
  uint64_t words = e1 - e0;
  if (A.ws.var_off) {
    const uint64_t v0 = A.ws.var_off[e0], v1 = A.ws.var_off[e1];
    words = v1 >= v0 && v1 - v0 < ~words ? words + (v1 - v0) : ~0ull;
  }
  return words <= AM_EAGER_SMALL_WORDS ? CLS_SMALL : CLS_BIG;
}

// the write set's effect columns as the op log am_block.h's effect readers take
__device__ __forceinline__ am_op_log effects_log(const am_writeset &ws) {
  am_op_log L{};
  L.p0 = ws.p0, L.p1 = ws.p1, L.var_off = ws.var_off, L.var_data = ws.var_data;
  return L;
}

__global__ void __launch_bounds__(256) k_eager_lane(EagerArgs A, uint32_t *big_list, uint32_t *big_count) {
  const uint64_t n = A.ws.n_ws;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t e0 = 0, e1 = 0;
    int32_t st = AM_OK;
    const int cls = eager_class(A, i, e0, e1, st);
    if (cls == CLS_BIG) big_list[atomicAdd(big_count, 1u)] = (uint32_t)i;
    if (cls == CLS_SMALL || cls == CLS_BIG) continue;  // the set kernels write the entry
    int64_t v0 = 0;
    uint64_t v1 = 0;
    uint32_t vflag = 0;
    if (cls == CLS_SCALAR) {
      const uint64_t row = A.ws.row[i];
      bool bad = false;
      for (uint64_t p = e0; p < e1; ++p) bad |= (A.ws.eff_meta[p] & AM_META_BAD) != 0;
      if (bad) {
        st = AM_ERR_UNEXPECTED_OPERATION;
      } else if (A.ws.type[i] == AM_PN) {
        PnVal v;
        v.reset();
        for (uint64_t p = e0; p < e1; ++p) v.add(A.ws.p0[p], 0);
        const int64_t b = A.in.v0 ? A.in.v0[row] : 0;
        add128(v.hi, v.lo, b < 0 ? -1 : 0, (uint64_t)b);
        st = v.hi != ((int64_t)v.lo < 0 ? -1 : 0) ? AM_ERR_OVERFLOW : AM_OK;
        v0 = (int64_t)v.lo;
      } else {  // erlang:max(Effect, State): the effect wins iff it sorts above the state
        LwwVal v;
        v.reset();
        for (uint64_t p = e0; p < e1; ++p) v.add(A.ws.p0[p], A.ws.p1[p]);
        const uint64_t bts = A.in.v0 ? (uint64_t)A.in.v0[row] : 0, bval = (A.in.v0 && A.in.v1) ? A.in.v1[row] : 0;
        const uint32_t bbin = A.in.v0 ? (A.in.vflag ? A.in.vflag[row] : 0) : 1;  // new() = {0, <<>>}
        const bool win = v.has && (v.ts > bts || (v.ts == bts && !bbin && v.val > bval));
        v0 = (int64_t)(win ? v.ts : bts), v1 = win ? v.val : bval, vflag = win ? 0 : bbin;
        st = AM_OK;
      }
    }
    if (st != AM_OK) v0 = 0, v1 = 0, vflag = 0;
    A.out_status[i] = st;
    if (A.out.v0) A.out.v0[i] = v0;
    if (A.out.v1) A.out.v1[i] = v1;
    if (A.out.vflag) A.out.vflag[i] = (uint8_t)vflag;
    if (A.out.set_len) A.out.set_len[i] = 0;
  }
}

template <uint32_t NB, uint32_t NK>
struct ListSink {
  Lds *s;
  uint32_t neff;
  __device__ void births(uint64_t e, const uint64_t *tok, uint32_t n, int32_t pos) {
    const uint32_t bi = atomicAdd(&s->ctr[1], n);
    if ((uint64_t)bi + n > NB) {
      s->ctr[2] = 1;
      return;
    }
    const uint32_t ord = (neff - 1u - (uint32_t)pos) << 16;
    for (uint32_t i = 0; i < n; ++i)
      s->ba[bi + i] = e, s->bb[bi + i] = tok[i], s->bp[bi + i] = (int32_t)(ord | (i < 0xFFFFu ? i : 0xFFFFu));
  }
  __device__ void birth(uint64_t a, uint64_t b, int32_t pos) { births(a, &b, 1u, pos); }
  __device__ void kills(const uint64_t *tok, uint32_t n, uint64_t e, int32_t pos) {
    const uint32_t ki = atomicAdd(&s->ctr[0], n);
    if ((uint64_t)ki + n > NK) {
      s->ctr[2] = 1;
      return;
    }
    for (uint32_t i = 0; i < n; ++i) s->ka[ki + i] = tok[i], s->kb[ki + i] = e, s->kp[ki + i] = pos;
  }
};

// the row of out the entry's threads fill; an error leaves it empty
__device__ __forceinline__ void finish(const EagerArgs &A, uint64_t i, int32_t st, uint32_t len) {
  A.out_status[i] = st;
  A.out.set_len[i] = st == AM_OK ? len : 0u;
  if (A.out.v0) A.out.v0[i] = 0;
  if (A.out.v1) A.out.v1[i] = 0;
  if (A.out.vflag) A.out.vflag[i] = 0;
}

// bounded counter: the slots as 128-bit LDS sums
template <int TPE>
__device__ void eager_bc(const EagerArgs &A, uint64_t i, uint64_t e0, uint64_t e1, Lds &s, uint32_t t) {
  const uint32_t nd = A.nd, ns = nd * nd + nd;
  const uint64_t row = A.ws.row[i];
  const am_op_log Lf = effects_log(A.ws);
  for (uint32_t k = t; k < ns; k += TPE) s.slo[k] = 0, s.shi[k] = 0, s.spres[k] = 0;
  gsync<TPE>();
  if (A.in.set_off && A.in.set_len && A.in.set_a && A.in.set_b) {
    const uint64_t bo = A.in.set_off[row], bl = A.in.set_len[row];
    for (uint64_t x = t; x < bl; x += TPE) {
      const uint64_t slot = A.in.set_a[bo + x];
      const int64_t v = (int64_t)A.in.set_b[bo + x];
      if (slot < ns) s.slo[slot] = (uint64_t)v, s.shi[slot] = v < 0 ? -1 : 0, s.spres[slot] = 1;
    }
  }
  gsync<TPE>();
  for (uint64_t p = e0 + t; p < e1; p += TPE) {
    const uint32_t meta = A.ws.eff_meta[p];
    uint32_t slot;
    int64_t v;
    if ((meta & AM_META_BAD) || !bc_slot(Lf, p, meta, nd, slot, v)) {
      s.ctr[3] = 1;
      continue;
    }
    acc128_atomic(&s.slo[slot], &s.shi[slot], v < 0 ? -1 : 0, (uint64_t)v);
    atomicOr(&s.spres[slot], 1u);
  }
  gsync<TPE>();
  for (uint32_t k = t; k < ns; k += TPE)
    if (s.shi[k] != ((int64_t)s.slo[k] < 0 ? -1 : 0)) s.ctr[2] = 1;
  gsync<TPE>();
  int32_t st = s.ctr[3] ? AM_ERR_UNEXPECTED_OPERATION : s.ctr[2] ? AM_ERR_OVERFLOW : AM_OK;
  if (st == AM_OK) {
    if (t < WAVE) {  // one wave compacts the present slots into the entry's CSR range
      am_read_result R{};
      R.value = A.out;
      const uint32_t ne = bc_emit<WAVE>(R, i, ns, t, 0, [&](uint32_t k, int64_t &v) {
        v = (int64_t)s.slo[k];
        return s.spres[k] != 0;
      });
      if (t == 0) s.ctr[12] = ne;
    }
    gsync<TPE>();
    if (s.ctr[12] > A.out.set_off[i + 1] - A.out.set_off[i]) st = AM_ERR_CAPACITY;
  }
  if (t == 0) finish(A, i, st, s.ctr[12]);
}

template <int TPE, int TYPE>
__device__ void eager_set(const EagerArgs &A, uint64_t i, uint64_t e0, uint64_t e1, Lds &s, uint32_t t) {
  constexpr uint32_t NB = Shape<TPE>::NB, NK = Shape<TPE>::NK;
  constexpr bool AW = TYPE == AM_AWSET;
  const uint64_t row = A.ws.row[i];
  const am_op_log Lf = effects_log(A.ws);
  const uint64_t oo = A.out.set_off[i], cap = A.out.set_off[i + 1] - oo;

  // ---- 1. the write set's births and kills ----
  if (e1 - e0 > AM_EAGER_MAX_EFFECTS) {
    if (t == 0) s.ctr[2] = 1;
    for (uint64_t p = e0 + t; p < e1; p += TPE)  // a bad effect still wins over the limit
      if (A.ws.eff_meta[p] & AM_META_BAD) s.ctr[3] = 1;
  } else {
    ListSink<NB, NK> sink{&s, (uint32_t)(e1 - e0)};
    for (uint64_t p = e0 + t; p < e1; p += TPE) {
      const uint32_t meta = A.ws.eff_meta[p];
      bool ok = !(meta & AM_META_BAD);
      if (ok && A.ws.var_off) {
        const uint64_t vo = A.ws.var_off[p], ve = A.ws.var_off[p + 1];
        ok = vo <= ve && ve <= A.ws.n_var;
      }
      if (!ok || !set_effects<TYPE>(Lf, p, meta, (int32_t)(p - e0), sink)) s.ctr[3] = 1;
    }
  }
  gsync<TPE>();
  if (s.ctr[3] || s.ctr[2]) {
    if (t == 0) finish(A, i, s.ctr[3] ? AM_ERR_UNEXPECTED_OPERATION : AM_ERR_CAPACITY, 0);
    return;
  }
  const uint32_t nk = s.ctr[0], nb = s.ctr[1], neff = (uint32_t)(e1 - e0);
  gsort<TPE, false>(s.ka, s.kb, s.kp, nk, NK, t);  // by (token, elem, position)

  // the newest kill of key (qa, qb), or -1
  auto last_kill = [&](uint64_t qa, uint64_t qb) -> int32_t {
    uint32_t lo = 0, hi = nk;
    while (lo < hi) {  // upper bound of (qa, qb, +inf)
      const uint32_t mid = (lo + hi) >> 1;
      if (s.ka[mid] < qa || (s.ka[mid] == qa && s.kb[mid] <= qb)) lo = mid + 1;
      else hi = mid;
    }
    return (lo > 0 && s.ka[lo - 1] == qa && s.kb[lo - 1] == qb) ? s.kp[lo - 1] : -1;
  };

  // ---- 2. births without a later kill, in output order ----
  for (uint32_t b = t; b < nb; b += TPE) {
    const int32_t pos = (int32_t)(neff - 1u - ((uint32_t)s.bp[b] >> 16));
    if (last_kill(s.bb[b], AW ? s.ba[b] : 0ull) > pos) {
      s.ba[b] = ~0ull, s.bb[b] = ~0ull, s.bp[b] = POS_MAX;
      atomicAdd(&s.ctr[4], 1u);
    }
  }
  gsync<TPE>();
  uint32_t S = nb - s.ctr[4];
  gsort<TPE, AW>(s.ba, s.bb, s.bp, nb, NB, t);  // the dead sort last
  if (!AW) {  // insert_sorted keeps one of equal {Value, Token} pairs
    for (uint32_t b = t; b < S; b += TPE) s.bcnt[b] = b > 0 && s.ba[b] == s.ba[b - 1] && s.bb[b] == s.bb[b - 1];
    gsync<TPE>();
    for (uint32_t b = t; b < S; b += TPE)
      if (s.bcnt[b]) {
        s.ba[b] = ~0ull, s.bb[b] = ~0ull, s.bp[b] = POS_MAX;
        atomicAdd(&s.ctr[5], 1u);
      }
    gsync<TPE>();
    if (s.ctr[5]) {
      gsort<TPE, false>(s.ba, s.bb, s.bp, S, NB, t);
      S -= s.ctr[5];
    }
  }
  for (uint32_t b = t; b < S; b += TPE) s.bcnt[b] = UNSET;
  gsync<TPE>();

  // births that sort before base pair (a, b): set -- those of elems <= a (an elem's new tokens
  // precede its base tokens); MV -- those below (a, b)
  auto births_before = [&](uint64_t a, uint64_t b) -> uint32_t {
    uint32_t lo = 0, hi = S;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const bool before = AW ? s.ba[mid] <= a : (s.ba[mid] < a || (s.ba[mid] == a && s.bb[mid] < b));
      if (before) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };

  // ---- 3. one pass over the base value ----
  uint64_t bo = 0, bl = 0;
  if (A.in.set_off && A.in.set_len && A.in.set_a && A.in.set_b) bo = A.in.set_off[row], bl = A.in.set_len[row];
  const uint32_t lane = t & 63u, w = t >> 6;
  uint64_t kept = 0;  // surviving base pairs of the tiles before this one
  for (uint64_t x0 = 0; x0 < bl; x0 += TPE) {
    const uint64_t x = x0 + t;
    const bool has = x < bl;
    uint64_t a = 0, b = 0;
    if (has) a = A.in.set_a[bo + x], b = A.in.set_b[bo + x];
    const uint32_t j = has ? births_before(a, b) : S;
    uint32_t jp = (uint32_t)__shfl_up((int)j, 1u, WAVE);
    if (lane == 0) jp = (has && x > 0) ? births_before(A.in.set_a[bo + x - 1], A.in.set_b[bo + x - 1]) : 0u;
    bool keep = has && last_kill(b, AW ? a : 0ull) < 0;
    if (!AW && keep && j < S && s.ba[j] == a && s.bb[j] == b) keep = false;  // the birth stands for both
    const uint64_t m = __ballot(keep);
    uint64_t before = kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    uint32_t total = (uint32_t)__popcll(m);
    if constexpr (TPE > 64) {
      if (lane == 0) s.ctr[8 + w] = total;
      __syncthreads();
      total = 0;
      for (uint32_t k = 0; k < TPE / 64; ++k) {
        if (k < w) before += s.ctr[8 + k];
        total += s.ctr[8 + k];
      }
      __syncthreads();
    }
    if (has)  // births jp .. j-1 sort between the previous pair and this one
      for (uint32_t q = jp; q < j; ++q) s.bcnt[q] = (uint32_t)before;
    const uint64_t pos = before + j;
    if (keep && pos < cap) A.out.set_a[oo + pos] = a, A.out.set_b[oo + pos] = b;
    kept += total;
  }
  gsync<TPE>();

  // ---- 4. the births ----
  for (uint32_t b = t; b < S; b += TPE) {
    const uint64_t pos = (uint64_t)b + (s.bcnt[b] == UNSET ? kept : (uint64_t)s.bcnt[b]);
    if (pos < cap) A.out.set_a[oo + pos] = s.ba[b], A.out.set_b[oo + pos] = s.bb[b];
  }
  if (t == 0) finish(A, i, kept + S > cap ? AM_ERR_CAPACITY : AM_OK, (uint32_t)(kept + S));
}

template <int TPE>
__global__ void __launch_bounds__(256) k_eager_set(EagerArgs A, const uint32_t *big_list, const uint32_t *big_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int PER = Shape<TPE>::PER_BLOCK;
  const uint32_t g = threadIdx.x / TPE, t = threadIdx.x % TPE;
  Lds s = carve<TPE>(smem_raw + (size_t)g * Shape<TPE>::BYTES);
  const uint64_t n = TPE == 64 ? A.ws.n_ws : (uint64_t)uniform_u32(*big_count);
  for (uint64_t q = (uint64_t)blockIdx.x * PER + g; q < n; q += (uint64_t)gridDim.x * PER) {
    const uint64_t i = TPE == 64 ? q : (uint64_t)uniform_u32(big_list[q]);
    uint64_t e0 = 0, e1 = 0;
    int32_t st = AM_OK;
    const int cls = eager_class(A, i, e0, e1, st);
    if (cls != (TPE == 64 ? CLS_SMALL : CLS_BIG)) continue;
    if (t < 16) s.ctr[t] = 0;
    gsync<TPE>();
    const uint32_t type = A.ws.type[i];
    if (type == AM_BCOUNTER) eager_bc<TPE>(A, i, e0, e1, s, t);
    else if (type == AM_AWSET) eager_set<TPE, AM_AWSET>(A, i, e0, e1, s, t);
    else eager_set<TPE, AM_MVREG>(A, i, e0, e1, s, t);
    gsync<TPE>();
  }
}

// tmp row i -> row ws.row[i] of the result (am_read_objects_ws): status, scalars, set pairs
__global__ void __launch_bounds__(256) k_eager_scatter(am_writeset ws, am_values tmp, const int32_t *tmp_status,
                                                        am_read_result R) {
  for (uint64_t i = blockIdx.x; i < ws.n_ws; i += gridDim.x) {
    const uint64_t row = ws.row[i];
    const uint32_t len = tmp.set_len[i];
    if (R.value.set_off && R.value.set_a && R.value.set_b) {
      const uint64_t so = tmp.set_off[i], d = R.value.set_off[row], cap = R.value.set_off[row + 1] - d;
      for (uint64_t x = threadIdx.x; x < len && x < cap; x += blockDim.x)
        R.value.set_a[d + x] = tmp.set_a[so + x], R.value.set_b[d + x] = tmp.set_b[so + x];
    }
    if (threadIdx.x == 0) {
      R.status[row] = tmp_status[i];
      if (R.value.v0) R.value.v0[row] = tmp.v0[i];
      if (R.value.v1) R.value.v1[row] = tmp.v1[i];
      if (R.value.vflag) R.value.vflag[row] = tmp.vflag[i];
      if (R.value.set_len) R.value.set_len[row] = len;
    }
  }
}

int launch_eager(am_ctx *ctx, uint32_t nd, const am_writeset *ws, const am_values *in, const int32_t *in_status,
                 const am_values *out, int32_t *out_status) {
  const uint64_t n = ws->n_ws;
  if (n == 0) return AM_OK;
  if (n >= 0xFFFFFFFFull) {
    am_set_error("am_materialize_eager: more than 2^32 - 2 entries");
    return AM_ERR_UNSUPPORTED;
  }
  if (!ws->row || !ws->type || !ws->eff_off || (ws->n_eff && (!ws->eff_meta || !ws->p0 || !ws->p1)) ||
      (ws->var_off && ws->n_var && !ws->var_data)) {
    am_set_error("am_materialize_eager: the write set lacks a column");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  void *scr = nullptr;
  if (int rc = am_ctx_scratch(ctx, AM_SCR_EAGER, (n + 4) * sizeof(uint32_t), &scr)) return rc;
  uint32_t *big_count = (uint32_t *)scr, *big_list = big_count + 4;
  AM_HIP(hipMemsetAsync(big_count, 0, 16, ctx->stream));
  EagerArgs A{*ws, *in, in_status, *out, out_status, nd};
  uint64_t blocks = (n + 255) / 256;
  const uint64_t lane_cap = (uint64_t)ctx->n_cu * 8;
  hipLaunchKernelGGL(k_eager_lane, dim3((unsigned)(blocks < lane_cap ? blocks : lane_cap)), dim3(256), 0, ctx->stream, A,
                     big_list, big_count);
  static bool attr = false;
  if (!attr) {
    AM_HIP(hipFuncSetAttribute((const void *)k_eager_set<256>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)Shape<256>::BYTES));
    attr = true;
  }
  blocks = (n + 3) / 4;  // four wavefronts, four LDS slices (23 KB) per block
  hipLaunchKernelGGL(k_eager_set<64>, dim3((unsigned)(blocks < lane_cap ? blocks : lane_cap)), dim3(256),
                     Shape<64>::BYTES * 4, ctx->stream, A, big_list, big_count);
  const uint64_t wg_cap = (uint64_t)ctx->n_cu * 2;  // 66 KB of LDS each
  hipLaunchKernelGGL(k_eager_set<256>, dim3((unsigned)(n < wg_cap ? n : wg_cap)), dim3(256), Shape<256>::BYTES,
                     ctx->stream, A, big_list, big_count);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

// the device copy of a host write set inside a staged arena
struct WsStage {
  size_t row, type, eff_off, meta, p0, p1, var_off, var_data;
  bool has_var;
  void add(am_stage &st, const am_writeset *h) {
    const uint64_t n = h->n_ws, ne = h->n_eff;
    has_var = h->var_off != nullptr;
    row = st.add(h->row, n * 8), type = st.add(h->type, n), eff_off = st.add(h->eff_off, (n + 1) * 8);
    meta = st.add(h->eff_meta, ne), p0 = st.add(h->p0, ne * 8), p1 = st.add(h->p1, ne * 8);
    var_off = st.add(h->var_off, has_var ? (ne + 1) * 8 : 0);
    var_data = st.add(h->var_data, has_var ? h->n_var * 8 : 0);
  }
  am_writeset dev(const am_stage &st, const am_writeset *h) const {
    am_writeset d = *h;
    d.row = st.dev<uint64_t>(row), d.type = st.dev<uint8_t>(type), d.eff_off = st.dev<uint64_t>(eff_off);
    d.eff_meta = st.dev<uint8_t>(meta), d.p0 = st.dev<uint64_t>(p0), d.p1 = st.dev<uint64_t>(p1);
    d.var_off = has_var ? st.dev<uint64_t>(var_off) : nullptr;
    d.var_data = has_var ? st.dev<uint64_t>(var_data) : nullptr;
    return d;
  }
};

bool host_ws_ok(const am_writeset *h) {
  if (!h->row || !h->type || !h->eff_off) return false;
  if (h->n_eff && (!h->eff_meta || !h->p0 || !h->p1)) return false;
  if (h->var_off && h->n_var && !h->var_data) return false;
  if (h->var_off && h->var_off[h->n_eff] > h->n_var) return false;
  return h->eff_off[h->n_ws] <= h->n_eff;
}

}  // namespace

extern "C" int am_materialize_eager(am_ctx *ctx, uint32_t n_dc, const am_writeset *dev_ws, const am_values *dev_in,
                                    const int32_t *in_status, am_values *dev_out, int32_t *out_status) {
  if (!ctx || !dev_ws || !dev_in || !dev_out || !out_status || n_dc == 0 || n_dc > AM_MAX_DC) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  return launch_eager(ctx, n_dc, dev_ws, dev_in, in_status, dev_out, out_status);
}

extern "C" int am_materialize_eager_host(am_ctx *ctx, uint32_t n_dc, const am_writeset *hw, const am_values *hin,
                                         const int32_t *in_status, am_values *hout, int32_t *out_status) {
  if (!ctx || !hw || !hin || !hout || !out_status || n_dc == 0 || n_dc > AM_MAX_DC) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  const uint64_t n = hw->n_ws;
  if (n == 0) return AM_OK;
  if (!host_ws_ok(hw)) {
    am_set_error("am_materialize_eager_host: the write set lacks a column or its offsets exceed it");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  // the rows the write set names, gathered: entry i reads row i of the staged batch
  std::vector<uint64_t> rows(n), so(n + 1, 0), sa, sb, v1(n, 0);
  std::vector<int64_t> v0(n, 0);
  std::vector<uint8_t> vf(n, 1);
  std::vector<uint32_t> sl(n, 0);
  std::vector<int32_t> ist(n, AM_OK);
  const bool sets = hin->set_off && hin->set_len && hin->set_a && hin->set_b;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = hw->row[i];
    rows[i] = i;
    if (in_status) ist[i] = in_status[r];
    if (hin->v0) v0[i] = hin->v0[r], v1[i] = hin->v1 ? hin->v1[r] : 0, vf[i] = hin->vflag ? hin->vflag[r] : 0;
    if (sets) {
      sl[i] = hin->set_len[r];
      for (uint64_t x = 0; x < sl[i]; ++x) sa.push_back(hin->set_a[hin->set_off[r] + x]), sb.push_back(hin->set_b[hin->set_off[r] + x]);
    }
    so[i + 1] = sa.size();
  }
  am_writeset hw2 = *hw;
  hw2.row = rows.data();
  const uint64_t ocap = hout->set_off ? hout->set_off[n] : 0;
  am_stage st;
  WsStage wss;
  wss.add(st, &hw2);
  const size_t i_st = st.add(ist.data(), n * 4), i_v0 = st.add(v0.data(), n * 8), i_v1 = st.add(v1.data(), n * 8);
  const size_t i_vf = st.add(vf.data(), n), i_so = st.add(so.data(), (n + 1) * 8), i_sl = st.add(sl.data(), n * 4);
  const size_t i_sa = st.add(sa.data(), sa.size() * 8), i_sb = st.add(sb.data(), sb.size() * 8);
  const size_t o_so = st.add(hout->set_off, hout->set_off ? (n + 1) * 8 : 0);
  const size_t o_st = st.add(nullptr, n * 4), o_v0 = st.add(nullptr, n * 8), o_v1 = st.add(nullptr, n * 8);
  const size_t o_vf = st.add(nullptr, n), o_sl = st.add(nullptr, n * 4);
  const size_t o_sa = st.add(nullptr, ocap * 8), o_sb = st.add(nullptr, ocap * 8);
  int rc = st.upload(ctx);
  if (rc) {
    if (st.arena) am_dev_release(ctx, st.arena);
    return rc;
  }
  const am_writeset dws = wss.dev(st, &hw2);
  am_values din{}, dout{};
  din.v0 = st.dev<int64_t>(i_v0), din.v1 = st.dev<uint64_t>(i_v1), din.vflag = st.dev<uint8_t>(i_vf);
  if (!hin->v0) din.v0 = nullptr, din.v1 = nullptr, din.vflag = nullptr;
  din.set_off = st.dev<uint64_t>(i_so), din.set_len = st.dev<uint32_t>(i_sl);
  din.set_a = st.dev<uint64_t>(i_sa), din.set_b = st.dev<uint64_t>(i_sb);
  if (hout->v0) dout.v0 = st.dev<int64_t>(o_v0);
  if (hout->v1) dout.v1 = st.dev<uint64_t>(o_v1);
  if (hout->vflag) dout.vflag = st.dev<uint8_t>(o_vf);
  if (hout->set_off && hout->set_len && hout->set_a && hout->set_b)
    dout.set_off = st.dev<uint64_t>(o_so), dout.set_len = st.dev<uint32_t>(o_sl), dout.set_a = st.dev<uint64_t>(o_sa),
    dout.set_b = st.dev<uint64_t>(o_sb);
  hipError_t e = hipSuccess;
  rc = launch_eager(ctx, n_dc, &dws, &din, st.dev<int32_t>(i_st), &dout, st.dev<int32_t>(o_st));
  auto back = [&](void *h, const void *d, size_t bytes) {
    if (h && d && bytes && e == hipSuccess && !rc) e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
  };
  back(out_status, st.dev<int32_t>(o_st), n * 4);
  back(hout->v0, dout.v0, n * 8), back(hout->v1, dout.v1, n * 8), back(hout->vflag, dout.vflag, n);
  back(hout->set_len, dout.set_len, n * 4);
  back(hout->set_a, dout.set_a, ocap * 8), back(hout->set_b, dout.set_b, ocap * 8);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  am_dev_release(ctx, st.arena);
  if (e != hipSuccess) {
    am_set_error("am_materialize_eager_host: %s", hipGetErrorString(e));
    return AM_ERR_HIP;
  }
  return rc;
}

int am_eager_apply_result(am_ctx *ctx, uint32_t n_dc, const am_writeset *hw, const uint64_t *host_set_off,
                          am_read_result *dr) {
  if (!ctx || !dr || !dr->status) return AM_ERR_INVALID;
  if (!hw || hw->n_ws == 0) return AM_OK;
  AM_LOCK(ctx);
  if (!host_ws_ok(hw)) {
    am_set_error("am_read_objects_ws: the write set lacks a column or its offsets exceed it");
    return AM_ERR_INVALID;
  }
  const uint64_t n = hw->n_ws;
  const bool sets = host_set_off && dr->value.set_off && dr->value.set_len && dr->value.set_a && dr->value.set_b;
  std::vector<uint64_t> so(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i)
    so[i + 1] = so[i] + (sets ? host_set_off[hw->row[i] + 1] - host_set_off[hw->row[i]] : 0);
  am_stage st;
  WsStage wss;
  wss.add(st, hw);
  const size_t t_so = st.add(so.data(), (n + 1) * 8), t_st = st.add(nullptr, n * 4), t_v0 = st.add(nullptr, n * 8);
  const size_t t_v1 = st.add(nullptr, n * 8), t_vf = st.add(nullptr, n), t_sl = st.add(nullptr, n * 4);
  const size_t t_sa = st.add(nullptr, so[n] * 8), t_sb = st.add(nullptr, so[n] * 8);
  int rc = st.upload(ctx);
  if (!rc) {
    const am_writeset dws = wss.dev(st, hw);
    am_values tmp{};
    tmp.v0 = st.dev<int64_t>(t_v0), tmp.v1 = st.dev<uint64_t>(t_v1), tmp.vflag = st.dev<uint8_t>(t_vf);
    tmp.set_off = st.dev<uint64_t>(t_so), tmp.set_len = st.dev<uint32_t>(t_sl);
    tmp.set_a = st.dev<uint64_t>(t_sa), tmp.set_b = st.dev<uint64_t>(t_sb);
    rc = launch_eager(ctx, n_dc, &dws, &dr->value, dr->status, &tmp, st.dev<int32_t>(t_st));
    if (!rc) {
      const uint64_t cap = (uint64_t)ctx->n_cu * 8;
      hipLaunchKernelGGL(k_eager_scatter, dim3((unsigned)(n < cap ? n : cap)), dim3(256), 0, ctx->stream, dws, tmp,
                         st.dev<int32_t>(t_st), *dr);
      if (hipGetLastError() != hipSuccess) rc = AM_ERR_HIP;
    }
  }
  // `so` and the caller's write set were staged with stream-ordered copies: finish them here
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = AM_ERR_HIP;
  if (st.arena) am_dev_release(ctx, st.arena);
  return rc;
}
