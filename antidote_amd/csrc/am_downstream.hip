// am_downstream.hip -- clocksi_downstream:generate_downstream_op/6 (src/clocksi_downstream.erl:
// 41-68) for a batch: a client update plus the state it read becomes the effect
// Type:downstream/2 returns, on the device, in am_writeset's payload encoding.
//
// The types' downstream/2 live in antidote_crdt @4157110c, which the reference does not vendor
// (DESIGN.md 3 says the same of update/2).  The rules below are the project's standing
// restatement, tests/dcsim.downstream, which the bounded-counter and set suites pin
// (tests/golden/multidc_suites.json, system_suites.json), extended for the ops no suite issues:
//   PN        increment N -> N, decrement N -> -N (negating INT64_MIN: AM_ERR_OVERFLOW); no read
//   LWW       assign -> {Ts, Value}, Ts the caller's make_micro_epoch(); no read
//   AWSET     add / add_all (after lists:usort), remove / remove_all: per element E ascending
//             {E, [Token] or [], the current tokens of E}, an absent E with no tokens;
//             reset: {E, [], Tokens} for every element of the state, in state order
//   MVREG     assign -> {Value, Token, every token of the state in state order};
//             reset -> {reset, every token of the state}
//   BCOUNTER  increment (N, Dc) -> {{increment, N}, Dc}; N < 0 is a decrement of -N
//             (src/bcounter_mgr.erl:89-90); decrement / transfer only when
//             localPermissions(Dc / From) >= N, else {error, no_permissions} (:120-129);
//             localPermissions(Dc) = sum of P[{_, Dc}] (with {Dc, Dc}) - sum of P[{Dc, To}],
//             To =/= Dc, - D[Dc], summed exactly in 128 bits
// Unpinned: the type's is_operation/1 is not in the reference, so rejecting a bounded-counter
// amount <= 0 (after the sign rule) as AM_ERR_INVALID is this library's rule; so are the effects
// of an add-wins-set reset, an MV reset and an LWW assign, which no recorded suite issues.
//
// Three steps on the context stream, no host readback:
//   k_ds_size       one wavefront per update: its status and its effect's variable words.
//                   add / remove: lanes stride over the requested elements, each with a lower and
//                   an upper bound in the row's set_a run (the value CSR is sorted by element, so
//                   an element's tokens are one contiguous run of set_b) -- the base is never
//                   streamed; reset: set_a streamed in coalesced tiles, element boundaries counted
//                   with ballots, the last element of a tile carried into the next; MV: set_len;
//                   bounded counter: the sparse (slot, value) pairs into a 128-bit sum
//   exclusive scan  of the word counts into offsets (hipcub); the total goes to *n_var
//   k_ds_fill<64>   one wavefront per update writes eff_meta, p0, p1 and the words: set entries
//                   [elem, n_add, n_rm, add_tok..., rm_tok...] in element order, an element's offset
//                   a wave prefix over the per-element sizes, chunks of 64 elements carrying a
//                   running base (no limit on the element count, no LDS list); the remove tokens of
//                   a chunk are disjoint ascending runs of set_b, copied flat: consecutive lanes on
//                   consecutive output words, each finding its run by a shuffle search of the prefix
//   k_ds_fill<256>  one workgroup per update of a device list: the updates that copy more than
//                   AM_DS_TILE_WG state pairs whole (a reset, an MV assign over a big register),
//                   i.e. more than one full workgroup pass
// Capacity is all-or-nothing and decided on the device: the fill reads *n_var and, when it exceeds
// var_cap, branches uniformly -- every update with variable words gets AM_ERR_CAPACITY and no
// word is written.  A non-OK update has zero words and AM_META_BAD.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "am_block.h"

using namespace amk;

namespace {

struct DsArgs {
  am_updates up;
  am_values in;
  const int32_t *in_status;
  am_effects eff;
  int32_t *out_status;
  uint32_t nd;
  uint64_t *cnt;        // [n_up + 1] variable words per update (entry n_up = 0)
  uint64_t *off;        // [n_up + 1] their exclusive scan
  uint32_t *big_list;   // updates the workgroup fill takes
  uint32_t *ctr;        // [0] length of big_list [1] some row is named twice
};

__device__ __forceinline__ bool has_sets(const am_values &v) { return v.set_off && v.set_len && v.set_a && v.set_b; }
__device__ __forceinline__ bool state_type(uint32_t t) { return t == AM_AWSET || t == AM_MVREG || t == AM_BCOUNTER; }
// the update copies the row's pairs whole and has more than one workgroup pass of them
__device__ __forceinline__ bool ds_big(uint32_t type, uint32_t op, uint64_t bl) {
  return bl > AM_DS_TILE_WG && (type == AM_MVREG || (type == AM_AWSET && op == AM_UP_AW_RESET));
}

// first index in [0, n) of a with a[x] >= e (UPPER: > e)
template <bool UPPER>
__device__ __forceinline__ uint64_t bound(const uint64_t *a, uint64_t n, uint64_t e) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t v = a[mid];
    if (UPPER ? v <= e : v < e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  int64_t hi = 0;
  wave_sum_i128(hi, v);
  return v;
}
__device__ __forceinline__ uint64_t wave_excl_scan_u64(uint64_t v, uint32_t lane, uint64_t &total) {
  uint64_t s = v;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)s, (unsigned)o, WAVE);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(s >> 32), (unsigned)o, WAVE);
    if (lane >= (uint32_t)o) s += ((uint64_t)hi << 32) | lo;
  }
  total = lane_u64(s, 63);
  return s - v;
}

// The arguments of an add / remove: words [v0, v1) of var_data, `stride` words per element.
// False: offsets outside var_data or not a whole number of elements.
__device__ __forceinline__ bool set_args(const am_updates &U, uint64_t i, uint32_t stride, uint64_t &v0, uint64_t &ne) {
  v0 = 0, ne = 0;
  if (!U.var_off) return true;
  const uint64_t a = U.var_off[i], b = U.var_off[i + 1];
  if (a > b || b > U.n_var || (b > a && !U.var_data) || (b - a) % stride) return false;
  v0 = a, ne = (b - a) / stride;
  return true;
}

// bounded counter: the amount and DC arguments after the sign rule.  kind = AM_BC_*.
__device__ __forceinline__ int32_t bc_args(const am_updates &U, uint64_t i, uint32_t op, uint32_t nd, uint32_t &kind,
                                           int64_t &amount, uint32_t &from, uint32_t &to) {
  amount = (int64_t)U.a0[i];
  const uint64_t a1 = U.a1[i];
  kind = op;
  if (op == AM_UP_BC_TRANSFER) {
    if (a1 >> 16) return AM_ERR_INVALID;
    from = (uint32_t)(a1 & 0xFF), to = (uint32_t)(a1 >> 8);
  } else {
    if (a1 >= nd) return AM_ERR_INVALID;
    from = to = (uint32_t)a1;
    if (op == AM_UP_BC_INCREMENT && amount < 0) {  // src/bcounter_mgr.erl:89-90
      if (amount == INT64_MIN) return AM_ERR_OVERFLOW;
      amount = -amount, kind = AM_BC_DECREMENT;
    }
  }
  if (from >= nd || to >= nd) return AM_ERR_INVALID;
  return amount <= 0 ? AM_ERR_INVALID : AM_OK;
}

constexpr int PER_BLOCK = 256 / WAVE;

__global__ void __launch_bounds__(256) k_ds_size(DsArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n = A.up.n_up;
  const bool dup = A.ctr[1] != 0;
  for (uint64_t i = (uint64_t)blockIdx.x * PER_BLOCK + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * PER_BLOCK) {
    const uint64_t row = A.up.row[i];
    const uint32_t type = A.up.type[i], op = A.up.op[i];
    int32_t st = AM_OK;
    uint64_t words = 0;
    int64_t avail = 0;
    const uint32_t nops = type == AM_PN ? 2u : type == AM_LWW ? 1u : type == AM_AWSET ? 3u : type == AM_MVREG ? 2u
                          : type == AM_BCOUNTER ? 3u : 0u;
    if (dup || op >= nops) {
      st = AM_ERR_INVALID;
    } else if (type == AM_PN) {
      if (op == AM_UP_PN_DECREMENT && (int64_t)A.up.a0[i] == INT64_MIN) st = AM_ERR_OVERFLOW;
    } else if (type == AM_LWW) {
    } else if (A.in_status && A.in_status[row] != AM_OK) {
      st = A.in_status[row];  // {error, {gen_downstream_read_failed, Reason}}
    } else if (!has_sets(A.in)) {
      st = AM_ERR_INVALID;
    } else {
      const uint64_t bo = A.in.set_off[row], bl = A.in.set_len[row];
      const uint64_t *sa = A.in.set_a + bo, *sb = A.in.set_b + bo;
      if (type == AM_MVREG) {
        words = bl;
      } else if (type == AM_AWSET && op == AM_UP_AW_RESET) {
        uint64_t nel = 0, last = 0;  // elements so far; the last element of the tile before
        for (uint64_t x0 = 0; x0 < bl; x0 += WAVE) {
          const uint64_t x = x0 + lane;
          const bool has = x < bl;
          const uint64_t a = has ? sa[x] : 0;
          uint64_t prev = shfl_u64(a, (lane + 63u) & 63u);
          if (lane == 0) prev = last;
          nel += (uint64_t)__popcll(__ballot(has && (x == 0 || a != prev)));
          last = lane_u64(a, 63);
        }
        words = 3 * nel + bl;
      } else if (type == AM_AWSET) {
        const uint32_t stride = op == AM_UP_AW_ADD ? 2u : 1u;
        uint64_t v0, ne;
        if (!set_args(A.up, i, stride, v0, ne)) {
          st = AM_ERR_INVALID;
        } else {
          uint64_t w = 0;
          bool bad = false;
          for (uint64_t j = lane; j < ne; j += WAVE) {
            const uint64_t e = A.up.var_data[v0 + j * stride];
            if (j > 0 && A.up.var_data[v0 + (j - 1) * stride] >= e) bad = true;
            w += 3 + (stride - 1) + (bound<true>(sa, bl, e) - bound<false>(sa, bl, e));
          }
          if (__ballot(bad)) st = AM_ERR_INVALID;
          else words = wave_sum_u64(w);
        }
      } else {  // bounded counter
        uint32_t kind, from, to;
        int64_t amount;
        st = bc_args(A.up, i, op, A.nd, kind, amount, from, to);
        if (st == AM_OK && kind != AM_BC_INCREMENT) {
          const uint64_t nd = A.nd, np = nd * nd, dc = from;
          int64_t hi = 0;
          uint64_t lo = 0;
          for (uint64_t x = lane; x < bl; x += WAVE) {
            const uint64_t slot = sa[x];
            const int64_t v = (int64_t)sb[x];
            int sign = 0;
            if (slot < np) sign = (slot % nd == dc) ? 1 : (slot / nd == dc) ? -1 : 0;
            else if (slot - np == dc) sign = -1;
            // -v as a 128-bit value: exact for INT64_MIN too
            if (sign > 0) add128(hi, lo, v < 0 ? -1 : 0, (uint64_t)v);
            else if (sign < 0) add128(hi, lo, v > 0 ? -1 : 0, 0ull - (uint64_t)v);
          }
          wave_sum_i128(hi, lo);
          if (hi != ((int64_t)lo < 0 ? -1 : 0)) {
            st = AM_ERR_OVERFLOW;
          } else {
            avail = (int64_t)lo;
            if (avail < amount) st = AM_ERR_NO_PERMISSIONS;
          }
        }
      }
    }
    if (st != AM_OK) words = 0;
    if (lane == 0) {
      A.out_status[i] = st;
      A.cnt[i] = words;
      if (A.eff.avail) A.eff.avail[i] = avail;
      if (st == AM_OK && has_sets(A.in) && state_type(type) && ds_big(type, op, A.in.set_len[row]))
        A.big_list[atomicAdd(&A.ctr[0], 1u)] = (uint32_t)i;
      if (i == 0) A.cnt[n] = 0;
    }
  }
}

// the effect's fixed columns; a failed update carries AM_META_BAD and no payload
__device__ __forceinline__ void put_head(const DsArgs &A, uint64_t i, int32_t st, uint32_t kind, uint64_t p0, uint64_t p1,
                                         uint64_t vo, uint64_t total) {
  const bool ok = st == AM_OK;
  const uint64_t n = A.up.n_up;
  A.out_status[i] = st;
  A.eff.eff_meta[i] = AM_MAKE_META(0, ok ? kind : 0, !ok);
  A.eff.p0[i] = ok ? p0 : 0, A.eff.p1[i] = ok ? p1 : 0;
  A.eff.eff_off[i] = i, A.eff.var_off[i] = vo;
  if (i == n - 1) A.eff.eff_off[n] = n, A.eff.var_off[n] = total;
}

// Copies the row's pairs whole: MV tokens, or the entries of an add-wins-set reset.  TPE threads.
template <int TPE>
__device__ void fill_whole(const DsArgs &A, bool reset_aw, const uint64_t *sa, const uint64_t *sb, uint64_t bl,
                           uint64_t *out, uint32_t t, uint32_t *wsum) {
  if (!reset_aw) {
    for (uint64_t x = t; x < bl; x += TPE) out[x] = sb[x];
    return;
  }
  // pair x of element number k goes to 3 (k + 1) + x; the lane holding an element's last pair
  // writes its header [elem, 0, n] at 3 k + (the run's start)
  const uint32_t lane = t & 63u, w = t >> 6;
  uint64_t kbase = 0;  // elements begun in the tiles before this one
  for (uint64_t x0 = 0; x0 < bl; x0 += TPE) {
    const uint64_t x = x0 + t;
    const bool has = x < bl;
    const uint64_t a = has ? sa[x] : 0;
    uint64_t prev = shfl_u64(a, (lane + 63u) & 63u), next = shfl_u64(a, (lane + 1u) & 63u);
    if (lane == 0 && has && x > 0) prev = sa[x - 1];
    if (lane == 63 && x + 1 < bl) next = sa[x + 1];
    const bool first = has && (x == 0 || a != prev), end = has && (x + 1 == bl || a != next);
    const uint64_t m = __ballot(first);
    uint64_t before = kbase + (uint64_t)__popcll(m & ((2ull << lane) - 1ull));  // elements begun up to this pair
    uint32_t total = (uint32_t)__popcll(m);
    if constexpr (TPE > 64) {
      if (lane == 0) wsum[w] = total;
      __syncthreads();
      total = 0;
      for (uint32_t k = 0; k < TPE / 64; ++k) {
        if (k < w) before += wsum[k];
        total += wsum[k];
      }
      __syncthreads();
    }
    if (has) out[3 * before + x] = sb[x];
    if (end) {
      // the run's start: its first pair in this wave's tile, else found in the pairs before it
      const uint64_t mine = m & ((2ull << lane) - 1ull);
      const uint64_t start = mine ? x - lane + (63u - (uint32_t)__clzll(mine)) : bound<false>(sa, x, a);
      uint64_t *h = out + 3 * (before - 1) + start;
      h[0] = a, h[1] = 0, h[2] = x + 1 - start;
    }
    kbase += total;
  }
}

template <int TPE>
__global__ void __launch_bounds__(256) k_ds_fill(DsArgs A) {
  __shared__ uint32_t wsum[4];
  constexpr int PER = 256 / TPE;
  const uint32_t g = threadIdx.x / TPE, t = threadIdx.x % TPE, lane = t & 63u;
  const uint64_t n_up = A.up.n_up;
  const uint64_t total = uniform_u64(*A.eff.n_var);
  const bool over = total > A.eff.var_cap;
  const uint64_t n = TPE == 64 ? n_up : (uint64_t)uniform_u32(A.ctr[0]);
  if (TPE > 64 && over) return;  // the wavefront fill reports every update then
  for (uint64_t q = (uint64_t)blockIdx.x * PER + g; q < n; q += (uint64_t)gridDim.x * PER) {
    const uint64_t i = TPE == 64 ? q : (uint64_t)uniform_u32(A.big_list[q]);
    const uint64_t row = A.up.row[i];
    const uint32_t type = A.up.type[i], op = A.up.op[i];
    int32_t st = A.out_status[i];
    const uint64_t words = A.off[i + 1] - A.off[i];
    const uint64_t vo = over ? 0 : A.off[i];
    if (over && words) st = AM_ERR_CAPACITY;
    uint64_t bo = 0, bl = 0;
    if (st == AM_OK && state_type(type)) bo = A.in.set_off[row], bl = A.in.set_len[row];
    if (TPE == 64 && st == AM_OK && ds_big(type, op, bl)) continue;  // the workgroup fill's
    const uint64_t *sa = A.in.set_a + bo, *sb = A.in.set_b + bo;
    uint64_t *out = A.eff.var_data + vo;
    uint32_t kind = 0;
    uint64_t p0 = 0, p1 = 0;
    if (st != AM_OK) {
    } else if (type == AM_PN) {
      p0 = op == AM_UP_PN_INCREMENT ? A.up.a0[i] : 0ull - A.up.a0[i];
    } else if (type == AM_LWW) {
      p0 = A.up.a0[i], p1 = A.up.a1[i];
    } else if (type == AM_BCOUNTER) {
      uint32_t from, to;
      int64_t amount;
      bc_args(A.up, i, op, A.nd, kind, amount, from, to);
      p0 = (uint64_t)amount, p1 = from | (to << 8);
    } else if (type == AM_MVREG) {
      kind = op == AM_UP_MV_ASSIGN ? AM_MV_ASSIGN : AM_MV_RESET;
      if (op == AM_UP_MV_ASSIGN) p0 = A.up.a0[i], p1 = A.up.a1[i];
      fill_whole<TPE>(A, false, sa, sb, bl, out, t, wsum);
    } else if (op == AM_UP_AW_RESET) {
      fill_whole<TPE>(A, true, sa, sb, bl, out, t, wsum);
    } else if constexpr (TPE == 64) {  // add / remove
      const uint32_t stride = op == AM_UP_AW_ADD ? 2u : 1u;
      uint64_t v0, ne;
      set_args(A.up, i, stride, v0, ne);
      uint64_t base = 0;  // words of the chunks before this one
      for (uint64_t j0 = 0; j0 < ne; j0 += WAVE) {
        const uint64_t j = j0 + lane;
        const bool has = j < ne;
        uint64_t e = 0, lb = 0, nrm = 0;
        if (has) {
          e = A.up.var_data[v0 + j * stride];
          lb = bound<false>(sa, bl, e), nrm = bound<true>(sa, bl, e) - lb;
        }
        const uint64_t hdr = 3 + (stride - 1);
        uint64_t chunk_words, chunk_rm;
        const uint64_t eoff = base + wave_excl_scan_u64(has ? hdr + nrm : 0, lane, chunk_words);
        uint64_t rx = wave_excl_scan_u64(nrm, lane, chunk_rm);  // the element's first remove token in the chunk
        if (!has) rx = chunk_rm;
        if (has) {
          out[eoff] = e, out[eoff + 1] = stride - 1, out[eoff + 2] = nrm;
          if (stride == 2) out[eoff + 3] = A.up.var_data[v0 + j * 2 + 1];
        }
        // the chunk's remove tokens, flat: word r belongs to the last element whose run begins at
        // or before r (an empty run never is the last such: its successor begins there too)
        for (uint64_t r0 = 0; r0 < chunk_rm; r0 += WAVE) {
          const uint64_t r = r0 + lane;
          uint32_t lo = 0, hi = 63;
          for (int s = 0; s < 6; ++s) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (shfl_u64(rx, mid) <= r) lo = mid;
            else hi = mid - 1;
          }
          const uint64_t k = r - shfl_u64(rx, lo);
          const uint64_t src = shfl_u64(lb, lo) + k, dst = shfl_u64(eoff, lo) + hdr + k;
          if (r < chunk_rm) out[dst] = sb[src];
        }
        base += chunk_words;
      }
    }
    if (t == 0) put_head(A, i, st, kind, p0, p1, vo, over ? 0 : total);
  }
}

__global__ void __launch_bounds__(256) k_ds_dup(const uint64_t *sorted, uint64_t n, uint32_t *ctr) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (sorted[i] == sorted[i - 1]) ctr[1] = 1;
}

bool up_cols_ok(const am_updates *u) {
  if (!u->row || !u->type || !u->op || !u->a0 || !u->a1) return false;
  return !(u->var_off && u->n_var && !u->var_data);
}
bool eff_cols_ok(const am_effects *e) {
  return e->eff_off && e->eff_meta && e->p0 && e->p1 && e->var_off && e->n_var && (e->var_data || !e->var_cap);
}

// rows_checked: the caller has already found the rows distinct (the host paths), so the device
// check -- a sort of the rows and k_ds_dup -- is skipped
int launch_downstream(am_ctx *ctx, uint32_t nd, const am_updates *up, const am_values *in, const int32_t *in_status,
                      const am_effects *eff, int32_t *out_status, bool rows_checked) {
  const uint64_t n = up->n_up;
  AM_HIP(hipSetDevice(ctx->device));
  if (n == 0) {
    AM_HIP(hipMemsetAsync(eff->n_var, 0, 8, ctx->stream));
    AM_HIP(hipMemsetAsync(eff->eff_off, 0, 8, ctx->stream));
    AM_HIP(hipMemsetAsync(eff->var_off, 0, 8, ctx->stream));
    return AM_OK;
  }
  if (n >= 0x7FFFFFFFull) {
    am_set_error("am_generate_downstream: more than 2^31 - 2 updates");
    return AM_ERR_UNSUPPORTED;
  }
  uint64_t *cnt = nullptr, *off = nullptr, *srt = nullptr;
  size_t scan_b = 0, sort_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, cnt, off, (int)(n + 1), ctx->stream) != hipSuccess ||
      hipcub::DeviceRadixSort::SortKeys(nullptr, sort_b, up->row, srt, (int)n, 0, 64, ctx->stream) != hipSuccess) {
    am_set_error("am_generate_downstream: sizing the scan failed");
    return AM_ERR_HIP;
  }
  const size_t tmp_b = ((scan_b > sort_b ? scan_b : sort_b) + 255) & ~(size_t)255;
  const size_t col = ((n + 1) * 8 + 255) & ~(size_t)255;
  void *scr = nullptr;
  if (int rc = am_ctx_scratch(ctx, AM_SCR_DOWN, 256 + 4 * col + tmp_b, &scr)) return rc;
  char *p = (char *)scr;
  uint32_t *ctr = (uint32_t *)p;
  cnt = (uint64_t *)(p + 256), off = (uint64_t *)(p + 256 + col), srt = (uint64_t *)(p + 256 + 2 * col);
  uint32_t *big_list = (uint32_t *)(p + 256 + 3 * col);
  void *tmp = p + 256 + 4 * col;
  AM_HIP(hipMemsetAsync(ctr, 0, 16, ctx->stream));
  const uint64_t lane_cap = (uint64_t)ctx->n_cu * 8;
  uint64_t blocks = (n + 255) / 256;
  size_t tb = tmp_b;
  if (!rows_checked) {
    if (hipcub::DeviceRadixSort::SortKeys(tmp, tb, up->row, srt, (int)n, 0, 64, ctx->stream) != hipSuccess) {
      am_set_error("am_generate_downstream: sorting the rows failed");
      return AM_ERR_HIP;
    }
    hipLaunchKernelGGL(k_ds_dup, dim3((unsigned)(blocks < lane_cap ? blocks : lane_cap)), dim3(256), 0, ctx->stream, srt, n,
                       ctr);
  }
  DsArgs A{*up, *in, in_status, *eff, out_status, nd, cnt, off, big_list, ctr};
  blocks = (n + PER_BLOCK - 1) / PER_BLOCK;
  const unsigned grid = (unsigned)(blocks < lane_cap ? blocks : lane_cap);
  hipLaunchKernelGGL(k_ds_size, dim3(grid), dim3(256), 0, ctx->stream, A);
  tb = tmp_b;
  if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, off, (int)(n + 1), ctx->stream) != hipSuccess) {
    am_set_error("am_generate_downstream: the scan failed");
    return AM_ERR_HIP;
  }
  AM_HIP(hipMemcpyAsync(eff->n_var, off + n, 8, hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(k_ds_fill<64>, dim3(grid), dim3(256), 0, ctx->stream, A);
  const uint64_t wg_cap = (uint64_t)ctx->n_cu * 4;
  hipLaunchKernelGGL(k_ds_fill<256>, dim3((unsigned)(n < wg_cap ? n : wg_cap)), dim3(256), 0, ctx->stream, A);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

bool host_up_ok(const am_updates *u, uint64_t n_rows) {
  if (!up_cols_ok(u)) return false;
  if (u->var_off && u->n_up && u->var_off[u->n_up] > u->n_var) return false;
  for (uint64_t i = 0; i < u->n_up; ++i)
    if (u->row[i] >= n_rows) return false;
  return true;
}
bool rows_distinct(const am_updates *u) {
  std::vector<uint64_t> r(u->row, u->row + u->n_up);
  std::sort(r.begin(), r.end());
  return std::adjacent_find(r.begin(), r.end()) == r.end();
}

// Host updates (rows of the DEVICE values dv / statuses dst, found distinct by the caller) -> host
// effects: staged, generated,
// and only the effects copied back, with one readback of *n_var to size the copy.
int downstream_to_host(am_ctx *ctx, uint32_t nd, const am_updates *hu, const am_values *dv, const int32_t *dst,
                       am_effects *he, int32_t *out_status) {
  const uint64_t n = hu->n_up;
  const bool var = hu->var_off != nullptr;
  am_stage st;
  const size_t i_row = st.add(hu->row, n * 8), i_type = st.add(hu->type, n), i_op = st.add(hu->op, n);
  const size_t i_a0 = st.add(hu->a0, n * 8), i_a1 = st.add(hu->a1, n * 8);
  const size_t i_vo = st.add(hu->var_off, var ? (n + 1) * 8 : 0), i_vd = st.add(hu->var_data, var ? hu->n_var * 8 : 0);
  const size_t o_eo = st.add(nullptr, (n + 1) * 8), o_m = st.add(nullptr, n), o_p0 = st.add(nullptr, n * 8);
  const size_t o_p1 = st.add(nullptr, n * 8), o_vo = st.add(nullptr, (n + 1) * 8), o_vd = st.add(nullptr, he->var_cap * 8);
  const size_t o_nv = st.add(nullptr, 8), o_av = st.add(nullptr, n * 8), o_st = st.add(nullptr, n * 4);
  int rc = st.upload(ctx);
  hipError_t e = hipSuccess;
  if (!rc) {
    am_updates du = *hu;
    du.row = st.dev<uint64_t>(i_row), du.type = st.dev<uint8_t>(i_type), du.op = st.dev<uint8_t>(i_op);
    du.a0 = st.dev<uint64_t>(i_a0), du.a1 = st.dev<uint64_t>(i_a1);
    du.var_off = var ? st.dev<uint64_t>(i_vo) : nullptr, du.var_data = var ? st.dev<uint64_t>(i_vd) : nullptr;
    am_effects de{};
    de.var_cap = he->var_cap;
    de.eff_off = st.dev<uint64_t>(o_eo), de.eff_meta = st.dev<uint8_t>(o_m), de.p0 = st.dev<uint64_t>(o_p0);
    de.p1 = st.dev<uint64_t>(o_p1), de.var_off = st.dev<uint64_t>(o_vo), de.var_data = st.dev<uint64_t>(o_vd);
    de.n_var = st.dev<uint64_t>(o_nv), de.avail = he->avail ? st.dev<int64_t>(o_av) : nullptr;
    rc = launch_downstream(ctx, nd, &du, dv, dst, &de, st.dev<int32_t>(o_st), true);
    auto back = [&](void *h, const void *d, size_t bytes) {
      if (h && bytes && e == hipSuccess && !rc) e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    back(he->n_var, de.n_var, 8);
    back(out_status, st.dev<int32_t>(o_st), n * 4);
    back(he->eff_off, de.eff_off, (n + 1) * 8), back(he->eff_meta, de.eff_meta, n);
    back(he->p0, de.p0, n * 8), back(he->p1, de.p1, n * 8), back(he->var_off, de.var_off, (n + 1) * 8);
    back(he->avail, de.avail, n * 8);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // *n_var sizes the last copy
    if (e == hipSuccess && !rc && *he->n_var <= he->var_cap && *he->n_var) {
      e = hipMemcpyAsync(he->var_data, de.var_data, *he->n_var * 8, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
  } else {
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (st.arena) am_dev_release(ctx, st.arena);
  if (e != hipSuccess) {
    am_set_error("am_generate_downstream: %s", hipGetErrorString(e));
    return AM_ERR_HIP;
  }
  return rc;
}

}  // namespace

extern "C" int am_generate_downstream(am_ctx *ctx, uint32_t n_dc, const am_updates *up, const am_values *in,
                                      const int32_t *in_status, am_effects *eff, int32_t *out_status) {
  if (!ctx || !up || !in || !eff || !out_status || n_dc == 0 || n_dc > AM_MAX_DC) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  if (!eff_cols_ok(eff) || (up->n_up && !up_cols_ok(up))) {
    am_set_error("am_generate_downstream: the updates or the effects lack a column");
    return AM_ERR_INVALID;
  }
  return launch_downstream(ctx, n_dc, up, in, in_status, eff, out_status, false);
}

extern "C" int am_generate_downstream_host(am_ctx *ctx, uint32_t n_dc, const am_updates *hu, const am_values *hin,
                                           const int32_t *in_status, am_effects *he, int32_t *out_status) {
  if (!ctx || !hu || !hin || !he || !out_status || n_dc == 0 || n_dc > AM_MAX_DC) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  if (!eff_cols_ok(he) || (hu->n_up && !host_up_ok(hu, ~0ull))) {
    am_set_error("am_generate_downstream_host: the updates or the effects lack a column");
    return AM_ERR_INVALID;
  }
  const uint64_t n = hu->n_up;
  if (n == 0) {
    *he->n_var = 0, he->eff_off[0] = 0, he->var_off[0] = 0;
    return AM_OK;
  }
  if (!rows_distinct(hu)) {
    am_set_error("am_generate_downstream_host: two updates name one row (one key's updates are separate calls)");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  // the rows the updates name, gathered: update i reads row i of the staged values
  const bool sets = hin->set_off && hin->set_len && hin->set_a && hin->set_b;
  std::vector<uint64_t> rows(n), so(n + 1, 0), sa, sb;
  std::vector<uint32_t> sl(n, 0);
  std::vector<int32_t> ist(n, AM_OK);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = hu->row[i];
    rows[i] = i;
    if (in_status) ist[i] = in_status[r];
    const uint8_t t = hu->type[i];
    if (sets && ist[i] == AM_OK && (t == AM_AWSET || t == AM_MVREG || t == AM_BCOUNTER)) {
      sl[i] = hin->set_len[r];
      const uint64_t o = hin->set_off[r];
      sa.insert(sa.end(), hin->set_a + o, hin->set_a + o + sl[i]);
      sb.insert(sb.end(), hin->set_b + o, hin->set_b + o + sl[i]);
    }
    so[i + 1] = sa.size();
  }
  am_stage st;
  const size_t i_so = st.add(so.data(), (n + 1) * 8), i_sl = st.add(sl.data(), n * 4);
  const size_t i_sa = st.add(sa.data(), sa.size() * 8), i_sb = st.add(sb.data(), sb.size() * 8);
  const size_t i_st = st.add(ist.data(), n * 4);
  int rc = st.upload(ctx);
  if (!rc) {
    am_values dv{};
    if (sets)
      dv.set_off = st.dev<uint64_t>(i_so), dv.set_len = st.dev<uint32_t>(i_sl), dv.set_a = st.dev<uint64_t>(i_sa),
      dv.set_b = st.dev<uint64_t>(i_sb);
    am_updates hu2 = *hu;
    hu2.row = rows.data();
    rc = downstream_to_host(ctx, n_dc, &hu2, &dv, st.dev<int32_t>(i_st), he, out_status);
  }
  (void)hipStreamSynchronize(ctx->stream);
  if (st.arena) am_dev_release(ctx, st.arena);
  return rc;
}

int am_downstream_apply_result(am_ctx *ctx, uint32_t n_dc, uint64_t n_rows, const am_updates *hu, const am_read_result *dr,
                               am_effects *he, int32_t *out_status) {
  if (!ctx || !hu || !dr || !dr->status || !he || !out_status) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  if (!eff_cols_ok(he) || (hu->n_up && !host_up_ok(hu, n_rows))) {
    am_set_error("am_update_objects: the updates or the effects lack a column, or a row lies outside the batch");
    return AM_ERR_INVALID;
  }
  if (hu->n_up == 0) {
    *he->n_var = 0, he->eff_off[0] = 0, he->var_off[0] = 0;
    return AM_OK;
  }
  if (!rows_distinct(hu)) {
    am_set_error("am_update_objects: two updates name one request (one key's updates are separate calls)");
    return AM_ERR_INVALID;
  }
  return downstream_to_host(ctx, n_dc, hu, &dr->value, dr->status, he, out_status);
}
