// am_commit.hip -- the commit's op log, built on the device: clocksi_vnode:commit/5 ->
// update_materializer/3 (src/clocksi_vnode.erl:499-531, 634-657) stamps every effect of a
// transaction with {DcId, TxCommitTime}, its vec_snapshot_time and its TxId and hands it to
// materializer_vnode:update/2 -> op_insert_gc/3; inter_dc_dep_vnode does the same for a remote
// transaction (src/inter_dc_dep_vnode.erl:150-152).  A batch of committed transactions (am_commits:
// one row per transaction, one per effect) becomes the CSR log over the touched keys that
// am_store_apply takes as dev_new -- a sort, two scans and a gather:
//   k_cm_expand   one thread per effect: its transaction (a search of eff_off), the pair (key,
//                 effect index), its variable word count; every validity flag of the batch
//   radix sort    of the pairs by key, stable, over the key bits the caller names (hipcub): a
//                 key's ops end up ordered by (transaction, effect in the transaction)
//   k_cm_heads    head flag and word count per sorted op; two exclusive scans (hipcub) -> the key
//                 index of every op, var_off
//   k_cm_keys     keys, key_off, key_type, key_flags (a key whose adjacent ops disagree on the type)
//   k_cm_fill     one wavefront per 64 sorted ops: lane q loads its op's source index and
//                 transaction once; the scalar columns and each DC's snap_vc column leave as one
//                 coalesced store per column per wave; the tile's variable words are copied flat,
//                 consecutive lanes on consecutive output words, each finding its op by a shuffle
//                 search of the tile's word prefix (as k_ds_fill does for remove tokens), looping
//                 for as long as the tile has words (an add-wins reset over a large state)
// One readback: the status block (flags, n_touched).  The kernels are safe on an invalid batch:
// the word counts of bad offsets are 0, transaction indices are clamped, and the fill does nothing
// once a flag is set.
//   k_cm_slice_*  the ops [beg_i, end_i) of built key i as a smaller CSR log (a round of
//                 am_vnode_commit_host that stops at a GC trigger)
//   k_cm_spread   key_off / key_type / key_flags over all vnode keys from the touched list (the
//                 rebuild fallback; the keys are ascending, so the op columns are reused)
#include <hipcub/hipcub.hpp>

#include "am_block.h"

using namespace amk;

namespace {

struct CmArgs {
  am_commits C;
  am_commit_log O;
  uint32_t nd, key_bits;
  uint64_t *key_in, *key_srt;  // [n] the effects' keys, unsorted and sorted
  uint32_t *val_in, *tx_of;    // [n] effect index; the effect's transaction
  uint64_t *wcnt;              // [n] variable words per effect
  uint64_t *head, *rank;       // [n+1] head flags of the sorted ops, their exclusive scan
  uint64_t *wsrt;              // [n+1] variable words per sorted op
  uint64_t *stat;              // [0] AM_COMMIT_BAD_* [1] n_touched
};

// first index in [0, n) of a with a[x] > e
__device__ __forceinline__ uint64_t upper(const uint64_t *a, uint64_t n, uint64_t e) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void flag(uint64_t *stat, uint32_t f) { atomicOr((unsigned long long *)stat, (unsigned long long)f); }

__global__ void __launch_bounds__(256) k_cm_expand(CmArgs A) {
  const uint64_t n = A.C.n_eff, nt = A.C.n_tx;
  const uint64_t span = n > nt + 1 ? n : nt + 1;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < span; e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t bad = 0;
    if (e < nt) {
      if (A.C.dc[e] >= A.nd) bad |= AM_COMMIT_BAD_DC;
      if (A.C.eff_off[e] > A.C.eff_off[e + 1]) bad |= AM_COMMIT_BAD_EFF_OFF;
    }
    if (e == nt && (A.C.eff_off[0] != 0 || A.C.eff_off[nt] != n)) bad |= AM_COMMIT_BAD_EFF_OFF;
    if (e < n) {
      const uint64_t u = upper(A.C.eff_off, nt + 1, e);  // the last transaction beginning at or before e
      const uint64_t t = u == 0 ? 0 : (u - 1 < nt ? u - 1 : nt - 1);
      const uint64_t k = A.C.key[e];
      const uint32_t type = A.C.type[e];
      uint64_t w = 0;
      if (A.C.var_off) {
        const uint64_t a = A.C.var_off[e], b = A.C.var_off[e + 1];
        if (a > b || b > A.C.n_var) bad |= AM_COMMIT_BAD_VAR_OFF;
        else w = b - a;
      }
      if (type < AM_PN || type > AM_BCOUNTER) bad |= AM_COMMIT_BAD_TYPE;
      if (A.key_bits < 64 && (k >> A.key_bits)) bad |= AM_COMMIT_BAD_KEY;
      A.key_in[e] = k;
      A.val_in[e] = (uint32_t)e;
      A.tx_of[e] = (uint32_t)t;
      A.wcnt[e] = w;
    }
    if (bad) flag(A.stat, bad);
  }
}

__global__ void __launch_bounds__(256) k_cm_heads(CmArgs A) {
  const uint64_t n = A.C.n_eff;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n; q += (uint64_t)gridDim.x * blockDim.x) {
    A.head[q] = q < n && (q == 0 || A.key_srt[q] != A.key_srt[q - 1]) ? 1 : 0;
    A.wsrt[q] = q < n ? A.wcnt[A.O.src[q]] : 0;
  }
}

__global__ void __launch_bounds__(256) k_cm_keys(CmArgs A) {
  const uint64_t n = A.C.n_eff;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t type = A.C.type[A.O.src[q]];
    if (A.head[q]) {
      const uint64_t i = A.rank[q];
      A.O.keys[i] = A.key_srt[q];
      A.O.key_off[i] = q;
      A.O.key_type[i] = (uint8_t)type;
    } else if (type != A.C.type[A.O.src[q - 1]]) {
      // some adjacent pair of a key's run disagrees iff the run does (key_flags cleared before)
      A.O.key_flags[A.rank[q] - 1] = AM_KEY_MIXED_TYPES;
    }
    if (q == n - 1) {
      A.O.key_off[A.rank[n]] = n;
      A.stat[1] = A.rank[n];
    }
  }
}

__global__ void __launch_bounds__(256) k_cm_fill(CmArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n = A.C.n_eff, nd = A.nd;
  if (uniform_u64(A.stat[0])) return;  // an invalid batch: offsets and indices are not to be trusted
  const uint64_t tiles = (n + WAVE - 1) / WAVE, waves = (uint64_t)gridDim.x * (blockDim.x / WAVE);
  for (uint64_t tile = (uint64_t)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6); tile < tiles; tile += waves) {
    const uint64_t q = tile * WAVE + lane;
    const bool has = q < n;
    const uint64_t s = has ? A.O.src[q] : 0;
    const uint64_t t = has ? A.tx_of[s] : 0;
    if (has) {
      A.O.op_meta[q] = (uint8_t)((A.C.dc[t] & 0x1Fu) | (A.C.eff_meta[s] & 0xE0u));
      A.O.commit_time[q] = A.C.commit_time[t];
      if (A.C.snap_pres) A.O.snap_pres[q] = A.C.snap_pres[t];
      if (A.C.txid) A.O.op_txid[q] = A.C.txid[t];
      A.O.p0[q] = A.C.p0[s];
      A.O.p1[q] = A.C.p1[s];
      for (uint64_t d = 0; d < nd; ++d) A.O.snap_vc[d * A.O.snap_stride + q] = A.C.snap_vc[t * nd + d];
    }
    // the tile's variable words, flat: word w belongs to the last op whose words begin at or before
    // w (an op without words never is the last such: its successor begins there too)
    const uint64_t last = (tile + 1) * WAVE < n ? (tile + 1) * WAVE : n;
    const uint64_t tile_end = uniform_u64(A.O.var_off[last]);
    const uint64_t vo = has ? A.O.var_off[q] : tile_end;
    const uint64_t sv = has && A.C.var_off ? A.C.var_off[s] : 0;
    for (uint64_t r0 = lane_u64(vo, 0); r0 < tile_end; r0 += WAVE) {
      const uint64_t w = r0 + lane;
      uint32_t lo = 0, hi = 63;
      for (int step = 0; step < 6; ++step) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (shfl_u64(vo, mid) <= w) lo = mid;
        else hi = mid - 1;
      }
      const uint64_t from = shfl_u64(sv, lo) + (w - shfl_u64(vo, lo));
      if (w < tile_end) A.O.var_data[w] = A.C.var_data[from];
    }
  }
}

struct SlArgs {
  am_op_log B;
  am_commit_log O;
  uint64_t m, n_out, v_out;
  const uint64_t *idx, *beg, *ooff, *voff;
};

__global__ void __launch_bounds__(256) k_cm_slice_ops(SlArgs A) {
  const uint64_t nd = A.B.n_dc, bs = A.B.snap_stride ? A.B.snap_stride : A.B.n_ops;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < A.n_out; q += (uint64_t)gridDim.x * blockDim.x) {
    if (q < A.m) {  // every entry holds at least one op: q covers the entries
      A.O.key_off[q] = A.ooff[q];
      A.O.key_type[q] = A.B.key_type[A.idx[q]];
      A.O.key_flags[q] = A.B.key_flags[A.idx[q]];
      if (q == 0) A.O.key_off[A.m] = A.n_out, A.O.var_off[A.n_out] = A.v_out;
    }
    const uint64_t i = upper(A.ooff, A.m + 1, q) - 1;
    const uint64_t b = A.beg[i], p = b + (q - A.ooff[i]);
    A.O.op_meta[q] = A.B.op_meta[p];
    A.O.commit_time[q] = A.B.commit_time[p];
    if (A.B.snap_pres) A.O.snap_pres[q] = A.B.snap_pres[p];
    if (A.B.op_txid) A.O.op_txid[q] = A.B.op_txid[p];
    A.O.p0[q] = A.B.p0[p];
    A.O.p1[q] = A.B.p1[p];
    for (uint64_t d = 0; d < nd; ++d) A.O.snap_vc[d * A.O.snap_stride + q] = A.B.snap_vc[d * bs + p];
    A.O.var_off[q] = A.voff[i] + (A.B.var_off[p] - A.B.var_off[b]);
  }
}

// a key's ops are contiguous in B, so entry i's words are the run from B.var_off[beg_i]
__global__ void __launch_bounds__(256) k_cm_slice_words(SlArgs A) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < A.v_out; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = upper(A.voff, A.m + 1, w) - 1;
    A.O.var_data[w] = A.B.var_data[A.B.var_off[A.beg[i]] + (w - A.voff[i])];
  }
}

__global__ void __launch_bounds__(256) k_cm_spread(am_op_log T, const uint64_t *keys, uint64_t n_keys, uint64_t *off,
                                                   uint8_t *type, uint8_t *flags) {
  const uint64_t m = T.n_keys;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n_keys; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = k ? upper(keys, m, k - 1) : 0;  // the first touched key >= k
    off[k] = T.key_off[i];
    if (k == n_keys) continue;
    const bool hit = i < m && keys[i] == k;
    type[k] = hit ? T.key_type[i] : (uint8_t)AM_PN;
    flags[k] = hit && T.key_flags ? T.key_flags[i] : 0;
  }
}

unsigned grid_for(am_ctx *c, uint64_t items, uint64_t per_block) {
  const uint64_t b = (items + per_block - 1) / per_block, cap = (uint64_t)c->n_cu * 8;
  return (unsigned)(b == 0 ? 1 : b < cap ? b : cap);
}

bool out_cols_ok(const am_commit_log *o, bool pres, bool txid) {
  return o->keys && o->key_off && o->key_type && o->key_flags && o->op_meta && o->commit_time && o->snap_vc && o->p0 &&
         o->p1 && o->var_off && (o->var_data || !o->cap_var) && o->src && (!pres || o->snap_pres) && (!txid || o->op_txid);
}

void log_over(const am_commit_log &o, uint32_t nd, uint64_t nk, uint64_t n, uint64_t nv, bool pres, bool txid, am_op_log *L) {
  *L = am_op_log{};
  L->n_dc = nd, L->n_keys = nk, L->n_ops = n, L->n_var = nv, L->snap_stride = o.snap_stride;
  L->key_off = o.key_off, L->key_type = o.key_type, L->key_flags = o.key_flags;
  L->op_meta = o.op_meta, L->commit_time = o.commit_time, L->snap_vc = o.snap_vc;
  L->snap_pres = pres ? o.snap_pres : nullptr, L->op_txid = txid ? o.op_txid : nullptr;
  L->p0 = o.p0, L->p1 = o.p1, L->var_off = o.var_off, L->var_data = o.var_data;
}

}  // namespace

extern "C" int am_commit_build(am_ctx *ctx, uint32_t n_dc, const am_commits *cm, uint32_t key_bits, const am_commit_log *out,
                               am_op_log *out_log, uint64_t *n_touched, uint32_t *bad) {
  if (!ctx || !cm || !out || !out_log || !n_touched || n_dc == 0 || n_dc > AM_MAX_DC || key_bits == 0 || key_bits > 64)
    return AM_ERR_INVALID;
  AM_LOCK(ctx);
  *n_touched = 0;
  if (bad) *bad = 0;
  const uint64_t n = cm->n_eff, nt = cm->n_tx;
  if (n >> 32 || nt >> 32) {
    am_set_error("am_commit_build: 2^32 or more effects or transactions in one batch");
    return AM_ERR_INVALID;
  }
  if (nt == 0 || n == 0) {
    if (n) {
      am_set_error("am_commit_build: effects without a transaction");
      return AM_ERR_INVALID;
    }
    log_over(*out, n_dc, 0, 0, 0, false, false, out_log);
    return AM_OK;
  }
  const bool pres = cm->snap_pres != nullptr, txid = cm->txid != nullptr;
  if (!cm->dc || !cm->commit_time || !cm->snap_vc || !cm->eff_off || !cm->key || !cm->type || !cm->eff_meta || !cm->p0 ||
      !cm->p1 || (cm->var_off && cm->n_var && !cm->var_data) || !out_cols_ok(out, pres, txid) || out->cap_ops < n ||
      out->cap_var < (cm->var_off ? cm->n_var : 0) || out->snap_stride < n) {
    am_set_error("am_commit_build: the batch or the output lacks a column, or the output is smaller than the batch");
    return AM_ERR_INVALID;
  }
  if (n >= 0x7FFFFFFFull) {
    am_set_error("am_commit_build: more than 2^31 - 2 effects");
    return AM_ERR_UNSUPPORTED;
  }
  AM_HIP(hipSetDevice(ctx->device));
  CmArgs A{};
  A.C = *cm, A.O = *out, A.nd = n_dc, A.key_bits = key_bits;
  size_t scan_b = 0, sort_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, A.head, A.rank, (int)(n + 1), ctx->stream) != hipSuccess ||
      hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, A.key_in, A.key_srt, A.val_in, A.O.src, (int)n, 0, (int)key_bits,
                                         ctx->stream) != hipSuccess) {
    am_set_error("am_commit_build: sizing the sort failed");
    return AM_ERR_HIP;
  }
  const size_t tmp_b = ((scan_b > sort_b ? scan_b : sort_b) + 255) & ~(size_t)255;
  const size_t c8 = ((n + 1) * 8 + 255) & ~(size_t)255, c4 = ((n + 1) * 4 + 255) & ~(size_t)255;
  void *scr = nullptr;
  if (int rc = am_ctx_scratch(ctx, AM_SCR_COMMIT, 256 + 6 * c8 + 2 * c4 + tmp_b, &scr)) return rc;
  char *p = (char *)scr;
  A.stat = (uint64_t *)p, p += 256;
  A.key_in = (uint64_t *)p, p += c8;
  A.key_srt = (uint64_t *)p, p += c8;
  A.wcnt = (uint64_t *)p, p += c8;
  A.head = (uint64_t *)p, p += c8;
  A.rank = (uint64_t *)p, p += c8;
  A.wsrt = (uint64_t *)p, p += c8;
  A.val_in = (uint32_t *)p, p += c4;
  A.tx_of = (uint32_t *)p, p += c4;
  void *tmp = p;
  AM_HIP(hipMemsetAsync(A.stat, 0, 32, ctx->stream));
  AM_HIP(hipMemsetAsync(A.O.key_flags, 0, n, ctx->stream));
  const uint64_t span = n > nt + 1 ? n : nt + 1;
  hipLaunchKernelGGL(k_cm_expand, dim3(grid_for(ctx, span, 256)), dim3(256), 0, ctx->stream, A);
  size_t tb = tmp_b;
  if (hipcub::DeviceRadixSort::SortPairs(tmp, tb, A.key_in, A.key_srt, A.val_in, A.O.src, (int)n, 0, (int)key_bits,
                                         ctx->stream) != hipSuccess) {
    am_set_error("am_commit_build: the sort failed");
    return AM_ERR_HIP;
  }
  hipLaunchKernelGGL(k_cm_heads, dim3(grid_for(ctx, n + 1, 256)), dim3(256), 0, ctx->stream, A);
  tb = tmp_b;
  bool ok = hipcub::DeviceScan::ExclusiveSum(tmp, tb, A.head, A.rank, (int)(n + 1), ctx->stream) == hipSuccess;
  tb = tmp_b;
  ok = ok && hipcub::DeviceScan::ExclusiveSum(tmp, tb, A.wsrt, A.O.var_off, (int)(n + 1), ctx->stream) == hipSuccess;
  if (!ok) {
    am_set_error("am_commit_build: the scans failed");
    return AM_ERR_HIP;
  }
  hipLaunchKernelGGL(k_cm_keys, dim3(grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, A);
  hipLaunchKernelGGL(k_cm_fill, dim3(grid_for(ctx, (n + WAVE - 1) / WAVE, 4)), dim3(256), 0, ctx->stream, A);
  AM_HIP(hipGetLastError());
  uint64_t st[2] = {0, 0};
  if (int rc = am_ctx_fetch(ctx, A.stat, 2, st)) return rc;
  if (st[0]) {
    if (bad) *bad = (uint32_t)st[0];
    am_set_error("am_commit_build: invalid batch (AM_COMMIT_BAD_* 0x%x)", (unsigned)st[0]);
    return AM_ERR_INVALID;
  }
  *n_touched = st[1];
  log_over(*out, n_dc, st[1], n, cm->var_off ? cm->n_var : 0, pres, txid, out_log);
  return AM_OK;
}

int am_commit_slice(am_ctx *c, const am_op_log &B, uint64_t m, const uint64_t *idx, const uint64_t *beg,
                    const uint64_t *ooff, const uint64_t *voff, uint64_t n_out, uint64_t v_out, const am_commit_log &out,
                    am_op_log *out_log) {
  AM_LOCK(c);
  if (m == 0 || n_out < m || out.cap_ops < n_out || out.cap_var < v_out || out.snap_stride < n_out) return AM_ERR_INVALID;
  SlArgs A{B, out, m, n_out, v_out, idx, beg, ooff, voff};
  hipLaunchKernelGGL(k_cm_slice_ops, dim3(grid_for(c, n_out, 256)), dim3(256), 0, c->stream, A);
  if (v_out) hipLaunchKernelGGL(k_cm_slice_words, dim3(grid_for(c, v_out, 256)), dim3(256), 0, c->stream, A);
  AM_HIP(hipGetLastError());
  log_over(out, B.n_dc, m, n_out, v_out, B.snap_pres != nullptr, B.op_txid != nullptr, out_log);
  return AM_OK;
}

int am_commit_spread(am_ctx *c, const am_op_log &T, const uint64_t *keys, uint64_t n_keys, uint64_t *off, uint8_t *type,
                     uint8_t *flags) {
  AM_LOCK(c);
  hipLaunchKernelGGL(k_cm_spread, dim3(grid_for(c, n_keys + 1, 256)), dim3(256), 0, c->stream, T, keys, n_keys, off, type,
                     flags);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
