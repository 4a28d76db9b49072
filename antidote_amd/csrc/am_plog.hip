// am_plog.hip -- the partition's log in HBM and the cold read served from it:
// materializer_vnode:get_from_snapshot_log/3 -> logging_vnode:get_up_to_time/5
// (src/materializer_vnode.erl:415-419, src/logging_vnode.erl:522-545, 586-591, 676-779).  When no
// cached snapshot lies at or below a read's clock the reference rebuilds the key's ops from the log
// -- every update of a committed transaction whose snapshot_time is vectorclock:le the read clock,
// ids 0, 1, 2 ... oldest first -- and materializes them from new(Type) under the clock {}.
// The log is the sequence of commit batches (am_commits), kept transaction-major as they arrive:
//   per transaction   dc, commit_time, snap_vc (one row of n_dc words), snap_pres, txid
//   per effect        key, type, eff_meta, p0, p1, var_off (+ var_data)
//   link[e]           {the previous effect on e's key or PL_NONE, e's transaction}: one 16-byte
//                     record per chain hop
//   key_last[k]       the newest effect of key k, or PL_NONE
// Every column doubles when it fills (new block, device copy, the old block back to the context).
//   k_pl_append   one thread per transaction / effect of a batch: its rows, behind the log's
//   k_pl_link     the chain links from am_commit_build's output, where a key's ops are consecutive
//                 and src names their batch effects: a later op links to its predecessor, a key's
//                 first op to the old key_last, and its last op becomes key_last
//   k_pl_walk     one lane per read: key_last -> link newest to oldest, skipping transactions at or
//                 above the read's horizon, testing le(snapshot_time, read clock) on the
//                 transaction's row.  The next hop's link is loaded before the row is looked at.
//                 Counts survivors and their variable words; after two exclusive scans (hipcub) the
//                 same walk writes the survivors' effect indices oldest first
//   k_pl_gather   one thread per survivor: a plain am_op_log whose "keys" are the reads
//   k_pl_words    the survivors' variable words
// am_launch_materialize then reads that log as it is, from new() under base clock {}.
#include <hipcub/hipcub.hpp>

#include "am_internal.h"

int am_run_host_batch(am_ctx *c, const am_store *st, const am_read_batch *hb, am_read_result *hr,
                      const void *extra_host, size_t extra_bytes,
                      int (*run)(void *arg, const am_read_batch *db, am_read_result *dr, const void *extra_dev),
                      void *arg, bool values_on_device = false);  // am_host.hip

namespace {

constexpr uint64_t PL_NONE = ~0ull;

}  // namespace

struct am_plog {
  am_ctx *ctx = nullptr;
  uint32_t n_dc = 0;
  uint64_t n_tx = 0, n_eff = 0, n_var = 0, n_keys = 0;  // used
  uint64_t cap_tx = 0, cap_eff = 0, cap_var = 0, cap_keys = 0;
  uint8_t *dc = nullptr;          // [cap_tx]
  uint64_t *commit_time = nullptr, *snap_vc = nullptr, *txid = nullptr;  // [cap_tx], [cap_tx][n_dc], [cap_tx]
  uint32_t *snap_pres = nullptr;  // [cap_tx]
  uint64_t *key = nullptr, *p0 = nullptr, *p1 = nullptr, *var_off = nullptr;  // [cap_eff] ([cap_eff+1])
  uint8_t *type = nullptr, *eff_meta = nullptr;  // [cap_eff]
  uint64_t *link = nullptr;       // [cap_eff][2]
  uint64_t *var_data = nullptr;   // [cap_var]
  uint64_t *key_last = nullptr;   // [cap_keys]
};

namespace {

// the log as the kernels take it
struct PlView {
  uint32_t nd;
  uint64_t n_tx, n_eff, n_keys;
  const uint8_t *dc;
  const uint64_t *commit_time, *snap_vc, *txid;
  const uint32_t *snap_pres;
  const uint8_t *type, *eff_meta;
  const uint64_t *p0, *p1, *var_off, *var_data;
  const ulonglong2 *link;
  const uint64_t *key_last;
};

PlView view_of(const am_plog *g) {
  return PlView{g->n_dc, g->n_tx, g->n_eff, g->n_keys, g->dc, g->commit_time, g->snap_vc, g->txid, g->snap_pres,
                g->type, g->eff_meta, g->p0, g->p1, g->var_off, g->var_data, (const ulonglong2 *)g->link, g->key_last};
}

unsigned grid_for(am_ctx *c, uint64_t items, uint64_t per_block) {
  const uint64_t b = (items + per_block - 1) / per_block, cap = (uint64_t)c->n_cu * 8;
  return (unsigned)(b == 0 ? 1 : b < cap ? b : cap);
}

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

struct ApArgs {
  am_commits C;  // the batch (device, validated by am_commit_build)
  uint32_t nd;
  uint64_t n_tx, n_eff, n_var;  // the log's sizes before the batch
  uint8_t *dc;
  uint64_t *commit_time, *snap_vc, *txid;
  uint32_t *snap_pres;
  uint64_t *key, *p0, *p1, *var_off;
  uint8_t *type, *eff_meta;
  uint64_t *link, *key_last;
  const uint32_t *src;      // [n_eff of the batch] the batch effect of every built op
  const uint64_t *bkey_off; // [m+1] the built log's key_off
  uint64_t m;
};

__global__ void __launch_bounds__(256) k_pl_append(ApArgs A) {
  const uint64_t n = A.C.n_eff, nt = A.C.n_tx, nd = A.nd;
  const uint64_t span = n > nt ? n : nt;
  const uint32_t all = nd >= 32 ? 0xFFFFFFFFu : ((1u << nd) - 1u);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < span; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i < nt) {
      const uint64_t t = A.n_tx + i;
      A.dc[t] = A.C.dc[i];
      A.commit_time[t] = A.C.commit_time[i];
      for (uint64_t d = 0; d < nd; ++d) A.snap_vc[t * nd + d] = A.C.snap_vc[i * nd + d];
      A.snap_pres[t] = A.C.snap_pres ? (A.C.snap_pres[i] & all) : all;
      A.txid[t] = A.C.txid ? A.C.txid[i] : 0;
    }
    if (i < n) {
      const uint64_t e = A.n_eff + i;
      const uint64_t u = upper(A.C.eff_off, nt + 1, i);  // the last transaction beginning at or before i
      const uint64_t t = u == 0 ? 0 : (u - 1 < nt ? u - 1 : nt - 1);
      A.key[e] = A.C.key[i];
      A.type[e] = A.C.type[i];
      A.eff_meta[e] = A.C.eff_meta[i];
      A.p0[e] = A.C.p0[i];
      A.p1[e] = A.C.p1[i];
      A.var_off[e + 1] = A.n_var + (A.C.var_off ? A.C.var_off[i + 1] : 0);
      A.link[2 * e + 1] = A.n_tx + t;
    }
  }
}

// Op q of the built log that is not its key's first links to its predecessor (thread q); key i's
// first op links to the old key_last and its last op becomes key_last (thread i): no word has two
// writers, and key_last[k] is read and written by one thread.
__global__ void __launch_bounds__(256) k_pl_link(ApArgs A) {
  const uint64_t n = A.C.n_eff;
  const uint64_t span = n > A.m ? n : A.m;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < span; q += (uint64_t)gridDim.x * blockDim.x) {
    if (q > 0 && q < n) {
      const uint64_t s = A.src[q], sp = A.src[q - 1];
      if (A.C.key[s] == A.C.key[sp]) A.link[2 * (A.n_eff + s)] = A.n_eff + sp;
    }
    if (q < A.m) {
      const uint64_t first = A.bkey_off[q], last = A.bkey_off[q + 1] - 1;
      const uint64_t sf = A.src[first], k = A.C.key[sf];
      A.link[2 * (A.n_eff + sf)] = A.key_last[k];
      A.key_last[k] = A.n_eff + A.src[last];
    }
  }
}

// the chain of `key` below `horizon`: its length in out[0], and (when it fits cap) the effect
// indices oldest first from out[1]; one thread (a test accessor)
__global__ void k_pl_chain(PlView P, uint64_t key, uint64_t horizon, uint64_t cap, uint64_t *out) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t c = 0;
  for (uint64_t e = key < P.n_keys ? P.key_last[key] : PL_NONE; e < P.n_eff; e = P.link[e].x)
    if (P.link[e].y < horizon) ++c;
  out[0] = c;
  if (c > cap) return;
  for (uint64_t e = key < P.n_keys ? P.key_last[key] : PL_NONE; e < P.n_eff; e = P.link[e].x)
    if (P.link[e].y < horizon) out[c--] = e;
}

// vectorclock:le(the transaction's snapshot_time, the read clock): over the keys of both, a missing
// entry is 0
__device__ __forceinline__ bool tx_le(const PlView &P, uint64_t t, const am_read_batch &B, uint64_t ci, uint64_t cs,
                                      uint32_t rp) {
  const uint32_t sp = P.snap_pres[t];
  const uint64_t *row = P.snap_vc + t * P.nd;
  bool ok = true;
  for (uint32_t d = 0; d < P.nd; ++d) {
    const uint64_t a = ((sp >> d) & 1u) ? row[d] : 0;
    const uint64_t b = ((rp >> d) & 1u) ? B.read_vc[(uint64_t)d * cs + ci] : 0;
    ok = ok && a <= b;
  }
  return ok;
}

// FILL = false: cnt[r] / wcnt[r] = read r's survivors and their variable words.  FILL = true: the
// survivors' effect indices at sel[koff[r] ..], oldest first.
template <bool FILL>
__global__ void __launch_bounds__(256)
k_pl_walk(PlView P, am_read_batch B, const uint64_t *hor, uint64_t *cnt, uint64_t *wcnt, const uint64_t *koff, uint64_t *sel) {
  const uint64_t n = B.n_reads;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = B.key[r];
    uint64_t h = hor ? hor[r] : P.n_tx;
    if (h > P.n_tx) h = P.n_tx;
    const uint64_t ci = B.per_read_clock ? r : 0, cs = B.per_read_clock ? n : 1;
    const uint32_t rp = B.read_pres[ci];
    uint64_t e = key < P.n_keys ? P.key_last[key] : PL_NONE;
    uint64_t c = 0, w = 0, pos = FILL ? koff[r + 1] : 0;
    ulonglong2 cur = e < P.n_eff ? P.link[e] : make_ulonglong2(PL_NONE, 0);
    while (e < P.n_eff) {
      // the next hop's record and this hop's transaction row are independent loads
      const ulonglong2 nxt = cur.x < P.n_eff ? P.link[cur.x] : make_ulonglong2(PL_NONE, 0);
      if (cur.y < h && tx_le(P, cur.y, B, ci, cs, rp)) {
        if (FILL) {
          if (pos > koff[r]) sel[--pos] = e;
        } else {
          ++c;
          w += P.var_off[e + 1] - P.var_off[e];
        }
      }
      e = cur.x;
      cur = nxt;
    }
    if (!FILL) cnt[r] = c, wcnt[r] = w;
  }
}

// the temporary log's columns (device)
struct TmpLog {
  uint64_t n_ops, stride;
  const uint64_t *koff, *sel;
  uint8_t *key_type, *key_flags, *op_meta;
  uint64_t *commit_time, *snap_vc, *op_txid, *p0, *p1, *wlen, *var_off, *var_data;
  uint32_t *snap_pres;
};

__global__ void __launch_bounds__(256) k_pl_gather(PlView P, uint64_t n_reads, TmpLog T) {
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < T.n_ops; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = T.sel[q];
    const uint64_t t = P.link[e].y;
    T.op_meta[q] = (uint8_t)((P.dc[t] & 0x1Fu) | (P.eff_meta[e] & 0xE0u));
    T.commit_time[q] = P.commit_time[t];
    for (uint32_t d = 0; d < P.nd; ++d) T.snap_vc[(uint64_t)d * T.stride + q] = P.snap_vc[t * P.nd + d];
    T.snap_pres[q] = P.snap_pres[t];
    T.op_txid[q] = P.txid[t];
    T.p0[q] = P.p0[e];
    T.p1[q] = P.p1[e];
    T.wlen[q] = P.var_off[e + 1] - P.var_off[e];
    // the key's type is its oldest survivor's; a survivor of another type marks the key
    const uint64_t r = upper(T.koff, n_reads + 1, q) - 1;
    const uint64_t first = T.koff[r];
    if (q == first) T.key_type[r] = P.type[e];
    else if (P.type[e] != P.type[T.sel[first]]) T.key_flags[r] = AM_KEY_MIXED_TYPES;
  }
}

__global__ void __launch_bounds__(256) k_pl_words(PlView P, TmpLog T) {
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < T.n_ops; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = T.sel[q], from = P.var_off[e], to = T.var_off[q], len = T.var_off[q + 1] - to;
    for (uint64_t w = 0; w < len; ++w) T.var_data[to + w] = P.var_data[from + w];
  }
}

__device__ __forceinline__ void relabel_word(uint64_t *w, const uint64_t *old, const uint64_t *nw, uint64_t n) {
  const uint64_t x = *w;
  if (x == 0 || x == ~0ull) return;  // the kernels' sentinels are never labels
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (old[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n && old[lo] == x) *w = nw[lo];
}

// the label words of every logged effect, by its type (as k_store_relabel maps a store's, am_codec.hip)
__global__ void __launch_bounds__(256) k_pl_relabel(uint64_t n_eff, const uint8_t *type, uint64_t *p0, uint64_t *p1,
                                                    const uint64_t *var_off, uint64_t *vd, const uint64_t *old,
                                                    const uint64_t *nw, uint64_t n) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_eff; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = type[e];
    if (t == AM_LWW) {
      relabel_word(p1 + e, old, nw, n);  // {Ts, Value}: the value
      continue;
    }
    const uint64_t vo = var_off[e], ve = var_off[e + 1];
    if (t == AM_MVREG) {  // {Value, Token, Overridden}
      relabel_word(p0 + e, old, nw, n);
      relabel_word(p1 + e, old, nw, n);
      for (uint64_t q = vo; q < ve; ++q) relabel_word(vd + q, old, nw, n);
    } else if (t == AM_AWSET) {
      for (uint64_t q = vo; q + 3 <= ve;) {  // [{Elem, AddTokens, RemoveTokens}]: [elem, na, nr, tok...]
        const uint64_t na = vd[q + 1], nr = vd[q + 2];
        if (na > ve - q || nr > ve - q || q + 3 + na + nr > ve) break;  // malformed: Type:update raises anyway
        relabel_word(vd + q, old, nw, n);
        for (uint64_t j = 0; j < na + nr; ++j) relabel_word(vd + q + 3 + j, old, nw, n);
        q += 3 + na + nr;
      }
    }
  }
}

// a column of `used` elements moved to a block of new_cap (+ pad) elements, the rest filled with
// the byte `fill`
template <class T>
int grow(am_ctx *c, T *&p, uint64_t used, uint64_t new_cap, uint64_t pad, int fill = 0) {
  T *np = nullptr;
  const size_t bytes = (new_cap + pad) * sizeof(T);
  if (int rc = am_dev_alloc(c, bytes, (void **)&np)) return rc;
  AM_HIP(hipMemsetAsync(np, fill, bytes, c->stream));
  if (p && used) AM_HIP(hipMemcpyAsync(np, p, used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  if (p) am_dev_release(c, p);  // stream-ordered: the copy above runs before any reuse
  p = np;
  return AM_OK;
}

uint64_t doubled(uint64_t cap, uint64_t need) {
  uint64_t c = cap ? cap : 1;
  while (c < need) c *= 2;
  return c;
}

int reserve(am_plog *g, uint64_t tx, uint64_t eff, uint64_t var, uint64_t keys) {
  am_ctx *c = g->ctx;
  const uint64_t nd = g->n_dc;
  if (tx > g->cap_tx || !g->dc) {
    const uint64_t nc = doubled(g->cap_tx, tx);
    int rc = grow(c, g->dc, g->n_tx, nc, 16);
    if (!rc) rc = grow(c, g->commit_time, g->n_tx, nc, 2);
    if (!rc) rc = grow(c, g->snap_vc, g->n_tx * nd, nc * nd, 2);
    if (!rc) rc = grow(c, g->snap_pres, g->n_tx, nc, 4);
    if (!rc) rc = grow(c, g->txid, g->n_tx, nc, 2);
    if (rc) return rc;
    g->cap_tx = nc;
  }
  if (eff > g->cap_eff || !g->key) {
    const uint64_t nc = doubled(g->cap_eff, eff);
    int rc = grow(c, g->key, g->n_eff, nc, 2);
    if (!rc) rc = grow(c, g->type, g->n_eff, nc, 16);
    if (!rc) rc = grow(c, g->eff_meta, g->n_eff, nc, 16);
    if (!rc) rc = grow(c, g->p0, g->n_eff, nc, 2);
    if (!rc) rc = grow(c, g->p1, g->n_eff, nc, 2);
    if (!rc) rc = grow(c, g->var_off, g->n_eff + 1, nc + 1, 2);  // var_off[0] = 0 from the fill
    if (!rc) rc = grow(c, g->link, g->n_eff * 2, nc * 2, 2);
    if (rc) return rc;
    g->cap_eff = nc;
  }
  if (var > g->cap_var || !g->var_data) {
    const uint64_t nc = doubled(g->cap_var, var);
    if (int rc = grow(c, g->var_data, g->n_var, nc, 4)) return rc;
    g->cap_var = nc;
  }
  if (keys > g->cap_keys || !g->key_last) {
    const uint64_t nc = doubled(g->cap_keys, keys);
    if (int rc = grow(c, g->key_last, g->n_keys, nc, 2, 0xFF)) return rc;  // PL_NONE
    g->cap_keys = nc;
  }
  return AM_OK;
}

}  // namespace

// A validated batch (am_commit_build returned AM_OK for dev_cm: src / bkey_off / m are its output)
// behind the log; max_key = the batch's largest key.  Stream-ordered, no readback.  The log is
// unchanged when the call fails.
int am_plog_append_built(am_plog *g, const am_commits *dev_cm, const uint32_t *src, const uint64_t *bkey_off, uint64_t m,
                         uint64_t max_key) {
  if (!g || !dev_cm) return AM_ERR_INVALID;
  am_ctx *c = g->ctx;
  AM_LOCK(c);
  const uint64_t n = dev_cm->n_eff, nt = dev_cm->n_tx;
  const uint64_t nv = dev_cm->var_off ? dev_cm->n_var : 0;
  if (nt == 0) return n ? AM_ERR_INVALID : AM_OK;
  if (n && (!src || !bkey_off || m == 0 || max_key == ~0ull)) return AM_ERR_INVALID;
  if (int rc = reserve(g, g->n_tx + nt, g->n_eff + n, g->n_var + nv, n ? max_key + 1 : g->n_keys)) return rc;
  ApArgs A{};
  A.C = *dev_cm, A.nd = g->n_dc, A.n_tx = g->n_tx, A.n_eff = g->n_eff, A.n_var = g->n_var;
  A.dc = g->dc, A.commit_time = g->commit_time, A.snap_vc = g->snap_vc, A.txid = g->txid, A.snap_pres = g->snap_pres;
  A.key = g->key, A.p0 = g->p0, A.p1 = g->p1, A.var_off = g->var_off, A.type = g->type, A.eff_meta = g->eff_meta;
  A.link = g->link, A.key_last = g->key_last, A.src = src, A.bkey_off = bkey_off, A.m = n ? m : 0;
  hipLaunchKernelGGL(k_pl_append, dim3(grid_for(c, n > nt ? n : nt, 256)), dim3(256), 0, c->stream, A);
  if (n) hipLaunchKernelGGL(k_pl_link, dim3(grid_for(c, n > m ? n : m, 256)), dim3(256), 0, c->stream, A);
  AM_HIP(hipGetLastError());
  if (nv) AM_HIP(hipMemcpyAsync(g->var_data + g->n_var, dev_cm->var_data, nv * 8, hipMemcpyDeviceToDevice, c->stream));
  g->n_tx += nt, g->n_eff += n, g->n_var += nv;
  if (n && max_key + 1 > g->n_keys) g->n_keys = max_key + 1;
  return AM_OK;
}

int am_plog_relabel(am_plog *g, const uint64_t *old_labels, const uint64_t *new_labels, uint64_t n) {
  if (!g || (n && (!old_labels || !new_labels))) return AM_ERR_INVALID;
  am_ctx *c = g->ctx;
  AM_LOCK(c);
  if (n == 0 || g->n_eff == 0) return AM_OK;
  AM_HIP(hipSetDevice(c->device));
  uint64_t *d_old = nullptr, *d_new = nullptr;
  if (int rc = am_relabel_upload(c, old_labels, new_labels, n, &d_old, &d_new)) return rc;
  hipLaunchKernelGGL(k_pl_relabel, dim3(grid_for(c, g->n_eff, 256)), dim3(256), 0, c->stream, g->n_eff, g->type, g->p0, g->p1,
                     g->var_off, g->var_data, d_old, d_new, n);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
  (void)hipFree(d_old);
  (void)hipFree(d_new);
  if (!ok) {
    am_set_error("am_plog_relabel: kernel failed");
    return AM_ERR_HIP;
  }
  return AM_OK;
}

// Every read of the device batch B served from the log (horizons: device [n] or null = the whole
// log), into the device result R.  survivors (device [n], or null) receives each read's op count.
int am_plog_launch_read(am_ctx *c, const am_plog *g, const am_read_batch *B, const uint64_t *hor, am_read_result *R,
                        uint64_t *survivors) {
  const uint64_t n = B->n_reads, nd = g->n_dc;
  if (n == 0) return AM_OK;
  if (n >= 0x7FFFFFF0ull) {
    am_set_error("am_plog_read: 2^31 or more reads in one batch");
    return AM_ERR_INVALID;
  }
  const PlView P = view_of(g);
  size_t scan_b = 0;
  uint64_t *nul = nullptr;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, nul, nul, (int)(n + 1), c->stream) != hipSuccess) {
    am_set_error("am_plog_read: sizing the scan failed");
    return AM_ERR_HIP;
  }
  // the work block: counts, offsets, the empty base of every read and the per-read columns of the
  // temporary log (all zero but what the kernels write)
  struct Cols {
    size_t total = 0;
    size_t add(size_t bytes) {
      const size_t o = total;
      total += (bytes + 255) & ~(size_t)255;
      return o;
    }
  } wc;
  const size_t c8 = (n + 1) * 8;
  const size_t w_cnt = wc.add(c8), w_wcnt = wc.add(c8), w_koff = wc.add(c8), w_vbase = wc.add(c8), w_tot = wc.add(16);
  const size_t w_bign = wc.add(n), w_bpres = wc.add(n * 4), w_bvc = wc.add(nd * n * 8), w_idb = wc.add(n * 8);
  const size_t w_kt = wc.add(n), w_kf = wc.add(n), w_key = wc.add(n * 8), w_tmp = wc.add(scan_b);
  char *W = nullptr, *TB = nullptr;
  if (int rc = am_dev_alloc(c, wc.total, (void **)&W)) return rc;
  auto done = [&](int rc) {
    c->type_masks.erase(W + w_kt);  // the block may come back as another log's key types
    if (TB) am_dev_release(c, TB);
    am_dev_release(c, W);
    return rc;
  };
  if (hipMemsetAsync(W, 0, wc.total, c->stream) != hipSuccess) return done(AM_ERR_HIP);
  uint64_t *cnt = (uint64_t *)(W + w_cnt), *wcnt = (uint64_t *)(W + w_wcnt), *koff = (uint64_t *)(W + w_koff);
  uint64_t *vbase = (uint64_t *)(W + w_vbase), *tot = (uint64_t *)(W + w_tot);
  hipLaunchKernelGGL(k_pl_walk<false>, dim3(grid_for(c, n, 256)), dim3(256), 0, c->stream, P, *B, hor, cnt, wcnt, koff, nul);
  size_t tb = scan_b;
  bool ok = hipcub::DeviceScan::ExclusiveSum(W + w_tmp, tb, cnt, koff, (int)(n + 1), c->stream) == hipSuccess;
  tb = scan_b;
  ok = ok && hipcub::DeviceScan::ExclusiveSum(W + w_tmp, tb, wcnt, vbase, (int)(n + 1), c->stream) == hipSuccess;
  if (!ok || hipGetLastError() != hipSuccess) {
    am_set_error("am_plog_read: the count or its scans failed");
    return done(AM_ERR_HIP);
  }
  if (survivors && hipMemcpyAsync(survivors, cnt, n * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return done(AM_ERR_HIP);
  if (hipMemcpyAsync(tot, koff + n, 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(tot + 1, vbase + n, 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return done(AM_ERR_HIP);
  uint64_t h[2] = {0, 0};
  if (int rc = am_ctx_fetch(c, tot, 2, h)) return done(rc);
  const uint64_t N = h[0], V = h[1];
  if (N >= 0x7FFFFFF0ull) {
    am_set_error("am_plog_read: the batch reads 2^31 or more logged effects");
    return done(AM_ERR_UNSUPPORTED);
  }
  // the temporary log: padded as a store's columns are, so tiles may read past the last op
  const uint64_t na = am_round_up(N, AM_OP_PAD) + AM_OP_PAD;
  size_t scan2_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan2_b, nul, nul, (int)(N + 1), c->stream) != hipSuccess)
    return done(AM_ERR_HIP);
  Cols tc;
  const size_t t_sel = tc.add(na * 8), t_m = tc.add(na), t_ct = tc.add(na * 8), t_vc = tc.add(nd * na * 8);
  const size_t t_sp = tc.add(na * 4), t_tx = tc.add(na * 8), t_p0 = tc.add(na * 8), t_p1 = tc.add(na * 8);
  const size_t t_wl = tc.add((na + 1) * 8), t_vo = tc.add((na + 1) * 8), t_vd = tc.add((V + 4) * 8), t_tmp = tc.add(scan2_b);
  if (int rc = am_dev_alloc(c, tc.total, (void **)&TB)) return done(rc);
  if (hipMemsetAsync(TB, 0, tc.total, c->stream) != hipSuccess) return done(AM_ERR_HIP);
  TmpLog T{};
  T.n_ops = N, T.stride = na, T.koff = koff, T.sel = (uint64_t *)(TB + t_sel);
  T.key_type = (uint8_t *)(W + w_kt), T.key_flags = (uint8_t *)(W + w_kf), T.op_meta = (uint8_t *)(TB + t_m);
  T.commit_time = (uint64_t *)(TB + t_ct), T.snap_vc = (uint64_t *)(TB + t_vc), T.op_txid = (uint64_t *)(TB + t_tx);
  T.p0 = (uint64_t *)(TB + t_p0), T.p1 = (uint64_t *)(TB + t_p1), T.wlen = (uint64_t *)(TB + t_wl);
  T.var_off = (uint64_t *)(TB + t_vo), T.var_data = (uint64_t *)(TB + t_vd), T.snap_pres = (uint32_t *)(TB + t_sp);
  // a read without survivors keeps its own type: an empty key is never a mismatch
  if (hipMemcpyAsync(T.key_type, B->type, n, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return done(AM_ERR_HIP);
  if (N) {
    hipLaunchKernelGGL(k_pl_walk<true>, dim3(grid_for(c, n, 256)), dim3(256), 0, c->stream, P, *B, hor, nul, nul, koff,
                       (uint64_t *)(TB + t_sel));
    hipLaunchKernelGGL(k_pl_gather, dim3(grid_for(c, N, 256)), dim3(256), 0, c->stream, P, n, T);
    tb = scan2_b;
    if (hipcub::DeviceScan::ExclusiveSum(TB + t_tmp, tb, T.wlen, T.var_off, (int)(N + 1), c->stream) != hipSuccess)
      return done(AM_ERR_HIP);
    if (V) hipLaunchKernelGGL(k_pl_words, dim3(grid_for(c, N, 256)), dim3(256), 0, c->stream, P, T);
    if (hipGetLastError() != hipSuccess) return done(AM_ERR_HIP);
  }
  am_op_log L{};
  L.n_dc = g->n_dc, L.n_keys = n, L.n_ops = N, L.n_var = V, L.snap_stride = na;
  L.key_off = koff, L.key_id_base = (const uint64_t *)(W + w_idb), L.key_type = T.key_type, L.key_flags = T.key_flags;
  L.op_meta = T.op_meta, L.commit_time = T.commit_time, L.snap_vc = T.snap_vc, L.snap_pres = T.snap_pres;
  L.op_txid = T.op_txid, L.p0 = T.p0, L.p1 = T.p1, L.var_off = T.var_off, L.var_data = T.var_data;
  // the reads as keys 0 .. n-1 of that log, from new() under the clock {}
  am_read_batch S = *B;
  uint64_t *keys = (uint64_t *)(W + w_key);
  std::vector<uint64_t> ident(n);
  for (uint64_t r = 0; r < n; ++r) ident[r] = r;
  if (hipMemcpyAsync(keys, ident.data(), n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return done(AM_ERR_HIP);
  S.key = keys;
  S.base_ignore = (const uint8_t *)(W + w_bign), S.base_vc = (const uint64_t *)(W + w_bvc);
  S.base_pres = (const uint32_t *)(W + w_bpres), S.base_last_op = nullptr, S.base = am_values{};
  c->type_masks.erase(L.key_type);
  int rc = am_launch_materialize(c, &L, &S, R);
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = AM_ERR_HIP;
  return done(rc);
}

extern "C" {

int am_plog_create(am_ctx *ctx, uint32_t n_dc, uint64_t cap_tx, uint64_t cap_eff, uint64_t cap_var, am_plog **out) {
  if (!ctx || !out || n_dc == 0 || n_dc > AM_MAX_DC) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  am_plog *g = new am_plog();
  g->ctx = ctx, g->n_dc = n_dc;
  if (int rc = reserve(g, cap_tx ? cap_tx : 1, cap_eff ? cap_eff : 1, cap_var ? cap_var : 1, 1)) {
    am_plog_destroy(g);
    return rc;
  }
  *out = g;
  return AM_OK;
}

int am_plog_destroy(am_plog *g) {
  if (!g) return AM_OK;
  am_ctx *c = g->ctx;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (void *p : {(void *)g->dc, (void *)g->commit_time, (void *)g->snap_vc, (void *)g->txid, (void *)g->snap_pres,
                  (void *)g->key, (void *)g->p0, (void *)g->p1, (void *)g->var_off, (void *)g->type, (void *)g->eff_meta,
                  (void *)g->link, (void *)g->var_data, (void *)g->key_last})
    if (p) am_dev_release(c, p);
  delete g;
  return AM_OK;
}

int am_plog_size(const am_plog *g, uint64_t *n_tx, uint64_t *n_eff, uint64_t *n_var) {
  if (!g) return AM_ERR_INVALID;
  AM_LOCK(g->ctx);
  if (n_tx) *n_tx = g->n_tx;
  if (n_eff) *n_eff = g->n_eff;
  if (n_var) *n_var = g->n_var;
  return AM_OK;
}

int am_plog_append_host(am_plog *g, const am_commits *h) {
  if (!g || !h) return AM_ERR_INVALID;
  am_ctx *c = g->ctx;
  AM_LOCK(c);
  const uint64_t n = h->n_eff, nt = h->n_tx, nd = g->n_dc;
  if (nt == 0) return n ? AM_ERR_INVALID : AM_OK;
  if (!h->dc || !h->commit_time || !h->snap_vc || !h->eff_off || (n >> 32) || (nt >> 32) ||
      (n && (!h->key || !h->type || !h->eff_meta || !h->p0 || !h->p1 || (h->var_off && h->n_var && !h->var_data)))) {
    am_set_error("am_plog_append_host: the batch lacks a column or holds 2^32 or more effects");
    return AM_ERR_INVALID;
  }
  uint64_t maxk = 0;
  for (uint64_t e = 0; e < n; ++e) maxk = h->key[e] > maxk ? h->key[e] : maxk;
  if (n && maxk == ~0ull) {
    am_set_error("am_plog_append_host: key 2^64 - 1 is outside every key space");
    return AM_ERR_INVALID;
  }
  if (n == 0) {  // transactions without effects only: am_commit_build has nothing to look at
    for (uint64_t t = 0; t < nt; ++t)
      if (h->dc[t] >= nd || h->eff_off[t] != 0) {
        am_set_error("am_plog_append_host: invalid batch (a dc >= n_dc or effect offsets without effects)");
        return AM_ERR_INVALID;
      }
    if (h->eff_off[nt] != 0) return AM_ERR_INVALID;
  }
  uint32_t key_bits = 1;
  while (key_bits < 64 && (maxk >> key_bits)) ++key_bits;
  AM_HIP(hipSetDevice(c->device));
  const bool var = n && h->var_off != nullptr;
  const uint64_t nv = var ? h->n_var : 0;
  am_stage st;
  const size_t i_dc = st.add(h->dc, nt), i_ct = st.add(h->commit_time, nt * 8), i_vc = st.add(h->snap_vc, nt * nd * 8);
  const size_t i_sp = st.add(h->snap_pres, h->snap_pres ? nt * 4 : 0), i_tx = st.add(h->txid, h->txid ? nt * 8 : 0);
  const size_t i_eo = st.add(h->eff_off, (nt + 1) * 8), i_k = st.add(h->key, n * 8), i_t = st.add(h->type, n);
  const size_t i_m = st.add(h->eff_meta, n), i_p0 = st.add(h->p0, n * 8), i_p1 = st.add(h->p1, n * 8);
  const size_t i_vo = st.add(h->var_off, var ? (n + 1) * 8 : 0), i_vd = st.add(h->var_data, nv * 8);
  const size_t o_k = st.add(nullptr, n * 8), o_ko = st.add(nullptr, (n + 1) * 8), o_kt = st.add(nullptr, n);
  const size_t o_kf = st.add(nullptr, n), o_m = st.add(nullptr, n), o_ct = st.add(nullptr, n * 8);
  const size_t o_vc = st.add(nullptr, nd * n * 8), o_sp = st.add(nullptr, n * 4), o_tx = st.add(nullptr, n * 8);
  const size_t o_p0 = st.add(nullptr, n * 8), o_p1 = st.add(nullptr, n * 8), o_vo = st.add(nullptr, (n + 1) * 8);
  const size_t o_vd = st.add(nullptr, nv * 8 + 8), o_src = st.add(nullptr, n * 4);
  auto done = [&](int rc) {
    (void)hipStreamSynchronize(c->stream);
    if (st.arena) am_dev_release(c, st.arena);
    return rc;
  };
  if (int rc = st.upload(c)) return done(rc);
  am_commits dc = *h;
  dc.n_var = nv;
  dc.dc = st.dev<uint8_t>(i_dc), dc.commit_time = st.dev<uint64_t>(i_ct), dc.snap_vc = st.dev<uint64_t>(i_vc);
  dc.snap_pres = h->snap_pres ? st.dev<uint32_t>(i_sp) : nullptr, dc.txid = h->txid ? st.dev<uint64_t>(i_tx) : nullptr;
  dc.eff_off = st.dev<uint64_t>(i_eo), dc.key = st.dev<uint64_t>(i_k), dc.type = st.dev<uint8_t>(i_t);
  dc.eff_meta = st.dev<uint8_t>(i_m), dc.p0 = st.dev<uint64_t>(i_p0), dc.p1 = st.dev<uint64_t>(i_p1);
  dc.var_off = var ? st.dev<uint64_t>(i_vo) : nullptr, dc.var_data = var ? st.dev<uint64_t>(i_vd) : nullptr;
  uint64_t m = 0;
  am_commit_log o{};
  if (n) {
    o.cap_ops = n, o.cap_var = nv, o.snap_stride = n;
    o.keys = st.dev<uint64_t>(o_k), o.key_off = st.dev<uint64_t>(o_ko), o.key_type = st.dev<uint8_t>(o_kt);
    o.key_flags = st.dev<uint8_t>(o_kf), o.op_meta = st.dev<uint8_t>(o_m), o.commit_time = st.dev<uint64_t>(o_ct);
    o.snap_vc = st.dev<uint64_t>(o_vc), o.snap_pres = st.dev<uint32_t>(o_sp), o.op_txid = st.dev<uint64_t>(o_tx);
    o.p0 = st.dev<uint64_t>(o_p0), o.p1 = st.dev<uint64_t>(o_p1), o.var_off = st.dev<uint64_t>(o_vo);
    o.var_data = st.dev<uint64_t>(o_vd), o.src = st.dev<uint32_t>(o_src);
    am_op_log built{};
    if (int rc = am_commit_build(c, g->n_dc, &dc, key_bits, &o, &built, &m, nullptr)) return done(rc);
  }
  return done(am_plog_append_built(g, &dc, o.src, o.key_off, m, maxk));
}

int am_plog_key_ops(am_plog *g, uint64_t key, uint64_t horizon, uint64_t cap, uint64_t *eff_idx, uint64_t *n_out) {
  if (!g || !n_out || (cap && !eff_idx)) return AM_ERR_INVALID;
  am_ctx *c = g->ctx;
  AM_LOCK(c);
  AM_HIP(hipSetDevice(c->device));
  uint64_t *d = nullptr;
  if (int rc = am_dev_alloc(c, (cap + 1) * 8, (void **)&d)) return rc;
  hipLaunchKernelGGL(k_pl_chain, dim3(1), dim3(64), 0, c->stream, view_of(g), key, horizon, cap, d);
  std::vector<uint64_t> h(cap + 1, 0);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, (cap + 1) * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  am_dev_release(c, d);
  if (e != hipSuccess) {
    am_set_error("am_plog_key_ops: %s", hipGetErrorString(e));
    return AM_ERR_HIP;
  }
  *n_out = h[0];
  if (h[0] > cap) return AM_ERR_CAPACITY;
  for (uint64_t i = 0; i < h[0]; ++i) eff_idx[i] = h[1 + i];
  return AM_OK;
}

int am_plog_read(am_ctx *ctx, am_plog *g, const am_read_batch *B, const uint64_t *dev_horizon, am_read_result *R) {
  if (!ctx || !g || !B || !R || g->ctx != ctx) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  if (B->n_reads && (!B->key || !B->type || !B->read_vc || !B->read_pres)) return AM_ERR_INVALID;
  AM_HIP(hipSetDevice(ctx->device));
  return am_plog_launch_read(ctx, g, B, dev_horizon, R, nullptr);
}

namespace {
struct PlRead {
  am_plog *g;
  bool hor;
};
int run_plog_read(void *arg, const am_read_batch *db, am_read_result *dr, const void *extra_dev) {
  const PlRead *a = static_cast<PlRead *>(arg);
  return am_plog_launch_read(a->g->ctx, a->g, db, a->hor ? (const uint64_t *)extra_dev : nullptr, dr, nullptr);
}
}  // namespace

int am_plog_read_host(am_ctx *ctx, am_plog *g, const am_read_batch *hb, const uint64_t *host_horizon, am_read_result *hr) {
  if (!ctx || !g || !hb || !hr || g->ctx != ctx) return AM_ERR_INVALID;
  AM_LOCK(ctx);
  am_store shape;  // the host-batch staging takes the clock width from a store
  shape.ctx = ctx, shape.dev.n_dc = g->n_dc;
  PlRead a{g, host_horizon != nullptr};
  return am_run_host_batch(ctx, &shape, hb, hr, host_horizon, host_horizon ? hb->n_reads * 8 : 0, run_plog_read, &a);
}

}  // extern "C"
