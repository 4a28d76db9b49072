// am_cert.hip -- the partition's write-write certification on the device: clocksi_vnode:prepare/6,
// certification_check/4, commit/5's committed_tx insert, clean_prepared/3 (src/clocksi_vnode.erl:
// 450-632), get_min_prep/1 (:671-678) and the read servers' check_clock/4 + check_prepared_list/3
// (src/clocksi_readitem_server.erl:236-264), for batches.  A call leaves the tables, and returns the
// statuses, that serving its transactions one at a time in batch order gives.
//
// Two open-addressed tables (linear probing, hashed on the key alone), sized by create / reserve only:
//   committed  {state, key, time}: inserts and overwrites, never removes
//   prepared   {state, key, txid, time}, a multimap: a key's entries all lie on its probe sequence, a
//              removal leaves a tombstone, and a walk ends at a never-used slot.  Used slots (live +
//              tombstones) stay within three quarters of the table; a prepare whose pairs could pass
//              that compacts the live entries into the second buffer first and swaps the two.
// Nothing grows, moves or is allocated between the kernels of a call: the table pointers and slot
// counts reach every kernel by value at its launch, every index derived from table content is masked
// by that slot count, every probe loop is bounded by it, and scratch (sized for the largest batch seen,
// the sort's temporary storage included) is grown before a call's first kernel only.
//
// prepare, one thread per (transaction, key) pair where the work is per pair:
//   k_ct_pairs    validity of key_off; the pair's transaction (a search of key_off, clamped); the sort
//                 input (txid, pair)
//   k_ct_probe    the pair's key in both tables -> the transaction's external-conflict bit (one
//                 atomic per wave where the wave's lanes share a transaction)
//   radix sorts   stable, by txid and then by key (hipcub): pairs ordered by (key, txid, transaction),
//                 so the repeats of a key in one transaction, and in transactions of one TxId, are
//                 adjacent
//   k_ct_runs     a pair's key run (the position of the run's first pair); initial statuses are
//                 k_ct_status's: decided at once unless the transaction certifies and has keys
//   rounds        k_ct_mins: per run the lowest decided-OK transaction and the lowest undecided one;
//                 k_ct_decide: an undecided transaction conflicts when a run of its holds a lower OK
//                 transaction, is OK when no run of its holds a lower undecided one, else waits.  The
//                 lowest undecided transaction is always decidable, so the loop ends; it runs to the
//                 fixed point, in groups of rounds with one readback of the status block per group.
//   k_ct_count    after the last round of a group, once nothing is undecided: per (key, txid) run the
//                 first OK transaction, the walk for the TxId's own entry, and the number of entries
//                 the batch adds -- the capacity verdict, before any insert
//   k_ct_insert   the marked pairs claim never-used slots with a 64-bit compare-and-swap on the state
// finish: one stable sort by key; per run the last committed transaction (an atomic max of sorted
// positions) is the key's writer; k_ct_fcount finds its slot or counts a new key (the capacity
// verdict); k_ct_fapply writes the commit times and turns each pair's (key, txid) entry into a
// tombstone.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "am_cert_plan.h"
#include "am_internal.h"

namespace plan = am_cert_plan;

namespace {

enum : uint64_t { S_EMPTY = 0, S_FULL = 1, S_TOMB = 2 };
constexpr int32_t ST_UNDECIDED = -100;
constexpr uint32_t NONE32 = 0xFFFFFFFFu;
constexpr uint64_t NONE64 = ~0ull;
constexpr uint32_t INFO_ROOM = 256;
// status block words
enum { W_BAD = 0, W_UNDECIDED = 1, W_FRESH = 2, W_REMOVED = 3, W_MIN = 4, W_PRESENT = 5, W_INFO_N = 6, W_INFO_CT = 7, W_N = 8 };

struct CSlot {
  uint64_t state, key, time, pad;
};
struct PSlot {
  uint64_t state, key, txid, time;
};

struct Tables {
  CSlot *ct;
  PSlot *pt;
  uint64_t cmask, pmask;  // slot counts - 1
};

struct Scratch {
  uint64_t *k0, *k1, *k2;
  uint32_t *v0, *v1, *tx_of, *head, *run_of, *first_ok, *low[2], *ins;
  int32_t *st;
  uint32_t *ext;
  uint64_t *stat;
};

__host__ __device__ __forceinline__ uint64_t mix(uint64_t x) {  // splitmix64's finalizer
  x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27, x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
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
// first index in [0, n) of a with a[x] >= e
__device__ __forceinline__ uint64_t lower(const uint64_t *a, uint64_t n, uint64_t e) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the committed slot of key, or NONE64
__device__ __forceinline__ uint64_t c_find(const Tables &T, uint64_t key) {
  uint64_t i = mix(key) & T.cmask;
  for (uint64_t n = 0; n <= T.cmask; ++n, i = (i + 1) & T.cmask) {
    const uint64_t s = T.ct[i].state;
    if (s == S_EMPTY) return NONE64;
    if (T.ct[i].key == key) return i;
  }
  return NONE64;
}
// Walks key's probe sequence in the prepared table.  any: some live entry of the key; le: some live
// entry with time <= start; own: the slot of (key, txid) or NONE64
__device__ __forceinline__ void p_walk(const Tables &T, uint64_t key, uint64_t txid, uint64_t start, bool *any, bool *le,
                                       uint64_t *own) {
  *any = false, *le = false, *own = NONE64;
  uint64_t i = mix(key) & T.pmask;
  for (uint64_t n = 0; n <= T.pmask; ++n, i = (i + 1) & T.pmask) {
    const PSlot s = T.pt[i];
    if (s.state == S_EMPTY) return;
    if (s.state == S_FULL && s.key == key) {
      *any = true;
      if (s.time <= start) *le = true;
      if (s.txid == txid) *own = i;
    }
  }
}
// claims a never-used slot on key's probe sequence (nobody reads the slot's fields in this kernel)
__device__ __forceinline__ void p_claim(PSlot *pt, uint64_t pmask, uint64_t key, uint64_t txid, uint64_t time) {
  uint64_t i = mix(key) & pmask;
  for (uint64_t n = 0; n <= pmask; ++n, i = (i + 1) & pmask) {
    if (atomicCAS((unsigned long long *)&pt[i].state, (unsigned long long)S_EMPTY, (unsigned long long)S_FULL) == S_EMPTY) {
      pt[i].key = key, pt[i].txid = txid, pt[i].time = time;
      return;
    }
  }
}
__device__ __forceinline__ void c_claim(CSlot *ct, uint64_t cmask, uint64_t key, uint64_t time) {
  uint64_t i = mix(key) & cmask;
  for (uint64_t n = 0; n <= cmask; ++n, i = (i + 1) & cmask) {
    if (atomicCAS((unsigned long long *)&ct[i].state, (unsigned long long)S_EMPTY, (unsigned long long)S_FULL) == S_EMPTY) {
      ct[i].key = key, ct[i].time = time;
      return;
    }
  }
}

__device__ __forceinline__ void bump(uint64_t *w, uint64_t by = 1) { atomicAdd((unsigned long long *)w, (unsigned long long)by); }

#define CT_GRID_LOOP(i, n) \
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

// the columns both batches share
struct Batch {
  uint64_t n_tx, n_pairs;
  const uint64_t *txid, *key_off, *key;
};

// validity, the pair's transaction, and the first sort's input: (by_txid ? txid : key, pair)
__global__ void __launch_bounds__(256) k_ct_pairs(Batch B, Scratch S, int by_txid) {
  const uint64_t n = B.n_pairs, nt = B.n_tx;
  const uint64_t span = n > nt + 1 ? n : nt + 1;
  CT_GRID_LOOP(e, span) {
    bool bad = false;
    if (e < nt && B.key_off[e] > B.key_off[e + 1]) bad = true;
    if (e == nt && (B.key_off[0] != 0 || B.key_off[nt] != n)) bad = true;
    if (bad) atomicOr((unsigned long long *)&S.stat[W_BAD], 1ull);
    if (e < n) {
      const uint64_t u = upper(B.key_off, nt + 1, e);  // the last transaction beginning at or before e
      const uint64_t t = u == 0 ? 0 : (u - 1 < nt ? u - 1 : nt - 1);
      S.tx_of[e] = (uint32_t)t;
      S.k0[e] = by_txid ? B.txid[t] : B.key[e];
      S.v0[e] = (uint32_t)e;
    }
  }
}

// the pair's key in both tables -> ext[transaction]; whole waves walk together so that the vote is
// taken with every lane present
__global__ void __launch_bounds__(256) k_ct_probe(Batch B, const uint64_t *start, const uint8_t *certify, Scratch S, Tables T) {
  const uint64_t n = B.n_pairs;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t p = base + lane;
    const bool has = p < n;
    const uint32_t t = has ? S.tx_of[p] : NONE32;
    bool hit = false;
    if (has && certify[t]) {
      const uint64_t k = B.key[p];
      const uint64_t c = c_find(T, k);
      if (c != NONE64 && T.ct[c & T.cmask].time > start[t]) hit = true;
      if (!hit) {
        bool any, le;
        uint64_t own;
        p_walk(T, k, 0, 0, &any, &le, &own);
        hit = any;
      }
    }
    const uint32_t t0 = (uint32_t)__shfl((int)t, 0);  // lane 0 has a pair: base < n
    const bool same = __all(!has || t == t0);
    const bool some = __any(hit);
    if (same) {
      if (lane == 0 && some) atomicOr(&S.ext[t0], 1u);
    } else if (hit) {
      atomicOr(&S.ext[t], 1u);
    }
  }
}

// the second sort's input: the keys in the first sort's order
__global__ void __launch_bounds__(256) k_ct_gather(Batch B, Scratch S) {
  CT_GRID_LOOP(q, B.n_pairs) S.k0[q] = B.key[S.v1[q] < B.n_pairs ? S.v1[q] : 0];
}

__global__ void __launch_bounds__(256) k_ct_status(Batch B, const uint8_t *certify, Scratch S) {
  CT_GRID_LOOP(t, B.n_tx) {
    const bool keys = B.key_off[t + 1] > B.key_off[t];
    int32_t s;
    if (!certify[t]) s = keys ? AM_OK : AM_ERR_NO_UPDATES;
    else if (S.ext[t]) s = AM_ERR_WRITE_CONFLICT;
    else s = keys ? ST_UNDECIDED : AM_ERR_NO_UPDATES;
    S.st[t] = s;
  }
}
__global__ void __launch_bounds__(256) k_ct_fstatus(Batch B, Scratch S) {
  CT_GRID_LOOP(t, B.n_tx) S.st[t] = B.key_off[t + 1] > B.key_off[t] ? AM_OK : AM_ERR_NO_UPDATES;
}

// sorted keys in skey, their pairs in sval: the run of every sorted position and of every pair
__global__ void __launch_bounds__(256) k_ct_runs(uint64_t n, const uint64_t *skey, const uint32_t *sval, Scratch S) {
  CT_GRID_LOOP(q, n) {
    const uint32_t h = (uint32_t)lower(skey, n, skey[q]);
    S.head[q] = h;
    const uint32_t p = sval[q];
    if (p < n) S.run_of[p] = h;
  }
}

// per run: the lowest OK and the lowest undecided transaction; the other parity's column is reset for
// the next round (nobody reads it in this one)
__global__ void __launch_bounds__(256) k_ct_mins(uint64_t n, const uint32_t *sval, Scratch S, int par) {
  if (S.stat[W_BAD]) return;
  CT_GRID_LOOP(q, n) {
    const uint32_t h = S.head[q], p = sval[q];
    if (h >= n || p >= n) continue;
    if (h == q) S.low[par ^ 1][q] = NONE32;
    const uint32_t t = S.tx_of[p];
    const int32_t s = S.st[t];
    if (s == AM_OK) atomicMin(&S.first_ok[h], t);
    else if (s == ST_UNDECIDED) atomicMin(&S.low[par][h], t);
  }
}

__global__ void __launch_bounds__(256) k_ct_decide(Batch B, Scratch S, int par, int count) {
  if (S.stat[W_BAD]) return;
  const uint64_t n = B.n_pairs;
  CT_GRID_LOOP(t, B.n_tx) {
    if (S.st[t] != ST_UNDECIDED) continue;
    const uint64_t a = B.key_off[t], b = B.key_off[t + 1] < n ? B.key_off[t + 1] : n;
    bool conflict = false, blocked = false;
    for (uint64_t p = a; p < b; ++p) {
      const uint32_t h = S.run_of[p];
      if (h >= n) continue;
      if (S.first_ok[h] < t) conflict = true;
      if (S.low[par][h] < t) blocked = true;
    }
    if (conflict) S.st[t] = AM_ERR_WRITE_CONFLICT;
    else if (!blocked) S.st[t] = AM_OK;
    else if (count) bump(&S.stat[W_UNDECIDED]);
  }
}

// Once nothing is undecided: the first pair of every (key, txid) run finds the run's first OK
// transaction and whether the table already holds the TxId's entry; ins[q] = that pair's sorted
// position when the batch adds the entry.  txs = the sorted pairs' TxIds.
__global__ void __launch_bounds__(256) k_ct_count(Batch B, const uint64_t *skey, const uint32_t *sval, Scratch S, Tables T) {
  if (S.stat[W_BAD] || S.stat[W_UNDECIDED]) return;
  const uint64_t n = B.n_pairs;
  CT_GRID_LOOP(q, n) {
    S.ins[q] = NONE32;
    const uint64_t k = skey[q];
    const uint64_t x = B.txid[S.tx_of[sval[q]]];
    if (q > 0 && skey[q - 1] == k && B.txid[S.tx_of[sval[q - 1]]] == x) continue;
    uint64_t r = q;
    bool found = false;
    for (; r < n && skey[r] == k; ++r) {
      const uint32_t t = S.tx_of[sval[r]];
      if (B.txid[t] != x) break;
      if (S.st[t] == AM_OK) {
        found = true;
        break;
      }
    }
    if (!found) continue;
    bool any, le;
    uint64_t own;
    p_walk(T, k, x, 0, &any, &le, &own);
    if (own != NONE64) continue;
    S.ins[q] = (uint32_t)r;
    bump(&S.stat[W_FRESH]);
  }
}

__global__ void __launch_bounds__(256) k_ct_insert(Batch B, const uint64_t *prepare_time, const uint64_t *skey,
                                                   const uint32_t *sval, Scratch S, Tables T) {
  const uint64_t n = B.n_pairs;
  CT_GRID_LOOP(q, n) {
    const uint32_t r = S.ins[q];
    if (r >= n) continue;
    const uint32_t t = S.tx_of[sval[r]];
    p_claim(T.pt, T.pmask, skey[q], B.txid[t], prepare_time[t]);
  }
}

__global__ void __launch_bounds__(256) k_ct_copy_status(uint64_t n, const int32_t *st, int32_t *out) {
  CT_GRID_LOOP(t, n) out[t] = st[t];
}

// finish: the last committed pair of every run (sorted positions ascend in batch order inside a run)
__global__ void __launch_bounds__(256) k_ct_flast(uint64_t n, const uint32_t *sval, const uint8_t *committed, Scratch S) {
  if (S.stat[W_BAD]) return;
  CT_GRID_LOOP(q, n) {
    const uint32_t h = S.head[q], p = sval[q];
    if (h >= n || p >= n) continue;
    if (committed[S.tx_of[p]]) atomicMax(&S.first_ok[h], (uint32_t)q + 1);
  }
}
// the writer of a run finds the key's slot (k2[q] = slot, or NONE64 - 1 for a new key; NONE64: not a
// writer)
__global__ void __launch_bounds__(256) k_ct_fcount(uint64_t n, const uint64_t *skey, Scratch S, Tables T) {
  if (S.stat[W_BAD]) return;
  CT_GRID_LOOP(q, n) {
    uint64_t w = NONE64;
    const uint32_t h = S.head[q];
    if (h < n && S.first_ok[h] == (uint32_t)q + 1) {
      w = c_find(T, skey[q]);
      if (w == NONE64) w = NONE64 - 1, bump(&S.stat[W_FRESH]);
    }
    S.k2[q] = w;
  }
}
__global__ void __launch_bounds__(256) k_ct_fapply(Batch B, const uint64_t *commit_time, const uint64_t *skey,
                                                   const uint32_t *sval, Scratch S, Tables T, int record) {
  const uint64_t n = B.n_pairs;
  CT_GRID_LOOP(q, n) {
    const uint32_t p = sval[q];
    if (p >= n) continue;
    const uint32_t t = S.tx_of[p];
    const uint64_t k = skey[q];
    if (record) {
      const uint64_t w = S.k2[q];
      if (w == NONE64 - 1) c_claim(T.ct, T.cmask, k, commit_time[t]);
      else if (w != NONE64) T.ct[w & T.cmask].time = commit_time[t];
    }
    // clean_prepared/3: at most one live entry (k, txid); repeated pairs race for it, one wins
    const uint64_t x = B.txid[t];
    uint64_t i = mix(k) & T.pmask;
    for (uint64_t m = 0; m <= T.pmask; ++m, i = (i + 1) & T.pmask) {
      const uint64_t s = T.pt[i].state;
      if (s == S_EMPTY) break;
      if (s == S_FULL && T.pt[i].key == k && T.pt[i].txid == x) {
        if (atomicCAS((unsigned long long *)&T.pt[i].state, (unsigned long long)S_FULL, (unsigned long long)S_TOMB) == S_FULL)
          bump(&S.stat[W_REMOVED]);
        break;
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_ct_read_ready(uint64_t n, const uint64_t *key, const uint64_t *start, uint64_t now,
                                                       uint64_t *wait, Tables T) {
  CT_GRID_LOOP(r, n) {
    const uint64_t s = start[r];
    uint64_t w = 0;
    if (s > now) {
      w = (s - now) / 1000 + 1;
    } else {
      bool any, le;
      uint64_t own;
      p_walk(T, key[r], 0, s, &any, &le, &own);
      if (le) w = AM_CERT_SPIN_WAIT_MS;
    }
    wait[r] = w;
  }
}

__global__ void __launch_bounds__(256) k_ct_min(const PSlot *pt, uint64_t slots, uint64_t *stat) {
  uint64_t m = NONE64, cnt = 0;
  CT_GRID_LOOP(i, slots) {
    if (pt[i].state == S_FULL) {
      ++cnt;
      m = pt[i].time < m ? pt[i].time : m;
    }
  }
  if (cnt) {
    atomicMin((unsigned long long *)&stat[W_MIN], (unsigned long long)m);
    bump(&stat[W_PRESENT], cnt);
  }
}

// rehash of the live slots into an empty table (compaction and reserve)
__global__ void __launch_bounds__(256) k_ct_rehash_p(const PSlot *from, uint64_t from_slots, PSlot *to, uint64_t to_mask) {
  CT_GRID_LOOP(i, from_slots) {
    const PSlot s = from[i];
    if (s.state == S_FULL) p_claim(to, to_mask, s.key, s.txid, s.time);
  }
}
__global__ void __launch_bounds__(256) k_ct_rehash_c(const CSlot *from, uint64_t from_slots, CSlot *to, uint64_t to_mask) {
  CT_GRID_LOOP(i, from_slots) {
    const CSlot s = from[i];
    if (s.state == S_FULL) c_claim(to, to_mask, s.key, s.time);
  }
}

// one thread: the key's commit time and its entries skip .. skip + INFO_ROOM - 1 in probe order
__global__ void k_ct_info(uint64_t key, uint64_t skip, uint64_t *out_txid, uint64_t *out_time, uint64_t *stat, Tables T) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t c = c_find(T, key);
  stat[W_INFO_CT] = c == NONE64 ? 0 : T.ct[c & T.cmask].time;
  uint64_t n = 0;
  uint64_t i = mix(key) & T.pmask;
  for (uint64_t m = 0; m <= T.pmask; ++m, i = (i + 1) & T.pmask) {
    const PSlot s = T.pt[i];
    if (s.state == S_EMPTY) break;
    if (s.state == S_FULL && s.key == key) {
      if (n >= skip && n - skip < INFO_ROOM) out_txid[n - skip] = s.txid, out_time[n - skip] = s.time;
      ++n;
    }
  }
  stat[W_INFO_N] = n;
}

unsigned grid_for(am_ctx *c, uint64_t items) {
  const uint64_t b = (items + 255) / 256, cap = (uint64_t)c->n_cu * 8;
  return (unsigned)(b == 0 ? 1 : b < cap ? b : cap);
}

constexpr int GROUP_FIRST = 4, GROUP_MAX = 64;  // rounds per readback: 4, then doubling up to 64

}  // namespace

struct am_cert {
  am_ctx *ctx = nullptr;
  int record = 1;
  uint64_t cap_keys = 0, cap_entries = 0;
  uint64_t cslots = 0, pslots = 0;
  CSlot *ct = nullptr;
  PSlot *pt = nullptr, *pt2 = nullptr;  // pt2: the compaction target, as large as pt
  // host mirror of the tables' counts (every call that changes them reads them back or knows them)
  uint64_t n_committed = 0, live = 0, used = 0;
  uint64_t *stat = nullptr, *info = nullptr;  // status block; key_info's 2 x INFO_ROOM words
  char *scr = nullptr;
  uint64_t scr_tx = 0, scr_pairs = 0;
  size_t sort_bytes = 0;
  char *stage = nullptr;  // the _host twins' upload area
  size_t stage_bytes = 0;
  uint64_t rounds = 0, readbacks = 0, compactions = 0;
};

namespace {

Tables tables_of(const am_cert *c) { return Tables{c->ct, c->pt, c->cslots - 1, c->pslots - 1}; }

int dev_zeroed(am_ctx *ctx, size_t bytes, void **out) {
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    am_set_error("am_cert: hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return AM_ERR_NOMEM;
  }
  const hipError_t m = hipMemsetAsync(p, 0, bytes, ctx->stream);
  if (m != hipSuccess) {
    (void)hipFree(p);
    am_set_error("am_cert: hipMemsetAsync: %s", hipGetErrorString(m));
    return AM_ERR_HIP;
  }
  *out = p;
  return AM_OK;
}

int fetch(am_cert *c, uint64_t *host) {
  ++c->readbacks;
  return am_ctx_fetch(c->ctx, c->stat, W_N, host);
}

// scratch for a batch of n_tx transactions and n_pairs pairs: grown here, before the call's first kernel
int ensure_scratch(am_cert *c, uint64_t n_tx, uint64_t n_pairs, Scratch *S) {
  am_ctx *ctx = c->ctx;
  // what this batch's sorts need (the library's answer for this very count, not assumed monotone)
  size_t sort_b = 0;
  {
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, k, k, v, v, (int)(n_pairs ? n_pairs : 1), 0, 64, ctx->stream) !=
        hipSuccess) {
      am_set_error("am_cert: sizing the sort failed");
      return AM_ERR_HIP;
    }
  }
  if (!c->scr || n_tx > c->scr_tx || n_pairs > c->scr_pairs || plan::up256(sort_b) > c->sort_bytes) {
    const uint64_t nt = n_tx > c->scr_tx ? n_tx : c->scr_tx, np = n_pairs > c->scr_pairs ? n_pairs : c->scr_pairs;
    if (sort_b < c->sort_bytes) sort_b = c->sort_bytes;
    const plan::Layout L = plan::layout(nt, np, sort_b);
    AM_HIP(hipStreamSynchronize(ctx->stream));
    if (c->scr) AM_HIP(hipFree(c->scr));
    c->scr = nullptr, c->scr_tx = c->scr_pairs = 0;
    void *p = nullptr;
    if (int rc = dev_zeroed(ctx, L.total, &p)) return rc;
    c->scr = (char *)p, c->scr_tx = nt, c->scr_pairs = np, c->sort_bytes = plan::up256(sort_b);
  }
  const plan::Layout L = plan::layout(c->scr_tx, c->scr_pairs, c->sort_bytes);
  char *b = c->scr;
  S->k0 = (uint64_t *)(b + L.k0), S->k1 = (uint64_t *)(b + L.k1), S->k2 = (uint64_t *)(b + L.k2);
  S->v0 = (uint32_t *)(b + L.v0), S->v1 = (uint32_t *)(b + L.v1), S->tx_of = (uint32_t *)(b + L.tx_of);
  S->head = (uint32_t *)(b + L.head), S->run_of = (uint32_t *)(b + L.run_of), S->first_ok = (uint32_t *)(b + L.first_ok);
  S->low[0] = (uint32_t *)(b + L.low0), S->low[1] = (uint32_t *)(b + L.low1), S->ins = (uint32_t *)(b + L.ins);
  S->st = (int32_t *)(b + L.st), S->ext = (uint32_t *)(b + L.ext);
  S->stat = c->stat;
  return AM_OK;
}
void *sort_tmp(am_cert *c) { return c->scr + plan::layout(c->scr_tx, c->scr_pairs, c->sort_bytes).tmp; }

int sort_pairs(am_cert *c, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, uint64_t n) {
  size_t tb = c->sort_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(sort_tmp(c), tb, kin, kout, vin, vout, (int)n, 0, 64, c->ctx->stream) != hipSuccess) {
    am_set_error("am_cert: the sort failed");
    return AM_ERR_HIP;
  }
  return AM_OK;
}

int compact(am_cert *c) {
  am_ctx *ctx = c->ctx;
  AM_HIP(hipMemsetAsync(c->pt2, 0, c->pslots * sizeof(PSlot), ctx->stream));
  hipLaunchKernelGGL(k_ct_rehash_p, dim3(grid_for(ctx, c->pslots)), dim3(256), 0, ctx->stream, (const PSlot *)c->pt, c->pslots,
                     c->pt2, c->pslots - 1);
  AM_HIP(hipGetLastError());
  PSlot *t = c->pt;
  c->pt = c->pt2, c->pt2 = t;
  c->used = c->live;
  ++c->compactions;
  return AM_OK;
}

int batch_args_ok(uint64_t n_tx, uint64_t n_pairs, const void *txid, const void *a, const void *b, const void *key_off,
                  const void *key, const char *who) {
  if (!plan::counts_ok(n_tx, n_pairs)) {
    am_set_error("%s: 2^32 or more pairs or transactions in one batch", who);
    return AM_ERR_INVALID;
  }
  if (n_tx == 0 && n_pairs) {
    am_set_error("%s: keys without a transaction", who);
    return AM_ERR_INVALID;
  }
  if (n_tx && (!txid || !a || !b || !key_off || (n_pairs && !key))) {
    am_set_error("%s: the batch lacks a column", who);
    return AM_ERR_INVALID;
  }
  if (n_pairs >= 0x7FFFFFFFull) {
    am_set_error("%s: more than 2^31 - 2 pairs", who);
    return AM_ERR_UNSUPPORTED;
  }
  return AM_OK;
}

// stage host columns in the certifier's upload area (grown before the call's first kernel)
struct Stage {
  struct Item {
    const void *h;
    size_t bytes, off;
  };
  std::vector<Item> items;
  size_t total = 0;
  size_t add(const void *h, size_t bytes) {
    items.push_back({h, bytes, total});
    total += plan::up256(bytes ? bytes : 1);
    return items.size() - 1;
  }
  int upload(am_cert *c) {
    am_ctx *ctx = c->ctx;
    if (c->stage_bytes < total) {
      AM_HIP(hipStreamSynchronize(ctx->stream));
      if (c->stage) AM_HIP(hipFree(c->stage));
      c->stage = nullptr, c->stage_bytes = 0;
      void *p = nullptr;
      if (int rc = dev_zeroed(ctx, total + total / 4, &p)) return rc;
      c->stage = (char *)p, c->stage_bytes = total + total / 4;
    }
    for (const Item &it : items)
      if (it.h && it.bytes) AM_HIP(hipMemcpyAsync(c->stage + it.off, it.h, it.bytes, hipMemcpyHostToDevice, ctx->stream));
    return AM_OK;
  }
  template <class T>
  T *dev(am_cert *c, size_t item) const {
    return (T *)(c->stage + items[item].off);
  }
};

}  // namespace

extern "C" {

int am_cert_create(am_ctx *ctx, uint64_t cap_keys, uint64_t cap_entries, int record_commits, am_cert **out) {
  if (!ctx || !out) return AM_ERR_INVALID;
  if (!plan::cap_ok(cap_keys) || !plan::cap_ok(cap_entries)) {
    am_set_error("am_cert_create: a capacity above 2^40");
    return AM_ERR_INVALID;
  }
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  am_cert *c = new am_cert();
  c->ctx = ctx, c->record = record_commits ? 1 : 0;
  c->cap_keys = cap_keys ? cap_keys : 1, c->cap_entries = cap_entries ? cap_entries : 1;
  c->cslots = plan::slots_for(c->cap_keys), c->pslots = plan::slots_for(c->cap_entries);
  int rc = dev_zeroed(ctx, c->cslots * sizeof(CSlot), (void **)&c->ct);
  if (!rc) rc = dev_zeroed(ctx, c->pslots * sizeof(PSlot), (void **)&c->pt);
  if (!rc) rc = dev_zeroed(ctx, c->pslots * sizeof(PSlot), (void **)&c->pt2);
  if (!rc) rc = dev_zeroed(ctx, 256, (void **)&c->stat);
  if (!rc) rc = dev_zeroed(ctx, 2 * INFO_ROOM * sizeof(uint64_t), (void **)&c->info);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = AM_ERR_HIP;
  if (rc) {
    am_cert_destroy(c);
    return rc;
  }
  *out = c;
  return AM_OK;
}

int am_cert_destroy(am_cert *c) {
  if (!c) return AM_OK;
  am_ctx *ctx = c->ctx;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (void *p : {(void *)c->ct, (void *)c->pt, (void *)c->pt2, (void *)c->stat, (void *)c->info, (void *)c->scr, (void *)c->stage})
    if (p) (void)hipFree(p);
  delete c;
  return AM_OK;
}

int am_cert_reserve(am_cert *c, uint64_t cap_keys, uint64_t cap_entries) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (!plan::cap_ok(cap_keys) || !plan::cap_ok(cap_entries) || cap_keys == 0 || cap_entries == 0 ||
      cap_keys < c->n_committed || cap_entries < c->live) {
    am_set_error("am_cert_reserve: capacities (%llu keys, %llu entries) below the content (%llu, %llu) or above 2^40",
                 (unsigned long long)cap_keys, (unsigned long long)cap_entries, (unsigned long long)c->n_committed,
                 (unsigned long long)c->live);
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t cs = plan::slots_for(cap_keys), ps = plan::slots_for(cap_entries);
  CSlot *nct = nullptr;
  PSlot *npt = nullptr, *npt2 = nullptr;
  int rc = dev_zeroed(ctx, cs * sizeof(CSlot), (void **)&nct);
  if (!rc) rc = dev_zeroed(ctx, ps * sizeof(PSlot), (void **)&npt);
  if (!rc) rc = dev_zeroed(ctx, ps * sizeof(PSlot), (void **)&npt2);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    for (void *p : {(void *)nct, (void *)npt, (void *)npt2})
      if (p) (void)hipFree(p);
    return rc;
  }
  hipLaunchKernelGGL(k_ct_rehash_c, dim3(grid_for(ctx, c->cslots)), dim3(256), 0, ctx->stream, (const CSlot *)c->ct, c->cslots,
                     nct, cs - 1);
  hipLaunchKernelGGL(k_ct_rehash_p, dim3(grid_for(ctx, c->pslots)), dim3(256), 0, ctx->stream, (const PSlot *)c->pt, c->pslots,
                     npt, ps - 1);
  AM_HIP(hipGetLastError());
  AM_HIP(hipStreamSynchronize(ctx->stream));
  AM_HIP(hipFree(c->ct));
  AM_HIP(hipFree(c->pt));
  AM_HIP(hipFree(c->pt2));
  c->ct = nct, c->pt = npt, c->pt2 = npt2;
  c->cslots = cs, c->pslots = ps, c->cap_keys = cap_keys, c->cap_entries = cap_entries;
  c->used = c->live;
  return AM_OK;
}

int am_cert_prepare(am_cert *c, const am_prepares *P, int32_t *dev_status) {
  if (!c || !P || (P->n_tx && !dev_status)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (int rc = batch_args_ok(P->n_tx, P->n_pairs, P->txid, P->start_time, P->prepare_time, P->key_off, P->key, "am_cert_prepare"))
    return rc;
  if (P->n_tx && !P->certify) {
    am_set_error("am_cert_prepare: the batch lacks a column");
    return AM_ERR_INVALID;
  }
  const uint64_t n = P->n_pairs, nt = P->n_tx;
  if (nt == 0) return AM_OK;
  AM_HIP(hipSetDevice(ctx->device));
  Scratch S{};
  if (int rc = ensure_scratch(c, nt, n, &S)) return rc;
  if (plan::must_compact(c->live, c->used, n, c->pslots))
    if (int rc = compact(c)) return rc;
  const Tables T = tables_of(c);
  const Batch B{nt, n, P->txid, P->key_off, P->key};
  hipStream_t s = ctx->stream;
  const uint64_t span = n > nt + 1 ? n : nt + 1;
  AM_HIP(hipMemsetAsync(S.stat, 0, W_N * sizeof(uint64_t), s));
  AM_HIP(hipMemsetAsync(S.ext, 0, nt * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_ct_pairs, dim3(grid_for(ctx, span)), dim3(256), 0, s, B, S, 1);
  const uint64_t *skey = S.k1;
  const uint32_t *sval = S.v0;
  if (n) {
    hipLaunchKernelGGL(k_ct_probe, dim3(grid_for(ctx, n)), dim3(256), 0, s, B, P->start_time, P->certify, S, T);
    if (int rc = sort_pairs(c, S.k0, S.k1, S.v0, S.v1, n)) return rc;  // by txid
    hipLaunchKernelGGL(k_ct_gather, dim3(grid_for(ctx, n)), dim3(256), 0, s, B, S);
    if (int rc = sort_pairs(c, S.k0, S.k1, S.v1, S.v0, n)) return rc;  // then by key: (key, txid, transaction)
    hipLaunchKernelGGL(k_ct_runs, dim3(grid_for(ctx, n)), dim3(256), 0, s, n, skey, sval, S);
    AM_HIP(hipMemsetAsync(S.first_ok, 0xFF, n * sizeof(uint32_t), s));
    AM_HIP(hipMemsetAsync(S.low[0], 0xFF, n * sizeof(uint32_t), s));
    AM_HIP(hipMemsetAsync(S.low[1], 0xFF, n * sizeof(uint32_t), s));
  }
  hipLaunchKernelGGL(k_ct_status, dim3(grid_for(ctx, nt)), dim3(256), 0, s, B, P->certify, S);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  int par = 0;
  for (int group = GROUP_FIRST;; group = group * 2 > GROUP_MAX ? GROUP_MAX : group * 2) {
    for (int r = 0; r < group && n; ++r, par ^= 1) {
      const int last = r == group - 1;
      hipLaunchKernelGGL(k_ct_mins, dim3(grid_for(ctx, n)), dim3(256), 0, s, n, sval, S, par);
      if (last) AM_HIP(hipMemsetAsync(&S.stat[W_UNDECIDED], 0, 2 * sizeof(uint64_t), s));  // W_UNDECIDED, W_FRESH
      hipLaunchKernelGGL(k_ct_decide, dim3(grid_for(ctx, nt)), dim3(256), 0, s, B, S, par, last);
      ++c->rounds;
    }
    if (n) hipLaunchKernelGGL(k_ct_count, dim3(grid_for(ctx, n)), dim3(256), 0, s, B, skey, sval, S, T);
    AM_HIP(hipGetLastError());
    if (int rc = fetch(c, st)) return rc;
    if (st[W_BAD]) {
      am_set_error("am_cert_prepare: key_off is not non-decreasing from 0 to n_pairs");
      return AM_ERR_INVALID;
    }
    if (st[W_UNDECIDED] == 0) break;
  }
  if (!plan::fits(c->live, st[W_FRESH], c->cap_entries)) {
    am_set_error("am_cert_prepare: %llu live entries + %llu new ones exceed cap_entries %llu", (unsigned long long)c->live,
                 (unsigned long long)st[W_FRESH], (unsigned long long)c->cap_entries);
    return AM_ERR_CAPACITY;
  }
  if (n && st[W_FRESH]) {
    hipLaunchKernelGGL(k_ct_insert, dim3(grid_for(ctx, n)), dim3(256), 0, s, B, P->prepare_time, skey, sval, S, T);
    c->live += st[W_FRESH], c->used += st[W_FRESH];
  }
  hipLaunchKernelGGL(k_ct_copy_status, dim3(grid_for(ctx, nt)), dim3(256), 0, s, nt, (const int32_t *)S.st, dev_status);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

int am_cert_finish(am_cert *c, const am_finishes *F, int32_t *dev_status) {
  if (!c || !F || (F->n_tx && !dev_status)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (int rc = batch_args_ok(F->n_tx, F->n_pairs, F->txid, F->commit_time, F->committed, F->key_off, F->key, "am_cert_finish"))
    return rc;
  const uint64_t n = F->n_pairs, nt = F->n_tx;
  if (nt == 0) return AM_OK;
  AM_HIP(hipSetDevice(ctx->device));
  Scratch S{};
  if (int rc = ensure_scratch(c, nt, n, &S)) return rc;
  const Tables T = tables_of(c);
  const Batch B{nt, n, F->txid, F->key_off, F->key};
  hipStream_t s = ctx->stream;
  const uint64_t span = n > nt + 1 ? n : nt + 1;
  AM_HIP(hipMemsetAsync(S.stat, 0, W_N * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_ct_pairs, dim3(grid_for(ctx, span)), dim3(256), 0, s, B, S, 0);
  hipLaunchKernelGGL(k_ct_fstatus, dim3(grid_for(ctx, nt)), dim3(256), 0, s, B, S);
  const uint64_t *skey = S.k1;
  const uint32_t *sval = S.v1;
  if (n) {
    if (int rc = sort_pairs(c, S.k0, S.k1, S.v0, S.v1, n)) return rc;  // by key: (key, transaction)
    hipLaunchKernelGGL(k_ct_runs, dim3(grid_for(ctx, n)), dim3(256), 0, s, n, skey, sval, S);
    if (c->record) {
      AM_HIP(hipMemsetAsync(S.first_ok, 0, n * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_ct_flast, dim3(grid_for(ctx, n)), dim3(256), 0, s, n, sval, F->committed, S);
      hipLaunchKernelGGL(k_ct_fcount, dim3(grid_for(ctx, n)), dim3(256), 0, s, n, skey, S, T);
    }
  }
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  if (int rc = fetch(c, st)) return rc;
  if (st[W_BAD]) {
    am_set_error("am_cert_finish: key_off is not non-decreasing from 0 to n_pairs");
    return AM_ERR_INVALID;
  }
  if (!plan::fits(c->n_committed, st[W_FRESH], c->cap_keys)) {
    am_set_error("am_cert_finish: %llu committed keys + %llu new ones exceed cap_keys %llu", (unsigned long long)c->n_committed,
                 (unsigned long long)st[W_FRESH], (unsigned long long)c->cap_keys);
    return AM_ERR_CAPACITY;
  }
  if (n) {
    hipLaunchKernelGGL(k_ct_fapply, dim3(grid_for(ctx, n)), dim3(256), 0, s, B, F->commit_time, skey, sval, S, T, c->record);
    c->n_committed += st[W_FRESH];
  }
  hipLaunchKernelGGL(k_ct_copy_status, dim3(grid_for(ctx, nt)), dim3(256), 0, s, nt, (const int32_t *)S.st, dev_status);
  AM_HIP(hipGetLastError());
  if (n) {
    if (int rc = fetch(c, st)) return rc;
    c->live -= st[W_REMOVED] < c->live ? st[W_REMOVED] : c->live;  // the slots stay used, as tombstones
  }
  return AM_OK;
}

int am_cert_prepare_host(am_cert *c, const am_prepares *h, int32_t *host_status) {
  if (!c || !h || (h->n_tx && !host_status)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (int rc = batch_args_ok(h->n_tx, h->n_pairs, h->txid, h->start_time, h->prepare_time, h->key_off, h->key,
                             "am_cert_prepare_host"))
    return rc;
  if (h->n_tx && !h->certify) return AM_ERR_INVALID;
  const uint64_t nt = h->n_tx, n = h->n_pairs;
  if (nt == 0) return AM_OK;
  AM_HIP(hipSetDevice(ctx->device));
  Stage G;
  const size_t i_tx = G.add(h->txid, nt * 8), i_st = G.add(h->start_time, nt * 8), i_pt = G.add(h->prepare_time, nt * 8);
  const size_t i_ce = G.add(h->certify, nt), i_ko = G.add(h->key_off, (nt + 1) * 8), i_k = G.add(h->key, n * 8);
  const size_t i_out = G.add(nullptr, nt * 4);
  if (int rc = G.upload(c)) return rc;
  am_prepares d = *h;
  d.txid = G.dev<uint64_t>(c, i_tx), d.start_time = G.dev<uint64_t>(c, i_st), d.prepare_time = G.dev<uint64_t>(c, i_pt);
  d.certify = G.dev<uint8_t>(c, i_ce), d.key_off = G.dev<uint64_t>(c, i_ko), d.key = G.dev<uint64_t>(c, i_k);
  int32_t *out = G.dev<int32_t>(c, i_out);
  if (int rc = am_cert_prepare(c, &d, out)) {
    (void)hipStreamSynchronize(ctx->stream);  // the host columns may go away
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_status, out, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_cert_finish_host(am_cert *c, const am_finishes *h, int32_t *host_status) {
  if (!c || !h || (h->n_tx && !host_status)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (int rc = batch_args_ok(h->n_tx, h->n_pairs, h->txid, h->commit_time, h->committed, h->key_off, h->key,
                             "am_cert_finish_host"))
    return rc;
  const uint64_t nt = h->n_tx, n = h->n_pairs;
  if (nt == 0) return AM_OK;
  AM_HIP(hipSetDevice(ctx->device));
  Stage G;
  const size_t i_tx = G.add(h->txid, nt * 8), i_ct = G.add(h->commit_time, nt * 8), i_co = G.add(h->committed, nt);
  const size_t i_ko = G.add(h->key_off, (nt + 1) * 8), i_k = G.add(h->key, n * 8), i_out = G.add(nullptr, nt * 4);
  if (int rc = G.upload(c)) return rc;
  am_finishes d = *h;
  d.txid = G.dev<uint64_t>(c, i_tx), d.commit_time = G.dev<uint64_t>(c, i_ct), d.committed = G.dev<uint8_t>(c, i_co);
  d.key_off = G.dev<uint64_t>(c, i_ko), d.key = G.dev<uint64_t>(c, i_k);
  int32_t *out = G.dev<int32_t>(c, i_out);
  if (int rc = am_cert_finish(c, &d, out)) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_status, out, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_cert_read_ready(am_cert *c, uint64_t n, const uint64_t *dev_key, const uint64_t *dev_start, uint64_t now,
                       uint64_t *dev_wait_ms) {
  if (!c || (n && (!dev_key || !dev_start || !dev_wait_ms))) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (n == 0) return AM_OK;
  AM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_ct_read_ready, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, n, dev_key, dev_start, now, dev_wait_ms,
                     tables_of(c));
  AM_HIP(hipGetLastError());
  return AM_OK;
}

int am_cert_read_ready_host(am_cert *c, uint64_t n, const uint64_t *host_key, const uint64_t *host_start, uint64_t now,
                            uint64_t *host_wait_ms) {
  if (!c || (n && (!host_key || !host_start || !host_wait_ms))) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (n == 0) return AM_OK;
  if (n >> 40) return AM_ERR_INVALID;
  AM_HIP(hipSetDevice(ctx->device));
  Stage G;
  const size_t i_k = G.add(host_key, n * 8), i_s = G.add(host_start, n * 8), i_w = G.add(nullptr, n * 8);
  if (int rc = G.upload(c)) return rc;
  uint64_t *w = G.dev<uint64_t>(c, i_w);
  if (int rc = am_cert_read_ready(c, n, G.dev<uint64_t>(c, i_k), G.dev<uint64_t>(c, i_s), now, w)) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_wait_ms, w, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_cert_min_prepared(am_cert *c, uint64_t *time, int *present) {
  if (!c || !time || !present) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  AM_HIP(hipMemsetAsync(c->stat, 0, W_N * sizeof(uint64_t), ctx->stream));
  AM_HIP(hipMemsetAsync(&c->stat[W_MIN], 0xFF, sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(k_ct_min, dim3(grid_for(ctx, c->pslots)), dim3(256), 0, ctx->stream, (const PSlot *)c->pt, c->pslots, c->stat);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  if (int rc = fetch(c, st)) return rc;
  *present = st[W_PRESENT] ? 1 : 0;
  *time = st[W_PRESENT] ? st[W_MIN] : 0;
  return AM_OK;
}

int am_cert_key_info(am_cert *c, uint64_t key, uint64_t *commit_time, uint64_t cap, uint64_t *txid, uint64_t *time,
                     uint64_t *n) {
  if (!c || !commit_time || !n || (cap && (!txid || !time))) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  std::vector<std::pair<uint64_t, uint64_t>> got;  // (time, txid)
  std::vector<uint64_t> buf(2 * INFO_ROOM);
  uint64_t total = 0;
  for (uint64_t skip = 0;; skip += INFO_ROOM) {
    hipLaunchKernelGGL(k_ct_info, dim3(1), dim3(64), 0, ctx->stream, key, skip, c->info, c->info + INFO_ROOM, c->stat,
                       tables_of(c));
    AM_HIP(hipGetLastError());
    uint64_t st[W_N] = {};
    if (int rc = fetch(c, st)) return rc;
    total = st[W_INFO_N];
    *commit_time = st[W_INFO_CT];
    *n = total;
    if (total > cap) return AM_ERR_CAPACITY;
    const uint64_t m = total > skip ? (total - skip < INFO_ROOM ? total - skip : INFO_ROOM) : 0;
    if (m) {
      AM_HIP(hipMemcpyAsync(buf.data(), c->info, 2 * INFO_ROOM * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
      AM_HIP(hipStreamSynchronize(ctx->stream));
      for (uint64_t i = 0; i < m; ++i) got.emplace_back(buf[INFO_ROOM + i], buf[i]);
    }
    if (skip + INFO_ROOM >= total) break;
  }
  std::sort(got.begin(), got.end());
  for (size_t i = 0; i < got.size(); ++i) time[i] = got[i].first, txid[i] = got[i].second;
  return AM_OK;
}

int am_cert_size(am_cert *c, uint64_t *committed_keys, uint64_t *prepared_entries, uint64_t *cap_keys, uint64_t *cap_entries) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (committed_keys) *committed_keys = c->n_committed;
  if (prepared_entries) *prepared_entries = c->live;
  if (cap_keys) *cap_keys = c->cap_keys;
  if (cap_entries) *cap_entries = c->cap_entries;
  return AM_OK;
}

int am_cert_stats(am_cert *c, uint64_t *rounds, uint64_t *readbacks, uint64_t *compactions) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (rounds) *rounds = c->rounds;
  if (readbacks) *readbacks = c->readbacks;
  if (compactions) *compactions = c->compactions;
  return AM_OK;
}

}  // extern "C"
