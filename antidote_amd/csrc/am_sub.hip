// am_sub.hip -- the subscriber buffers of every partition a GPU owns, on the device: one
// inter_dc_sub_buf state machine per (partition, origin DC) stream (src/inter_dc_sub_buf.erl:57-162,
// src/inter_dc_sub_vnode.erl:84-94), for batches of arrivals.  A call leaves the streams, and returns the
// deliveries, gaps and counters, that serving the batch's rows one at a time in batch order gives
// (tests/subsim.py is the contract).
//
// State, sized by create / reserve only:
//   last [n_part * n_dc], mode [n_part * n_dc]   last_observed_opid and normal / buffering.  Never moved.
//   A, B                                         two queue buffers of cap_queued entries, structure of
//                                                arrays {key = partition * n_dc + dc, prev, last, tag,
//                                                timestamp, ping, snapshot row}; `last` holds
//                                                last_log_opid, which for a ping is prev.  A is the
//                                                state: the queued entries sorted by key, each queue
//                                                oldest first.  B is the call's working copy (it also
//                                                holds a row's kind).
// process, all on the context's stream, one readback of the status block at the end:
//   k_sb_check    validity of kind / part / dc / timestamp; the sort input (key, entry) over the carried
//                 entries followed by the rows, key = stream * 2 + (the row is a response row)
//   radix sort    stable (hipcub): a stream's carried entries, then its TXN rows in batch order -- its
//                 queue once every row is pushed -- then its RESP_TXN / RESP_END rows in batch order
//   k_sb_gather   the entries into B in sorted order
//   k_sb_run      one wave per stream.  The stream's rows split into segments at its RESP_END rows.  A
//                 segment that starts in normal mode makes its whole run of TXN rows visible and walks the
//                 queue once: what a row-at-a-time run does differently is only to look again at a head
//                 that cannot move.  A segment in buffering mode only extends the tail, and its RESP_TXN
//                 rows deliver themselves; its RESP_END sets last to the head's prev and walks.  The walk
//                 tests 64 entries a step: lane j compares prev[j] with last_log_opid[j-1] (lane 0 with
//                 the stream's last), a ballot gives the leading run, which is delivered at once; the
//                 first mismatch is compared with the true last: smaller is dropped, greater is a gap
//                 (or, with logging disabled, a delivery).  Every delivered entry records the row that
//                 triggered it: max(its own row, the row that started the walk).
//   k_sb_scan     exclusive sums of the streams' remaining counts
//   k_sb_compact  the undelivered suffixes from B back into A
//   k_sb_keys, radix sort, k_sb_offsets, k_sb_emit
//                 the delivered entries by (partition, triggering row), stable, so queue order breaks
//                 ties: the columns of am_dep_txns, partition-major
//   scan, k_sb_gaps   the gaps in triggering-row order (a row triggers at most one)
// An invalid batch sets the status block's flag in the first kernel and every later kernel returns on
// it, so A, last and mode are still the state.
//
// Nothing grows, moves or is allocated between the kernels of a call: buffers come from create /
// reserve, the scratch (the sorts' and the scan's temporary storage for this very count included) is
// grown before the call's first kernel, pointers and dimensions reach every kernel by value, and every
// index derived from part, dc or a sorted position is range-checked or clamped.
#include <hipcub/hipcub.hpp>

#include "am_internal.h"
#include "am_sub_plan.h"

namespace plan = am_sub_plan;

namespace {

enum { W_BAD = 0, W_DELIV = 1, W_GAPS = 2, W_DROP = 3, W_UNEXP = 4, W_QUEUED = 5, W_LO = 6, W_HI = 7, W_N = 8 };

struct Buf {
  uint64_t *key, *prev, *last, *tag, *ts, *snap;
  uint8_t *ping, *kind;  // kind: B only
};

struct Scratch {
  uint64_t *k0, *k1, *dk1, *gfrom, *gto;
  uint32_t *v0, *v1, *dv1, *trig, *gflag, *gpos;
};

struct Rows {
  uint64_t n;
  const uint8_t *kind;
  const uint32_t *part;
  const uint8_t *dc;
  const uint64_t *prev, *last, *ts, *snap;
  const uint8_t *ping;
  const uint64_t *tag;
};

struct Out {
  uint32_t *part;
  uint8_t *dc;
  uint64_t *ts, *snap;
  uint8_t *ping;
  uint64_t *tag;
};

// what every kernel of a call takes by value
struct Dims {
  uint64_t n, q, nr, cap, ns;  // n = q carried entries + nr rows; ns = n_part * n_dc streams
  uint32_t n_part, n_dc;
};

#define SB_GRID_LOOP(i, n) \
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

// first index in [0, n) of a with a[x] >= e
template <class T>
__device__ __forceinline__ uint64_t lower(const T *a, uint64_t n, uint64_t e) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)a[mid] < e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(256) k_sb_check(Dims D, Rows R, const uint64_t *akey, Scratch S, uint64_t *stat) {
  SB_GRID_LOOP(i, D.n) {
    if (i < D.q) {
      const uint64_t s = akey[i] < D.ns ? akey[i] : D.ns - 1;
      S.k0[i] = plan::stream_key(s, false), S.v0[i] = (uint32_t)i;
      continue;
    }
    const uint64_t t = i - D.q;
    uint32_t kind = R.kind[t], p = R.part[t], d = R.dc[t], bad = 0;
    if (kind > plan::KIND_RESP_END) bad |= plan::BAD_KIND, kind = plan::KIND_TXN;
    if (p >= D.n_part) bad |= plan::BAD_PART, p = 0;
    if (d >= D.n_dc) bad |= plan::BAD_DC, d = 0;
    if (kind != plan::KIND_RESP_END && R.ts[t] == 0 && !(R.ping && R.ping[t])) bad |= plan::BAD_TIME;
    if (bad) atomicOr((unsigned long long *)&stat[W_BAD], (unsigned long long)bad);
    S.k0[i] = plan::stream_key((uint64_t)p * D.n_dc + d, kind != plan::KIND_TXN), S.v0[i] = (uint32_t)i;
    S.gflag[t] = 0;
  }
}

__global__ void __launch_bounds__(256) k_sb_gather(Dims D, Rows R, Buf A, Buf W, Scratch S, const uint64_t *stat) {
  if (stat[W_BAD]) return;
  SB_GRID_LOOP(q, D.n) {
    const uint64_t src = S.v1[q];
    if (src < D.q) {
      W.prev[q] = A.prev[src], W.last[q] = A.last[src], W.tag[q] = A.tag[src], W.ts[q] = A.ts[src], W.ping[q] = A.ping[src];
      W.kind[q] = (uint8_t)plan::KIND_TXN;
    } else {
      const uint64_t t = src - D.q < D.nr ? src - D.q : D.nr - 1;
      const uint8_t pg = R.ping && R.ping[t] ? 1 : 0, kd = R.kind[t];
      const uint64_t pv = R.prev[t];
      W.prev[q] = pv, W.last[q] = pg ? pv : R.last[t];  // inter_dc_txn:last_log_opid/1 of a ping is prev_log_opid
      W.tag[q] = R.tag[t], W.ts[q] = R.ts[t], W.ping[q] = pg;
      W.kind[q] = kd <= plan::KIND_RESP_END ? kd : (uint8_t)plan::KIND_TXN;
    }
  }
  SB_GRID_LOOP(i, D.n * D.n_dc) {
    const uint64_t q = i / D.n_dc, k = i - q * D.n_dc, src = S.v1[q];
    if (src < D.q) {
      W.snap[i] = A.snap[src * D.n_dc + k];
    } else {
      const uint64_t t = src - D.q < D.nr ? src - D.q : D.nr - 1;
      W.snap[i] = R.snap[t * D.n_dc + k];
    }
  }
}

struct Run {
  Dims D;
  uint32_t reach, logging;
  Buf W;
  Scratch S;
  uint64_t *last;
  uint32_t *mode;
  uint64_t *qstart, *qhead, *remain;  // [ns]
  uint64_t *stat;
};

struct Walk {
  uint64_t last, head, buf_from, ndrop, budget;
  uint32_t mode;
};

// process_queue/1 over the visible entries [head, tail) of the queue that starts at B[qst]; base is the
// row (1-based) that started the walk.  Uniform over the wave.
__device__ __forceinline__ void sb_walk(const Run &R, uint64_t qst, uint64_t tail, uint64_t base, uint32_t dc, uint32_t lane, Walk &S) {
  const Dims &D = R.D;
  while (S.head < tail) {
    if (S.budget == 0) return;
    --S.budget;
    const uint32_t cnt = tail - S.head < plan::TILE ? (uint32_t)(tail - S.head) : plan::TILE;
    const bool valid = lane < cnt;
    const uint64_t q = qst + S.head + lane;
    uint64_t prev = 0, eff = 0, row1 = 0;
    if (valid && q < D.n) {
      prev = R.W.prev[q], eff = R.W.last[q];
      const uint64_t src = R.S.v1[q];
      row1 = src < D.q ? 0 : src - D.q + 1;
    }
    uint64_t up = shfl64(eff, lane ? lane - 1 : 0);
    if (lane == 0) up = S.last;
    const uint64_t miss = __ballot(!(valid && prev == up));
    const uint32_t f = miss ? (uint32_t)__builtin_ctzll(miss) : plan::TILE;  // the leading run; f <= cnt
    const uint64_t trg = row1 > base ? row1 : base;
    if (f) {
      if (lane < f && q < D.n) R.S.trig[q] = (uint32_t)trg;
      S.last = shfl64(eff, f - 1), S.head += f;
    }
    if (f >= cnt) continue;
    const uint64_t pf = shfl64(prev, f), ef = shfl64(eff, f), tf = shfl64(trg, f);
    if (pf < S.last) {  // a duplicate
      ++S.head, ++S.ndrop;
      continue;
    }
    if (pf == S.last || !R.logging) {  // logging disabled: delivered as if it followed on
      if (lane == f && q < D.n) R.S.trig[q] = (uint32_t)trg;
      S.last = ef, ++S.head;
      continue;
    }
    if ((R.reach >> dc) & 1u) {  // query/3 = ok: the gap [last + 1, prev], and everything waits
      if (lane == 0 && tf >= 1 && tf - 1 < D.nr) R.S.gflag[tf - 1] = 1, R.S.gfrom[tf - 1] = S.last + 1, R.S.gto[tf - 1] = pf;
      S.mode = plan::MODE_BUFFERING, S.buf_from = tf;
      return;
    }
    S.mode = plan::MODE_NORMAL;  // "will retry on next ping message"
    return;
  }
  S.mode = plan::MODE_NORMAL;
}

__global__ void __launch_bounds__(64) k_sb_run(Run R) {
  if (R.stat[W_BAD]) return;
  const Dims &D = R.D;
  const uint32_t lane = threadIdx.x;
  const uint64_t *K1 = R.S.k1;
  const uint32_t *V1 = R.S.v1;
  for (uint64_t s = blockIdx.x; s < D.ns; s += gridDim.x) {
    const uint64_t qst = lower(K1, D.n, plan::stream_key(s, false)), mid = lower(K1, D.n, plan::stream_key(s, true));
    const uint64_t end = lower(K1, D.n, plan::stream_key(s + 1, false));
    const uint64_t qlen = mid - qst, rlen = end - mid;
    const uint64_t carried = lower(V1 + qst, qlen, D.q);  // a stream's entry indices ascend
    Walk S{};
    if (carried < qlen || rlen) {
      const uint32_t dc = (uint32_t)(s % D.n_dc);
      S.last = R.last[s], S.mode = R.mode[s] ? plan::MODE_BUFFERING : plan::MODE_NORMAL;
      S.budget = plan::step_bound(qlen, rlen);
      uint64_t seen = carried, ri = 0, unexp = 0;
      for (uint64_t seg = plan::segment_bound(rlen); seg; --seg) {
        uint64_t e = rlen;  // the segment's RESP_END, or none
        for (uint64_t t = ri; t < rlen; t += plan::TILE) {
          const bool in = t + lane < rlen && mid + t + lane < D.n;
          const uint64_t m = __ballot(in && R.W.kind[mid + t + lane] == plan::KIND_RESP_END);
          if (m) {
            e = t + (uint32_t)__builtin_ctzll(m);
            break;
          }
        }
        uint64_t end_row1 = 0, tail = qlen;
        if (e < rlen) {
          const uint64_t src = V1[mid + e < D.n ? mid + e : D.n - 1];
          end_row1 = src < D.q ? 0 : src - D.q + 1;
          tail = lower(V1 + qst, qlen, D.q + end_row1 - 1);  // the TXN rows before it are pushed
        }
        S.buf_from = S.mode == plan::MODE_BUFFERING ? 0 : ~0ull;
        if (S.mode == plan::MODE_NORMAL && tail > seen) {
          const uint64_t src = V1[qst + seen < D.n ? qst + seen : D.n - 1];
          sb_walk(R, qst, tail, src < D.q ? 0 : src - D.q + 1, dc, lane, S);
        }
        for (uint64_t t = ri; t < e; t += plan::TILE) {  // the RESP_TXN rows: delivered at once while buffering
          const uint64_t q = mid + t + lane;
          const bool in = t + lane < e && q < D.n;
          uint64_t row1 = 0;
          if (in) {
            const uint64_t src = V1[q];
            row1 = src < D.q ? 0 : src - D.q + 1;
          }
          const bool del = in && row1 > S.buf_from;
          if (del) R.S.trig[q] = (uint32_t)row1;
          unexp += (uint64_t)__popcll(__ballot(in && !del));
        }
        if (e >= rlen) break;
        if (S.mode == plan::MODE_BUFFERING) {
          if (S.head < tail) {
            const uint64_t hq = qst + S.head < D.n ? qst + S.head : D.n - 1;
            S.last = R.W.prev[hq];
            sb_walk(R, qst, tail, end_row1, dc, lane, S);
          } else {
            S.mode = plan::MODE_NORMAL;
          }
        } else {
          ++unexp;  // "This case must not happen"
        }
        seen = tail, ri = e + 1;
      }
      if (lane == 0) {
        R.last[s] = S.last, R.mode[s] = S.mode;
        if (S.ndrop) atomicAdd((unsigned long long *)&R.stat[W_DROP], (unsigned long long)S.ndrop);
        if (unexp) atomicAdd((unsigned long long *)&R.stat[W_UNEXP], (unsigned long long)unexp);
      }
    }
    if (lane == 0) R.qstart[s] = qst, R.qhead[s] = S.head, R.remain[s] = qlen - S.head;
  }
}

// one block: exclusive sums over the streams; the total goes to the status block
__global__ void __launch_bounds__(256) k_sb_scan(uint64_t ns, const uint64_t *remain, uint64_t *rem_off, uint64_t *stat) {
  if (stat[W_BAD]) return;
  typedef hipcub::BlockScan<uint64_t, 256> Scan;
  __shared__ typename Scan::TempStorage tmp;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < ns; base += 256) {
    const uint64_t s = base + threadIdx.x;
    const uint64_t r = s < ns ? remain[s] : 0;
    uint64_t x, sum;
    Scan(tmp).ExclusiveSum(r, x, sum);
    __syncthreads();
    if (s < ns) rem_off[s] = carry + x;
    carry += sum;
  }
  if (threadIdx.x == 0) rem_off[ns] = carry, stat[W_QUEUED] = carry;
}

struct Compact {
  Dims D;
  Buf W, A;
  const uint64_t *k1, *qstart, *qhead, *rem_off;
  const uint64_t *stat;
};
// where the sorted entry q goes in A, or ~0 when it left the queue or never was in it
__device__ __forceinline__ uint64_t sb_dest(const Compact &C, uint64_t q, uint64_t *stream) {
  const uint64_t kk = C.k1[q];
  const uint64_t s = (kk >> 1) < C.D.ns ? kk >> 1 : C.D.ns - 1;
  *stream = s;
  if (kk & 1) return ~0ull;
  const uint64_t idx = q - C.qstart[s];
  if (q < C.qstart[s] || idx < C.qhead[s]) return ~0ull;
  const uint64_t dst = C.rem_off[s] + (idx - C.qhead[s]);
  return dst < C.D.cap ? dst : ~0ull;
}
__global__ void __launch_bounds__(256) k_sb_compact(Compact C) {
  if (C.stat[W_BAD]) return;
  const uint32_t n_dc = C.D.n_dc;
  SB_GRID_LOOP(q, C.D.n) {
    uint64_t s;
    const uint64_t dst = sb_dest(C, q, &s);
    if (dst == ~0ull) continue;
    C.A.key[dst] = s, C.A.prev[dst] = C.W.prev[q], C.A.last[dst] = C.W.last[q], C.A.tag[dst] = C.W.tag[q];
    C.A.ts[dst] = C.W.ts[q], C.A.ping[dst] = C.W.ping[q];
  }
  SB_GRID_LOOP(i, C.D.n * n_dc) {
    const uint64_t q = i / n_dc, k = i - q * n_dc;
    uint64_t s;
    const uint64_t dst = sb_dest(C, q, &s);
    if (dst != ~0ull) C.A.snap[dst * n_dc + k] = C.W.snap[i];
  }
}

__global__ void __launch_bounds__(256) k_sb_keys(Dims D, Scratch S, int rbits, const uint64_t *stat) {
  if (stat[W_BAD]) return;
  SB_GRID_LOOP(q, D.n) {
    const uint64_t t = S.trig[q], kk = S.k1[q] >> 1;
    const uint64_t s = kk < D.ns ? kk : D.ns - 1;
    S.k0[q] = t && t <= D.nr ? plan::deliver_key(s / D.n_dc, t, rbits) : plan::deliver_key(D.n_part, 0, rbits);
    S.v0[q] = (uint32_t)q;
  }
}

__global__ void __launch_bounds__(256) k_sb_offsets(Dims D, const uint64_t *dk1, int rbits, uint64_t *out_off, uint64_t *stat) {
  if (stat[W_BAD]) return;
  SB_GRID_LOOP(p, (uint64_t)D.n_part + 1) {
    const uint64_t o = lower(dk1, D.n, plan::deliver_key(p, 0, rbits));
    out_off[p] = o;
    if (p == D.n_part) stat[W_DELIV] = o;
  }
}

__global__ void __launch_bounds__(256) k_sb_emit(Dims D, Buf W, Scratch S, int rbits, uint64_t cap_out, Out O, const uint64_t *stat) {
  if (stat[W_BAD]) return;
  const uint32_t n_dc = D.n_dc;
  SB_GRID_LOOP(i, D.n) {
    if ((S.dk1[i] >> rbits) >= D.n_part || i >= cap_out) continue;
    const uint64_t q = S.dv1[i] < D.n ? S.dv1[i] : D.n - 1, kk = S.k1[q] >> 1;
    const uint64_t s = kk < D.ns ? kk : D.ns - 1;
    if (O.part) O.part[i] = (uint32_t)(s / n_dc);
    if (O.dc) O.dc[i] = (uint8_t)(s % n_dc);
    if (O.ts) O.ts[i] = W.ts[q];
    if (O.ping) O.ping[i] = W.ping[q];
    if (O.tag) O.tag[i] = W.tag[q];
  }
  if (!O.snap) return;
  SB_GRID_LOOP(j, D.n * n_dc) {
    const uint64_t i = j / n_dc, k = j - i * n_dc;
    if ((S.dk1[i] >> rbits) >= D.n_part || i >= cap_out) continue;
    const uint64_t q = S.dv1[i] < D.n ? S.dv1[i] : D.n - 1;
    O.snap[j] = W.snap[q * n_dc + k];
  }
}

__global__ void __launch_bounds__(256) k_sb_gaps(Dims D, Rows R, Scratch S, uint64_t cap_gaps, am_sub_gaps G, uint64_t *stat) {
  if (stat[W_BAD]) return;
  SB_GRID_LOOP(t, D.nr) {
    const uint64_t i = S.gpos[t];
    if (t == D.nr - 1) stat[W_GAPS] = i + S.gflag[t];
    if (!S.gflag[t] || i >= cap_gaps) continue;
    G.part[i] = R.part[t], G.dc[i] = R.dc[t], G.from[i] = S.gfrom[t], G.to[i] = S.gto[t];
  }
}

__global__ void k_sb_find(const uint64_t *akey, uint64_t q, uint64_t s, uint64_t *stat) {
  if (blockIdx.x || threadIdx.x) return;
  stat[W_LO] = lower(akey, q, s), stat[W_HI] = lower(akey, q, s + 1);
}

unsigned grid_for(am_ctx *c, uint64_t items) {
  const uint64_t b = (items + 255) / 256, cap = (uint64_t)c->n_cu * 8;
  return (unsigned)(b == 0 ? 1 : b < cap ? b : cap);
}

}  // namespace

struct am_sub {
  am_ctx *ctx = nullptr;
  uint32_t n_dc = 0, n_part = 0, logging = 1, reach = 0xFFFFFFFFu;
  uint64_t cap = 0, queued = 0;
  Buf A{}, B{};
  uint64_t *last = nullptr;
  uint32_t *mode = nullptr;
  uint64_t *pers = nullptr;  // qstart, qhead, remain [ns]; rem_off [ns + 1]
  uint64_t *stat = nullptr;
  char *scr = nullptr;
  uint64_t scr_n = 0, scr_rows = 0;
  size_t tmp_bytes = 0;
  char *stage = nullptr;  // the host calls' staging
  size_t stage_bytes = 0;
  char *hand = nullptr;   // the chained call's am_dep_txns columns
  size_t hand_bytes = 0;
  uint64_t readbacks = 0;
};

namespace {

int dev_zeroed(am_ctx *ctx, size_t bytes, void **out) {
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
  if (e != hipSuccess) {
    am_set_error("am_sub: hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return AM_ERR_NOMEM;
  }
  const hipError_t m = hipMemsetAsync(p, 0, bytes ? bytes : 1, ctx->stream);
  if (m != hipSuccess) {
    (void)hipFree(p);
    am_set_error("am_sub: hipMemsetAsync: %s", hipGetErrorString(m));
    return AM_ERR_HIP;
  }
  *out = p;
  return AM_OK;
}

int buf_alloc(am_ctx *ctx, uint64_t cap, uint32_t n_dc, Buf *b) {
  int rc = dev_zeroed(ctx, cap * 8, (void **)&b->key);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->prev);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->last);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->tag);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->ts);
  if (!rc) rc = dev_zeroed(ctx, cap * 8 * n_dc, (void **)&b->snap);
  if (!rc) rc = dev_zeroed(ctx, cap, (void **)&b->ping);
  if (!rc) rc = dev_zeroed(ctx, cap, (void **)&b->kind);
  return rc;
}
void buf_free(Buf *b) {
  for (void *p : {(void *)b->key, (void *)b->prev, (void *)b->last, (void *)b->tag, (void *)b->ts, (void *)b->snap, (void *)b->ping,
                  (void *)b->kind})
    if (p) (void)hipFree(p);
  *b = Buf{};
}

// scratch for n = queued + n_rows entries: grown here, before the call's first kernel
int ensure_scratch(am_sub *c, uint64_t n, uint64_t nr, int sbits, int dbits, Scratch *S) {
  am_ctx *ctx = c->ctx;
  size_t tmp_b = 0;
  {
    size_t b1 = 0, b2 = 0, b3 = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k, k, v, v, (int)(n ? n : 1), 0, sbits, ctx->stream) != hipSuccess ||
        hipcub::DeviceRadixSort::SortPairs(nullptr, b2, k, k, v, v, (int)(n ? n : 1), 0, dbits, ctx->stream) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, b3, v, v, (int)(nr ? nr : 1), ctx->stream) != hipSuccess) {
      am_set_error("am_sub: sizing the sorts failed");
      return AM_ERR_HIP;
    }
    tmp_b = b1 > b2 ? b1 : b2;
    if (b3 > tmp_b) tmp_b = b3;
  }
  if (!c->scr || n > c->scr_n || nr > c->scr_rows || plan::up256(tmp_b) > c->tmp_bytes) {
    const uint64_t nn = n > c->scr_n ? n : c->scr_n, nt = nr > c->scr_rows ? nr : c->scr_rows;
    if (tmp_b < c->tmp_bytes) tmp_b = c->tmp_bytes;
    const plan::Layout L = plan::layout(nn, nt, tmp_b);
    AM_HIP(hipStreamSynchronize(ctx->stream));
    if (c->scr) AM_HIP(hipFree(c->scr));
    c->scr = nullptr, c->scr_n = c->scr_rows = 0;
    void *p = nullptr;
    if (int rc = dev_zeroed(ctx, L.total, &p)) return rc;
    c->scr = (char *)p, c->scr_n = nn, c->scr_rows = nt, c->tmp_bytes = plan::up256(tmp_b);
  }
  const plan::Layout L = plan::layout(c->scr_n, c->scr_rows, c->tmp_bytes);
  char *b = c->scr;
  S->k0 = (uint64_t *)(b + L.k0), S->k1 = (uint64_t *)(b + L.k1), S->dk1 = (uint64_t *)(b + L.dk1);
  S->v0 = (uint32_t *)(b + L.v0), S->v1 = (uint32_t *)(b + L.v1), S->dv1 = (uint32_t *)(b + L.dv1), S->trig = (uint32_t *)(b + L.trig);
  S->gfrom = (uint64_t *)(b + L.gfrom), S->gto = (uint64_t *)(b + L.gto);
  S->gflag = (uint32_t *)(b + L.gflag), S->gpos = (uint32_t *)(b + L.gpos);
  return AM_OK;
}

int ensure_block(am_ctx *ctx, char **blk, size_t *have, size_t total) {
  if (*have >= total) return AM_OK;
  AM_HIP(hipStreamSynchronize(ctx->stream));
  if (*blk) AM_HIP(hipFree(*blk));
  *blk = nullptr, *have = 0;
  void *p = nullptr;
  if (int rc = dev_zeroed(ctx, total + total / 4, &p)) return rc;
  *blk = (char *)p, *have = total + total / 4;
  return AM_OK;
}

// the checks that need no device: AM_OK, or the verdict with the error text set
int host_verdict(const char *who, am_sub *c, const am_sub_rows *T, bool need_cols, uint64_t cap_out, uint64_t cap_gaps) {
  const uint64_t nr = T->n_rows;
  if (nr >> 31) {
    am_set_error("%s: 2^31 or more rows in one batch", who);
    return AM_ERR_INVALID;
  }
  if (need_cols && nr && (!T->kind || !T->part || !T->dc || !T->prev_opid || !T->last_opid || !T->timestamp || !T->snap_vc || !T->tag)) {
    am_set_error("%s: the batch lacks a column", who);
    return AM_ERR_INVALID;
  }
  if (!plan::fits(c->queued, nr, c->cap)) {
    am_set_error("%s: %llu queued entries + %llu rows exceed cap_queued %llu", who, (unsigned long long)c->queued, (unsigned long long)nr,
                 (unsigned long long)c->cap);
    return AM_ERR_CAPACITY;
  }
  if (nr && (cap_out < c->queued + nr || cap_gaps < nr)) {
    am_set_error("%s: cap_out %llu below queued + n_rows = %llu, or cap_gaps %llu below n_rows", who, (unsigned long long)cap_out,
                 (unsigned long long)(c->queued + nr), (unsigned long long)cap_gaps);
    return AM_ERR_INVALID;
  }
  return AM_OK;
}

// The kernels of a call and the readback.  The caller holds the lock and has run host_verdict.
int process_impl(am_sub *c, const am_sub_rows *T, uint64_t cap_out, uint64_t *dev_out_off, const Out &O, uint64_t cap_gaps,
                 const am_sub_gaps &G, uint64_t *counts, uint32_t *bad) {
  am_ctx *ctx = c->ctx;
  hipStream_t s = ctx->stream;
  const uint64_t nr = T->n_rows;
  if (nr == 0) {
    AM_HIP(hipMemsetAsync(dev_out_off, 0, ((uint64_t)c->n_part + 1) * 8, s));
    counts[0] = counts[1] = counts[2] = counts[3] = 0, counts[4] = c->queued;
    return AM_OK;
  }
  const uint64_t n = c->queued + nr, ns = (uint64_t)c->n_part * c->n_dc;
  const int sbits = plan::stream_bits(ns), rbits = plan::row_bits(nr), dbits = plan::deliver_bits(c->n_part, nr);
  Scratch S{};
  if (int rc = ensure_scratch(c, n, nr, sbits, dbits, &S)) return rc;
  const plan::Layout L = plan::layout(c->scr_n, c->scr_rows, c->tmp_bytes);
  const Dims D{n, c->queued, nr, c->cap, ns, c->n_part, c->n_dc};
  const Rows R{nr, T->kind, T->part, T->dc, T->prev_opid, T->last_opid, T->timestamp, T->snap_vc, T->ping, T->tag};
  uint64_t *qstart = c->pers, *qhead = c->pers + ns, *remain = c->pers + 2 * ns, *rem_off = c->pers + 3 * ns;
  AM_HIP(hipMemsetAsync(c->stat, 0, W_N * sizeof(uint64_t), s));
  AM_HIP(hipMemsetAsync(S.trig, 0, n * 4, s));
  hipLaunchKernelGGL(k_sb_check, dim3(grid_for(ctx, n)), dim3(256), 0, s, D, R, (const uint64_t *)c->A.key, S, c->stat);
  size_t tb = c->tmp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(c->scr + L.tmp, tb, (const uint64_t *)S.k0, S.k1, (const uint32_t *)S.v0, S.v1, (int)n, 0, sbits,
                                         s) != hipSuccess) {
    am_set_error("am_sub_process: the sort by stream failed");
    return AM_ERR_HIP;
  }
  hipLaunchKernelGGL(k_sb_gather, dim3(grid_for(ctx, n * c->n_dc)), dim3(256), 0, s, D, R, c->A, c->B, S, (const uint64_t *)c->stat);
  Run U{};
  U.D = D, U.reach = c->reach, U.logging = c->logging, U.W = c->B, U.S = S, U.last = c->last, U.mode = c->mode;
  U.qstart = qstart, U.qhead = qhead, U.remain = remain, U.stat = c->stat;
  const uint64_t run_cap = (uint64_t)ctx->n_cu * 64;
  hipLaunchKernelGGL(k_sb_run, dim3((unsigned)(ns < run_cap ? ns : run_cap)), dim3(64), 0, s, U);
  hipLaunchKernelGGL(k_sb_scan, dim3(1), dim3(256), 0, s, ns, (const uint64_t *)remain, rem_off, c->stat);
  Compact C{};
  C.D = D, C.W = c->B, C.A = c->A, C.k1 = S.k1, C.qstart = qstart, C.qhead = qhead, C.rem_off = rem_off, C.stat = c->stat;
  hipLaunchKernelGGL(k_sb_compact, dim3(grid_for(ctx, n * c->n_dc)), dim3(256), 0, s, C);
  hipLaunchKernelGGL(k_sb_keys, dim3(grid_for(ctx, n)), dim3(256), 0, s, D, S, rbits, (const uint64_t *)c->stat);
  tb = c->tmp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(c->scr + L.tmp, tb, (const uint64_t *)S.k0, S.dk1, (const uint32_t *)S.v0, S.dv1, (int)n, 0,
                                         dbits, s) != hipSuccess) {
    am_set_error("am_sub_process: the sort of the deliveries failed");
    return AM_ERR_HIP;
  }
  hipLaunchKernelGGL(k_sb_offsets, dim3(grid_for(ctx, (uint64_t)c->n_part + 1)), dim3(256), 0, s, D, (const uint64_t *)S.dk1, rbits,
                     dev_out_off, c->stat);
  hipLaunchKernelGGL(k_sb_emit, dim3(grid_for(ctx, n * c->n_dc)), dim3(256), 0, s, D, c->B, S, rbits, cap_out, O, (const uint64_t *)c->stat);
  tb = c->tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(c->scr + L.tmp, tb, (const uint32_t *)S.gflag, S.gpos, (int)nr, s) != hipSuccess) {
    am_set_error("am_sub_process: the scan of the gaps failed");
    return AM_ERR_HIP;
  }
  hipLaunchKernelGGL(k_sb_gaps, dim3(grid_for(ctx, nr)), dim3(256), 0, s, D, R, S, cap_gaps, G, c->stat);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  ++c->readbacks;
  if (int rc = am_ctx_fetch(ctx, c->stat, W_N, st)) return rc;
  if (st[W_BAD]) {
    if (bad) *bad = (uint32_t)st[W_BAD];
    am_set_error("am_sub_process: a row names a kind, partition or DC out of range, or is a transaction with timestamp 0 (bits 0x%x)",
                 (unsigned)st[W_BAD]);
    return AM_ERR_INVALID;
  }
  c->queued = st[W_QUEUED];
  counts[0] = st[W_DELIV], counts[1] = st[W_GAPS], counts[2] = st[W_DROP], counts[3] = st[W_UNEXP], counts[4] = st[W_QUEUED];
  return AM_OK;
}

// Where a host call stages its rows and gaps: offsets into the staging block, taken from *off.
struct Stage {
  size_t o[9], g[4];
};
Stage stage_layout(uint64_t nr, uint32_t n_dc, size_t *off) {
  auto take = [off](size_t bytes) {
    const size_t o = *off;
    *off += plan::up256(bytes ? bytes : 1);
    return o;
  };
  return Stage{{take(nr), take(nr * 4), take(nr), take(nr * 8), take(nr * 8), take(nr * 8), take(nr * 8 * n_dc), take(nr), take(nr * 8)},
               {take(nr * 4), take(nr), take(nr * 8), take(nr * 8)}};
}
// the host rows into the staging block g; *d = the rows over the device copies
int stage_rows(am_sub *c, const am_sub_rows *h, char *g, const Stage &L, am_sub_rows *d) {
  hipStream_t s = c->ctx->stream;
  const uint64_t nr = h->n_rows;
  const size_t *o = L.o;
  *d = *h;
  d->kind = (const uint8_t *)(g + o[0]), d->part = (const uint32_t *)(g + o[1]), d->dc = (const uint8_t *)(g + o[2]);
  d->prev_opid = (const uint64_t *)(g + o[3]), d->last_opid = (const uint64_t *)(g + o[4]), d->timestamp = (const uint64_t *)(g + o[5]);
  d->snap_vc = (const uint64_t *)(g + o[6]), d->ping = h->ping ? (const uint8_t *)(g + o[7]) : nullptr, d->tag = (const uint64_t *)(g + o[8]);
  if (!nr) return AM_OK;
  AM_HIP(hipMemcpyAsync(g + o[0], h->kind, nr, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[1], h->part, nr * 4, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[2], h->dc, nr, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[3], h->prev_opid, nr * 8, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[4], h->last_opid, nr * 8, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[5], h->timestamp, nr * 8, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[6], h->snap_vc, nr * 8 * c->n_dc, hipMemcpyHostToDevice, s));
  if (h->ping) AM_HIP(hipMemcpyAsync(g + o[7], h->ping, nr, hipMemcpyHostToDevice, s));
  AM_HIP(hipMemcpyAsync(g + o[8], h->tag, nr * 8, hipMemcpyHostToDevice, s));
  return AM_OK;
}
am_sub_gaps staged_gaps(char *g, const Stage &L) {
  return am_sub_gaps{(uint32_t *)(g + L.g[0]), (uint8_t *)(g + L.g[1]), (uint64_t *)(g + L.g[2]), (uint64_t *)(g + L.g[3])};
}
// the first ng staged gaps to the host columns
int fetch_gaps(am_sub *c, const am_sub_gaps *host, const am_sub_gaps &G, uint64_t ng) {
  hipStream_t s = c->ctx->stream;
  if (!ng) return AM_OK;
  AM_HIP(hipMemcpyAsync(host->part, G.part, ng * 4, hipMemcpyDeviceToHost, s));
  AM_HIP(hipMemcpyAsync(host->dc, G.dc, ng, hipMemcpyDeviceToHost, s));
  AM_HIP(hipMemcpyAsync(host->from, G.from, ng * 8, hipMemcpyDeviceToHost, s));
  AM_HIP(hipMemcpyAsync(host->to, G.to, ng * 8, hipMemcpyDeviceToHost, s));
  return AM_OK;
}
bool gaps_ok(const am_sub_gaps *g) { return g && g->part && g->dc && g->from && g->to; }

// The chained call's verdicts that need no device, all before any kernel: both buffers share the
// context, n_part and n_dc; this buffer's own verdicts; what am_dep may have to hold afterwards fits
// its cap_queued, and cap_out reaches that bound (*bound).
int joint_verdict(const char *who, am_sub *c, am_dep *dep, const am_sub_rows *T, uint64_t cap_out, uint64_t cap_gaps, uint64_t *bound) {
  am_ctx *dctx = nullptr;
  uint32_t d_dc = 0, d_part = 0;
  if (am_dep_shape(dep, &dctx, &d_dc, &d_part) || dctx != c->ctx || d_dc != c->n_dc || d_part != c->n_part) {
    am_set_error("%s: the dependency buffer has another context, n_part or n_dc", who);
    return AM_ERR_INVALID;
  }
  const uint64_t nr = T->n_rows;
  if (int rc = host_verdict(who, c, T, true, c->queued + nr, cap_gaps)) return rc;
  uint64_t dq = 0, dcap = 0;
  if (int rc = am_dep_size(dep, &dq, &dcap)) return rc;
  *bound = plan::joint_bound(dq, c->queued, nr);
  if (*bound > dcap) {
    am_set_error("%s: %llu queued in am_dep + %llu queued here + %llu rows exceed am_dep's cap_queued %llu", who, (unsigned long long)dq,
                 (unsigned long long)c->queued, (unsigned long long)nr, (unsigned long long)dcap);
    return AM_ERR_CAPACITY;
  }
  if (nr && cap_out < *bound) {
    am_set_error("%s: cap_out %llu below the bound %llu", who, (unsigned long long)cap_out, (unsigned long long)*bound);
    return AM_ERR_INVALID;
  }
  return AM_OK;
}

}  // namespace

extern "C" {

int am_sub_destroy(am_sub *c) {
  if (!c) return AM_OK;
  am_ctx *ctx = c->ctx;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  buf_free(&c->A), buf_free(&c->B);
  for (void *p : {(void *)c->last, (void *)c->mode, (void *)c->pers, (void *)c->stat, (void *)c->scr, (void *)c->stage, (void *)c->hand})
    if (p) (void)hipFree(p);
  delete c;
  return AM_OK;
}

int am_sub_create(am_ctx *ctx, uint32_t n_dc, uint32_t n_part, uint64_t cap_queued, int logging_enabled, am_sub **out) {
  if (!ctx || !out) return AM_ERR_INVALID;
  if (!plan::create_ok(n_dc, n_part, cap_queued)) {
    am_set_error("am_sub_create: n_dc in 1..32, n_part >= 1, cap_queued in 1..2^30");
    return AM_ERR_INVALID;
  }
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  am_sub *c = new am_sub();
  c->ctx = ctx, c->n_dc = n_dc, c->n_part = n_part, c->cap = cap_queued, c->logging = logging_enabled ? 1 : 0;
  c->reach = plan::dc_mask(n_dc);
  const uint64_t ns = (uint64_t)n_part * n_dc;
  int rc = buf_alloc(ctx, cap_queued, n_dc, &c->A);
  if (!rc) rc = buf_alloc(ctx, cap_queued, n_dc, &c->B);
  if (!rc) rc = dev_zeroed(ctx, ns * 8, (void **)&c->last);
  if (!rc) rc = dev_zeroed(ctx, ns * 4, (void **)&c->mode);
  if (!rc) rc = dev_zeroed(ctx, (4 * ns + 1) * 8, (void **)&c->pers);
  if (!rc) rc = dev_zeroed(ctx, 256, (void **)&c->stat);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = AM_ERR_HIP;
  if (rc) {
    am_sub_destroy(c);
    return rc;
  }
  *out = c;
  return AM_OK;
}

int am_sub_reserve(am_sub *c, uint64_t cap_queued) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (!plan::cap_ok(cap_queued) || cap_queued < c->queued) {
    am_set_error("am_sub_reserve: cap_queued %llu below the %llu queued entries or outside 1..2^30", (unsigned long long)cap_queued,
                 (unsigned long long)c->queued);
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  Buf na{}, nb{};
  int rc = buf_alloc(ctx, cap_queued, c->n_dc, &na);
  if (!rc) rc = buf_alloc(ctx, cap_queued, c->n_dc, &nb);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    buf_free(&na), buf_free(&nb);
    return rc;
  }
  const uint64_t q = c->queued;
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  if (q) {
    uint64_t *const dst[] = {na.key, na.prev, na.last, na.tag, na.ts};
    uint64_t *const src[] = {c->A.key, c->A.prev, c->A.last, c->A.tag, c->A.ts};
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipMemcpyAsync(dst[i], src[i], q * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.snap, c->A.snap, q * 8 * c->n_dc, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.ping, c->A.ping, q, hipMemcpyDeviceToDevice, s);
  }
  const hipError_t y = hipStreamSynchronize(s);
  if (e == hipSuccess) e = y;
  if (e != hipSuccess) {  // the old buffers are still the state
    buf_free(&na), buf_free(&nb);
    am_set_error("am_sub_reserve: copying the queues failed: %s", hipGetErrorString(e));
    return AM_ERR_HIP;
  }
  buf_free(&c->A), buf_free(&c->B);
  c->A = na, c->B = nb, c->cap = cap_queued;
  return AM_OK;
}

int am_sub_clear(am_sub *c) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t ns = (uint64_t)c->n_part * c->n_dc;
  AM_HIP(hipMemsetAsync(c->last, 0, ns * 8, ctx->stream));
  AM_HIP(hipMemsetAsync(c->mode, 0, ns * 4, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  c->queued = 0;
  return AM_OK;
}

int am_sub_set_last(am_sub *c, uint32_t part, uint32_t dc, uint64_t opid) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (part >= c->n_part || dc >= c->n_dc) {
    am_set_error("am_sub_set_last: partition %u of %u, DC %u of %u", part, c->n_part, dc, c->n_dc);
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  AM_HIP(hipMemcpyAsync(c->last + (uint64_t)part * c->n_dc + dc, &opid, 8, hipMemcpyHostToDevice, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_sub_set_reachable(am_sub *c, uint32_t dc_mask) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  c->reach = dc_mask & plan::dc_mask(c->n_dc);
  return AM_OK;
}

int am_sub_process(am_sub *c, const am_sub_rows *T, uint64_t cap_out, uint64_t *dev_out_off, const am_dep_txns *dev_out,
                   uint64_t cap_gaps, const am_sub_gaps *dev_gaps, uint64_t *counts, uint32_t *bad) {
  if (!c || !T || !dev_out_off || !counts) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  if (int rc = host_verdict("am_sub_process", c, T, true, cap_out, cap_gaps)) return rc;
  if (T->n_rows && (!dev_out || !gaps_ok(dev_gaps))) {
    am_set_error("am_sub_process: the outputs lack a column");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  Out O{};
  am_sub_gaps G{};
  if (T->n_rows) {
    O = Out{(uint32_t *)dev_out->part, (uint8_t *)dev_out->dc, (uint64_t *)dev_out->timestamp, (uint64_t *)dev_out->snap_vc,
            (uint8_t *)dev_out->ping, (uint64_t *)dev_out->tag};
    G = *dev_gaps;
  }
  return process_impl(c, T, cap_out, dev_out_off, O, cap_gaps, G, counts, bad);
}

int am_sub_process_host(am_sub *c, const am_sub_rows *h, uint64_t cap_out, uint64_t *host_out_off, const am_dep_txns *host_out,
                        uint64_t cap_gaps, const am_sub_gaps *host_gaps, uint64_t *counts, uint32_t *bad) {
  if (!c || !h || !host_out_off || !counts) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  // the host-only verdicts first: a batch they refuse pays no allocation and no upload
  if (int rc = host_verdict("am_sub_process_host", c, h, true, cap_out, cap_gaps)) return rc;
  const uint64_t nr = h->n_rows;
  if (nr && (!host_out || !gaps_ok(host_gaps))) {
    am_set_error("am_sub_process_host: the outputs lack a column");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t room = nr ? c->queued + nr : 0;
  size_t off = 0;
  const Stage L = stage_layout(nr, c->n_dc, &off);
  const plan::Columns K = plan::columns(room, c->n_dc, c->n_part);
  const size_t o_cols = off;
  off += plan::up256(K.total);
  if (int rc = ensure_block(ctx, &c->stage, &c->stage_bytes, off)) return rc;
  hipStream_t s = ctx->stream;
  char *g = c->stage, *k = g + o_cols;
  am_sub_rows d;
  if (int rc = stage_rows(c, h, g, L, &d)) return rc;
  const Out O{(uint32_t *)(k + K.part), (uint8_t *)(k + K.dc), (uint64_t *)(k + K.ts), (uint64_t *)(k + K.snap), (uint8_t *)(k + K.ping),
              (uint64_t *)(k + K.tag)};
  const am_sub_gaps G = staged_gaps(g, L);
  uint64_t cnt[5] = {};
  if (int rc = process_impl(c, &d, room, (uint64_t *)(k + K.off), O, nr, G, cnt, bad)) {
    (void)hipStreamSynchronize(s);  // the host columns may go away
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_out_off, k + K.off, ((size_t)c->n_part + 1) * 8, hipMemcpyDeviceToHost, s));
  const uint64_t nd = cnt[0];
  if (nd) {
    if (host_out->part) AM_HIP(hipMemcpyAsync((void *)host_out->part, O.part, nd * 4, hipMemcpyDeviceToHost, s));
    if (host_out->dc) AM_HIP(hipMemcpyAsync((void *)host_out->dc, O.dc, nd, hipMemcpyDeviceToHost, s));
    if (host_out->timestamp) AM_HIP(hipMemcpyAsync((void *)host_out->timestamp, O.ts, nd * 8, hipMemcpyDeviceToHost, s));
    if (host_out->snap_vc) AM_HIP(hipMemcpyAsync((void *)host_out->snap_vc, O.snap, nd * 8 * c->n_dc, hipMemcpyDeviceToHost, s));
    if (host_out->ping) AM_HIP(hipMemcpyAsync((void *)host_out->ping, O.ping, nd, hipMemcpyDeviceToHost, s));
    if (host_out->tag) AM_HIP(hipMemcpyAsync((void *)host_out->tag, O.tag, nd * 8, hipMemcpyDeviceToHost, s));
  }
  if (int rc = fetch_gaps(c, host_gaps, G, cnt[1])) return rc;
  AM_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 5; ++i) counts[i] = cnt[i];
  return AM_OK;
}

int am_sub_deliver(am_sub *c, am_dep *dep, const am_sub_rows *T, uint64_t now, uint64_t cap_out, uint64_t *dev_out_off,
                   uint64_t *dev_out_tag, uint64_t *n_delivered, uint64_t cap_gaps, const am_sub_gaps *dev_gaps, uint64_t *counts,
                   uint32_t *bad) {
  if (!c || !dep || !T || !dev_out_off || !n_delivered || !counts) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  uint64_t bound = 0;
  // all or nothing: every verdict of either buffer that needs no device, before any kernel
  if (int rc = joint_verdict("am_sub_deliver", c, dep, T, cap_out, cap_gaps, &bound)) return rc;
  const uint64_t nr = T->n_rows;
  if (nr && (!dev_out_tag || !gaps_ok(dev_gaps))) {
    am_set_error("am_sub_deliver: the outputs lack a column");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t room = c->queued + nr;
  const plan::Columns K = plan::columns(room, c->n_dc, c->n_part);
  if (int rc = ensure_block(ctx, &c->hand, &c->hand_bytes, K.total)) return rc;
  char *k = c->hand;
  const Out O{(uint32_t *)(k + K.part), (uint8_t *)(k + K.dc), (uint64_t *)(k + K.ts), (uint64_t *)(k + K.snap), (uint8_t *)(k + K.ping),
              (uint64_t *)(k + K.tag)};
  am_sub_gaps G{};
  if (nr) G = *dev_gaps;
  if (int rc = process_impl(c, T, room, (uint64_t *)(k + K.off), O, cap_gaps, G, counts, bad)) return rc;
  am_dep_txns X{};
  X.n_tx = counts[0];
  X.part = O.part, X.dc = O.dc, X.timestamp = O.ts, X.snap_vc = O.snap, X.ping = O.ping, X.tag = O.tag;
  uint32_t dbad = 0;
  const int rc = am_dep_deliver(dep, &X, now, cap_out, dev_out_off, dev_out_tag, n_delivered, &dbad);
  if (rc && bad) *bad = dbad;
  return rc;
}

int am_sub_deliver_host(am_sub *c, am_dep *dep, const am_sub_rows *h, uint64_t now, uint64_t cap_out, uint64_t *host_out_off,
                        uint64_t *host_out_tag, uint64_t *n_delivered, uint64_t cap_gaps, const am_sub_gaps *host_gaps,
                        uint64_t *counts, uint32_t *bad) {
  if (!c || !dep || !h || !host_out_off || !n_delivered || !counts) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  uint64_t bound = 0;
  // every verdict that needs no device before the staging is touched
  if (int rc = joint_verdict("am_sub_deliver_host", c, dep, h, cap_out, cap_gaps, &bound)) return rc;
  const uint64_t nr = h->n_rows;
  if (nr && (!host_out_tag || !gaps_ok(host_gaps))) {
    am_set_error("am_sub_deliver_host: the outputs lack a column");
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  size_t off = 0;
  const Stage L = stage_layout(nr, c->n_dc, &off);
  const uint64_t room = nr ? bound : 0;
  const size_t o_off = off, o_tag = o_off + plan::up256(((size_t)c->n_part + 1) * 8);
  off = o_tag + plan::up256(room * 8 + 1);
  if (int rc = ensure_block(ctx, &c->stage, &c->stage_bytes, off)) return rc;
  hipStream_t s = ctx->stream;
  char *g = c->stage;
  am_sub_rows d;
  if (int rc = stage_rows(c, h, g, L, &d)) return rc;
  const am_sub_gaps G = staged_gaps(g, L);
  uint64_t cnt[5] = {}, nd = 0;
  if (int rc = am_sub_deliver(c, dep, &d, now, room, (uint64_t *)(g + o_off), (uint64_t *)(g + o_tag), &nd, nr, &G, cnt, bad)) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_out_off, g + o_off, ((size_t)c->n_part + 1) * 8, hipMemcpyDeviceToHost, s));
  if (nd) AM_HIP(hipMemcpyAsync(host_out_tag, g + o_tag, nd * 8, hipMemcpyDeviceToHost, s));
  if (int rc = fetch_gaps(c, host_gaps, G, cnt[1])) return rc;
  AM_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 5; ++i) counts[i] = cnt[i];
  *n_delivered = nd;
  return AM_OK;
}

int am_sub_stream(am_sub *c, uint32_t part, uint32_t dc, uint64_t *last, uint32_t *mode, uint64_t cap, uint64_t *tag, uint64_t *n) {
  if (!c || !last || !mode || !n || (cap && !tag)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (part >= c->n_part || dc >= c->n_dc) return AM_ERR_INVALID;
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t s = (uint64_t)part * c->n_dc + dc;
  hipLaunchKernelGGL(k_sb_find, dim3(1), dim3(64), 0, ctx->stream, (const uint64_t *)c->A.key, c->queued, s, c->stat);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  if (int rc = am_ctx_fetch(ctx, c->stat, W_N, st)) return rc;
  AM_HIP(hipMemcpyAsync(last, c->last + s, 8, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipMemcpyAsync(mode, c->mode + s, 4, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  const uint64_t lo = st[W_LO] < c->queued ? st[W_LO] : c->queued, hi = st[W_HI] < c->queued ? st[W_HI] : c->queued;
  const uint64_t m = hi > lo ? hi - lo : 0;
  *n = m;
  if (m > cap) return AM_ERR_CAPACITY;
  if (m) {
    AM_HIP(hipMemcpyAsync(tag, c->A.tag + lo, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    AM_HIP(hipStreamSynchronize(ctx->stream));
  }
  return AM_OK;
}

int am_sub_size(am_sub *c, uint64_t *queued, uint64_t *cap_queued) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (queued) *queued = c->queued;
  if (cap_queued) *cap_queued = c->cap;
  return AM_OK;
}

int am_sub_stats(am_sub *c, uint64_t *readbacks) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (readbacks) *readbacks = c->readbacks;
  return AM_OK;
}

}  // extern "C"
