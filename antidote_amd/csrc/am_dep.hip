// am_dep.hip -- the dependency buffer of every partition a GPU owns, on the device:
// inter_dc_dep_vnode's queues, try_store/2 and partition clock (src/inter_dc_dep_vnode.erl:94-154,
// 187-238), for batches of arrivals.  A call leaves the queues and clocks, and returns the deliveries,
// that serving the batch one arrival at a time in batch order gives (tests/depsim.py is the contract).
//
// State, sized by create / reserve only:
//   clock [n_part][n_dc], pres [n_part]   the partition clocks, in the layout am_gst_local_min reads; an
//                                         absent entry holds 0.  Never moved.
//   A, B                                  two queue buffers of cap_queued entries, structure of arrays
//                                         {key = partition * n_dc + dc, tag, timestamp, ping, snapshot
//                                         row}.  A is the state: the queued entries sorted by key, each
//                                         queue oldest first.  B is the call's working copy.
// deliver, all on the context's stream, one readback of the status block at the end:
//   k_dp_check    validity of part / dc / timestamp; the sort inputs: (key, entry) over the carried
//                 entries followed by the arrivals, and (partition, arrival) over the arrivals
//   radix sorts   stable (hipcub): entries by key -- a queue's carried entries, then its arrivals in
//                 batch order; arrivals by partition -- each partition's arrival order
//   k_dp_gather   the entries into B in sorted order, so a queue is contiguous; the arrivals' DCs in
//                 partition order
//   k_dp_run      one wave per partition plays that partition's arrivals in batch order: an arrival
//                 makes one more entry of its queue visible, then the rounds of process_all_queues/1
//                 run.  Within process_queue(d) only clock[d] changes and Dependencies[d] is 0, so the
//                 stored prefix of queue d is everything before the first visible entry whose
//                 dependencies fail against the current clock: a step evaluates 64 / group entries
//                 (group = the power of two >= n_dc; lane k of a group compares DC k), a ballot finds
//                 the first failure.  Clock, heads and tails live in registers.  A round that cannot
//                 change anything is skipped: the last round stored nothing and changed no clock entry,
//                 and the arrival went behind a blocked head.
//   k_dp_scan     exclusive sums of the partitions' delivered and remaining counts
//   k_dp_compact  the undelivered suffixes from B back into A, the deliveries into out_tag
// An invalid batch sets the status block's flag in the first kernel and every later kernel returns on
// it, so A and the clocks are still the state.
//
// Nothing grows, moves or is allocated between the kernels of a call: buffers come from create /
// reserve, the scratch (the sorts' temporary storage for this very count included) is grown before the
// call's first kernel, pointers and n_part / n_dc / capacities reach every kernel by value, and every
// index derived from part, dc or a sorted position is range-checked or clamped.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "am_dep_plan.h"
#include "am_internal.h"

namespace plan = am_dep_plan;

namespace {

enum { W_BAD = 0, W_DELIV = 1, W_QUEUED = 2, W_LO = 3, W_HI = 4, W_N = 8 };

struct Buf {
  uint64_t *key, *tag, *ts, *snap;
  uint8_t *ping;
};

struct Scratch {
  uint64_t *k0, *k1, *out;
  uint32_t *v0, *v1, *p0, *p1, *pv0, *pv1;
  uint8_t *adc;
};

struct Batch {
  uint64_t n_tx;
  const uint32_t *part;
  const uint8_t *dc;
  const uint64_t *ts, *snap;
  const uint8_t *ping;
  const uint64_t *tag;
};

// what every kernel of a call takes by value
struct Dims {
  uint64_t n, q, n_tx, cap;  // n = q carried + n_tx arriving entries
  uint32_t n_part, n_dc;
};

#define DP_GRID_LOOP(i, n) \
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

__global__ void __launch_bounds__(256) k_dp_check(Dims D, Batch B, const uint64_t *akey, Scratch S, uint64_t *stat) {
  DP_GRID_LOOP(i, D.n) {
    if (i < D.q) {
      S.k0[i] = akey[i], S.v0[i] = (uint32_t)i;
      continue;
    }
    const uint64_t t = i - D.q;
    uint32_t p = B.part[t], d = B.dc[t], bad = 0;
    if (p >= D.n_part) bad |= plan::BAD_PART, p = 0;
    if (d >= D.n_dc) bad |= plan::BAD_DC, d = 0;
    if (B.ts[t] == 0 && !(B.ping && B.ping[t])) bad |= plan::BAD_TIME;
    if (bad) atomicOr((unsigned long long *)&stat[W_BAD], (unsigned long long)bad);
    S.k0[i] = (uint64_t)p * D.n_dc + d, S.v0[i] = (uint32_t)i;
    S.p0[t] = p, S.pv0[t] = (uint32_t)t;
  }
}

__global__ void __launch_bounds__(256) k_dp_gather(Dims D, Batch B, Buf A, Buf W, Scratch S, const uint64_t *stat) {
  if (stat[W_BAD]) return;
  DP_GRID_LOOP(q, D.n) {
    const uint64_t src = S.v1[q];
    if (src < D.q) {
      W.tag[q] = A.tag[src], W.ts[q] = A.ts[src], W.ping[q] = A.ping[src];
    } else {
      const uint64_t t = src - D.q < D.n_tx ? src - D.q : D.n_tx - 1;
      W.tag[q] = B.tag[t], W.ts[q] = B.ts[t], W.ping[q] = B.ping && B.ping[t] ? 1 : 0;
    }
  }
  DP_GRID_LOOP(i, D.n * D.n_dc) {
    const uint64_t q = i / D.n_dc, k = i - q * D.n_dc, src = S.v1[q];
    if (src < D.q) {
      W.snap[i] = A.snap[src * D.n_dc + k];
    } else {
      const uint64_t t = src - D.q < D.n_tx ? src - D.q : D.n_tx - 1;
      W.snap[i] = B.snap[t * D.n_dc + k];
    }
  }
  DP_GRID_LOOP(j, D.n_tx) {
    const uint64_t t = S.pv1[j] < D.n_tx ? S.pv1[j] : D.n_tx - 1;
    const uint8_t d = B.dc[t];
    S.adc[j] = d < D.n_dc ? d : (uint8_t)(D.n_dc - 1);
  }
}

struct Run {
  Dims D;
  uint32_t own, drop, glog;
  uint64_t now;
  const uint8_t *ord, *inv;  // [n_dc]: the round's queue order and its inverse
  Buf W;
  Scratch S;
  uint64_t *clock;
  uint32_t *pres;
  uint64_t *qstart, *qhead, *rbefore;  // [n_part * n_dc]
  uint64_t *deliv, *remain;            // [n_part]
  const uint64_t *stat;
};

// One wave per partition.  Lane = (entry e of the step, DC k): k = lane & (group - 1), e = lane >> glog.
// The per-DC state of DC k (queue start, length, head, visible tail, clock entry) lives in every lane
// whose k it is; shfl64(x, d) reads DC d's.
__global__ void __launch_bounds__(64) k_dp_run(Run R) {
  if (R.stat[W_BAD]) return;
  const Dims &D = R.D;
  const uint32_t lane = threadIdx.x, n_dc = D.n_dc, gl = R.glog;
  const uint32_t k = lane & ((1u << gl) - 1u), e = lane >> gl, per = 64u >> gl;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  const uint64_t *K1 = R.S.k1;
  for (uint64_t p = blockIdx.x; p < D.n_part; p += gridDim.x) {
    const uint64_t kd = p * n_dc + (k < n_dc ? k : n_dc - 1);
    uint64_t st = 0, len = 0, head = 0, tail = 0, clk = 0;
    if (k < n_dc) {
      st = lower(K1, D.n, kd);
      len = lower(K1, D.n, kd + 1) - st;
      tail = lower(R.S.v1 + st, len, D.q);  // the carried entries: a segment's entry indices ascend
      clk = R.clock[kd];
    }
    uint32_t pres = R.pres[p];
    const uint64_t pst = shfl64(st, 0), pend = shfl64(st + len, n_dc - 1);
    const uint64_t a_lo = lower(R.S.p1, D.n_tx, p), a_hi = lower(R.S.p1, D.n_tx, p + 1);
    uint64_t ndel = 0;
    uint32_t nonempty = 0;  // bit i: the queue of DC ord[i] has a visible entry
    {
      uint64_t m = __ballot(lane < n_dc && tail > 0);
      while (m) {
        const uint32_t d = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        nonempty |= 1u << R.inv[d];
      }
    }
    bool stable = false;
    uint64_t budget = plan::round_bound(a_hi - a_lo, pend - pst);
    uint32_t adc_tile = 0;  // 64 arrivals' DCs, one per lane, loaded a tile ahead of use
    for (uint64_t a = a_lo; a < a_hi; ++a) {
      const uint32_t at = (uint32_t)(a - a_lo) & 63u;
      if (at == 0) adc_tile = a + lane < a_hi ? R.S.adc[a + lane] : 0;
      uint32_t d = (uint32_t)__shfl((int)adc_tile, (int)at, 64);
      d = d < n_dc ? d : n_dc - 1;
      const uint64_t hd = shfl64(head, d), tl = shfl64(tail, d), ln = shfl64(len, d);
      if (k == d && tail < len) ++tail;  // push_txn/2
      if (tl < ln) nonempty |= 1u << R.inv[d];
      if (stable && hd < tl) continue;   // behind a blocked head, nothing changed since it failed
      for (;;) {                         // process_all_queues/1
        if (budget == 0) break;
        --budget;
        uint64_t stored = 0;
        bool changed = false;
        uint32_t m = nonempty;
        while (m) {                      // process_queue/2 of DC dq
          const uint32_t oi = (uint32_t)__builtin_ctz(m);
          m &= m - 1;
          const uint32_t dq = R.ord[oi];
          uint64_t hq = shfl64(head, dq);
          const uint64_t tq = shfl64(tail, dq), sq = shfl64(st, dq);
          const uint64_t cur = k == R.own ? R.now : clk;  // get_partition_clock/1; an absent entry is 0
          while (hq < tq) {
            const uint32_t cnt = tq - hq < per ? (uint32_t)(tq - hq) : per;
            const bool valid = e < cnt;
            const uint64_t q = sq + hq + e;
            uint64_t ts = 0, tg = 0;
            uint32_t pg = 0;
            bool fail = false;
            if (valid && q < D.n) {
              ts = R.W.ts[q], pg = R.W.ping[q];
              if (k == 0) tg = R.W.tag[q];  // with the other columns, not after the vote
              if (!pg && k < n_dc && k != dq) fail = R.W.snap[q * n_dc + k] > cur;
            }
            const uint64_t failm = __ballot(fail);
            const uint32_t f = failm ? (uint32_t)__builtin_ctzll(failm) >> gl : cnt;  // the first entry that fails
            const bool lead = valid && k == 0 && e < f;
            const bool del = lead && !pg;
            const uint64_t delm = __ballot(del);
            if (del) {
              const uint64_t pos = pst + ndel + (uint64_t)__popcll(delm & lt_mask);
              if (pos < pend) R.S.out[pos] = tg;
            }
            ndel += (uint64_t)__popcll(delm);
            const uint64_t setm = __ballot(lead && !(pg && R.drop));
            if (setm) {  // the last stored entry that updates the clock: set, not max
              const uint64_t nts = shfl64(ts, 63u - (uint32_t)__builtin_clzll(setm));
              if (k == dq) clk = nts;
              pres |= 1u << dq;
            }
            hq += f, stored += f;
            if (f < cnt) {  // the head fails: clock[dq] = timestamp - 1
              const uint64_t nv = shfl64(ts, f << gl) - 1, old = shfl64(clk, dq);
              if (old != nv || !((pres >> dq) & 1u)) changed = true;
              if (k == dq) clk = nv;
              pres |= 1u << dq;
              break;
            }
          }
          if (k == dq) head = hq;
          if (hq >= tq) nonempty &= ~(1u << oi);
        }
        if (!stored) {
          stable = !changed;
          break;
        }
      }
    }
    if (lane < n_dc) {
      if (a_hi > a_lo) R.clock[kd] = clk;
      R.qstart[kd] = st, R.qhead[kd] = head;
    }
    const uint64_t rem = len - head;
    uint64_t before = 0, total = 0;
    for (uint32_t j = 0; j < n_dc; ++j) {
      const uint64_t v = shfl64(rem, j);
      if (j < k) before += v;
      total += v;
    }
    if (lane < n_dc) R.rbefore[kd] = before;
    if (lane == 0) {
      if (a_hi > a_lo) R.pres[p] = pres;
      R.deliv[p] = ndel, R.remain[p] = total;
    }
  }
}

// one block: exclusive sums over the partitions; the totals go to the status block
__global__ void __launch_bounds__(256) k_dp_scan(uint32_t n_part, const uint64_t *deliv, const uint64_t *remain,
                                                 uint64_t *out_off, uint64_t *rem_off, uint64_t *stat) {
  if (stat[W_BAD]) return;
  typedef hipcub::BlockScan<uint64_t, 256> Scan;
  __shared__ typename Scan::TempStorage tmp;
  uint64_t carry_d = 0, carry_r = 0;
  for (uint64_t base = 0; base < n_part; base += 256) {
    const uint64_t p = base + threadIdx.x;
    const uint64_t d = p < n_part ? deliv[p] : 0, r = p < n_part ? remain[p] : 0;
    uint64_t xd, xr, sd, sr;
    Scan(tmp).ExclusiveSum(d, xd, sd);
    __syncthreads();
    Scan(tmp).ExclusiveSum(r, xr, sr);
    __syncthreads();
    if (p < n_part) out_off[p] = carry_d + xd, rem_off[p] = carry_r + xr;
    carry_d += sd, carry_r += sr;
  }
  if (threadIdx.x == 0) {
    out_off[n_part] = carry_d, rem_off[n_part] = carry_r;
    stat[W_DELIV] = carry_d, stat[W_QUEUED] = carry_r;
  }
}

struct Compact {
  Dims D;
  Buf W, A;
  const uint64_t *k1, *out, *qstart, *qhead, *rbefore, *deliv, *out_off, *rem_off;
  uint64_t *out_tag;
  uint64_t cap_out;
  const uint64_t *stat;
};
// where the sorted entry q goes in A, or ~0 when it was stored
__device__ __forceinline__ uint64_t dp_dest(const Compact &C, uint64_t q, uint64_t *part) {
  const uint64_t nq = (uint64_t)C.D.n_part * C.D.n_dc;
  const uint64_t kd = C.k1[q] < nq ? C.k1[q] : nq - 1, p = kd / C.D.n_dc;
  *part = p;
  const uint64_t idx = q - C.qstart[kd];
  if (q < C.qstart[kd] || idx < C.qhead[kd]) return ~0ull;
  const uint64_t dst = C.rem_off[p] + C.rbefore[kd] + (idx - C.qhead[kd]);
  return dst < C.D.cap ? dst : ~0ull;
}
__global__ void __launch_bounds__(256) k_dp_compact(Compact C) {
  if (C.stat[W_BAD]) return;
  const uint32_t n_dc = C.D.n_dc;
  DP_GRID_LOOP(q, C.D.n) {
    uint64_t p;
    const uint64_t dst = dp_dest(C, q, &p);
    if (dst != ~0ull) C.A.key[dst] = C.k1[q], C.A.tag[dst] = C.W.tag[q], C.A.ts[dst] = C.W.ts[q], C.A.ping[dst] = C.W.ping[q];
    const uint64_t pst = C.qstart[p * n_dc];
    if (q >= pst && q - pst < C.deliv[p]) {
      const uint64_t o = C.out_off[p] + (q - pst);
      if (o < C.cap_out) C.out_tag[o] = C.out[q];
    }
  }
  DP_GRID_LOOP(i, C.D.n * n_dc) {
    const uint64_t q = i / n_dc, k = i - q * n_dc;
    uint64_t p;
    const uint64_t dst = dp_dest(C, q, &p);
    if (dst != ~0ull) C.A.snap[dst * n_dc + k] = C.W.snap[i];
  }
}

__global__ void k_dp_find(const uint64_t *akey, uint64_t q, uint64_t kd, uint64_t *stat) {
  if (blockIdx.x || threadIdx.x) return;
  stat[W_LO] = lower(akey, q, kd), stat[W_HI] = lower(akey, q, kd + 1);
}

unsigned grid_for(am_ctx *c, uint64_t items) {
  const uint64_t b = (items + 255) / 256, cap = (uint64_t)c->n_cu * 8;
  return (unsigned)(b == 0 ? 1 : b < cap ? b : cap);
}

}  // namespace

struct am_dep {
  am_ctx *ctx = nullptr;
  uint32_t n_dc = 0, own = 0, n_part = 0, drop = 0;
  uint8_t *order = nullptr;   // device: ord [MAX_DC], inv [MAX_DC]
  uint64_t cap = 0, queued = 0;
  Buf A{}, B{};
  uint64_t *clock = nullptr;
  uint32_t *pres = nullptr;
  uint64_t *perq = nullptr;   // qstart, qhead, rbefore: 3 x [n_part * n_dc]
  uint64_t *perp = nullptr;   // deliv, remain [n_part]; rem_off [n_part + 1]
  uint64_t *stat = nullptr;
  char *scr = nullptr;
  uint64_t scr_n = 0, scr_tx = 0;
  size_t sort_bytes = 0;
  char *stage = nullptr;
  size_t stage_bytes = 0;
  uint64_t readbacks = 0;
};

namespace {

int dev_zeroed(am_ctx *ctx, size_t bytes, void **out) {
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
  if (e != hipSuccess) {
    am_set_error("am_dep: hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return AM_ERR_NOMEM;
  }
  const hipError_t m = hipMemsetAsync(p, 0, bytes ? bytes : 1, ctx->stream);
  if (m != hipSuccess) {
    (void)hipFree(p);
    am_set_error("am_dep: hipMemsetAsync: %s", hipGetErrorString(m));
    return AM_ERR_HIP;
  }
  *out = p;
  return AM_OK;
}

int buf_alloc(am_ctx *ctx, uint64_t cap, uint32_t n_dc, Buf *b) {
  int rc = dev_zeroed(ctx, cap * 8, (void **)&b->key);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->tag);
  if (!rc) rc = dev_zeroed(ctx, cap * 8, (void **)&b->ts);
  if (!rc) rc = dev_zeroed(ctx, cap * 8 * n_dc, (void **)&b->snap);
  if (!rc) rc = dev_zeroed(ctx, cap, (void **)&b->ping);
  return rc;
}
void buf_free(Buf *b) {
  for (void *p : {(void *)b->key, (void *)b->tag, (void *)b->ts, (void *)b->snap, (void *)b->ping})
    if (p) (void)hipFree(p);
  *b = Buf{};
}

// scratch for n = queued + n_tx entries: grown here, before the call's first kernel
int ensure_scratch(am_dep *c, uint64_t n, uint64_t n_tx, int qbits, int pbits, Scratch *S) {
  am_ctx *ctx = c->ctx;
  size_t sort_b = 0;
  {
    size_t b1 = 0, b2 = 0;
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k, k, v, v, (int)(n ? n : 1), 0, qbits, ctx->stream) != hipSuccess ||
        hipcub::DeviceRadixSort::SortPairs(nullptr, b2, v, v, v, v, (int)(n_tx ? n_tx : 1), 0, pbits, ctx->stream) != hipSuccess) {
      am_set_error("am_dep: sizing the sorts failed");
      return AM_ERR_HIP;
    }
    sort_b = b1 > b2 ? b1 : b2;
  }
  if (!c->scr || n > c->scr_n || n_tx > c->scr_tx || plan::up256(sort_b) > c->sort_bytes) {
    const uint64_t nn = n > c->scr_n ? n : c->scr_n, nt = n_tx > c->scr_tx ? n_tx : c->scr_tx;
    if (sort_b < c->sort_bytes) sort_b = c->sort_bytes;
    const plan::Layout L = plan::layout(nn, nt, sort_b);
    AM_HIP(hipStreamSynchronize(ctx->stream));
    if (c->scr) AM_HIP(hipFree(c->scr));
    c->scr = nullptr, c->scr_n = c->scr_tx = 0;
    void *p = nullptr;
    if (int rc = dev_zeroed(ctx, L.total, &p)) return rc;
    c->scr = (char *)p, c->scr_n = nn, c->scr_tx = nt, c->sort_bytes = plan::up256(sort_b);
  }
  const plan::Layout L = plan::layout(c->scr_n, c->scr_tx, c->sort_bytes);
  char *b = c->scr;
  S->k0 = (uint64_t *)(b + L.k0), S->k1 = (uint64_t *)(b + L.k1), S->out = (uint64_t *)(b + L.out);
  S->v0 = (uint32_t *)(b + L.v0), S->v1 = (uint32_t *)(b + L.v1);
  S->p0 = (uint32_t *)(b + L.p0), S->p1 = (uint32_t *)(b + L.p1), S->pv0 = (uint32_t *)(b + L.pv0), S->pv1 = (uint32_t *)(b + L.pv1);
  S->adc = (uint8_t *)(b + L.adc);
  return AM_OK;
}

int ensure_stage(am_dep *c, size_t total) {
  if (c->stage_bytes >= total) return AM_OK;
  am_ctx *ctx = c->ctx;
  AM_HIP(hipStreamSynchronize(ctx->stream));
  if (c->stage) AM_HIP(hipFree(c->stage));
  c->stage = nullptr, c->stage_bytes = 0;
  void *p = nullptr;
  if (int rc = dev_zeroed(ctx, total + total / 4, &p)) return rc;
  c->stage = (char *)p, c->stage_bytes = total + total / 4;
  return AM_OK;
}

}  // namespace

extern "C" {

int am_dep_destroy(am_dep *c) {
  if (!c) return AM_OK;
  am_ctx *ctx = c->ctx;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  buf_free(&c->A), buf_free(&c->B);
  for (void *p : {(void *)c->clock, (void *)c->pres, (void *)c->perq, (void *)c->perp, (void *)c->stat, (void *)c->scr, (void *)c->stage,
                  (void *)c->order})
    if (p) (void)hipFree(p);
  delete c;
  return AM_OK;
}

int am_dep_create(am_ctx *ctx, uint32_t n_dc, uint32_t own_dc, uint32_t n_part, uint64_t cap_queued, const uint8_t *order,
                  am_dep **out) {
  if (!ctx || !out) return AM_ERR_INVALID;
  if (!plan::create_ok(n_dc, own_dc, n_part, cap_queued, order)) {
    am_set_error("am_dep_create: n_dc in 1..32, own_dc < n_dc, n_part >= 1, cap_queued in 1..2^30, order a permutation");
    return AM_ERR_INVALID;
  }
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  am_dep *c = new am_dep();
  c->ctx = ctx, c->n_dc = n_dc, c->own = own_dc, c->n_part = n_part, c->cap = cap_queued;
  uint8_t oi[2 * plan::MAX_DC] = {};
  for (uint32_t i = 0; i < n_dc; ++i) {
    const uint8_t d = order ? order[i] : (uint8_t)i;
    oi[i] = d, oi[plan::MAX_DC + d] = (uint8_t)i;
  }
  const uint64_t nq = (uint64_t)n_part * n_dc;
  int rc = buf_alloc(ctx, cap_queued, n_dc, &c->A);
  if (!rc) rc = buf_alloc(ctx, cap_queued, n_dc, &c->B);
  if (!rc) rc = dev_zeroed(ctx, nq * 8, (void **)&c->clock);
  if (!rc) rc = dev_zeroed(ctx, (uint64_t)n_part * 4, (void **)&c->pres);
  if (!rc) rc = dev_zeroed(ctx, 3 * nq * 8, (void **)&c->perq);
  if (!rc) rc = dev_zeroed(ctx, (3 * (uint64_t)n_part + 1) * 8, (void **)&c->perp);
  if (!rc) rc = dev_zeroed(ctx, 256, (void **)&c->stat);
  if (!rc) rc = dev_zeroed(ctx, sizeof oi, (void **)&c->order);
  if (!rc && hipMemcpyAsync(c->order, oi, sizeof oi, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = AM_ERR_HIP;
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = AM_ERR_HIP;
  if (rc) {
    am_dep_destroy(c);
    return rc;
  }
  *out = c;
  return AM_OK;
}

int am_dep_reserve(am_dep *c, uint64_t cap_queued) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (!plan::cap_ok(cap_queued) || cap_queued < c->queued) {
    am_set_error("am_dep_reserve: cap_queued %llu below the %llu queued entries or outside 1..2^30", (unsigned long long)cap_queued,
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
    e = hipMemcpyAsync(na.key, c->A.key, q * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.tag, c->A.tag, q * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.ts, c->A.ts, q * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.snap, c->A.snap, q * 8 * c->n_dc, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(na.ping, c->A.ping, q, hipMemcpyDeviceToDevice, s);
  }
  const hipError_t y = hipStreamSynchronize(s);
  if (e == hipSuccess) e = y;
  if (e != hipSuccess) {  // the old buffers are still the state
    buf_free(&na), buf_free(&nb);
    am_set_error("am_dep_reserve: copying the queues failed: %s", hipGetErrorString(e));
    return AM_ERR_HIP;
  }
  buf_free(&c->A), buf_free(&c->B);
  c->A = na, c->B = nb, c->cap = cap_queued;
  return AM_OK;
}

int am_dep_clear(am_dep *c) {
  if (!c) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  AM_HIP(hipSetDevice(ctx->device));
  AM_HIP(hipMemsetAsync(c->clock, 0, (uint64_t)c->n_part * c->n_dc * 8, ctx->stream));
  AM_HIP(hipMemsetAsync(c->pres, 0, (uint64_t)c->n_part * 4, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  c->queued = 0;
  return AM_OK;
}

int am_dep_set_clock(am_dep *c, uint32_t part, const uint64_t *host_vc, uint32_t pres) {
  if (!c || !host_vc) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (part >= c->n_part || (c->n_dc < 32 && (pres >> c->n_dc))) {
    am_set_error("am_dep_set_clock: partition %u of %u, presence 0x%x over %u DCs", part, c->n_part, pres, c->n_dc);
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  uint64_t row[plan::MAX_DC];
  for (uint32_t d = 0; d < c->n_dc; ++d) row[d] = ((pres >> d) & 1u) ? host_vc[d] : 0;  // an absent entry holds 0
  AM_HIP(hipMemcpyAsync(c->clock + (uint64_t)part * c->n_dc, row, c->n_dc * 8, hipMemcpyHostToDevice, ctx->stream));
  AM_HIP(hipMemcpyAsync(c->pres + part, &pres, 4, hipMemcpyHostToDevice, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_dep_set_drop_ping(am_dep *c, int on) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  c->drop = on ? 1 : 0;
  return AM_OK;
}

int am_dep_deliver(am_dep *c, const am_dep_txns *T, uint64_t now, uint64_t cap_out, uint64_t *dev_out_off, uint64_t *dev_out_tag,
                   uint64_t *n_delivered, uint32_t *bad) {
  if (!c || !T || !dev_out_off || !n_delivered) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  const uint64_t nt = T->n_tx;
  if (!plan::count_ok(nt)) {
    am_set_error("am_dep_deliver: 2^32 or more arrivals in one batch");
    return AM_ERR_INVALID;
  }
  if (nt && (!T->part || !T->dc || !T->timestamp || !T->snap_vc || !T->tag || !dev_out_tag)) {
    am_set_error("am_dep_deliver: the batch lacks a column");
    return AM_ERR_INVALID;
  }
  if (!plan::fits(c->queued, nt, c->cap)) {
    am_set_error("am_dep_deliver: %llu queued + %llu arriving entries exceed cap_queued %llu", (unsigned long long)c->queued,
                 (unsigned long long)nt, (unsigned long long)c->cap);
    return AM_ERR_CAPACITY;
  }
  const uint64_t n = c->queued + nt;
  if (nt && cap_out < n) {
    am_set_error("am_dep_deliver: cap_out %llu below queued + n_tx = %llu", (unsigned long long)cap_out, (unsigned long long)n);
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (nt == 0) {  // process_all_queues/1 runs only on an arrival
    AM_HIP(hipMemsetAsync(dev_out_off, 0, ((uint64_t)c->n_part + 1) * 8, s));
    *n_delivered = 0;
    return AM_OK;
  }
  Scratch S{};
  const int qbits = plan::bits_for((uint64_t)c->n_part * c->n_dc), pbits = plan::bits_for(c->n_part);
  if (int rc = ensure_scratch(c, n, nt, qbits, pbits, &S)) return rc;
  const plan::Layout L = plan::layout(c->scr_n, c->scr_tx, c->sort_bytes);
  const Dims D{n, c->queued, nt, c->cap, c->n_part, c->n_dc};
  const Batch B{nt, T->part, T->dc, T->timestamp, T->snap_vc, T->ping, T->tag};
  const uint64_t nq = (uint64_t)c->n_part * c->n_dc;
  uint64_t *qstart = c->perq, *qhead = c->perq + nq, *rbefore = c->perq + 2 * nq;
  uint64_t *deliv = c->perp, *remain = c->perp + c->n_part, *rem_off = c->perp + 2 * (uint64_t)c->n_part;
  AM_HIP(hipMemsetAsync(c->stat, 0, W_N * sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_dp_check, dim3(grid_for(ctx, n)), dim3(256), 0, s, D, B, (const uint64_t *)c->A.key, S, c->stat);
  {
    size_t tb = c->sort_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(c->scr + L.tmp, tb, (const uint64_t *)S.k0, S.k1, (const uint32_t *)S.v0, S.v1, (int)n, 0,
                                           qbits, s) != hipSuccess) {
      am_set_error("am_dep_deliver: the sort by queue failed");
      return AM_ERR_HIP;
    }
    tb = c->sort_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(c->scr + L.tmp, tb, (const uint32_t *)S.p0, S.p1, (const uint32_t *)S.pv0, S.pv1, (int)nt, 0,
                                           pbits, s) != hipSuccess) {
      am_set_error("am_dep_deliver: the sort by partition failed");
      return AM_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(k_dp_gather, dim3(grid_for(ctx, n * c->n_dc)), dim3(256), 0, s, D, B, c->A, c->B, S, (const uint64_t *)c->stat);
  Run R{};
  R.D = D, R.own = c->own, R.drop = c->drop, R.glog = plan::group_log2(c->n_dc), R.now = now, R.ord = c->order, R.inv = c->order + plan::MAX_DC;
  R.W = c->B, R.S = S, R.clock = c->clock, R.pres = c->pres;
  R.qstart = qstart, R.qhead = qhead, R.rbefore = rbefore, R.deliv = deliv, R.remain = remain, R.stat = c->stat;
  const uint64_t run_cap = (uint64_t)ctx->n_cu * 64;
  hipLaunchKernelGGL(k_dp_run, dim3((unsigned)(c->n_part < run_cap ? c->n_part : run_cap)), dim3(64), 0, s, R);
  hipLaunchKernelGGL(k_dp_scan, dim3(1), dim3(256), 0, s, c->n_part, (const uint64_t *)deliv, (const uint64_t *)remain, dev_out_off,
                     rem_off, c->stat);
  Compact C{};
  C.D = D, C.W = c->B, C.A = c->A, C.k1 = S.k1, C.out = S.out, C.qstart = qstart, C.qhead = qhead, C.rbefore = rbefore;
  C.deliv = deliv, C.out_off = dev_out_off, C.rem_off = rem_off, C.out_tag = dev_out_tag, C.cap_out = cap_out, C.stat = c->stat;
  hipLaunchKernelGGL(k_dp_compact, dim3(grid_for(ctx, n * c->n_dc)), dim3(256), 0, s, C);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  ++c->readbacks;
  if (int rc = am_ctx_fetch(ctx, c->stat, W_N, st)) return rc;
  if (st[W_BAD]) {
    if (bad) *bad = (uint32_t)st[W_BAD];
    am_set_error("am_dep_deliver: an arrival names a partition or DC out of range, or is a transaction with timestamp 0 (bits 0x%x)",
                 (unsigned)st[W_BAD]);
    return AM_ERR_INVALID;
  }
  c->queued = st[W_QUEUED];
  *n_delivered = st[W_DELIV];
  return AM_OK;
}

int am_dep_deliver_host(am_dep *c, const am_dep_txns *h, uint64_t now, uint64_t cap_out, uint64_t *host_out_off,
                        uint64_t *host_out_tag, uint64_t *n_delivered, uint32_t *bad) {
  if (!c || !h || !host_out_off || !n_delivered) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (bad) *bad = 0;
  const uint64_t nt = h->n_tx;
  if (!plan::count_ok(nt)) return AM_ERR_INVALID;
  if (nt && (!h->part || !h->dc || !h->timestamp || !h->snap_vc || !h->tag || !host_out_tag)) return AM_ERR_INVALID;
  // the host-only verdicts first: a batch they refuse pays no allocation and no upload
  if (!plan::fits(c->queued, nt, c->cap)) {
    am_set_error("am_dep_deliver_host: %llu queued + %llu arriving entries exceed cap_queued %llu", (unsigned long long)c->queued,
                 (unsigned long long)nt, (unsigned long long)c->cap);
    return AM_ERR_CAPACITY;
  }
  if (nt && cap_out < c->queued + nt) {
    am_set_error("am_dep_deliver_host: cap_out %llu below queued + n_tx = %llu", (unsigned long long)cap_out,
                 (unsigned long long)(c->queued + nt));
    return AM_ERR_INVALID;
  }
  AM_HIP(hipSetDevice(ctx->device));
  const uint64_t n = c->queued + nt, room = nt ? n : 0;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t o = off;
    off += plan::up256(bytes ? bytes : 1);
    return o;
  };
  const size_t o_part = take(nt * 4), o_dc = take(nt), o_ts = take(nt * 8), o_snap = take(nt * 8 * c->n_dc), o_ping = take(nt);
  const size_t o_tag = take(nt * 8), o_off = take(((size_t)c->n_part + 1) * 8), o_out = take(room * 8);
  if (int rc = ensure_stage(c, off)) return rc;
  hipStream_t s = ctx->stream;
  char *g = c->stage;
  if (nt) {
    AM_HIP(hipMemcpyAsync(g + o_part, h->part, nt * 4, hipMemcpyHostToDevice, s));
    AM_HIP(hipMemcpyAsync(g + o_dc, h->dc, nt, hipMemcpyHostToDevice, s));
    AM_HIP(hipMemcpyAsync(g + o_ts, h->timestamp, nt * 8, hipMemcpyHostToDevice, s));
    AM_HIP(hipMemcpyAsync(g + o_snap, h->snap_vc, nt * 8 * c->n_dc, hipMemcpyHostToDevice, s));
    if (h->ping) AM_HIP(hipMemcpyAsync(g + o_ping, h->ping, nt, hipMemcpyHostToDevice, s));
    AM_HIP(hipMemcpyAsync(g + o_tag, h->tag, nt * 8, hipMemcpyHostToDevice, s));
  }
  am_dep_txns d = *h;
  d.part = (const uint32_t *)(g + o_part), d.dc = (const uint8_t *)(g + o_dc), d.timestamp = (const uint64_t *)(g + o_ts);
  d.snap_vc = (const uint64_t *)(g + o_snap), d.ping = h->ping ? (const uint8_t *)(g + o_ping) : nullptr;
  d.tag = (const uint64_t *)(g + o_tag);
  uint64_t nd = 0;
  if (int rc = am_dep_deliver(c, &d, now, cap_out, (uint64_t *)(g + o_off), (uint64_t *)(g + o_out), &nd, bad)) {
    (void)hipStreamSynchronize(s);  // the host columns may go away
    return rc;
  }
  AM_HIP(hipMemcpyAsync(host_out_off, g + o_off, ((size_t)c->n_part + 1) * 8, hipMemcpyDeviceToHost, s));
  if (nd) AM_HIP(hipMemcpyAsync(host_out_tag, g + o_out, nd * 8, hipMemcpyDeviceToHost, s));
  AM_HIP(hipStreamSynchronize(s));
  *n_delivered = nd;
  return AM_OK;
}

int am_dep_clocks(am_dep *c, const uint64_t **part_vc, const uint32_t **part_pres) {
  if (!c || !part_vc || !part_pres) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  *part_vc = c->clock, *part_pres = c->pres;
  return AM_OK;
}

int am_dep_clock_host(am_dep *c, uint32_t part, uint64_t *vc, uint32_t *pres) {
  if (!c || !vc || !pres) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (part >= c->n_part) return AM_ERR_INVALID;
  AM_HIP(hipSetDevice(ctx->device));
  AM_HIP(hipMemcpyAsync(vc, c->clock + (uint64_t)part * c->n_dc, c->n_dc * 8, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipMemcpyAsync(pres, c->pres + part, 4, hipMemcpyDeviceToHost, ctx->stream));
  AM_HIP(hipStreamSynchronize(ctx->stream));
  return AM_OK;
}

int am_dep_queue(am_dep *c, uint32_t part, uint32_t dc, uint64_t cap, uint64_t *tag, uint64_t *n) {
  if (!c || !n || (cap && !tag)) return AM_ERR_INVALID;
  am_ctx *ctx = c->ctx;
  AM_LOCK(ctx);
  if (part >= c->n_part || dc >= c->n_dc) return AM_ERR_INVALID;
  AM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dp_find, dim3(1), dim3(64), 0, ctx->stream, (const uint64_t *)c->A.key, c->queued,
                     (uint64_t)part * c->n_dc + dc, c->stat);
  AM_HIP(hipGetLastError());
  uint64_t st[W_N] = {};
  if (int rc = am_ctx_fetch(ctx, c->stat, W_N, st)) return rc;
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

int am_dep_size(am_dep *c, uint64_t *queued, uint64_t *cap_queued) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (queued) *queued = c->queued;
  if (cap_queued) *cap_queued = c->cap;
  return AM_OK;
}

int am_dep_stats(am_dep *c, uint64_t *readbacks) {
  if (!c) return AM_ERR_INVALID;
  AM_LOCK(c->ctx);
  if (readbacks) *readbacks = c->readbacks;
  return AM_OK;
}

}  // extern "C"

// am_internal.h: for am_sub.hip's chained call
int am_dep_shape(const am_dep *c, am_ctx **ctx, uint32_t *n_dc, uint32_t *n_part) {
  if (!c || !ctx || !n_dc || !n_part) return AM_ERR_INVALID;
  *ctx = c->ctx, *n_dc = c->n_dc, *n_part = c->n_part;
  return AM_OK;
}
