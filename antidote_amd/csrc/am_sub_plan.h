// am_sub_plan.h -- the host arithmetic of the subscriber buffer (am_sub.hip), plain C++ without HIP so
// that scripts/sub_cpu.cpp includes it too and a sanitizer build of that program covers it: the create
// arguments, the capacity and output verdicts, the sort keys and their widths, the tile of the walk,
// the termination bounds and the scratch layout.
#pragma once
#include <cstddef>
#include <cstdint>

namespace am_sub_plan {

constexpr uint32_t MAX_DC = 32;
constexpr uint32_t BAD_PART = 0x1u, BAD_DC = 0x2u, BAD_TIME = 0x4u, BAD_KIND = 0x8u;
constexpr uint32_t KIND_TXN = 0, KIND_RESP_TXN = 1, KIND_RESP_END = 2;
constexpr uint32_t MODE_NORMAL = 0, MODE_BUFFERING = 1;
// entries of a queue one step of the walk tests: one per lane of a wave
constexpr uint32_t TILE = 64;

// queue entries a buffer may hold: the sorts index carried entries + rows with 32-bit values and take
// an int count
inline bool cap_ok(uint64_t cap) { return cap >= 1 && cap <= (1ull << 30); }
inline bool create_ok(uint32_t n_dc, uint32_t n_part, uint64_t cap) {
  return n_dc >= 1 && n_dc <= MAX_DC && n_part >= 1 && cap_ok(cap);
}
// queued + n_rows within cap, without wrapping
inline bool fits(uint64_t queued, uint64_t n_rows, uint64_t cap) { return queued <= cap && n_rows <= cap - queued; }
// the chained call: what am_dep may have to hold afterwards, or ~0 when the sum wraps
inline uint64_t joint_bound(uint64_t dep_queued, uint64_t sub_queued, uint64_t n_rows) {
  const uint64_t a = dep_queued + sub_queued;
  if (a < dep_queued || a + n_rows < a) return ~0ull;
  return a + n_rows;
}
// the DCs a mask may name
inline uint32_t dc_mask(uint32_t n_dc) { return n_dc >= 32 ? 0xFFFFFFFFu : (1u << n_dc) - 1u; }

// bits of a radix sort's keys: values below n (at least 1 bit)
inline int bits_for(uint64_t n) {
  int b = 1;
  while (b < 64 && (n - 1) >> b) ++b;
  return b;
}

// The first sort's key: a stream's queue entries (carried, then this call's TXN rows) before its
// response rows (RESP_TXN, RESP_END), each in batch order under a stable sort.
constexpr uint64_t stream_key(uint64_t stream, bool response) { return stream * 2 + (response ? 1 : 0); }
inline int stream_bits(uint64_t n_streams) { return bits_for(n_streams * 2); }

// The second sort's key: the deliveries by (partition, triggering row); a row is named 1-based so that
// 0 can stand for "not delivered".  What is not delivered sorts behind every partition.
inline int row_bits(uint64_t n_rows) { return bits_for(n_rows + 2); }
inline int deliver_bits(uint32_t n_part, uint64_t n_rows) { return bits_for((uint64_t)n_part + 1) + row_bits(n_rows); }
constexpr uint64_t deliver_key(uint64_t part, uint64_t row1, int rbits) { return (part << rbits) | row1; }

// A stream's rows split into at most rows + 1 segments.  A walk starts at a RESP_END row or, once per
// segment, at the segment's first TXN row, so a call runs at most 2 * (rows + 1) walks on a stream.
// Every step of a walk delivers or drops at least one entry, or ends the walk.  So a stream takes at
// most entries + 2 * (rows + 1) steps in one call.
constexpr uint64_t step_bound(uint64_t entries, uint64_t rows) { return entries + 2 * (rows + 1); }
constexpr uint64_t segment_bound(uint64_t rows) { return rows + 1; }

// The per-call scratch, carved from one block: offsets in bytes, every array 256-byte aligned.
// n = carried entries + rows, n_rows = rows.
struct Layout {
  size_t k0, k1, dk1;          // u64 [n]: stream keys in / out (k0 again: delivery keys in), delivery keys out
  size_t v0, v1, dv1, trig;    // u32 [n]: entry index in / out (v0 again: delivery values in), delivery
                               //          values out, the triggering row (1-based) of a delivered entry
  size_t gfrom, gto;           // u64 [n_rows]: the gap a row triggered
  size_t gflag, gpos;          // u32 [n_rows]: whether it triggered one, and the exclusive sum
  size_t tmp, total;           // the sorts' and the scan's temporary storage
};
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline Layout layout(uint64_t n, uint64_t n_rows, size_t tmp_bytes) {
  Layout L{};
  size_t off = 0;
  const size_t a8 = up256((size_t)(n + 1) * 8), a4 = up256((size_t)(n + 1) * 4);
  const size_t r8 = up256((size_t)(n_rows + 1) * 8), r4 = up256((size_t)(n_rows + 1) * 4);
  size_t *const p8[] = {&L.k0, &L.k1, &L.dk1};
  for (size_t *p : p8) *p = off, off += a8;
  size_t *const p4[] = {&L.v0, &L.v1, &L.dv1, &L.trig};
  for (size_t *p : p4) *p = off, off += a4;
  size_t *const q8[] = {&L.gfrom, &L.gto};
  for (size_t *p : q8) *p = off, off += r8;
  size_t *const q4[] = {&L.gflag, &L.gpos};
  for (size_t *p : q4) *p = off, off += r4;
  L.tmp = off, off += up256(tmp_bytes);
  L.total = off;
  return L;
}

// The columns of am_dep_txns for cap entries, carved from one block (the chained call's hand-off and
// the host call's staging): part u32, dc u8, timestamp u64, snap u64 [n_dc], ping u8, tag u64, and the
// offsets u64 [n_part + 1].
struct Columns {
  size_t part, dc, ts, snap, ping, tag, off, total;
};
inline Columns columns(uint64_t cap, uint32_t n_dc, uint32_t n_part) {
  Columns C{};
  size_t o = 0;
  const size_t c = (size_t)cap + 1;
  C.part = o, o += up256(c * 4);
  C.dc = o, o += up256(c);
  C.ts = o, o += up256(c * 8);
  C.snap = o, o += up256(c * 8 * n_dc);
  C.ping = o, o += up256(c);
  C.tag = o, o += up256(c * 8);
  C.off = o, o += up256(((size_t)n_part + 1) * 8);
  C.total = o;
  return C;
}

}  // namespace am_sub_plan
