// am_dep_plan.h -- the host arithmetic of the dependency buffer (am_dep.hip), plain C++ without HIP so
// that scripts/dep_cpu.cpp includes it too and a sanitizer build of that program covers it: the create
// arguments, the capacity and output verdicts, the lane tiling of the run kernel, the sort widths, the
// termination bound and the scratch layout.
#pragma once
#include <cstddef>
#include <cstdint>

namespace am_dep_plan {

constexpr uint32_t MAX_DC = 32;
constexpr uint32_t BAD_PART = 0x1u, BAD_DC = 0x2u, BAD_TIME = 0x4u;

// queue entries a buffer may hold: the sorts index carried + arriving entries with 32-bit values and
// take an int count
inline bool cap_ok(uint64_t cap) { return cap >= 1 && cap <= (1ull << 30); }

// order == nullptr (ascending) or a permutation of 0 .. n_dc - 1
inline bool order_ok(const uint8_t *order, uint32_t n_dc) {
  if (!order) return true;
  uint64_t seen = 0;
  for (uint32_t i = 0; i < n_dc; ++i) {
    if (order[i] >= n_dc || ((seen >> order[i]) & 1)) return false;
    seen |= 1ull << order[i];
  }
  return true;
}
inline bool create_ok(uint32_t n_dc, uint32_t own_dc, uint32_t n_part, uint64_t cap, const uint8_t *order) {
  return n_dc >= 1 && n_dc <= MAX_DC && own_dc < n_dc && n_part >= 1 && cap_ok(cap) && order_ok(order, n_dc);
}

// a batch the 32-bit indices can address
inline bool count_ok(uint64_t n_tx) { return !(n_tx >> 32); }
// queued + n_tx within cap, without wrapping
inline bool fits(uint64_t queued, uint64_t n_tx, uint64_t cap) { return queued <= cap && n_tx <= cap - queued; }

// The run kernel's tiling of a wave: group = the power of two >= n_dc lanes that evaluate one entry
// (lane k of a group compares DC k), per_step = 64 / group entries per step.
inline uint32_t group_log2(uint32_t n_dc) {
  uint32_t l = 0;
  while ((1u << l) < n_dc) ++l;
  return l;
}
inline uint32_t per_step(uint32_t n_dc) { return 64u >> group_log2(n_dc); }

// bits of the radix sorts' keys: values below n (at least 1 bit)
inline int bits_for(uint64_t n) {
  int b = 1;
  while (b < 64 && (n - 1) >> b) ++b;
  return b;
}

// Every round of process_all_queues either stores an entry or is the last of its arrival, so a
// partition plays at most arrivals + entries rounds in one call.
constexpr uint64_t round_bound(uint64_t arrivals, uint64_t entries) { return arrivals + entries; }

// The per-call scratch, carved from one block: offsets in bytes, every array 256-byte aligned.
// n = carried + arriving entries, n_tx = arriving.
struct Layout {
  size_t k0, k1, out;          // u64 [n]: sort keys in / out, a partition's deliveries before the scan
  size_t v0, v1;               // u32 [n]: entry index in / out
  size_t p0, p1, pv0, pv1;     // u32 [n_tx]: partition in / out, arrival in / out
  size_t adc;                  // u8 [n_tx]: the origin DCs in (partition, arrival) order
  size_t tmp, total;           // the sorts' temporary storage
};
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline Layout layout(uint64_t n, uint64_t n_tx, size_t sort_bytes) {
  Layout L{};
  size_t off = 0;
  const size_t a8 = up256((size_t)(n + 1) * 8), a4 = up256((size_t)(n + 1) * 4), t4 = up256((size_t)(n_tx + 1) * 4);
  size_t *const p8[] = {&L.k0, &L.k1, &L.out};
  for (size_t *p : p8) *p = off, off += a8;
  size_t *const p4[] = {&L.v0, &L.v1};
  for (size_t *p : p4) *p = off, off += a4;
  size_t *const pt[] = {&L.p0, &L.p1, &L.pv0, &L.pv1};
  for (size_t *p : pt) *p = off, off += t4;
  L.adc = off, off += up256((size_t)n_tx + 1);
  L.tmp = off, off += up256(sort_bytes);
  L.total = off;
  return L;
}

}  // namespace am_dep_plan
