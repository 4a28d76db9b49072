// am_cert_plan.h -- the host arithmetic of the certifier (am_cert.hip), plain C++ without HIP so that
// scripts/cert_cpu.cpp includes it too and a sanitizer build of that program covers it: table sizing,
// the load limit, when a prepare compacts first, the capacity verdicts, the scratch layout, and the
// offset check in its host form (the library runs the same predicate on the device).
#pragma once
#include <cstddef>
#include <cstdint>

namespace am_cert_plan {

// slots of a table that holds up to cap items: a power of two, at least twice cap, at least 16
inline uint64_t slots_for(uint64_t cap) {
  uint64_t s = 16;
  while (s < cap * 2 && s < (1ull << 62)) s <<= 1;
  return s;
}
// a capacity whose table a device can hold and whose doubling does not wrap
inline bool cap_ok(uint64_t cap) { return cap <= (1ull << 40); }

// used slots (live + tombstones) a prepared table may reach: three quarters, so every probe loop ends
// at a never-used slot
inline uint64_t load_limit(uint64_t slots) { return slots - slots / 4; }

// a prepare of `incoming` pairs compacts first when the pairs could pass the load limit and there are
// tombstones to drop.  After compaction used == live <= cap <= slots / 2, and the capacity verdict
// keeps the inserts within cap, so the limit holds either way.
inline bool must_compact(uint64_t live, uint64_t used, uint64_t incoming, uint64_t slots) {
  const uint64_t lim = load_limit(slots);
  return used > live && (incoming > lim || used > lim - incoming);
}

// live + fresh items within cap, without wrapping
inline bool fits(uint64_t live, uint64_t fresh, uint64_t cap) { return live <= cap && fresh <= cap - live; }

// a batch the 32-bit pair and transaction indices can address
inline bool counts_ok(uint64_t n_tx, uint64_t n_pairs) { return !(n_tx >> 32) && !(n_pairs >> 32); }

// key_off non-decreasing from 0 to n_pairs
inline bool offsets_ok(const uint64_t *key_off, uint64_t n_tx, uint64_t n_pairs) {
  if (!key_off) return n_tx == 0 && n_pairs == 0;
  if (key_off[0] != 0 || key_off[n_tx] != n_pairs) return false;
  for (uint64_t t = 0; t < n_tx; ++t)
    if (key_off[t] > key_off[t + 1]) return false;
  return true;
}

// The per-call scratch, carved from one block: offsets in bytes, every array 256-byte aligned.
struct Layout {
  size_t k0, k1, k2;                                            // u64 [n_pairs]
  size_t v0, v1, tx_of, head, run_of, first_ok, low0, low1, ins;  // u32 [n_pairs]
  size_t st, ext;                                               // i32 / u32 [n_tx]
  size_t tmp, total;                                            // the sort's temporary storage
};
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline Layout layout(uint64_t n_tx, uint64_t n_pairs, size_t sort_bytes) {
  Layout L{};
  size_t off = 0;
  const size_t a8 = up256((size_t)(n_pairs + 1) * 8), a4 = up256((size_t)(n_pairs + 1) * 4), t4 = up256((size_t)(n_tx + 1) * 4);
  size_t *const p8[] = {&L.k0, &L.k1, &L.k2};
  for (size_t *p : p8) *p = off, off += a8;
  size_t *const p4[] = {&L.v0, &L.v1, &L.tx_of, &L.head, &L.run_of, &L.first_ok, &L.low0, &L.low1, &L.ins};
  for (size_t *p : p4) *p = off, off += a4;
  L.st = off, off += t4;
  L.ext = off, off += t4;
  L.tmp = off, off += up256(sort_bytes);
  L.total = off;
  return L;
}

}  // namespace am_cert_plan
