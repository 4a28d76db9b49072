// sub_cpu.cpp -- the subscriber buffer, single-threaded: one inter_dc_sub_buf state machine per
// (partition, origin DC) stream, served one row at a time over the columns am_sub_process takes.  It is
// the CPU baseline of scripts/bench_sub.py and a second restatement of tests/subsim.py (a CPU test pins
// the two together).  It shares antidote_amd/csrc/am_sub_plan.h with the library, so a build of this
// program with -fsanitize=address,undefined covers the library's host arithmetic: --selfcheck walks it.
//
//   g++ -O2 -std=c++17 -I antidote_amd/csrc scripts/sub_cpu.cpp -o sub_cpu
//   sub_cpu [--quiet] [--selfcheck] < history
//   sub_cpu [--quiet] --columns FILE        one batch from a binary file, little-endian: u64 n_dc, n_part,
//                                           logging_enabled, n_rows, then the columns of am_sub_rows in the
//                                           struct's order and element types (ping always present)
//
// A history is whitespace-separated tokens, every number a decimal u64:
//   C n_dc n_part logging_enabled                                       (a new buffer)
//   P n_rows { kind part dc prev_opid last_opid timestamp ping tag snap*n_dc }*
//        -> "D n { part tag }*" partition-major, "G n { part dc from to }*",
//           "N delivered gaps dropped unexpected queued"; an invalid batch: "E bad" and nothing changes
//   L part dc opid                                                      set_last
//   R dc_mask                                                           set_reachable
//   Z                                                                   clear
//   X   -> "S part dc last mode n tag*" per stream that is not new, "X"
// The history is parsed first; the commands then run under a clock, and the last line is
// "T <milliseconds> <rows served>".  --quiet prints that line only.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "am_sub_plan.h"

namespace plan = am_sub_plan;

struct Stream {
  uint64_t last = 0;
  uint32_t mode = plan::MODE_NORMAL;
  std::deque<uint32_t> q;  // rows of the arena
};

// the transactions the queues hold, by column
struct Arena {
  std::vector<uint64_t> prev, eff, tag;
  std::vector<uint32_t> free_;
  uint32_t put(uint64_t p, uint64_t e, uint64_t t) {
    if (!free_.empty()) {
      const uint32_t i = free_.back();
      free_.pop_back();
      prev[i] = p, eff[i] = e, tag[i] = t;
      return i;
    }
    prev.push_back(p), eff.push_back(e), tag.push_back(t);
    return (uint32_t)(prev.size() - 1);
  }
};

struct Gap {
  uint32_t part, dc;
  uint64_t from, to;
};

struct Sub {
  uint32_t n_dc = 1, n_part = 1, reach = 0xFFFFFFFFu;
  bool logging = true;
  std::vector<Stream> streams;
  Arena ar;
  uint64_t queued = 0, dropped = 0, unexpected = 0;

  void process_queue(Stream &s, uint32_t part, uint32_t dc, std::vector<uint64_t> *out, std::vector<Gap> *gaps) {
    for (;;) {
      if (s.q.empty()) {
        s.mode = plan::MODE_NORMAL;
        return;
      }
      const uint32_t h = s.q.front();
      const uint64_t prev = ar.prev[h];
      if (prev == s.last || (prev > s.last && !logging)) {
        out->push_back(ar.tag[h]);
        s.last = ar.eff[h];
      } else if (prev < s.last) {
        ++dropped;
      } else if ((reach >> dc) & 1u) {
        gaps->push_back(Gap{part, dc, s.last + 1, prev});
        s.mode = plan::MODE_BUFFERING;
        return;
      } else {
        s.mode = plan::MODE_NORMAL;
        return;
      }
      s.q.pop_front(), ar.free_.push_back(h), --queued;
    }
  }

  void handle(uint32_t kind, uint32_t part, uint32_t dc, uint64_t prev, uint64_t last, bool ping, uint64_t tag,
              std::vector<uint64_t> *out, std::vector<Gap> *gaps) {
    Stream &s = streams[(size_t)part * n_dc + dc];
    if (kind == plan::KIND_TXN) {
      s.q.push_back(ar.put(prev, ping ? prev : last, tag)), ++queued;
      if (s.mode == plan::MODE_NORMAL) process_queue(s, part, dc, out, gaps);
    } else if (kind == plan::KIND_RESP_TXN) {
      if (s.mode == plan::MODE_BUFFERING) out->push_back(tag);
      else ++unexpected;
    } else if (s.mode == plan::MODE_BUFFERING) {
      if (!s.q.empty()) s.last = ar.prev[s.q.front()];
      process_queue(s, part, dc, out, gaps);
    } else {
      ++unexpected;
    }
  }
};

struct Cmd {
  char op;
  uint64_t a = 0, b = 0, c = 0;  // C: n_dc n_part logging; L: part dc opid; R: mask
  std::vector<uint8_t> kind, dc, ping;
  std::vector<uint32_t> part;
  std::vector<uint64_t> prev, last, ts, tag, snap;
};

static bool next_u64(uint64_t *v) {
  char tok[64];
  if (scanf("%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = strtoull(tok, &end, 10);
  if (*end) {
    fprintf(stderr, "sub_cpu: bad number '%s'\n", tok);
    exit(2);
  }
  return true;
}
static uint64_t need() {
  uint64_t v = 0;
  if (!next_u64(&v)) {
    fprintf(stderr, "sub_cpu: truncated history\n");
    exit(2);
  }
  return v;
}

// one C and one P command from a file of columns
static bool read_columns(const char *path, std::vector<Cmd> *cmds) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint64_t h[4] = {};
  bool ok = fread(h, 8, 4, f) == 4 && h[0] <= plan::MAX_DC && !(h[1] >> 32) && plan::create_ok((uint32_t)h[0], (uint32_t)h[1], 1) &&
            !(h[3] >> 31);
  Cmd c, p;
  c.op = 'C', c.a = h[0], c.b = h[1], c.c = h[2];
  p.op = 'P';
  if (ok) {
    const size_t n = (size_t)h[3];
    p.kind.resize(n), p.part.resize(n), p.dc.resize(n), p.prev.resize(n), p.last.resize(n), p.ts.resize(n);
    p.snap.resize(n * (size_t)h[0]), p.ping.resize(n), p.tag.resize(n);
    auto rd = [&](void *dst, size_t size, size_t count) { ok = ok && (count == 0 || fread(dst, size, count, f) == count); };
    rd(p.kind.data(), 1, n), rd(p.part.data(), 4, n), rd(p.dc.data(), 1, n), rd(p.prev.data(), 8, n), rd(p.last.data(), 8, n);
    rd(p.ts.data(), 8, n), rd(p.snap.data(), 8, p.snap.size()), rd(p.ping.data(), 1, n), rd(p.tag.data(), 8, n);
  }
  fclose(f);
  if (ok) cmds->push_back(std::move(c)), cmds->push_back(std::move(p));
  return ok;
}

static int selfcheck() {
  int bad = 0;
  bad += !plan::create_ok(1, 1, 1) || !plan::create_ok(32, ~0u, 1ull << 30);
  bad += plan::create_ok(0, 1, 1) || plan::create_ok(33, 1, 1) || plan::create_ok(4, 0, 1) || plan::create_ok(4, 1, 0) ||
         plan::create_ok(4, 1, (1ull << 30) + 1);
  bad += !plan::fits(0, 0, 1) || !plan::fits(3, 5, 8) || plan::fits(3, 6, 8) || plan::fits(9, 0, 8) || plan::fits(1, ~0ull, 8);
  bad += plan::joint_bound(1, 2, 3) != 6 || plan::joint_bound(~0ull, 1, 0) != ~0ull || plan::joint_bound(1, 2, ~0ull - 2) != ~0ull ||
         plan::joint_bound(0, 0, 0) != 0;
  bad += plan::dc_mask(1) != 1u || plan::dc_mask(3) != 7u || plan::dc_mask(31) != 0x7FFFFFFFu || plan::dc_mask(32) != 0xFFFFFFFFu;
  const uint64_t ns[] = {1, 2, 3, 4, 5, 64, 65, 1ull << 32, (1ull << 37) - 1, 1ull << 37, ~0ull};
  for (uint64_t n : ns) {
    const int b = plan::bits_for(n);
    bad += !(b >= 1 && b <= 64 && (b == 64 || (n - 1) >> b == 0) && (b == 1 || (n - 1) >> (b - 1) != 0));
  }
  // a stream's queue entries sort before its response rows, and both before the next stream's
  bad += !(plan::stream_key(5, false) < plan::stream_key(5, true) && plan::stream_key(5, true) < plan::stream_key(6, false));
  for (uint64_t s : {(uint64_t)1, (uint64_t)2, (uint64_t)2080, (uint64_t)1 << 37})
    bad += (plan::stream_key(s - 1, true) >> plan::stream_bits(s)) != 0 && plan::stream_bits(s) < 64;
  // the deliveries' key: the largest row and the sentinel partition fit the declared width
  for (uint32_t np : {1u, 2u, 65u, 1024u, ~0u})
    for (uint64_t nr : {(uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)1 << 20, ((uint64_t)1 << 31) - 1}) {
      const int rb = plan::row_bits(nr), db = plan::deliver_bits(np, nr);
      bad += !(db <= 64 && (nr >> rb) == 0);
      const uint64_t top = plan::deliver_key(np, 0, rb), in = plan::deliver_key((uint64_t)np - 1, nr, rb);
      bad += !(in < top && (db == 64 || (top >> db) == 0));
      bad += !(plan::deliver_key(0, 1, rb) < plan::deliver_key(0, 2, rb) && plan::deliver_key(0, nr, rb) < plan::deliver_key(1, 1, rb));
    }
  bad += plan::step_bound(3, 4) != 13 || plan::segment_bound(4) != 5 || plan::TILE != 64;
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)129, (uint64_t)1000})
    for (uint64_t nr : {(uint64_t)0, (uint64_t)1, (uint64_t)129}) {
      const plan::Layout L = plan::layout(n, nr, 777);
      const size_t offs[] = {L.k0, L.k1, L.dk1, L.v0, L.v1, L.dv1, L.trig, L.gfrom, L.gto, L.gflag, L.gpos, L.tmp, L.total};
      for (size_t i = 0; i + 1 < sizeof offs / sizeof *offs; ++i) {
        const size_t need_b = i < 3 ? n * 8 : i < 7 ? n * 4 : i < 9 ? nr * 8 : i < 11 ? nr * 4 : 777;
        bad += !(offs[i] % 256 == 0 && offs[i + 1] >= offs[i] + need_b);
      }
    }
  for (uint64_t cap : {(uint64_t)0, (uint64_t)1, (uint64_t)200})
    for (uint32_t nd : {1u, 3u, 32u}) {
      const plan::Columns K = plan::columns(cap, nd, 65);
      const size_t offs[] = {K.part, K.dc, K.ts, K.snap, K.ping, K.tag, K.off, K.total};
      const size_t need_b[] = {cap * 4, cap, cap * 8, cap * 8 * nd, cap, cap * 8, 66 * 8};
      for (size_t i = 0; i + 1 < sizeof offs / sizeof *offs; ++i) bad += !(offs[i] % 256 == 0 && offs[i + 1] >= offs[i] + need_b[i]);
    }
  printf("selfcheck %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  bool quiet = false;
  const char *columns = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--quiet")) quiet = true;
    else if (!strcmp(argv[i], "--selfcheck")) return selfcheck();
    else if (!strcmp(argv[i], "--columns") && i + 1 < argc) columns = argv[++i];
    else {
      fprintf(stderr, "usage: sub_cpu [--quiet] [--selfcheck] [--columns FILE] < history\n");
      return 2;
    }
  }
  std::vector<Cmd> cmds;
  char op[8];
  uint64_t n_dc = 0, n_part = 0;
  if (columns && !read_columns(columns, &cmds)) {
    fprintf(stderr, "sub_cpu: cannot read the columns of '%s'\n", columns);
    return 2;
  }
  while (!columns && scanf("%7s", op) == 1) {
    Cmd c;
    c.op = op[0];
    if (c.op == 'C') {
      c.a = need(), c.b = need(), c.c = need();
      if (c.a >> 32 || c.b >> 32 || !plan::create_ok((uint32_t)c.a, (uint32_t)c.b, 1)) {
        fprintf(stderr, "sub_cpu: bad C command\n");
        return 2;
      }
      n_dc = c.a, n_part = c.b;
    } else if (c.op == 'P') {
      const uint64_t nr = need();
      if (!n_dc || nr >> 31) {
        fprintf(stderr, "sub_cpu: P before C, or too many rows\n");
        return 2;
      }
      for (uint64_t t = 0; t < nr; ++t) {
        const uint64_t k = need(), p = need(), d = need(), pv = need(), la = need(), ts = need(), pg = need(), tag = need();
        // out-of-range values are kept (clamped to their columns' widths): the batch is then invalid
        c.kind.push_back((uint8_t)(k < 255 ? k : 255)), c.part.push_back((uint32_t)(p >> 32 ? ~0u : p));
        c.dc.push_back((uint8_t)(d < 255 ? d : 255));
        c.prev.push_back(pv), c.last.push_back(la), c.ts.push_back(ts), c.ping.push_back(pg != 0), c.tag.push_back(tag);
        for (uint64_t j = 0; j < n_dc; ++j) c.snap.push_back(need());
      }
    } else if (c.op == 'L') {
      c.a = need(), c.b = need(), c.c = need();
      if (!n_dc || c.a >= n_part || c.b >= n_dc) {
        fprintf(stderr, "sub_cpu: bad L command\n");
        return 2;
      }
    } else if (c.op == 'R') {
      c.a = need();
    } else if (c.op != 'X' && c.op != 'Z') {
      fprintf(stderr, "sub_cpu: unknown command '%s'\n", op);
      return 2;
    }
    cmds.push_back(std::move(c));
  }
  Sub sub;
  std::string out;
  char buf[64];
  uint64_t served = 0;
  auto put = [&](uint64_t v) {
    snprintf(buf, sizeof buf, " %" PRIu64, v);
    out += buf;
  };
  std::vector<std::vector<uint64_t>> got;
  std::vector<Gap> gaps;
  const auto t_begin = std::chrono::steady_clock::now();
  for (const Cmd &c : cmds) {
    switch (c.op) {
      case 'C':
        sub = Sub();
        sub.n_dc = (uint32_t)c.a, sub.n_part = (uint32_t)c.b, sub.logging = c.c != 0;
        sub.reach = plan::dc_mask(sub.n_dc);
        sub.streams.assign((size_t)c.a * c.b, Stream());
        got.assign(c.b, {});
        break;
      case 'P': {
        const size_t nr = c.kind.size();
        uint32_t bad = 0;
        for (size_t t = 0; t < nr; ++t) {  // the verdicts of k_sb_check
          if (c.kind[t] > plan::KIND_RESP_END) bad |= plan::BAD_KIND;
          if (c.part[t] >= sub.n_part) bad |= plan::BAD_PART;
          if (c.dc[t] >= sub.n_dc) bad |= plan::BAD_DC;
          if (c.kind[t] != plan::KIND_RESP_END && c.ts[t] == 0 && !c.ping[t]) bad |= plan::BAD_TIME;
        }
        if (bad) {
          if (!quiet) out += 'E', put(bad), out += '\n';
          break;
        }
        for (auto &g : got) g.clear();
        gaps.clear();
        const uint64_t d0 = sub.dropped, u0 = sub.unexpected;
        for (size_t t = 0; t < nr; ++t)
          sub.handle(c.kind[t], c.part[t], c.dc[t], c.prev[t], c.last[t], c.ping[t] != 0, c.tag[t], &got[c.part[t]], &gaps);
        served += nr;
        if (!quiet) {
          uint64_t n = 0;
          for (auto &g : got) n += g.size();
          out += 'D';
          put(n);
          for (size_t p = 0; p < got.size(); ++p)
            for (uint64_t tag : got[p]) put(p), put(tag);
          out += "\nG";
          put(gaps.size());
          for (const Gap &g : gaps) put(g.part), put(g.dc), put(g.from), put(g.to);
          out += "\nN";
          put(n), put(gaps.size()), put(sub.dropped - d0), put(sub.unexpected - u0), put(sub.queued);
          out += '\n';
        }
        break;
      }
      case 'L':
        sub.streams[(size_t)c.a * sub.n_dc + c.b].last = c.c;
        break;
      case 'R':
        sub.reach = (uint32_t)c.a & plan::dc_mask(sub.n_dc);
        break;
      case 'Z':
        sub.streams.assign(sub.streams.size(), Stream());
        sub.ar = Arena(), sub.queued = 0;
        break;
      case 'X':
        if (!quiet) {
          for (size_t i = 0; i < sub.streams.size(); ++i) {
            const Stream &s = sub.streams[i];
            if (s.last == 0 && s.mode == plan::MODE_NORMAL && s.q.empty()) continue;
            out += 'S';
            put(i / sub.n_dc), put(i % sub.n_dc), put(s.last), put(s.mode), put(s.q.size());
            for (uint32_t h : s.q) put(sub.ar.tag[h]);
            out += '\n';
          }
          out += "X\n";
        }
        break;
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  fputs(out.c_str(), stdout);
  printf("T %.3f %" PRIu64 "\n", ms, served);
  return 0;
}
