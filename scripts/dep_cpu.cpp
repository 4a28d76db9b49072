// dep_cpu.cpp -- the dependency buffer, single-threaded: one FIFO per (partition, origin DC) and one
// clock per partition, served one arrival at a time.  It is the CPU baseline of scripts/bench_dep.py
// and a second restatement of tests/depsim.py (a CPU test pins the two together).  It shares
// antidote_amd/csrc/am_dep_plan.h with the library, so a build of this program with
// -fsanitize=address,undefined covers the library's host arithmetic: --selfcheck walks it.
//
//   g++ -O2 -std=c++17 -I antidote_amd/csrc scripts/dep_cpu.cpp -o dep_cpu
//   dep_cpu [--quiet] [--selfcheck] < history
//
// A history is whitespace-separated tokens, every number a decimal u64:
//   C n_dc own_dc n_part order*n_dc                         (a new buffer)
//   D now n_tx { part dc timestamp ping tag snap*n_dc }*    -> "D n { part tag }*" partition-major
//   S part pres vc*n_dc                                     set_dependency_clock
//   P on                                                    drop_ping
//   X                                                       -> "K part pres vc*n_dc" per partition,
//                                                              "Q part dc n tag*" per non-empty queue, "X"
// The history is parsed first; the commands then run under a clock, and the last line is
// "T <milliseconds> <arrivals served>".  --quiet prints that line only.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "am_dep_plan.h"

namespace plan = am_dep_plan;

struct Txn {
  uint64_t ts, tag;
  const uint64_t *snap;  // [n_dc], in the command's storage
  bool ping;
};

struct Part {
  std::vector<uint64_t> clock;
  uint32_t pres = 0;
  std::vector<std::deque<Txn>> q;
};

struct Dep {
  uint32_t n_dc = 1, own = 0;
  bool drop = false;
  std::vector<uint8_t> order;
  std::vector<Part> parts;

  void set(Part &P, uint32_t d, uint64_t v) { P.clock[d] = v, P.pres |= 1u << d; }
  bool try_store(Part &P, uint32_t d, const Txn &t, uint64_t now, std::vector<uint64_t> *out) {
    if (t.ping) {
      if (!drop) set(P, d, t.ts);
      return true;
    }
    for (uint32_t k = 0; k < n_dc; ++k) {
      if (k == d) continue;
      const uint64_t cur = k == own ? now : P.clock[k];  // an absent entry holds 0
      if (t.snap[k] > cur) {
        set(P, d, t.ts - 1);
        return false;
      }
    }
    out->push_back(t.tag);
    set(P, d, t.ts);
    return true;
  }
  void handle(uint32_t p, uint32_t d, const Txn &t, uint64_t now, std::vector<uint64_t> *out) {
    Part &P = parts[p];
    P.q[d].push_back(t);
    for (;;) {
      uint64_t stored = 0;
      for (uint8_t dq : order) {
        auto &q = P.q[dq];
        while (!q.empty() && try_store(P, dq, q.front(), now, out)) q.pop_front(), ++stored;
      }
      if (!stored) return;
    }
  }
};

struct Cmd {
  char op;
  uint64_t a = 0, b = 0, c = 0;    // C: n_dc own n_part; D: now; S: part pres; P: on
  std::vector<uint64_t> v;         // C: order; S: vc; D: snapshots
  std::vector<uint32_t> part, dc;  // D
  std::vector<uint64_t> ts, tag;
  std::vector<uint8_t> ping;
};

static bool next_u64(uint64_t *v) {
  char tok[64];
  if (scanf("%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = strtoull(tok, &end, 10);
  if (*end) {
    fprintf(stderr, "dep_cpu: bad number '%s'\n", tok);
    exit(2);
  }
  return true;
}
static uint64_t need() {
  uint64_t v = 0;
  if (!next_u64(&v)) {
    fprintf(stderr, "dep_cpu: truncated history\n");
    exit(2);
  }
  return v;
}

static int selfcheck() {
  int bad = 0;
  const uint8_t asc[] = {0, 1, 2, 3}, rev[] = {3, 2, 1, 0}, dup[] = {0, 1, 1, 3}, big[] = {0, 1, 2, 4};
  bad += !plan::order_ok(nullptr, 4) || !plan::order_ok(asc, 4) || !plan::order_ok(rev, 4) || plan::order_ok(dup, 4) ||
         plan::order_ok(big, 4);
  bad += !plan::create_ok(1, 0, 1, 1, nullptr) || !plan::create_ok(32, 31, ~0u, 1ull << 30, nullptr);
  bad += plan::create_ok(0, 0, 1, 1, nullptr) || plan::create_ok(33, 0, 1, 1, nullptr) || plan::create_ok(4, 4, 1, 1, nullptr) ||
         plan::create_ok(4, 0, 0, 1, nullptr) || plan::create_ok(4, 0, 1, 0, nullptr) || plan::create_ok(4, 0, 1, (1ull << 30) + 1, nullptr) ||
         plan::create_ok(4, 0, 1, 1, dup);
  uint8_t full[32];
  for (int i = 0; i < 32; ++i) full[i] = (uint8_t)(31 - i);
  bad += !plan::order_ok(full, 32);
  bad += !plan::count_ok(~0u) || plan::count_ok(1ull << 32);
  bad += !plan::fits(0, 0, 1) || !plan::fits(3, 5, 8) || plan::fits(3, 6, 8) || plan::fits(9, 0, 8) || plan::fits(1, ~0ull, 8);
  for (uint32_t n = 1; n <= 32; ++n) {
    const uint32_t g = 1u << plan::group_log2(n), per = plan::per_step(n);
    bad += !(g >= n && (n == 1 || g / 2 < n) && per * g == 64 && per >= 2);
  }
  const uint64_t ns[] = {1, 2, 3, 4, 5, 64, 65, 1ull << 32, (1ull << 37) - 1, 1ull << 37, ~0ull};
  for (uint64_t n : ns) {
    const int b = plan::bits_for(n);
    bad += !(b >= 1 && b <= 64 && (b == 64 || (n - 1) >> b == 0) && (b == 1 || (n - 1) >> (b - 1) != 0));
  }
  bad += plan::round_bound(3, 4) != 7;
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)129, (uint64_t)1000})
    for (uint64_t nt : {(uint64_t)0, (uint64_t)1, (uint64_t)129}) {
      const plan::Layout L = plan::layout(n, nt, 777);
      const size_t offs[] = {L.k0, L.k1, L.out, L.v0, L.v1, L.p0, L.p1, L.pv0, L.pv1, L.adc, L.tmp, L.total};
      for (size_t i = 0; i + 1 < sizeof offs / sizeof *offs; ++i) {
        const size_t need_b = i < 3 ? n * 8 : i < 5 ? n * 4 : i < 9 ? nt * 4 : i < 10 ? nt : 777;
        bad += !(offs[i] % 256 == 0 && offs[i + 1] >= offs[i] + need_b);
      }
    }
  printf("selfcheck %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  bool quiet = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--quiet")) quiet = true;
    else if (!strcmp(argv[i], "--selfcheck")) return selfcheck();
    else {
      fprintf(stderr, "usage: dep_cpu [--quiet] [--selfcheck] < history\n");
      return 2;
    }
  }
  std::vector<Cmd> cmds;
  char op[8];
  uint64_t n_dc = 0, n_part = 0;
  while (scanf("%7s", op) == 1) {
    Cmd c;
    c.op = op[0];
    if (c.op == 'C') {
      c.a = need(), c.b = need(), c.c = need();
      for (uint64_t i = 0; i < c.a && i < plan::MAX_DC; ++i) c.v.push_back(need());
      std::vector<uint8_t> o(c.v.begin(), c.v.end());
      bool ok = c.v.size() == c.a;
      for (uint64_t x : c.v) ok = ok && x < plan::MAX_DC;
      if (!ok || c.c >> 32 || !plan::create_ok((uint32_t)c.a, (uint32_t)c.b, (uint32_t)c.c, 1, o.data())) {
        fprintf(stderr, "dep_cpu: bad C command\n");
        return 2;
      }
      n_dc = c.a, n_part = c.c;
    } else if (c.op == 'D') {
      c.a = need();
      const uint64_t nt = need();
      if (!n_dc || !plan::count_ok(nt)) {
        fprintf(stderr, "dep_cpu: D before C, or too many arrivals\n");
        return 2;
      }
      for (uint64_t t = 0; t < nt; ++t) {
        const uint64_t p = need(), d = need(), ts = need(), pg = need(), tag = need();
        if (p >= n_part || d >= n_dc || (ts == 0 && !pg)) {
          fprintf(stderr, "dep_cpu: invalid arrival %" PRIu64 "\n", t);
          return 2;
        }
        c.part.push_back((uint32_t)p), c.dc.push_back((uint32_t)d), c.ts.push_back(ts), c.ping.push_back(pg != 0), c.tag.push_back(tag);
        for (uint64_t k = 0; k < n_dc; ++k) c.v.push_back(need());
      }
    } else if (c.op == 'S') {
      c.a = need(), c.b = need();
      if (!n_dc || c.a >= n_part || (n_dc < 32 && c.b >> n_dc) || c.b >> 32) {
        fprintf(stderr, "dep_cpu: bad S command\n");
        return 2;
      }
      for (uint64_t k = 0; k < n_dc; ++k) c.v.push_back(need());
    } else if (c.op == 'P') {
      c.a = need();
    } else if (c.op != 'X') {
      fprintf(stderr, "dep_cpu: unknown command '%s'\n", op);
      return 2;
    }
    cmds.push_back(std::move(c));
  }
  Dep dep;
  std::string out;
  char buf[64];
  uint64_t served = 0;
  auto put = [&](uint64_t v) {
    snprintf(buf, sizeof buf, " %" PRIu64, v);
    out += buf;
  };
  std::vector<std::vector<uint64_t>> got;
  const auto t_begin = std::chrono::steady_clock::now();
  for (const Cmd &c : cmds) {
    switch (c.op) {
      case 'C':
        dep = Dep();
        dep.n_dc = (uint32_t)c.a, dep.own = (uint32_t)c.b;
        dep.order.assign(c.v.begin(), c.v.end());
        dep.parts.assign(c.c, Part());
        for (Part &P : dep.parts) P.clock.assign(dep.n_dc, 0), P.q.resize(dep.n_dc);
        got.assign(c.c, {});
        break;
      case 'D': {
        for (auto &g : got) g.clear();
        for (size_t t = 0; t < c.ts.size(); ++t) {
          const Txn x{c.ts[t], c.tag[t], c.v.data() + t * dep.n_dc, c.ping[t] != 0};
          dep.handle(c.part[t], c.dc[t], x, c.a, &got[c.part[t]]);
        }
        served += c.ts.size();
        if (!quiet) {
          uint64_t n = 0;
          for (auto &g : got) n += g.size();
          out += 'D';
          put(n);
          for (size_t p = 0; p < got.size(); ++p)
            for (uint64_t tag : got[p]) put(p), put(tag);
          out += '\n';
        }
        break;
      }
      case 'S': {
        Part &P = dep.parts[c.a];
        P.pres = (uint32_t)c.b;
        for (uint32_t k = 0; k < dep.n_dc; ++k) P.clock[k] = ((c.b >> k) & 1) ? c.v[k] : 0;
        break;
      }
      case 'P':
        dep.drop = c.a != 0;
        break;
      case 'X':
        if (!quiet) {
          for (size_t p = 0; p < dep.parts.size(); ++p) {
            out += 'K';
            put(p), put(dep.parts[p].pres);
            for (uint64_t v : dep.parts[p].clock) put(v);
            out += '\n';
          }
          for (size_t p = 0; p < dep.parts.size(); ++p)
            for (uint32_t d = 0; d < dep.n_dc; ++d) {
              const auto &q = dep.parts[p].q[d];
              if (q.empty()) continue;
              out += 'Q';
              put(p), put(d), put(q.size());
              for (const Txn &t : q) put(t.tag);
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
