// cert_cpu.cpp -- the partition's certification, single-threaded over std::unordered_map: the CPU
// baseline of scripts/bench_cert.py and a second restatement of tests/certsim.py (a CPU test pins the
// two together).  It shares antidote_amd/csrc/am_cert_plan.h with the library, so a build of this
// program with -fsanitize=address,undefined covers the library's host arithmetic (table sizing, the
// compaction and capacity predicates, the scratch layout, the offset check): --selfcheck walks them.
//
//   g++ -O2 -std=c++17 -I antidote_amd/csrc scripts/cert_cpu.cpp -o cert_cpu
//   cert_cpu [--quiet] [--selfcheck] < history
//
// A history is whitespace-separated tokens, every number a decimal u64:
//   C record_commits                                  (first; a new certifier)
//   P n_tx  { txid start prepare certify n_keys key* }*    -> "P status*"
//   F n_tx  { txid commit_time committed n_keys key* }*    -> "F status*"
//   R n now { key start }*                                 -> "R wait_ms*"
//   M                                                      -> "M time" or "M none"
//   I key                                                  -> "I commit_time n { txid time }*" by (time, txid)
// The history is parsed first; the commands then run under a clock, and the last line is
// "T <milliseconds> <transactions prepared and finished>".  --quiet prints that line only.
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "am_cert_plan.h"

namespace plan = am_cert_plan;

enum { OK = 0, WRITE_CONFLICT = 7, NO_UPDATES = 8, SPIN_WAIT_MS = 10 };

struct Cmd {
  char op;
  uint64_t a = 0;                       // R: now; I: key; C: record_commits
  std::vector<uint64_t> txid, t0, t1;   // P: start, prepare; F: commit_time; R: key, start in txid, t0
  std::vector<uint8_t> flag;            // certify / committed
  std::vector<uint64_t> key_off, key;
};

struct Cert {
  bool record = true;
  std::unordered_map<uint64_t, uint64_t> committed;
  std::unordered_map<uint64_t, std::vector<std::pair<uint64_t, uint64_t>>> prepared;  // newest first

  int prepare(uint64_t txid, uint64_t start, uint64_t ptime, bool certify, const uint64_t *k, uint64_t n) {
    if (certify)
      for (uint64_t i = 0; i < n; ++i) {
        auto c = committed.find(k[i]);
        if (c != committed.end() && c->second > start) return WRITE_CONFLICT;
        auto p = prepared.find(k[i]);
        if (p != prepared.end() && !p->second.empty()) return WRITE_CONFLICT;
      }
    if (n == 0) return NO_UPDATES;
    for (uint64_t i = 0; i < n; ++i) {
      auto &lst = prepared[k[i]];
      bool mine = false;
      for (auto &e : lst) mine = mine || e.first == txid;
      if (!mine) lst.insert(lst.begin(), {txid, ptime});
    }
    return OK;
  }
  int finish(uint64_t txid, uint64_t ctime, bool was_committed, const uint64_t *k, uint64_t n) {
    if (n == 0) return NO_UPDATES;
    if (was_committed && record)
      for (uint64_t i = 0; i < n; ++i) committed[k[i]] = ctime;
    for (uint64_t i = 0; i < n; ++i) {
      auto p = prepared.find(k[i]);
      if (p == prepared.end()) continue;
      auto &lst = p->second;
      for (size_t j = 0; j < lst.size(); ++j)
        if (lst[j].first == txid) {
          lst.erase(lst.begin() + (long)j);
          break;
        }
      if (lst.empty()) prepared.erase(p);
    }
    return OK;
  }
  uint64_t read_ready(uint64_t key, uint64_t start, uint64_t now) const {
    if (start > now) return (start - now) / 1000 + 1;
    auto p = prepared.find(key);
    if (p != prepared.end())
      for (auto &e : p->second)
        if (e.second <= start) return SPIN_WAIT_MS;
    return 0;
  }
};

static bool next_u64(uint64_t *v) {
  char tok[64];
  if (scanf("%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = strtoull(tok, &end, 10);
  if (*end) {
    fprintf(stderr, "cert_cpu: bad number '%s'\n", tok);
    exit(2);
  }
  return true;
}
static uint64_t need() {
  uint64_t v = 0;
  if (!next_u64(&v)) {
    fprintf(stderr, "cert_cpu: truncated history\n");
    exit(2);
  }
  return v;
}

static int selfcheck() {
  int bad = 0;
  const uint64_t caps[] = {0, 1, 4, 7, 8, 9, 1023, 1024, 1025, (1ull << 40) - 1, 1ull << 40};
  for (uint64_t cap : caps) {
    const uint64_t s = plan::slots_for(cap), lim = plan::load_limit(s);
    bad += !(s >= 16 && (s & (s - 1)) == 0 && s >= 2 * cap && plan::cap_ok(cap));
    bad += !(lim < s && lim >= cap);
    // whatever a prepare finds, after its compaction decision the used slots stay below the table
    const uint64_t lives[] = {0, cap / 2, cap};
    for (uint64_t live : lives)
      for (uint64_t tomb : {(uint64_t)0, (uint64_t)1, lim > live ? lim - live : 0})
        for (uint64_t inc : {(uint64_t)0, (uint64_t)1, cap, s, (uint64_t)(~0ull >> 32)}) {
          uint64_t used = live + tomb;
          if (plan::must_compact(live, used, inc, s)) used = live;
          const uint64_t room = cap - live, adds = inc < room ? inc : room;  // the capacity verdict's bound
          const uint64_t worst = used > live ? used + inc : used + adds;    // tombstones kept: inc passed the limit test
          bad += !(worst < s);
        }
    bad += !plan::fits(cap, 0, cap) || plan::fits(cap, 1, cap) || plan::fits(0, cap + 1, cap) || plan::fits(1, ~0ull, cap);
  }
  bad += plan::cap_ok((1ull << 40) + 1) || plan::counts_ok(1ull << 32, 0) || plan::counts_ok(0, 1ull << 32) || !plan::counts_ok(~0u, ~0u);
  for (uint64_t nt : {(uint64_t)0, (uint64_t)1, (uint64_t)129})
    for (uint64_t np : {(uint64_t)0, (uint64_t)3, (uint64_t)1000}) {
      const plan::Layout L = plan::layout(nt, np, 777);
      const size_t offs[] = {L.k0, L.k1, L.k2, L.v0, L.v1, L.tx_of, L.head, L.run_of, L.first_ok, L.low0, L.low1, L.ins, L.st, L.ext, L.tmp, L.total};
      for (size_t i = 0; i + 1 < sizeof offs / sizeof *offs; ++i) {
        const size_t need_b = i < 3 ? np * 8 : i < 12 ? np * 4 : i < 14 ? nt * 4 : 777;
        bad += !(offs[i] % 256 == 0 && offs[i + 1] >= offs[i] + need_b);
      }
    }
  const uint64_t good[] = {0, 2, 2, 5}, dec[] = {0, 3, 2, 5}, first[] = {1, 2, 2, 5}, last[] = {0, 2, 2, 4};
  bad += !plan::offsets_ok(good, 3, 5) || plan::offsets_ok(dec, 3, 5) || plan::offsets_ok(first, 3, 5) || plan::offsets_ok(last, 3, 5);
  bad += !plan::offsets_ok(nullptr, 0, 0) || plan::offsets_ok(nullptr, 1, 0);
  printf("selfcheck %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  bool quiet = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--quiet")) quiet = true;
    else if (!strcmp(argv[i], "--selfcheck")) return selfcheck();
    else {
      fprintf(stderr, "usage: cert_cpu [--quiet] [--selfcheck] < history\n");
      return 2;
    }
  }
  std::vector<Cmd> cmds;
  char op[8];
  while (scanf("%7s", op) == 1) {
    Cmd c;
    c.op = op[0];
    if (c.op == 'C' || c.op == 'I') {
      c.a = need();
    } else if (c.op == 'P' || c.op == 'F') {
      const uint64_t nt = need();
      c.key_off.push_back(0);
      for (uint64_t t = 0; t < nt; ++t) {
        c.txid.push_back(need());
        c.t0.push_back(need());
        if (c.op == 'P') c.t1.push_back(need());
        c.flag.push_back(need() != 0);
        const uint64_t nk = need();
        for (uint64_t i = 0; i < nk; ++i) c.key.push_back(need());
        c.key_off.push_back(c.key.size());
      }
      if (!plan::counts_ok(nt, c.key.size()) || !plan::offsets_ok(c.key_off.data(), nt, c.key.size())) {
        fprintf(stderr, "cert_cpu: malformed batch\n");
        return 2;
      }
    } else if (c.op == 'R') {
      const uint64_t n = need();
      c.a = need();
      for (uint64_t i = 0; i < n; ++i) c.txid.push_back(need()), c.t0.push_back(need());
    } else if (c.op != 'M') {
      fprintf(stderr, "cert_cpu: unknown command '%s'\n", op);
      return 2;
    }
    cmds.push_back(std::move(c));
  }
  Cert cert;
  std::string out;
  char buf[64];
  uint64_t served = 0;
  auto put = [&](uint64_t v) {
    snprintf(buf, sizeof buf, " %" PRIu64, v);
    out += buf;
  };
  const auto t_begin = std::chrono::steady_clock::now();
  for (const Cmd &c : cmds) {
    switch (c.op) {
      case 'C':
        cert = Cert();
        cert.record = c.a != 0;
        break;
      case 'P':
      case 'F': {
        if (!quiet) out += c.op;
        const uint64_t *keys = c.key.data();
        for (size_t t = 0; t < c.txid.size(); ++t) {
          const uint64_t a = c.key_off[t], n = c.key_off[t + 1] - a;
          const int s = c.op == 'P' ? cert.prepare(c.txid[t], c.t0[t], c.t1[t], c.flag[t], keys + a, n)
                                    : cert.finish(c.txid[t], c.t0[t], c.flag[t], keys + a, n);
          if (!quiet) put((uint64_t)s);
        }
        served += c.txid.size();
        if (!quiet) out += '\n';
        break;
      }
      case 'R':
        if (!quiet) out += 'R';
        for (size_t i = 0; i < c.txid.size(); ++i) {
          const uint64_t w = cert.read_ready(c.txid[i], c.t0[i], c.a);
          if (!quiet) put(w);
        }
        if (!quiet) out += '\n';
        break;
      case 'M': {
        bool any = false;
        uint64_t m = ~0ull;
        for (auto &kv : cert.prepared)
          for (auto &e : kv.second) any = true, m = std::min(m, e.second);
        if (!quiet) {
          out += 'M';
          if (any) put(m);
          else out += " none";
          out += '\n';
        }
        break;
      }
      case 'I': {
        auto ci = cert.committed.find(c.a);
        std::vector<std::pair<uint64_t, uint64_t>> es;  // (time, txid)
        auto p = cert.prepared.find(c.a);
        if (p != cert.prepared.end())
          for (auto &e : p->second) es.push_back({e.second, e.first});
        std::sort(es.begin(), es.end());
        if (!quiet) {
          out += 'I';
          put(ci == cert.committed.end() ? 0 : ci->second);
          put(es.size());
          for (auto &e : es) put(e.second), put(e.first);
          out += '\n';
        }
        break;
      }
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  fputs(out.c_str(), stdout);
  printf("T %.3f %" PRIu64 "\n", ms, served);
  return 0;
}
