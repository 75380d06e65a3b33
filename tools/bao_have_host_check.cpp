// bao_have_host_check.cpp — the host mirrors of the arrival bitmap (b3w_bao_have_layout, b3w_bao_have_runs, b3w_bao_have_from_status) run
// stand-alone over the patterns of tests/test_bao_have_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_have_host_check.cpp -o bao_have_host_check && ./bao_have_host_check          (one command line)
// Every buffer is exactly as large as the contract says (the bitmap ceil(n / 64) words, the rows `capacity` entries, the statuses one byte
// a unit), so a read or write past one is the sanitizer's to report; the results are held against a bit-by-bit restatement.  No device
// call is made and no kernel compiled: the mirrors live in b3w_bao_host.cpp, plain C++ that names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <utility>
#include <vector>

#include "b3wit.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

// the definition read aloud: unit by unit over a vector of bools
static std::vector<std::pair<uint64_t, uint64_t>> ref_runs(const std::vector<bool> &bits, uint32_t g, uint32_t kind) {
  std::vector<std::pair<uint64_t, uint64_t>> rows;
  const uint64_t n = bits.size(), F = 1ull << g;
  bool open = false;
  uint64_t open_at = 0;
  for (uint64_t c = 0; c < n; c += F) {
    bool all = true;
    for (uint64_t k = c; k < n && k < c + F; ++k) all = all && bits[k];
    const bool sel = kind == B3W_BAO_HAVE_PRESENT ? all : !all;
    if (sel && !open) { open = true; open_at = c; }
    if (!sel && open) { rows.push_back({open_at, c - open_at}); open = false; }
  }
  if (open) rows.push_back({open_at, n - open_at});
  return rows;
}

static std::vector<uint64_t> pack(const std::vector<bool> &bits, bool pad) {
  std::vector<uint64_t> w((bits.size() + 63) / 64, pad ? ~0ull : 0ull);
  for (uint64_t c = 0; c < bits.size(); ++c) {
    if (bits[c]) w[c >> 6] |= 1ull << (c & 63);
    else w[c >> 6] &= ~(1ull << (c & 63));
  }
  return w;
}

static void check_file(uint64_t len, const std::vector<bool> &bits, bool pad) {
  const uint64_t n = bits.size();
  const std::vector<uint64_t> have = pack(bits, pad);
  uint64_t set = 0;
  for (bool b : bits) set += b;
  for (uint32_t g : {0u, 1u, 4u, 6u})
    for (uint32_t kind : {(uint32_t)B3W_BAO_HAVE_MISSING, (uint32_t)B3W_BAO_HAVE_PRESENT}) {
      const auto want = ref_runs(bits, g, kind);
      const uint64_t units = (n + (1ull << g) - 1) >> g;
      CHECK(want.size() <= (units + 1) / 2, "more than ceil(u / 2) runs");
      for (uint64_t cap : {(uint64_t)want.size(), (uint64_t)want.size() / 2, (uint64_t)0}) {
        std::vector<uint64_t> first(cap), count(cap);
        uint64_t n_runs = ~0ull, n_have = ~0ull;
        const int32_t rc = b3w_bao_have_runs(have.data(), len, g, kind, cap, cap ? first.data() : nullptr, cap ? count.data() : nullptr, &n_runs, &n_have);
        CHECK(rc == 0 && n_runs == want.size() && n_have == set, "len %llu g %u kind %u cap %llu: rc %d, %llu runs for %zu, %llu set for %llu",
              (unsigned long long)len, g, kind, (unsigned long long)cap, rc, (unsigned long long)n_runs, want.size(), (unsigned long long)n_have,
              (unsigned long long)set);
        for (uint64_t r = 0; r < cap; ++r)
          CHECK(first[r] == want[r].first && count[r] == want[r].second, "len %llu g %u kind %u row %llu", (unsigned long long)len, g, kind, (unsigned long long)r);
      }
    }
}

int main() {
  std::mt19937_64 rng(22);
  std::vector<uint64_t> lens = {0, 1, 1023, 1024, 1025, 17 * 1024 + 300, 33 * 1024 - 1, 128 * 1024 + 1};
  for (uint64_t k = 2; k <= 40; ++k) lens.push_back(k * 1024);
  for (uint64_t k : {63, 64, 65, 127, 128, 129}) lens.push_back(k * 1024);
  // the layout
  {
    std::vector<uint64_t> word_first(lens.size() + 1);
    uint64_t at = 0;
    const uint64_t total = b3w_bao_have_layout(lens.data(), (uint32_t)lens.size(), word_first.data());
    for (size_t f = 0; f < lens.size(); ++f) {
      CHECK(word_first[f] == at, "word_first[%zu]", f);
      at += ((lens[f] ? (lens[f] + 1023) / 1024 : 1) + 63) / 64;
    }
    CHECK(total == at && word_first[lens.size()] == at, "the total");
    CHECK(b3w_bao_have_layout(lens.data(), 1, nullptr) == 0, "a null table");
  }
  for (uint64_t len : lens) {
    const uint64_t n = len ? (len + 1023) / 1024 : 1;
    std::vector<std::pair<std::vector<bool>, bool>> patterns;
    auto add = [&](auto &&f, bool pad = false) {
      std::vector<bool> b(n);
      for (uint64_t c = 0; c < n; ++c) b[c] = f(c);
      patterns.push_back({b, pad});
    };
    add([](uint64_t) { return false; });
    add([](uint64_t) { return true; });
    add([](uint64_t c) { return c % 2 == 0; });
    add([](uint64_t c) { return c % 2 == 1; });
    for (uint32_t g : {1u, 4u, 6u}) {
      add([g](uint64_t c) { return (c >> g) % 2 == 0; });
      add([g](uint64_t c) { return (c >> g) % 2 == 1; });
    }
    for (uint64_t one : {(uint64_t)0, (uint64_t)63, (uint64_t)64, n - 1})
      if (one < n) {
        add([one](uint64_t c) { return c == one; });
        add([one](uint64_t c) { return c != one; });
      }
    add([](uint64_t c) { return c >= 60 && c < 70; });
    add([](uint64_t c) { return !(c >= 60 && c < 70); });
    const uint64_t tail = n < 10 ? n : 10;
    add([&](uint64_t c) { return c >= n - tail; });
    add([&](uint64_t c) { return c < n - tail; });
    add([](uint64_t) { return false; }, true);
    add([&](uint64_t) { return (rng() & 1) != 0; }, true);
    for (double density : {0.01, 0.5, 0.99}) add([&](uint64_t) { return (double)(rng() >> 11) / 9007199254740992.0 < density; });
    for (auto &p : patterns) check_file(len, p.first, p.second);
    // the bitmap from statuses: 0, 1, 2, 3 and 0xFF
    for (uint32_t g : {0u, 1u, 4u, 6u}) {
      const uint64_t units = (n + (1ull << g) - 1) >> g;
      std::vector<uint8_t> status(units);
      static const uint8_t codes[7] = {0, 0, 0, 1, 2, 3, 0xFF};
      for (auto &s : status) s = codes[rng() % 7];
      std::vector<uint64_t> have((n + 63) / 64, 0xEEEEEEEEEEEEEEEEull);
      CHECK(b3w_bao_have_from_status(status.data(), len, g, have.data()) == 0, "from_status");
      for (uint64_t c = 0; c < have.size() * 64; ++c)
        CHECK(((have[c >> 6] >> (c & 63)) & 1) == (uint64_t)(c < n && status[c >> g] == 0), "len %llu g %u chunk %llu", (unsigned long long)len, g,
              (unsigned long long)c);
    }
  }
  // refusals
  {
    uint64_t w = 0, first = 0, count = 0, n_runs = 0;
    uint8_t st = 0;
    CHECK(b3w_bao_have_runs(nullptr, 1, 0, 0, 1, &first, &count, &n_runs, nullptr) == B3W_E_BAD_ARGUMENT, "a null bitmap");
    CHECK(b3w_bao_have_runs(&w, 1, 7, 0, 1, &first, &count, &n_runs, nullptr) == B3W_E_BAD_ARGUMENT, "group_log 7");
    CHECK(b3w_bao_have_runs(&w, 1, 0, 2, 1, &first, &count, &n_runs, nullptr) == B3W_E_BAD_ARGUMENT, "kind 2");
    CHECK(b3w_bao_have_runs(&w, 1, 0, 0, 1, nullptr, &count, &n_runs, nullptr) == B3W_E_BAD_ARGUMENT, "null rows");
    CHECK(b3w_bao_have_runs(&w, 1, 0, 0, 1, &first, &count, nullptr, nullptr) == B3W_E_BAD_ARGUMENT, "a null count");
    CHECK(b3w_bao_have_from_status(nullptr, 1, 0, &w) == B3W_E_BAD_ARGUMENT && b3w_bao_have_from_status(&st, 1, 0, nullptr) == B3W_E_BAD_ARGUMENT &&
              b3w_bao_have_from_status(&st, 1, 7, &w) == B3W_E_BAD_ARGUMENT, "from_status refusals");
  }
  printf("bao_have_host_check: %ld checks passed\n", checks);
  return 0;
}
