// bao_range_plan_host_check.cpp — the host call of the range planner (b3w_sample_rows_ranges) run stand-alone over the files and range
// kinds of tests/test_bao_range_plan_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_range_plan_host_check.cpp -o bao_range_plan_host_check && ./bao_range_plan_host_check          (one command line)
// Every buffer is exactly as large as the contract says (n_ranges + 1 range firsts, total chunks + 1 chunk firsts, total chunks
// flags), so a read or write past one is the sanitizer's to report.  The results are held against a restatement written out here chunk
// by chunk: a row a 64-byte block and one a path node; a path is provable where the index bits spell the tree's directions.  No device
// call is made and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "b3wit.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

static uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }
static uint64_t left_of(uint64_t m) { uint64_t k = 1; while (k * 2 < m) k *= 2; return k; }

// the restatement: a chunk's rows and whether its path is provable
static uint64_t rows_of(uint64_t len, uint64_t c, bool *provable) {
  const uint64_t bytes = len - c * 1024 < 1024 ? len - c * 1024 : 1024;
  std::vector<bool> lefts;
  for (uint64_t cc = c, m = chunks_of(len); m > 1;) {
    const uint64_t k = left_of(m);
    lefts.push_back(cc < k);
    if (cc < k) m = k; else { cc -= k; m -= k; }
  }
  *provable = true;
  for (size_t j = 0; j < lefts.size(); ++j)
    if (lefts[j] != (((c >> (lefts.size() - 1 - j)) & 1) == 0)) *provable = false;
  return (bytes ? (bytes + 63) / 64 : 1) + lefts.size();
}

// the range kinds of the CPU test: the whole file, the ends, both sides of and across the top three splits, the group and tile boundaries
static std::set<std::pair<uint64_t, uint64_t>> ranges_of(uint64_t n) {
  std::set<std::pair<uint64_t, uint64_t>> out = {{0, n}, {n - 1, 1}};
  if (n >= 2) out.insert({n - 2, 2});
  struct Walk {
    std::set<std::pair<uint64_t, uint64_t>> &out;
    void go(uint64_t lo, uint64_t m, int depth) {
      if (m < 2 || !depth) return;
      const uint64_t k = left_of(m);
      out.insert({lo, k}); out.insert({lo + k, m - k}); out.insert({lo + k - 1, 2});
      go(lo, k, depth - 1); go(lo + k, m - k, depth - 1);
    }
  } w{out};
  w.go(0, n, 3);
  for (uint32_t g : {1u, 4u, 6u}) {
    const uint64_t G = 1ull << g;
    for (uint64_t gs : {(uint64_t)0, ((n - 1) / G) * G}) {
      const uint64_t in_group = (n - gs < G ? n - gs : G);
      if (in_group >= 3) out.insert({gs + 1, in_group - 2});
      if (gs + G + 1 <= n) { out.insert({gs, G + 1}); out.insert({gs + G - 1, 2}); }
    }
  }
  if (n > 1024) { out.insert({1022, n - 1022 < 4 ? n - 1022 : 4}); out.insert({1023, n - 1023 < 1026 ? n - 1023 : 1026}); }
  if (n <= 70) for (uint64_t c = 0; c < n; ++c) out.insert({c, 1});
  return out;
}

static void check_file(uint64_t len, std::mt19937_64 &rng) {
  const uint64_t n = chunks_of(len);
  const uint64_t lens[2] = {3 * 1024 + 1, len};            // the file is not the batch's first
  std::vector<uint64_t> first, count;
  for (const auto &r : ranges_of(n)) { first.push_back(r.first); count.push_back(r.second); }
  for (size_t i = first.size(); i > 1; --i) {              // any order, and one range twice
    const size_t j = rng() % i;
    std::swap(first[i - 1], first[j]); std::swap(count[i - 1], count[j]);
  }
  first.push_back(first[0]); count.push_back(count[0]);
  const uint32_t k = (uint32_t)first.size();
  const std::vector<uint32_t> files(k, 1);
  uint64_t total = 0;
  for (uint64_t x : count) total += x;
  std::vector<uint64_t> rrf(k + 1, 0xEEEEEEEEull), crf(total + 1, 0xEEEEEEEEull), rrf2(k + 1, 0xEEEEEEEEull);
  std::vector<uint8_t> prov(total, 0xEE);
  const int64_t rows = b3w_sample_rows_ranges(lens, 2, files.data(), first.data(), count.data(), k, rrf.data(), crf.data(), prov.data());
  CHECK(rows >= 0, "refused a good list of %u ranges of a file of %llu bytes", k, (unsigned long long)len);
  uint64_t row = 0, at = 0;
  for (uint32_t i = 0; i < k; ++i) {
    CHECK(rrf[i] == row, "range %u of %llu starts at %llu, not %llu", i, (unsigned long long)len, (unsigned long long)rrf[i], (unsigned long long)row);
    for (uint64_t c = first[i]; c < first[i] + count[i]; ++c, ++at) {
      bool p = false;
      const uint64_t r = rows_of(len, c, &p);
      CHECK(crf[at] == row, "chunk %llu of range %u of %llu starts at %llu, not %llu", (unsigned long long)c, i, (unsigned long long)len, (unsigned long long)crf[at],
            (unsigned long long)row);
      CHECK(prov[at] == (p ? 1 : 0), "provable of chunk %llu of %llu chunks", (unsigned long long)c, (unsigned long long)n);
      row += r;
    }
  }
  CHECK(rrf[k] == row && crf[total] == row && (uint64_t)rows == row, "the total of %llu", (unsigned long long)len);
  // the per-range totals alone: no per-chunk array is touched (there is none)
  CHECK(b3w_sample_rows_ranges(lens, 2, files.data(), first.data(), count.data(), k, rrf2.data(), nullptr, nullptr) == rows && rrf2 == rrf, "the closed form alone");
}

static void check_refusals() {
  const uint64_t lens[3] = {5 * 1024 + 7, 0, 70 * 1024};
  const int64_t BAD = -(int64_t)B3W_E_BAD_ARGUMENT;
  const struct { uint32_t f; uint64_t a, k; } bad[] = {{3, 0, 1}, {0, 0, 0}, {0, 5, 2}, {0, 6, 1}, {1, 1, 1}, {1, 0, 2}, {2, 2, ~0ull}};
  for (const auto &b : bad) {
    const uint32_t files[2] = {2, b.f};
    const uint64_t first[2] = {0, b.a}, count[2] = {70, b.k};
    std::vector<uint64_t> rrf(3, 77), crf(71, 77);          // (sized for the good range alone: a refusal writes nothing)
    std::vector<uint8_t> prov(70, 77);
    CHECK(b3w_sample_rows_ranges(lens, 3, files, first, count, 2, rrf.data(), crf.data(), prov.data()) == BAD, "(%u, %llu, %llu) was taken", b.f,
          (unsigned long long)b.a, (unsigned long long)b.k);
    for (uint64_t x : rrf) CHECK(x == 77, "range firsts touched");
    for (uint64_t x : crf) CHECK(x == 77, "chunk firsts touched");
    for (uint8_t x : prov) CHECK(x == 77, "flags touched");
  }
  const uint32_t files[1] = {0};
  const uint64_t first[1] = {0}, count[1] = {1};
  uint64_t rrf[2] = {77, 77};
  CHECK(b3w_sample_rows_ranges(lens, 3, files, first, count, 1, nullptr, nullptr, nullptr) == BAD, "null range firsts");
  CHECK(b3w_sample_rows_ranges(nullptr, 3, files, first, count, 1, rrf, nullptr, nullptr) == BAD, "null lengths");
  CHECK(b3w_sample_rows_ranges(lens, 3, nullptr, first, count, 1, rrf, nullptr, nullptr) == BAD, "null files");
  CHECK(b3w_sample_rows_ranges(lens, 3, files, nullptr, count, 1, rrf, nullptr, nullptr) == BAD, "null firsts");
  CHECK(b3w_sample_rows_ranges(lens, 3, files, first, nullptr, 1, rrf, nullptr, nullptr) == BAD && rrf[0] == 77 && rrf[1] == 77, "null counts");
  CHECK(b3w_sample_rows_ranges(nullptr, 0, nullptr, nullptr, nullptr, 0, rrf, nullptr, nullptr) == 0 && rrf[0] == 0 && rrf[1] == 77, "no range");
  CHECK(b3w_sample_rows_ranges(lens, 3, files, first, count, 1, rrf, nullptr, nullptr) == 19 && rrf[0] == 0 && rrf[1] == 19, "one chunk of six");
  // a whole 1 GiB file and the ragged end of one past 4 GiB: counted in 64 bits and without a walk over the chunks
  const uint64_t big[2] = {1ull << 30, (5ull << 30) + 300};
  const uint32_t bf[2] = {0, 1};
  const uint64_t ba[2] = {0, 5 * (1ull << 20) - 1}, bk[2] = {1ull << 20, 2};
  uint64_t br[3];
  bool p = false;
  const uint64_t tail = rows_of(big[1], ba[1], &p) + rows_of(big[1], ba[1] + 1, &p);
  CHECK(b3w_sample_rows_ranges(big, 2, bf, ba, bk, 2, br, nullptr, nullptr) == (int64_t)(37748736 + tail) && br[1] == 37748736, "the whole 1 GiB file");
}

int main() {
  std::mt19937_64 rng(25);
  std::vector<uint64_t> lens = {0, 1, 1023, 1024, 1025, 17 * 1024 + 300, 33 * 1024 - 1};
  for (uint64_t n = 2; n <= 40; ++n) lens.push_back(n * 1024);
  for (uint64_t n : {63, 64, 65, 1025, 2049}) lens.push_back(n * 1024);
  for (uint64_t len : lens) check_file(len, rng);
  check_refusals();
  printf("bao_range_plan_host_check: %ld checks passed over %zu files\n", checks, lens.size());
  return 0;
}
