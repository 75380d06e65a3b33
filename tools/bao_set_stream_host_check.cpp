// bao_set_stream_host_check.cpp — the host side of set slices taken in windows (b3w_bao_set_slice_stream_cuts,
// b3w_bao_set_slice_stream_scratch_bytes; b3w_bao_plan.h: b3w_int_set_stream_cuts) run stand-alone over the set shapes and lengths of
// tests/test_bao_set_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include -I hot-proofs-blake3-circom_amd/csrc
//       hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp tools/bao_set_stream_host_check.cpp -o bao_set_stream_host_check
//       && ./bao_set_stream_host_check                                                            (one command line)
// Every buffer is a heap allocation of exactly the size the contract says (the run lists their runs, the cut list windows + 1 values),
// so a read or write past one is the sanitizer's to report.
//   - THE ROWS' CUTS of every shape are held against a walk of the slice in its own order (the encoder's recursion without the
//     hashing: offset and least wanted chunk of every element), and the last cut against b3w_bao_set_slice_size.
//   - THE GREEDY WINDOWS at the least window, twice that and more than the slice: cap exact, cap one too small (the count comes back
//     and the guard value behind the last slot the call may use stays), a null list; every cut but 0 at 8 modulo 16.
//   - THE SCRATCH: 1 552 bytes and 16 a row of the fullest window, against a count over the rows' cuts.
//   - One file of 2^30 chunks, whole and as every 1 024th chunk, and a file of 5 GiB + 300 bytes: places past 2^32.
// No device call is made and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "b3wit.h"
#include "b3w_bao_plan.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

typedef std::vector<std::pair<uint64_t, uint64_t>> Runs;
typedef unsigned long long ull;
static const uint64_t MIN = B3W_BAO_SET_SLICE_STREAM_MIN_WINDOW;

// the set shapes of the CPU test that fit a file of n chunks
static std::map<std::string, Runs> shapes_of(uint64_t n) {
  std::map<std::string, Runs> out;
  out["one run"] = {{n / 3, n / 4 ? n / 4 : 1}};
  out["the whole file"] = {{0, n}};
  const uint64_t pairs[3][2] = {{0, 2}, {63, 65}, {1023, 1025}};
  for (auto &p : pairs)
    if (p[1] < n) out["{" + std::to_string(p[0]) + ", " + std::to_string(p[1]) + "}"] = {{p[0], 1}, {p[1], 1}};
  if (n >= 2) {
    out["first and last chunk"] = {{0, 1}, {n - 1, 1}};
    Runs even, odd;
    for (uint64_t c = 0; c < n; c += 2) even.push_back({c, 1});
    for (uint64_t c = 1; c < n; c += 2) odd.push_back({c, 1});
    out["every second chunk"] = even;
    out["the odd chunks"] = odd;
  }
  if (n >= 4) {
    out["a run ending on the last chunk"] = {{0, 1}, {n - 2, 2}};
    out["touching runs"] = n < 8 ? Runs{{1, 1}, {2, 1}, {3, 1}} : Runs{{1, 2}, {3, 1}, {4, 3}, {n - 1, 1}};
  }
  if (n > 70) out["runs across the 64-chunk blocks"] = {{60, 3}, {63, 2}, {66, 1}, {n - 3, 2}};
  return out;
}

static uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }
static uint64_t left_len(uint64_t m) { uint64_t k = 1; while (2 * k < m) k *= 2; return k; }

// the walk: the slice's elements in order; a new row where the least wanted chunk enters another block
struct Walk {
  uint64_t len, B, at = 8, last = ~0ull;
  const Runs &runs;
  std::vector<uint64_t> cut;
  bool meets(uint64_t lo, uint64_t hi, uint64_t *c0) const {
    for (auto &r : runs)
      if (r.first + r.second > lo) { if (r.first >= hi) return false; *c0 = r.first > lo ? r.first : lo; return true; }
    return false;
  }
  void element(uint64_t c0, uint64_t bytes) {
    if (c0 / B != last) { last = c0 / B; cut.push_back(cut.empty() ? 0 : at); }
    at += bytes;
  }
  void go(uint64_t lo, uint64_t m) {
    uint64_t c0 = 0, x;
    if (!meets(lo, lo + m, &c0)) return;
    if (m == 1) { element(lo, ((lo + 1) * 1024 < len ? (lo + 1) * 1024 : len) - lo * 1024); return; }
    element(c0, 64);
    const uint64_t k = left_len(m);
    if (meets(lo, lo + k, &x)) go(lo, k);
    if (meets(lo + k, lo + m, &x)) go(lo + k, m - k);
  }
};

// exact-size heap copies of a run list
struct Lists {
  std::unique_ptr<uint64_t[]> first, count;
  uint32_t k;
  explicit Lists(const Runs &r) : first(new uint64_t[r.size()]), count(new uint64_t[r.size()]), k((uint32_t)r.size()) {
    for (size_t i = 0; i < r.size(); ++i) { first[i] = r[i].first; count[i] = r[i].second; }
  }
};

static std::vector<uint64_t> greedy(const std::vector<uint64_t> &cut, uint64_t window) {
  std::vector<uint64_t> out{cut[0]};
  for (size_t i = 0; i + 1 < cut.size();) {
    size_t j = i + 1;
    while (j + 1 < cut.size() && cut[j + 1] - cut[i] <= window) ++j;
    out.push_back(cut[j]);
    i = j;
  }
  return out;
}

static void check_set(uint64_t len, const Runs &runs, const std::vector<uint64_t> *want_rows, const char *what) {
  const Lists l(runs);
  std::vector<uint64_t> rows;
  bool shrt = false;
  std::string why;
  CHECK(b3w_int_set_stream_cuts(len, l.first.get(), l.count.get(), l.k, rows, &shrt, why), "%s (%llu): %s", what, (ull)len, why.c_str());
  const uint64_t size = b3w_bao_set_slice_size(len, l.first.get(), l.count.get(), l.k);
  CHECK(rows.front() == 0 && rows.back() == size, "%s (%llu): the ends", what, (ull)len);
  if (want_rows) {
    CHECK(rows == *want_rows, "%s (%llu): the rows' cuts differ from the walk (%zu against %zu)", what, (ull)len, rows.size(), want_rows->size());
    CHECK(shrt == ((runs.back().first + runs.back().second - 1) / 64 - runs.front().first / 64 <= 1), "%s: the rows' kind", what);
  }
  for (size_t r = 0; r + 1 < rows.size(); ++r) {
    CHECK(rows[r + 1] > rows[r] && rows[r + 1] - rows[r] <= MIN, "%s (%llu): row %zu is %llu bytes", what, (ull)len, r, (ull)(rows[r + 1] - rows[r]));
    CHECK(r == 0 || rows[r] % 16 == 8, "%s (%llu): cut %zu is not 8 modulo 16", what, (ull)len, r);
  }
  const uint64_t windows[3] = {MIN, 2 * MIN, size + MIN};
  for (uint64_t w : windows) {
    const std::vector<uint64_t> want = greedy(rows, w);
    const int64_t n = b3w_bao_set_slice_stream_cuts(len, l.first.get(), l.count.get(), l.k, w, nullptr, 0);
    CHECK(n == (int64_t)want.size() - 1, "%s (%llu), window %llu: %lld windows against %zu", what, (ull)len, (ull)w, (long long)n, want.size() - 1);
    std::unique_ptr<uint64_t[]> exact(new uint64_t[want.size()]);
    CHECK(b3w_bao_set_slice_stream_cuts(len, l.first.get(), l.count.get(), l.k, w, exact.get(), want.size()) == n, "%s: exact cap", what);
    for (size_t i = 0; i < want.size(); ++i) CHECK(exact[i] == want[i], "%s (%llu), window %llu: cut %zu", what, (ull)len, (ull)w, i);
    std::unique_ptr<uint64_t[]> small(new uint64_t[want.size() - 1]);                         // cap one too small: nothing is written
    for (size_t i = 0; i + 1 < want.size(); ++i) small[i] = 0xEEEEEEEEEEEEEEEEull;
    CHECK(b3w_bao_set_slice_stream_cuts(len, l.first.get(), l.count.get(), l.k, w, small.get(), want.size() - 1) == n, "%s: cap one too small", what);
    for (size_t i = 0; i + 1 < want.size(); ++i) CHECK(small[i] == 0xEEEEEEEEEEEEEEEEull, "%s: a list that is too short was written", what);
    uint64_t most = 0;
    for (size_t i = 0, j = 0; i + 1 < rows.size(); ++i) {
      if (j < i + 1) j = i + 1;
      while (j + 1 < rows.size() && rows[j + 1] - rows[i] <= w) ++j;
      if (j - i > most) most = j - i;
    }
    CHECK(b3w_bao_set_slice_stream_scratch_bytes(len, l.first.get(), l.count.get(), l.k, w) == B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES + 16 * most,
          "%s (%llu), window %llu: the scratch", what, (ull)len, (ull)w);
  }
  CHECK(b3w_bao_set_slice_stream_cuts(len, l.first.get(), l.count.get(), l.k, MIN - 1, nullptr, 0) < 0, "%s: a window below the least one", what);
  CHECK(b3w_bao_set_slice_stream_scratch_bytes(len, l.first.get(), l.count.get(), l.k, MIN - 1) == 0, "%s: the scratch of a refused window", what);
}

int main() {
  const uint64_t lengths[] = {0, 1, 1023, 1024, 1025, 2048, 2049, 3 * 1024 + 17, 5 * 1024 + 7, 17 * 1024 + 300, 40 * 1024, 63 * 1024, 64 * 1024, 65 * 1024,
                              70 * 1024 + 1, 1025 * 1024, 2049 * 1024, 3 * (1 << 20) + 5, 5 * (1 << 20) + 300};
  for (uint64_t len : lengths) {
    const uint64_t n = chunks_of(len);
    for (auto &sh : shapes_of(n)) {
      const Runs &runs = sh.second;
      Walk w{len, (runs.back().first + runs.back().second - 1) / 64 - runs.front().first / 64 <= 1 ? 64ull : 1024ull, 8, ~0ull, runs, {}};
      w.go(0, n);
      w.cut.push_back(w.at);
      check_set(len, runs, &w.cut, sh.first.c_str());
    }
  }
  // refused lists: unsorted, overlapping, empty run, past the file, no run, null lists
  {
    const uint64_t len = 5 * 1024 + 7;
    const Runs bad[] = {{{4, 1}, {1, 1}}, {{1, 2}, {2, 1}}, {{1, 0}}, {{5, 2}}, {{6, 1}}};
    for (auto &r : bad) {
      const Lists l(r);
      CHECK(b3w_bao_set_slice_stream_cuts(len, l.first.get(), l.count.get(), l.k, MIN, nullptr, 0) < 0, "a refused list");
      CHECK(b3w_bao_set_slice_stream_scratch_bytes(len, l.first.get(), l.count.get(), l.k, MIN) == 0, "a refused list's scratch");
    }
    const Lists good(Runs{{1, 2}, {4, 2}});
    CHECK(b3w_bao_set_slice_stream_cuts(len, good.first.get(), good.count.get(), 0, MIN, nullptr, 0) < 0, "no run");
    CHECK(b3w_bao_set_slice_stream_cuts(len, nullptr, good.count.get(), 2, MIN, nullptr, 0) < 0, "a null list");
    CHECK(b3w_bao_set_slice_stream_cuts(len, good.first.get(), nullptr, 2, MIN, nullptr, 0) < 0, "a null list");
    CHECK(b3w_bao_set_slice_stream_cuts((1ull << 40) + 1, good.first.get(), good.count.get(), 2, MIN, nullptr, 0) < 0, "more than 2^30 chunks");
  }
  // the largest file: 2^30 chunks whole (2^20 rows, places past 2^40), and every 1 024th chunk of it (a row a chunk, 30 nodes above most)
  {
    const uint64_t len = 1ull << 40, n = 1ull << 30;
    check_set(len, Runs{{0, n}}, nullptr, "2^30 chunks, whole");
    Runs sparse;
    for (uint64_t c = 5; c < n; c += 1024 * 1024) sparse.push_back({c, 1});
    Walk w{len, 1024, 8, ~0ull, sparse, {}};
    w.go(0, n);
    w.cut.push_back(w.at);
    check_set(len, sparse, &w.cut, "2^30 chunks, a chunk every 2^20");
    const uint64_t big = (5ull << 30) + 300, bn = chunks_of(big);
    const Runs far{{7, 1}, {(1ull << 22) - 1, 3}, {bn - 1, 1}};
    Walk v{big, 1024, 8, ~0ull, far, {}};
    v.go(0, bn);
    v.cut.push_back(v.at);
    CHECK(v.cut.size() == 5, "5 GiB + 300 B: four rows");
    check_set(big, far, &v.cut, "5 GiB + 300 B");
  }
  printf("bao_set_stream_host_check: %ld checks passed, no sanitizer report\n", checks);
  return 0;
}
