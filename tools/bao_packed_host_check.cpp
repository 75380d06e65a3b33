// bao_packed_host_check.cpp — the packed layout of the sparse bao calls (b3w_bao_packed_layout) run stand-alone over the lengths and the
// kinds of ranges of tests/test_bao_packed_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_packed_host_check.cpp -o bao_packed_host_check && ./bao_packed_host_check          (one command line)
// Every buffer is exactly as large as the contract says (host_lens up to the last listed file, the range arrays n_ranges entries), so a
// read or write past one is the sanitizer's to report; the results are held against a restatement that builds the set of listed
// (file, chunk) pairs chunk by chunk and ranks it.  No device call is made and no kernel compiled.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
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

struct Range { uint32_t file; uint64_t first, count; };
static uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }

// the chunks a range lists, one by one
static std::vector<uint64_t> listed_of(uint64_t len, uint32_t g, uint64_t a, uint64_t c) {
  std::vector<uint64_t> out;
  const uint64_t n = chunks_of(len);
  if (!c) return out;
  for (uint64_t ch = 0; ch < n; ++ch)
    if (n <= 64 || ((ch >> g) >= (a >> g) && (ch >> g) <= ((a + c - 1) >> g))) out.push_back(ch);
  return out;
}

static void check_call(const std::vector<uint64_t> &lens, uint32_t g, const std::vector<Range> &ranges) {
  std::set<std::pair<uint32_t, uint64_t>> listed;
  for (const Range &r : ranges)
    for (uint64_t ch : listed_of(lens[r.file], g, r.first, r.count)) listed.insert({r.file, ch});
  std::map<std::pair<uint32_t, uint64_t>, uint64_t> rank;
  uint64_t at = 0, want_bytes = 0;
  for (const auto &fc : listed) rank[fc] = at++;
  if (!listed.empty()) {
    const auto last = *listed.rbegin();
    const uint64_t left = lens[last.first] - 1024 * last.second;
    want_bytes = 1024 * (listed.size() - 1) + (left < 1024 ? left : 1024);
  }
  const size_t k = ranges.size();
  std::vector<uint32_t> files(k);
  std::vector<uint64_t> first(k), count(k);
  for (size_t i = 0; i < k; ++i) { files[i] = ranges[i].file; first[i] = ranges[i].first; count[i] = ranges[i].count; }
  for (int nulls = 0; nulls < 8; nulls += 7) {                         // every range output given, then none
    std::vector<uint64_t> slot(nulls ? 0 : k, ~0ull), lo(nulls ? 0 : k, ~0ull), cnt(nulls ? 0 : k, ~0ull);
    uint64_t slots = ~0ull, bytes = ~0ull;
    const int32_t rc = b3w_bao_packed_layout(lens.data(), (uint32_t)lens.size(), g, files.data(), first.data(), count.data(), (uint32_t)k,
                                             nulls ? nullptr : slot.data(), nulls ? nullptr : lo.data(), nulls ? nullptr : cnt.data(), &slots, &bytes);
    CHECK(rc == 0 && slots == listed.size() && bytes == want_bytes, "g %u, %zu ranges: rc %d, %llu slots for %zu, %llu bytes for %llu", g, k, rc,
          (unsigned long long)slots, listed.size(), (unsigned long long)bytes, (unsigned long long)want_bytes);
    if (nulls) continue;
    for (size_t i = 0; i < k; ++i) {
      const std::vector<uint64_t> mine = listed_of(lens[files[i]], g, first[i], count[i]);
      CHECK(cnt[i] == mine.size(), "g %u range %zu: %llu chunks for %zu", g, i, (unsigned long long)cnt[i], mine.size());
      if (mine.empty()) { CHECK(slot[i] == 0 && lo[i] == 0, "g %u range %zu: an empty range's slot and first chunk", g, i); continue; }
      CHECK(lo[i] == mine[0] && lo[i] <= first[i] && first[i] + count[i] <= lo[i] + cnt[i], "g %u range %zu: its first listed chunk", g, i);
      for (size_t j = 0; j < mine.size(); ++j) {
        const uint64_t want = rank[std::make_pair(files[i], mine[j])];
        CHECK(mine[j] == lo[i] + j && want == slot[i] + j, "g %u range %zu chunk %llu: its slot", g, i, (unsigned long long)mine[j]);
      }
    }
  }
}

// the kinds of tests/test_bao_packed_cpu.py that exist in a file of n chunks
static std::vector<std::vector<std::pair<uint64_t, uint64_t>>> kinds(uint64_t n, uint32_t g) {
  const uint64_t G = 1ull << g;
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> out;
  for (uint64_t c : {(uint64_t)0, n / 2, n - 1, std::min<uint64_t>(n - 1, 64), std::min<uint64_t>(n - 1, 1023), std::min<uint64_t>(n - 1, 1024)}) out.push_back({{c, 1}});
  out.push_back({{0, n}});
  out.push_back({{0, 0}});
  out.push_back({{n, 0}});
  const uint64_t b = G * std::max<uint64_t>(1, n / 2 / G);
  if (b + 1 <= n) out.push_back({{b - 1, 2}});
  if (b + G + 1 <= n) out.push_back({{b - 1, G + 2}});
  if (n > 1024) {
    out.push_back({{1022, std::min<uint64_t>(4, n - 1022)}});
    out.push_back({{1000 - G, std::min<uint64_t>(n - 1000 + G, 40 + 2 * G)}});
  }
  for (uint64_t t0 : {(uint64_t)0, (uint64_t)1024})
    if (n >= t0 + 5 * G + 4) out.push_back({{t0 + 1, 2}, {t0 + 3 * G + 1, std::min<uint64_t>(n - t0 - 3 * G - 1, G + 1)}});
  if (n >= 3) {
    out.push_back({{n - 2, 2}, {0, 2}, {1, n - 2}, {0, 2}, {n - 1, 1}, {n / 2, 0}, {0, 1}});
    out.push_back({{n / 2, 1}, {n / 2 - 1, 2}, {n / 2, 1}});
  }
  return out;
}

int main() {
  std::mt19937_64 rng(27);
  std::vector<uint64_t> lens = {0, 1, 1023, 1024, 1025, 17 * 1024 + 300, 33 * 1024 - 1};
  for (uint64_t k = 2; k <= 40; ++k) lens.push_back(k * 1024);
  for (uint64_t k : {63, 64, 65, 1025, 2049}) lens.push_back(k * 1024);
  CHECK(lens.size() == 51, "the 51 lengths");
  for (uint32_t g : {0u, 1u, 4u, 6u}) {
    // every kind on every length alone: host_lens is that one length
    for (uint64_t len : lens)
      for (const auto &kind : kinds(chunks_of(len), g)) {
        std::vector<Range> ranges;
        for (const auto &r : kind) ranges.push_back(Range{0, r.first, r.second});
        check_call({len}, g, ranges);
      }
    // all of them in one call, shuffled, a small file between every two large ones
    std::vector<uint64_t> world = {lens[3], lens[49], lens[0], lens[48], lens[1], lens[50]};
    for (size_t i = 0; i < lens.size(); ++i)
      if (i != 0 && i != 1 && i != 3 && i < 48) world.push_back(lens[i]);
    CHECK(world.size() == 51, "the world");
    std::vector<Range> every;
    for (uint32_t f = 0; f < world.size(); ++f)
      for (const auto &kind : kinds(chunks_of(world[f]), g))
        for (const auto &r : kind) every.push_back(Range{f, r.first, r.second});
    std::shuffle(every.begin(), every.end(), rng);
    check_call(world, g, every);
    // and without the whole-file ranges, so that the large files list runs with gaps
    std::vector<Range> some;
    for (const Range &r : every)
      if (!(r.first == 0 && r.count > 64) && r.count < 1000) some.push_back(r);
    check_call(world, g, some);
    // host_lens ends at the last listed file
    check_call({world[0], world[1]}, g, {Range{1, 70, 3}, Range{0, 0, 1}, Range{1, 1024, 1}});
  }
  // refusals: nothing is written
  {
    const uint64_t lens2[2] = {70 * 1024, 5 * 1024};
    uint32_t file = 0;
    uint64_t first = 0, count = 1, slot = 7, lo = 7, cnt = 7, slots = 7, bytes = 7;
    auto call = [&](uint32_t g = 0, uint32_t n_files = 2) {
      return b3w_bao_packed_layout(lens2, n_files, g, &file, &first, &count, 1, &slot, &lo, &cnt, &slots, &bytes);
    };
    CHECK(call() == 0 && slot == 0 && lo == 0 && cnt == 1 && slots == 1 && bytes == 1024, "one chunk");
    slot = lo = cnt = slots = bytes = 7;
    CHECK(call(7) == B3W_E_BAD_ARGUMENT, "group_log 7");
    file = 2; CHECK(call() == B3W_E_BAD_ARGUMENT, "a file index at the file count");
    file = 1; CHECK(call(0, 1) == B3W_E_BAD_ARGUMENT, "a file index past a smaller file count");
    file = 0;
    for (auto r : std::vector<std::pair<uint64_t, uint64_t>>{{70, 1}, {69, 2}, {0, 71}, {71, 0}, {1ull << 63, 1ull << 63}}) {
      first = r.first; count = r.second;
      CHECK(call() == B3W_E_BAD_ARGUMENT, "a range past the file's 70 chunks");
    }
    first = 0; count = 1;
    const uint64_t huge = (1ull << 40) + 1;
    CHECK(b3w_bao_packed_layout(&huge, 1, 0, &file, &first, &count, 1, &slot, &lo, &cnt, &slots, &bytes) == B3W_E_BAD_ARGUMENT, "more than 2^30 chunks");
    CHECK(b3w_bao_packed_layout(nullptr, 2, 0, &file, &first, &count, 1, &slot, &lo, &cnt, &slots, &bytes) == B3W_E_BAD_ARGUMENT, "null lengths");
    CHECK(b3w_bao_packed_layout(lens2, 2, 0, nullptr, &first, &count, 1, &slot, &lo, &cnt, &slots, &bytes) == B3W_E_BAD_ARGUMENT, "null files");
    CHECK(b3w_bao_packed_layout(lens2, 2, 0, &file, nullptr, &count, 1, &slot, &lo, &cnt, &slots, &bytes) == B3W_E_BAD_ARGUMENT, "null first chunks");
    CHECK(b3w_bao_packed_layout(lens2, 2, 0, &file, &first, nullptr, 1, &slot, &lo, &cnt, &slots, &bytes) == B3W_E_BAD_ARGUMENT, "null counts");
    CHECK(b3w_bao_packed_layout(lens2, 2, 0, &file, &first, &count, 1, &slot, &lo, &cnt, nullptr, &bytes) == B3W_E_BAD_ARGUMENT, "null total_slots");
    CHECK(b3w_bao_packed_layout(lens2, 2, 0, &file, &first, &count, 1, &slot, &lo, &cnt, &slots, nullptr) == B3W_E_BAD_ARGUMENT, "null total_bytes");
    CHECK(slot == 7 && lo == 7 && cnt == 7 && slots == 7 && bytes == 7, "a refused call writes nothing");
    CHECK(b3w_bao_packed_layout(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &slots, &bytes) == 0 && slots == 0 && bytes == 0, "no range");
  }
  printf("bao_packed_host_check: %ld checks passed over 51 files\n", checks);
  return 0;
}
