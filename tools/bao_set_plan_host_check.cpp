// bao_set_plan_host_check.cpp — the host arithmetic beside the set table (b3w_bao_plan.h: b3w_int_range_row_first, b3w_int_set_row_base for
// b3w_sample_plan_set_slices_device; b3w_int_set_row_slot for b3w_bao_set_slice_packed_device) run stand-alone over the set shapes and
// the 51 lengths of tests/test_bao_set_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include -I hot-proofs-blake3-circom_amd/csrc
//       hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp tools/bao_set_plan_host_check.cpp -o bao_set_plan_host_check
//       && ./bao_set_plan_host_check                                                              (one command line)
// Every buffer is exactly as large as the contract says (the run lists their runs, range_row_first the ranges + 1, chunk_row_first the
// chunks + 1, the layout's arrays the ranges or sets + 1), so a read or write past one is the sanitizer's to report.
//   - THE ROW BASE of every row of every set (the set table's rows: a block of 64 or 1 024 chunks with a wanted chunk) is held against
//     b3w_sample_rows_ranges' chunk_row_first at the rank of the block's first wanted chunk, one file a call and several files a call.
//   - THE PACKED SLOT of every row is held against b3w_bao_packed_layout at group_log 0, 4 and 6: the slot of the block's first LISTED
//     chunk, and every wanted chunk of the block at slot + its rank among the block's listed chunks.
//   - One file of 2^30 chunks, planned whole and as every second chunk of its first tile: the total rows pass 2^32, the bases are held
//     against the closed form 16 c + 30 c (every chunk has sixteen blocks and, the tree being whole, thirty path nodes).
// No device call is made and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <map>
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

// the set shapes of the CPU test that fit a file of n chunks
static std::map<std::string, Runs> shapes_of(uint64_t n) {
  std::map<std::string, Runs> out;
  out["one run"] = {{n / 3, n / 4 ? n / 4 : 1}};
  out["the whole file"] = {{0, n}};
  for (auto p : {std::pair<uint64_t, uint64_t>{0, 2}, {63, 65}, {1023, 1025}})
    if (p.second < n) out["{" + std::to_string(p.first) + ", " + std::to_string(p.second) + "}"] = {{p.first, 1}, {p.second, 1}};
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

// one call over these files' sets (a set a file, files ascending): every row of the set table against the two public host calls
static void check_call(const std::vector<uint64_t> &lens, const std::vector<Runs> &sets, const char *name) {
  const uint32_t n_files = (uint32_t)lens.size();
  std::vector<uint32_t> files;
  std::vector<uint64_t> first, count;
  for (uint32_t f = 0; f < n_files; ++f)
    for (const auto &r : sets[f]) { files.push_back(f); first.push_back(r.first); count.push_back(r.second); }
  const uint32_t k = (uint32_t)files.size();
  if (!k) return;
  SetList list;
  CHECK(b3w_int_set_list(lens.data(), n_files, files.data(), first.data(), count.data(), k, list), "%s: %s", name, list.why.c_str());
  // the facts the planner's layout rests on, through the public calls
  std::vector<uint64_t> rrf((size_t)k + 1), crf(list.chunks + 1);
  const int64_t total = b3w_sample_rows_ranges(lens.data(), n_files, files.data(), first.data(), count.data(), k, rrf.data(), crf.data(), nullptr);
  CHECK(total >= 0 && (uint64_t)total == crf[list.chunks] && rrf[k] == (uint64_t)total, "%s: rows", name);
  const std::vector<uint64_t> run_row = b3w_int_range_row_first(lens.data(), files.data(), first.data(), count.data(), k);
  CHECK(run_row.size() == (size_t)k + 1, "%s: run_row's size", name);
  for (uint32_t i = 0; i <= k; ++i) CHECK(run_row[i] == rrf[i], "%s: the first row of range %u", name, i);
  uint64_t sum = 0;
  for (const SetEnt &e : list.sets) {
    CHECK(e.chunk_first == sum, "%s: set_chunk_first is the running sum of the counts", name);
    for (uint32_t i = e.range_first; i < e.range_end; ++i) sum += count[i];
  }
  for (uint32_t gl : {0u, 4u, 6u}) {
    std::vector<uint64_t> slot(k), pfirst(k), pcount(k);
    uint64_t slots = 0, bytes = 0;
    CHECK(b3w_bao_packed_layout(lens.data(), n_files, gl, files.data(), first.data(), count.data(), k, slot.data(), pfirst.data(), pcount.data(), &slots, &bytes) == B3W_OK,
          "%s: packed layout at g %u", name, gl);
    const PkLayout pk = b3w_int_packed_layout(lens.data(), b3w_int_update_ranges(lens.data(), files.data(), first.data(), count.data(), k), gl);
    CHECK(pk.slots == slots && pk.bytes == bytes, "%s: the two layouts at g %u", name, gl);
    uint64_t rows = 0;
    for (const SetEnt &e : list.sets) {
      const uint64_t len = lens[e.file], n = len ? (len + 1023) / 1024 : 1, kk = e.range_end - e.range_first, B = e.shrt ? 64 : 1024, G = 1ull << gl;
      const uint64_t *fs = first.data() + e.range_first, *cs = count.data() + e.range_first;
      uint64_t last = ~0ull, rank = 0;                     // rank: the set's wanted chunks in front of run i
      for (uint64_t i = 0; i < kk; rank += cs[i], ++i)
        for (uint64_t blk = fs[i] / B; blk <= (fs[i] + cs[i] - 1) / B; ++blk) {
          if (blk == last) continue;
          last = blk;
          ++rows;
          const uint64_t a0 = blk * B, cf = fs[i] > a0 ? fs[i] : a0;      // (the first run that reaches the block is the one that made the row)
          if (gl == 0) {
            const uint64_t base = b3w_int_set_row_base(len, fs, cs, kk, run_row.data() + e.range_first, a0);
            CHECK(base == crf[e.chunk_first + rank + (cf - fs[i])], "%s: file %u block %llu: base %llu", name, e.file, (ull)blk, (ull)base);
          }
          // the packed slot: the block's first listed chunk, and every wanted chunk of the block at its rank among the listed ones
          const uint64_t got = b3w_int_set_row_slot(pk, e.file, len, gl, fs, cs, kk, a0);
          const uint64_t listed0 = n <= 64 ? 0 : cf & ~(G - 1);
          const uint32_t at = e.range_first + (uint32_t)i;                 // the public layout: range i lists [pfirst, + pcount) from slot[] on
          CHECK(listed0 >= pfirst[at] && listed0 < pfirst[at] + pcount[at] && got == slot[at] + (listed0 - pfirst[at]), "%s: file %u block %llu at g %u: slot %llu", name,
                e.file, (ull)blk, gl, (ull)got);
          uint64_t listed = 0, prev_group = ~0ull;           // walk the block's wanted chunks: listed = the listed chunks in front of the group
          for (uint64_t j = i; j < kk && fs[j] < a0 + B; ++j)
            for (uint64_t c = fs[j] > a0 ? fs[j] : a0; c < fs[j] + cs[j] && c < a0 + B; ++c) {
              uint64_t want;
              if (n <= 64) want = got + c;
              else {
                const uint64_t grp = c / G;
                if (grp != prev_group) { if (prev_group != ~0ull) listed += G; prev_group = grp; }
                want = got + listed + (c & (G - 1));
              }
              CHECK(pk.slot_of(e.file, c) == want, "%s: file %u chunk %llu at g %u", name, e.file, (ull)c, gl);
            }
        }
    }
    CHECK(rows == list.big + list.small, "%s: the rows add up", name);
  }
}

int main() {
  const uint64_t K = 1024;
  std::vector<uint64_t> lens = {0, 1, 1023, 1024, 1025};
  for (uint64_t c = 2; c <= 40; ++c) lens.push_back(c * K);
  for (uint64_t l : {17708ull, 33791ull, 64512ull, 65536ull, 66560ull, 1049600ull, 2098176ull}) lens.push_back(l);
  CHECK(lens.size() == 51, "the CPU test's 51 lengths");
  // a file a call, every shape
  std::map<std::string, std::vector<Runs>> together;
  for (size_t f = 0; f < lens.size(); ++f) {
    const uint64_t n = lens[f] ? (lens[f] + 1023) / 1024 : 1;
    for (const auto &shape : shapes_of(n)) {
      check_call({lens[f]}, {shape.second}, shape.first.c_str());
      auto &all = together[shape.first];
      all.resize(lens.size());
      all[f] = shape.second;
    }
  }
  // and every file that fits a shape in one call (files without it have no set)
  for (const auto &shape : together) check_call(lens, shape.second, shape.first.c_str());
  // one file of 2^30 chunks: whole, and every second chunk of its first tile
  {
    const uint64_t n = 1ull << 30, len = n * K;
    const uint32_t file = 0;
    const uint64_t a = 0;
    uint64_t rrf[2];
    CHECK(b3w_sample_rows_ranges(&len, 1, &file, &a, &n, 1, rrf, nullptr, nullptr) == (int64_t)(46 * n) && rrf[1] == 46 * n && rrf[1] > (1ull << 32), "2^30 chunks: rows");
    const std::vector<uint64_t> run_row = b3w_int_range_row_first(&len, &file, &a, &n, 1);
    CHECK(run_row[0] == 0 && run_row[1] == 46 * n, "2^30 chunks: run_row");
    for (uint64_t blk : {0ull, 1ull, 1ull << 19, (1ull << 19) + 1, (1ull << 20) - 1}) {
      const uint64_t base = b3w_int_set_row_base(len, &a, &n, 1, run_row.data(), blk * 1024);
      CHECK(base == 46 * 1024 * blk && (blk < (1ull << 19) || base * 128 > (1ull << 32)), "2^30 chunks: tile %llu starts at row %llu", (ull)blk, (ull)base);
    }
    std::vector<uint32_t> files(512, 0);
    std::vector<uint64_t> first(512), count(512, 1), rr(513);
    for (uint64_t i = 0; i < 512; ++i) first[i] = 2 * i;
    SetList list;
    CHECK(b3w_int_set_list(&len, 1, files.data(), first.data(), count.data(), 512, list) && list.big == 1 && list.small == 0 && list.chunks == 512, "2^30 chunks: the set");
    CHECK(b3w_sample_rows_ranges(&len, 1, files.data(), first.data(), count.data(), 512, rr.data(), nullptr, nullptr) == 46 * 512, "2^30 chunks: every second chunk");
    const std::vector<uint64_t> r2 = b3w_int_range_row_first(&len, files.data(), first.data(), count.data(), 512);
    for (uint64_t i = 0; i <= 512; ++i) CHECK(r2[i] == 46 * i && r2[i] == rr[i], "2^30 chunks: run %llu", (ull)i);
    CHECK(b3w_int_set_row_base(len, first.data(), count.data(), 512, r2.data(), 0) == 0, "2^30 chunks: the tile's base");
    const PkLayout pk = b3w_int_packed_layout(&len, b3w_int_update_ranges(&len, files.data(), first.data(), count.data(), 512), 4);
    CHECK(pk.slots == 1024 && b3w_int_set_row_slot(pk, 0, len, 4, first.data(), count.data(), 512, 0) == 0, "2^30 chunks: the packed tile");
  }
  printf("bao_set_plan_host_check: %ld checks passed, no sanitizer report\n", checks);
  return 0;
}
