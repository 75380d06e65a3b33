// bao_set_host_check.cpp — the host calls of the set slices (b3w_bao_set_slice_size, _batch_layout, b3w_bao_set_slice, _decode, _ingest,
// b3w_bao_set_slice_ingest_scratch_bytes) run stand-alone over the set shapes of tests/test_bao_set_cpu.py, for a sanitizer build of host
// code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_set_host_check.cpp -o bao_set_host_check && ./bao_set_host_check          (one command line)
// Every buffer is exactly as large as the contract says (the run lists their runs, the slice its size, the file its bytes, the decoder's
// output 1024 |S| less what the short last chunk lacks, the chunk statuses |S|, the bitmap ceil(n / 64) words, the layout's arrays the
// sets + 1), so a read or write past one is the sanitizer's to report.  The results are held against each other and against the range
// calls: the slice from the full outboard equals the one from every group outboard, one run gives b3w_bao_range_slice's bytes, the size
// never exceeds the sum of the runs' range slices, what is decoded is the file's wanted chunks, every set taken in leaves those chunks
// and, once every chunk has come, the provider's outboard; a flipped byte is reported and keeps its chunk out.  No device call is made
// and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "b3wit.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

typedef std::vector<std::pair<uint64_t, uint64_t>> Runs;
static uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }

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

static void check_file(uint64_t len, std::mt19937_64 &rng) {
  const uint64_t n = chunks_of(len);
  std::vector<uint8_t> data(len);
  for (auto &b : data) b = (uint8_t)rng();
  const uint64_t whole_first = 0;
  uint32_t root[8];
  std::vector<std::vector<uint8_t>> obs;
  const uint32_t gs[4] = {0, 1, 4, 6};
  for (uint32_t g : gs) {                                  // the provider's outboards: every chunk dirty
    std::vector<uint8_t> ob(b3w_bao_group_outboard_size(len, g), 0xEE);
    for (int k = 0; k < 8; ++k) ob[k] = (uint8_t)(len >> (8 * k));
    uint32_t r[8];
    CHECK(b3w_bao_outboard_update(data.data(), len, ob.data(), g, &whole_first, &n, 1, r) == B3W_OK, "outboard of %llu at g %u", (unsigned long long)len, g);
    if (g == 0) memcpy(root, r, 32);
    CHECK(memcmp(root, r, 32) == 0, "roots differ");
    obs.push_back(ob);
  }
  for (const auto &shape : shapes_of(n)) {
    const char *name = shape.first.c_str();
    const uint32_t k = (uint32_t)shape.second.size();
    std::vector<uint64_t> first(k), count(k), wanted;      // (exact: k entries each)
    uint64_t apart = 0, payload = 0;
    for (uint32_t i = 0; i < k; ++i) {
      first[i] = shape.second[i].first; count[i] = shape.second[i].second;
      apart += b3w_bao_range_slice_size(len, first[i], count[i]);
      for (uint64_t c = first[i]; c < first[i] + count[i]; ++c) { wanted.push_back(c); payload += len - c * 1024 < 1024 ? len - c * 1024 : 1024; }
    }
    const uint64_t size = b3w_bao_set_slice_size(len, first.data(), count.data(), k);
    CHECK(size >= 8 + payload && size <= apart && (size < apart || k == 1 || n == 1), "%llu %s: size %llu, apart %llu", (unsigned long long)len, name,
          (unsigned long long)size, (unsigned long long)apart);
    // the layout of this one set: arrays of n_sets + 1 = 2 entries (set_file: 1)
    const uint32_t zero = 0;
    std::vector<uint32_t> files(k, 0), set_file(1), set_range_first(2);
    std::vector<uint64_t> set_chunk_first(2), slice_first(2);
    uint32_t n_sets = 77;
    CHECK(b3w_bao_set_slice_batch_layout(&len, 1, files.data(), first.data(), count.data(), k, set_file.data(), set_range_first.data(), set_chunk_first.data(),
                                         slice_first.data(), &n_sets) == (int64_t)(((8 + size + 7) & ~15ull) + 8), "%llu %s: layout", (unsigned long long)len, name);
    CHECK(n_sets == 1 && set_file[0] == zero && set_range_first[1] == k && set_chunk_first[1] == wanted.size() && slice_first[0] == 8, "layout arrays");
    const uint64_t c0 = wanted.front(), c1 = wanted.back();
    uint64_t rows = 0;
    if (c1 / 64 - c0 / 64 <= 1) rows = c1 / 64 - c0 / 64 + 1;
    else { uint64_t last = ~0ull; for (uint64_t c : wanted) if (c / 1024 != last) { last = c / 1024; ++rows; } }
    CHECK(b3w_bao_set_slice_ingest_scratch_bytes(&len, 1, files.data(), first.data(), count.data(), k) == 16 * rows, "%llu %s: rows", (unsigned long long)len, name);
    // the encoder at every g: the same bytes, exact output
    std::vector<uint8_t> sl(size, 0xEE);
    for (int i = 0; i < 4; ++i) {
      std::vector<uint8_t> out(size, 0xEE);
      CHECK(b3w_bao_set_slice(obs[i].data(), len, gs[i], first.data(), count.data(), k, len ? data.data() : nullptr, nullptr, 0) == (int64_t)size, "size asked");
      CHECK(b3w_bao_set_slice(obs[i].data(), len, gs[i], first.data(), count.data(), k, len ? data.data() : nullptr, out.data(), size) == (int64_t)size, "encode");
      if (i == 0) sl = out;
      CHECK(out == sl, "%llu %s: the slice at g %u differs", (unsigned long long)len, name, gs[i]);
    }
    if (k == 1) {
      std::vector<uint8_t> rs(size, 0xEE);
      const uint64_t lo = first[0] * 1024, hi = (first[0] + count[0]) * 1024 < len ? (first[0] + count[0]) * 1024 : len;
      std::vector<uint8_t> bytes(data.begin() + lo, data.begin() + hi);
      CHECK(b3w_bao_range_slice(obs[0].data(), len, 0, first[0], count[0], bytes.data(), rs.data(), size) == (int64_t)size && rs == sl, "one run is the range slice");
    }
    // the decoder: exact outputs
    std::vector<uint8_t> got(payload ? payload : 1, 0xEE);
    std::vector<int32_t> cs(wanted.size(), -1);
    int32_t st = -1;
    uint64_t fb = 7;
    CHECK(b3w_bao_set_slice_decode(sl.data(), size, len, first.data(), count.data(), k, root, payload ? got.data() : nullptr, cs.data(), &st, &fb) == B3W_OK &&
          st == 0 && fb == UINT64_MAX, "%llu %s: decode", (unsigned long long)len, name);
    for (size_t r = 0; r < wanted.size(); ++r) {
      const uint64_t c = wanted[r], bytes = len - c * 1024 < 1024 ? len - c * 1024 : 1024;
      CHECK(cs[r] == 0 && (!bytes || memcmp(got.data() + r * 1024, data.data() + c * 1024, bytes) == 0), "%llu %s: chunk %llu", (unsigned long long)len, name, (unsigned long long)c);
    }
    // the receiver at every g, then the rest of the file as a second set: the file and the provider's outboard
    for (int i = 0; i < 4; ++i) {
      std::vector<uint8_t> d(len, 0xEE), ob(obs[i].size(), 0xEE);
      std::vector<uint64_t> have((n + 63) / 64, 0);
      std::fill(cs.begin(), cs.end(), -1);
      CHECK(b3w_bao_set_slice_ingest(sl.data(), size, len, first.data(), count.data(), k, root, gs[i], len ? d.data() : nullptr, ob.data(), have.data(), cs.data(), &st,
                                     &fb) == B3W_OK && st == 0 && fb == UINT64_MAX, "%llu %s: ingest at g %u", (unsigned long long)len, name, gs[i]);
      uint64_t bits = 0;
      for (uint64_t w : have) bits += (uint64_t)__builtin_popcountll(w);
      CHECK(bits == wanted.size(), "bits");
      for (uint64_t c : wanted) CHECK((have[c >> 6] >> (c & 63)) & 1, "bit %llu", (unsigned long long)c);
      std::vector<uint64_t> rf, rc;                        // the complement's runs
      uint64_t at = 0;
      for (uint32_t j = 0; j <= k; ++j) {
        const uint64_t stop = j < k ? first[j] : n;
        if (stop > at) { rf.push_back(at); rc.push_back(stop - at); }
        if (j < k) at = first[j] + count[j];
      }
      if (!rf.empty()) {
        const uint32_t k2 = (uint32_t)rf.size();
        const uint64_t size2 = b3w_bao_set_slice_size(len, rf.data(), rc.data(), k2);
        std::vector<uint8_t> sl2(size2, 0xEE);
        CHECK(b3w_bao_set_slice(obs[i].data(), len, gs[i], rf.data(), rc.data(), k2, data.data(), sl2.data(), size2) == (int64_t)size2, "complement");
        CHECK(b3w_bao_set_slice_ingest(sl2.data(), size2, len, rf.data(), rc.data(), k2, root, gs[i], d.data(), ob.data(), have.data(), nullptr, &st, nullptr) == B3W_OK &&
              st == 0, "%llu %s: the complement at g %u", (unsigned long long)len, name, gs[i]);
      }
      CHECK(d == data && ob == obs[i], "%llu %s: the file or its outboard at g %u", (unsigned long long)len, name, gs[i]);
    }
    // a flipped byte behind the header: reported, its chunks kept out, nothing else written beside the good chunks
    if (size > 8) {
      std::vector<uint8_t> bad = sl;
      bad[8 + (size - 8) / 2] ^= 0x20;
      std::vector<uint8_t> d(len, 0xEE), ob(obs[0].size(), 0xEE);
      std::vector<uint64_t> have((n + 63) / 64, 0);
      CHECK(b3w_bao_set_slice_ingest(bad.data(), size, len, first.data(), count.data(), k, root, 0, d.data(), ob.data(), have.data(), cs.data(), &st, &fb) == B3W_OK &&
            st != 0 && fb != UINT64_MAX, "%llu %s: the flip went unseen", (unsigned long long)len, name);
      for (size_t r = 0; r < wanted.size(); ++r) {
        const uint64_t c = wanted[r], bytes = len - c * 1024 < 1024 ? len - c * 1024 : 1024;
        const bool in = (have[c >> 6] >> (c & 63)) & 1;
        CHECK(in == (cs[r] == 0), "bit and status of chunk %llu", (unsigned long long)c);
        if (bytes) CHECK(in ? memcmp(d.data() + c * 1024, data.data() + c * 1024, bytes) == 0 : d[c * 1024] == 0xEE && d[c * 1024 + bytes - 1] == 0xEE, "chunk %llu", (unsigned long long)c);
      }
    }
  }
  // refusals: unsorted, overlapping, empty, past the file
  if (n >= 4) {
    const uint64_t f1[2] = {2, 0}, c1[2] = {1, 1}, f2[2] = {0, 1}, c2[2] = {2, 1}, f3[1] = {0}, c3[1] = {0}, f4[1] = {n - 1}, c4[1] = {2};
    CHECK(b3w_bao_set_slice_size(len, f1, c1, 2) == 0 && b3w_bao_set_slice_size(len, f2, c2, 2) == 0 && b3w_bao_set_slice_size(len, f3, c3, 1) == 0 &&
          b3w_bao_set_slice_size(len, f4, c4, 1) == 0 && b3w_bao_set_slice_size(len, nullptr, nullptr, 0) == 0, "refusals");
  }
}

int main() {
  std::mt19937_64 rng(28);
  const uint64_t lens[] = {0, 1, 1023, 1024, 1025, 2048, 3 * 1024 + 1, 5 * 1024 + 7, 17 * 1024 + 300, 63 * 1024, 64 * 1024, 65 * 1024, 70 * 1024 + 1, 100 * 1024 + 999,
                           1024 * 1024, 1025 * 1024, 1024 * 1024 + 300, 2049 * 1024, 3 * 1024 * 1024 + 5};
  for (uint64_t len : lens) check_file(len, rng);
  // several files in one layout: a set a file, files that do not ascend refused
  const uint64_t l3[3] = {5 * 1024 + 7, 0, 70 * 1024};
  const uint32_t files[5] = {0, 0, 1, 2, 2};
  const uint64_t first[5] = {1, 4, 0, 3, 64}, count[5] = {2, 2, 1, 1, 6};
  uint32_t set_file[3], set_range_first[4], n_sets = 0;
  uint64_t set_chunk_first[4], slice_first[4];
  CHECK(b3w_bao_set_slice_batch_layout(l3, 3, files, first, count, 5, set_file, set_range_first, set_chunk_first, slice_first, &n_sets) > 0 && n_sets == 3 &&
        set_range_first[3] == 5 && set_chunk_first[3] == 12, "three sets");
  const uint32_t back[3] = {0, 2, 0};
  CHECK(b3w_bao_set_slice_batch_layout(l3, 3, back, first, count, 3, nullptr, nullptr, nullptr, nullptr, nullptr) < 0, "a file that comes back");
  printf("bao_set_host_check: %ld checks passed, no sanitizer report\n", checks);
  return 0;
}
