// bao_range_host_check.cpp — the host calls of the range slices (b3w_bao_range_slice_size, _batch_layout, b3w_bao_range_slice, _decode,
// _ingest) run stand-alone over the files and range kinds of tests/test_bao_range_cpu.py, for a sanitizer build of host code that is never
// loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_range_host_check.cpp -o bao_range_host_check && ./bao_range_host_check          (one command line)
// Every buffer is exactly as large as the contract says (the slice its size, range_bytes the touched groups clipped to the file, the
// decoder's output the range's payload, the bitmap ceil(n / 64) words), so a read or write past one is the sanitizer's to report.  The
// results are held against each other and against the library's older host calls: the slice from the full outboard equals the one from
// every group outboard, a range of one chunk equals b3w_bao_slice, what is decoded is the file, every range taken in leaves the file
// and the provider's outboard, which b3w_bao_verify accepts; a flipped byte is reported and keeps its chunk out.  No device call is made
// and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
  if (n <= 65) for (uint64_t c = 0; c < n; ++c) out.insert({c, 1});
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
  const auto ranges = ranges_of(n);
  std::vector<std::vector<uint8_t>> got_data(4, std::vector<uint8_t>(len, 0xEE)), got_ob;
  std::vector<std::vector<uint64_t>> got_have(4, std::vector<uint64_t>((n + 63) / 64, 0));
  for (int i = 0; i < 4; ++i) got_ob.push_back(std::vector<uint8_t>(obs[i].size(), 0xEE));
  for (const auto &r : ranges) {
    const uint64_t a = r.first, k = r.second;
    const uint64_t end = (a + k) * 1024 < len ? (a + k) * 1024 : len, payload = end - a * 1024;
    const uint64_t size = b3w_bao_range_slice_size(len, a, k);
    CHECK(size >= 8 + payload && (size - 8 - payload) % 64 == 0, "size of (%llu, %llu)", (unsigned long long)a, (unsigned long long)k);
    CHECK(b3w_bao_range_slice(obs[0].data(), len, 0, a, k, nullptr, nullptr, 0) == (int64_t)size, "size query");
    std::vector<uint8_t> sl;
    for (int i = 0; i < 4; ++i) {                          // from the full and from every group outboard: the same bytes
      const uint32_t g = gs[i];
      const uint64_t g0 = (a >> g) << g, g1 = (((a + k - 1) >> g) + 1) << g;
      const uint64_t b0 = g0 * 1024, b1 = g1 * 1024 < len ? g1 * 1024 : len;
      const std::vector<uint8_t> bytes(data.begin() + b0, data.begin() + b1);
      std::vector<uint8_t> out(size, 0xEE);
      CHECK(b3w_bao_range_slice(obs[i].data(), len, g, a, k, bytes.empty() ? nullptr : bytes.data(), out.data(), size) == (int64_t)size, "extract at g %u", g);
      if (i == 0) sl = out;
      CHECK(out == sl, "the slice of (%llu, %llu) from the group outboard at g %u differs", (unsigned long long)a, (unsigned long long)k, g);
      CHECK(b3w_bao_range_slice(obs[i].data(), len, g, a, k, bytes.empty() ? nullptr : bytes.data(), out.data(), size - 1) == -B3W_E_BAD_ARGUMENT, "a short buffer");
    }
    if (k == 1) {
      std::vector<uint8_t> one(b3w_bao_slice_size(len, a), 0xEE);
      uint64_t one_len = one.size();
      CHECK(one.size() == size, "one-chunk size");
      CHECK(b3w_bao_slice(obs[0].data(), len, a, payload ? data.data() + a * 1024 : nullptr, one.data(), &one_len) == B3W_OK && one == sl, "k = 1 is b3w_bao_slice's slice");
    }
    std::vector<uint8_t> out(payload, 0xEE);
    int32_t st = -7;
    uint64_t fb = 77;
    CHECK(b3w_bao_range_slice_decode(sl.data(), size, len, a, k, root, out.empty() ? nullptr : out.data(), &st, &fb) == B3W_OK && st == 0 && fb == ~0ull, "decode");
    CHECK(payload == 0 || memcmp(out.data(), data.data() + a * 1024, payload) == 0, "decoded bytes");
    for (int i = 0; i < 4; ++i) {
      st = -7;
      CHECK(b3w_bao_range_slice_ingest(sl.data(), size, len, a, k, root, gs[i], len ? got_data[i].data() : nullptr, got_ob[i].data(), got_have[i].data(), &st, &fb) == B3W_OK &&
                st == 0 && fb == ~0ull, "ingest at g %u", gs[i]);
    }
    // a flipped byte in the first node (or the only chunk) and in the last chunk: reported, and nothing of the bad chunk is written
    for (int which = 0; which < 2; ++which) {
      if (size == 8) continue;
      std::vector<uint8_t> bad = sl;
      const uint64_t at = which == 0 ? 8 : size - 1;      // the root node (or the only chunk); the last chunk
      bad[at] ^= 1;
      std::vector<uint8_t> d(len, 0xEE), ob(obs[0].size(), 0xEE), o2(payload, 0xEE);
      std::vector<uint64_t> hv((n + 63) / 64, 0);
      CHECK(b3w_bao_range_slice_ingest(bad.data(), size, len, a, k, root, 0, len ? d.data() : nullptr, ob.data(), hv.data(), &st, &fb) == B3W_OK && st != 0 && fb >= a && fb < a + k,
            "a flipped byte at %llu of (%llu, %llu)", (unsigned long long)at, (unsigned long long)a, (unsigned long long)k);
      CHECK(!((hv[fb >> 6] >> (fb & 63)) & 1), "the bad chunk's bit");
      const uint64_t b0 = fb * 1024, b1 = (fb + 1) * 1024 < len ? (fb + 1) * 1024 : len;
      for (uint64_t x = b0; x < b1; ++x) CHECK(d[x] == 0xEE, "a byte of the bad chunk was written");
      int32_t st2 = -7;
      uint64_t fb2 = 77;
      CHECK(b3w_bao_range_slice_decode(bad.data(), size, len, a, k, root, o2.empty() ? nullptr : o2.data(), &st2, &fb2) == B3W_OK && st2 == st && fb2 == fb, "decode agrees");
    }
  }
  for (int i = 0; i < 4; ++i) {                            // (the whole file is one of the ranges)
    CHECK(got_data[i] == data && got_ob[i] == obs[i], "the file and the provider's outboard at g %u", gs[i]);
    for (uint64_t c = 0; c < n; ++c) CHECK((got_have[i][c >> 6] >> (c & 63)) & 1, "bit %llu", (unsigned long long)c);
    CHECK(n % 64 == 0 || (got_have[i].back() >> (n % 64)) == 0, "pad bits");
    std::vector<uint8_t> units((n + (1ull << gs[i]) - 1) >> gs[i], 0xEE);
    int32_t fs = -7;
    uint64_t fb = 77;
    CHECK(b3w_bao_verify(len ? got_data[i].data() : nullptr, len, got_ob[i].data(), gs[i], root, units.data(), &fs, &fb) == B3W_OK && fs == 0, "b3w_bao_verify at g %u", gs[i]);
  }
}

static void check_refusals() {
  const uint64_t len = 5 * 1024 + 7;
  std::vector<uint8_t> data(len, 3), ob(b3w_bao_outboard_size(len), 0xEE), sl, d(len, 0xEE), o(ob.size(), 0xEE);
  const uint64_t zero = 0, n = 6;
  uint32_t root[8];
  for (int k = 0; k < 8; ++k) ob[k] = (uint8_t)(len >> (8 * k));
  CHECK(b3w_bao_outboard_update(data.data(), len, ob.data(), 0, &zero, &n, 1, root) == B3W_OK, "outboard");
  sl.resize(b3w_bao_range_slice_size(len, 1, 3));
  CHECK(b3w_bao_range_slice(ob.data(), len, 0, 1, 3, data.data() + 1024, sl.data(), sl.size()) == (int64_t)sl.size(), "extract");
  CHECK(b3w_bao_range_slice_size(len, 0, 0) == 0 && b3w_bao_range_slice_size(len, 6, 1) == 0 && b3w_bao_range_slice_size(len, 5, 2) == 0 &&
            b3w_bao_range_slice_size(len, 2, ~0ull) == 0 && b3w_bao_range_slice_size(0, 0, 1) == 8, "sizes");
  int32_t st = -7;
  uint64_t fb = 77, hv = 0;
  const int32_t BAD = B3W_E_BAD_ARGUMENT;
  CHECK(b3w_bao_range_slice_ingest(nullptr, sl.size(), len, 1, 3, root, 0, d.data(), o.data(), &hv, &st, &fb) == BAD, "null slice");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 3, nullptr, 0, d.data(), o.data(), &hv, &st, &fb) == BAD, "null root");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 3, root, 0, nullptr, o.data(), &hv, &st, &fb) == BAD, "null data");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 3, root, 0, d.data(), nullptr, &hv, &st, &fb) == BAD, "null outboard");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 3, root, 0, d.data(), o.data(), &hv, nullptr, &fb) == BAD, "null status");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 3, root, 7, d.data(), o.data(), &hv, &st, &fb) == BAD, "group_log 7");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size() - 1, len, 1, 3, root, 0, d.data(), o.data(), &hv, &st, &fb) == BAD, "a short slice");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 1, 0, root, 0, d.data(), o.data(), &hv, &st, &fb) == BAD, "no chunk");
  CHECK(b3w_bao_range_slice_ingest(sl.data(), sl.size(), len, 4, 3, root, 0, d.data(), o.data(), &hv, &st, &fb) == BAD, "past the file");
  CHECK(b3w_bao_range_slice_decode(sl.data(), sl.size(), len, 1, 3, root, nullptr, nullptr, nullptr) == BAD, "decode without a status");
  for (uint8_t b : d) CHECK(b == 0xEE, "data touched");
  for (uint8_t b : o) CHECK(b == 0xEE, "outboard touched");
  CHECK(st == -7 && fb == 77 && hv == 0, "outputs touched");
  const uint64_t lens[3] = {len, 0, 70 * 1024}, first[4] = {1, 3, 0, 69}, count[4] = {3, 64, 1, 1};
  const uint32_t files[4] = {0, 2, 1, 2};
  uint64_t sf[5];
  CHECK(b3w_bao_range_slice_batch_layout(lens, 3, files, first, count, 4, sf) > 0, "layout");
  for (int i = 0; i < 4; ++i) CHECK(sf[i] % 16 == 8 && sf[i + 1] >= sf[i] + b3w_bao_range_slice_size(lens[files[i]], first[i], count[i]), "start %d", i);
  const uint32_t bad_file[1] = {3};
  const uint64_t bad_count[1] = {0};
  CHECK(b3w_bao_range_slice_batch_layout(lens, 3, bad_file, first, count, 1, sf) == -BAD && b3w_bao_range_slice_batch_layout(lens, 3, files, first, bad_count, 1, sf) == -BAD &&
            b3w_bao_range_slice_batch_layout(lens, 3, files, first, count, 4, nullptr) == -BAD, "layout refusals");
  CHECK(b3w_bao_range_slice_ingest_scratch_bytes(lens, 3, files, first, count, 4) == 16 * 5 && b3w_bao_range_slice_ingest_scratch_bytes(nullptr, 0, nullptr, nullptr, nullptr, 0) == 0,
        "scratch bytes");
}

int main() {
  std::mt19937_64 rng(23);
  std::vector<uint64_t> lens = {0, 1, 1023, 1024, 1025, 17 * 1024 + 300, 33 * 1024 - 1};
  for (uint64_t n = 2; n <= 40; ++n) lens.push_back(n * 1024);
  for (uint64_t n : {63, 64, 65, 1025, 2049}) lens.push_back(n * 1024);
  for (uint64_t len : lens) check_file(len, rng);
  check_refusals();
  printf("bao_range_host_check: %ld checks passed over %zu files\n", checks, lens.size());
  return 0;
}
