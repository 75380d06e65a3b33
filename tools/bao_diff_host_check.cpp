// bao_diff_host_check.cpp — the host mirror of the outboard diff (b3w_bao_outboard_diff) run stand-alone over the shapes of
// tests/test_bao_diff_cpu.py, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_diff_host_check.cpp -o bao_diff_host_check && ./bao_diff_host_check          (one command line)
// Every buffer is exactly as large as the contract says (an outboard b3w_bao_group_outboard_size bytes, a root 8 words, the words
// ceil(n / 64)), so a read or write past one is the sanitizer's to report.  The outboards are the host's own
// (b3w_bao_outboard_resize from nothing), and the result is held against what the bytes say: a unit is same iff both files have it
// with the same extent, every chunk of it has the same bytes, and it is the whole file in both or in neither.  No device call is made
// and no kernel compiled: the mirror lives in b3w_bao_host.cpp, plain C++ that names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
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

static const uint32_t GS[4] = {0, 1, 4, 6};

static uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }

struct Version {
  std::vector<uint8_t> data;
  std::vector<uint8_t> ob[4];                              // one outboard a group_log of GS, exactly its size
  std::vector<uint32_t> root;
  explicit Version(std::vector<uint8_t> d) : data(std::move(d)), root(8) {
    const uint8_t none[8] = {0};
    for (int k = 0; k < 4; ++k) {
      ob[k].resize(b3w_bao_group_outboard_size(data.size(), GS[k]));
      CHECK(b3w_bao_outboard_resize(data.data(), data.size(), none, 0, GS[k], ob[k].data(), root.data()) == 0, "the outboard of %zu bytes", data.size());
    }
  }
};

static std::vector<uint8_t> random_bytes(std::mt19937_64 &rng, uint64_t len) {
  std::vector<uint8_t> d(len);
  for (auto &x : d) x = (uint8_t)rng();
  return d;
}

// what the bytes say, for units of 2^G chunks: a bool per chunk of b
static std::vector<bool> truth(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, uint32_t G) {
  const uint64_t na = chunks_of(a.size()), nb = chunks_of(b.size()), F = 1ull << G;
  std::vector<bool> out(nb, false);
  for (uint64_t s = 0; s < nb; s += F) {
    const uint64_t eb = std::min(s + F, nb), ea = std::min(s + F, na);
    if (s >= na || ea != eb || (na <= F) != (nb <= F)) continue;
    bool eq = true;
    for (uint64_t c = s; c < eb && eq; ++c) {
      const uint64_t a0 = c * 1024, a1 = std::min<uint64_t>(a.size(), a0 + 1024), b1 = std::min<uint64_t>(b.size(), a0 + 1024);
      eq = a1 == b1 && (a1 <= a0 || !memcmp(a.data() + a0, b.data() + a0, a1 - a0));
    }
    for (uint64_t c = s; c < eb; ++c) out[c] = eq;
  }
  return out;
}

static void check_pair(const Version &a, const Version &b) {
  const uint64_t nb = chunks_of(b.data.size()), words = (nb + 63) / 64;
  for (int ka = 0; ka < 4; ++ka)
    for (int kb = 0; kb < 4; ++kb) {
      const uint32_t G = std::max(GS[ka], GS[kb]);
      std::vector<uint64_t> same(words, 0xEEEEEEEEEEEEEEEEull);
      const int32_t rc = b3w_bao_outboard_diff(a.ob[ka].data(), a.data.size(), a.root.data(), GS[ka], b.ob[kb].data(), b.data.size(), b.root.data(), GS[kb], same.data());
      CHECK(rc == 0, "%zu against %zu bytes, group_logs %u %u: rc %d", a.data.size(), b.data.size(), GS[ka], GS[kb], rc);
      const std::vector<bool> want = truth(a.data, b.data, G);
      for (uint64_t c = 0; c < words * 64; ++c)
        CHECK(((same[c >> 6] >> (c & 63)) & 1) == (uint64_t)(c < nb && want[c]), "%zu against %zu bytes, group_logs %u %u: chunk %llu", a.data.size(), b.data.size(),
              GS[ka], GS[kb], (unsigned long long)c);
    }
}

int main() {
  std::mt19937_64 rng(31);
  // equal lengths: no edit, and an edit in the first, a middle and the last chunk
  for (uint64_t n : {1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049})
    for (uint64_t last : {1, 1024}) {
      const Version a(random_bytes(rng, (n - 1) * 1024 + last));
      check_pair(a, a);
      for (uint64_t c : {(uint64_t)0, n / 2, n - 1}) {
        std::vector<uint8_t> d = a.data;
        d[std::min<uint64_t>(c * 1024 + 7, d.size() - 1)] ^= 0x20;
        check_pair(a, Version(d));
      }
    }
  // the empty file
  {
    const Version none(std::vector<uint8_t>{}), one(random_bytes(rng, 1));
    check_pair(none, none);
    check_pair(none, one);
    check_pair(one, none);
  }
  // b grown and b shrunk: one is the other's bytes cut off
  const std::pair<uint64_t, uint64_t> resized[] = {{1, 2}, {1, 3}, {1, 65}, {2, 3}, {16, 17}, {17, 18}, {32, 33}, {63, 64}, {64, 65}, {64, 128}, {65, 129},
                                                   {1023, 1025}, {1024, 1025}, {1025, 2049}, {1023, 2049}};
  for (const auto &r : resized)
    for (uint64_t last : {1, 1024})
      for (uint64_t cut : {(uint64_t)0, 1024 - last}) {
        const Version longer(random_bytes(rng, (r.second - 1) * 1024 + last));
        const Version shorter(std::vector<uint8_t>(longer.data.begin(), longer.data.begin() + (r.first * 1024 - cut)));
        check_pair(shorter, longer);
        check_pair(longer, shorter);
      }
  // refusals
  {
    const uint8_t ob[8] = {0};
    const uint32_t root[8] = {0};
    uint64_t w = 0xEE;
    const uint64_t huge = ((1ull << 30) + 1) * 1024;
    CHECK(b3w_bao_outboard_diff(nullptr, 1, root, 0, ob, 1, root, 0, &w) == B3W_E_BAD_ARGUMENT, "a null outboard of a");
    CHECK(b3w_bao_outboard_diff(ob, 1, nullptr, 0, ob, 1, root, 0, &w) == B3W_E_BAD_ARGUMENT, "a null root of a");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, nullptr, 1, root, 0, &w) == B3W_E_BAD_ARGUMENT, "a null outboard of b");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, ob, 1, nullptr, 0, &w) == B3W_E_BAD_ARGUMENT, "a null root of b");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, ob, 1, root, 0, nullptr) == B3W_E_BAD_ARGUMENT, "null words");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 7, ob, 1, root, 0, &w) == B3W_E_BAD_ARGUMENT, "group_log_a 7");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, ob, 1, root, 7, &w) == B3W_E_BAD_ARGUMENT, "group_log_b 7");
    CHECK(b3w_bao_outboard_diff(ob, huge, root, 0, ob, 1, root, 0, &w) == B3W_E_BAD_ARGUMENT, "a of more than 2^30 chunks");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, ob, huge, root, 0, &w) == B3W_E_BAD_ARGUMENT, "b of more than 2^30 chunks");
    CHECK(w == 0xEE, "a refusal wrote");
    CHECK(b3w_bao_outboard_diff(ob, 1, root, 0, ob, 1, root, 0, &w) == 0 && w == 1, "one chunk against itself");
  }
  printf("bao_diff_host_check: %ld checks passed\n", checks);
  return 0;
}
