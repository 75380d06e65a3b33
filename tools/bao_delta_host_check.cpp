// bao_delta_host_check.cpp — the host mirrors of the outboard delta (b3w_bao_outboard_delta, b3w_bao_outboard_delta_apply) run
// stand-alone, for a sanitizer build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp
//       tools/bao_delta_host_check.cpp -o bao_delta_host_check && ./bao_delta_host_check          (one command line)
// Every buffer is a heap block of exactly the size the contract says (an outboard b3w_bao_group_outboard_size bytes, a root 8 words,
// a blob its extent), so a read or write past one is the sanitizer's to report.  The outboards are the host's own
// (b3w_bao_outboard_resize from nothing).  Held: apply(delta(a, b)) onto a's outboard is b's outboard byte for byte, into a fresh
// buffer and (equal unit counts) in place; the capacity rule; and the UNTRUSTED side - every blob cut off at every length that still
// holds header and bitmap, every byte of a blob flipped, bitmaps and counts made up at random - ends in a status with the output
// untouched.  No device call is made and no kernel compiled.
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

static const uint32_t GS[3] = {0, 4, 6};

static uint64_t units_of(uint64_t len, uint32_t g) {
  const uint64_t n = len ? (len + 1023) / 1024 : 1;
  return (n + (1ull << g) - 1) >> g;
}

struct Version {
  std::vector<uint8_t> data;
  std::vector<uint8_t> ob[3];                              // one outboard a group_log of GS, exactly its size
  std::vector<uint32_t> root;
  explicit Version(std::vector<uint8_t> d) : data(std::move(d)), root(8) {
    const uint8_t none[8] = {0};
    for (int k = 0; k < 3; ++k) {
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

// the replica on a heap copy of exactly `blob`; a status leaves the output as it was -> the status
static int32_t apply(const Version *a, const Version &b, int k, const std::vector<uint8_t> &blob, uint64_t *bad_out = nullptr) {
  std::vector<uint8_t> out(b.ob[k].size(), 0xEE);
  int32_t status = 77;
  uint64_t bad = 77;
  const int32_t rc = b3w_bao_outboard_delta_apply(a ? a->ob[k].data() : nullptr, a ? a->data.size() : 0, a ? a->root.data() : nullptr, b.data.size(), b.root.data(),
                                                  GS[k], blob.data(), blob.size(), out.data(), &status, &bad);
  CHECK(rc == 0, "apply: rc %d", rc);
  if (status == 0) CHECK(out == b.ob[k] && bad == ~0ull, "a passed blob did not give b's outboard (%zu bytes, group_log %u)", b.data.size(), GS[k]);
  else CHECK(std::all_of(out.begin(), out.end(), [](uint8_t x) { return x == 0xEE; }) && status >= 1 && status <= 3, "status %d wrote", status);
  if (bad_out) *bad_out = bad;
  return status;
}

static void check_pair(const Version *a, const Version &b, std::mt19937_64 &rng, bool hostile) {
  for (int k = 0; k < 3; ++k) {
    const uint32_t g = GS[k];
    const uint64_t ub = units_of(b.data.size(), g), W = (ub - 1 + 63) / 64, head = 16 + 8 * W, bound = b3w_bao_outboard_delta_bound(b.data.size(), g);
    CHECK(bound == head + 64 * (ub - 1), "the bound");
    std::vector<uint8_t> full(bound);
    uint64_t found = 0;
    CHECK(b3w_bao_outboard_delta(a ? a->ob[k].data() : nullptr, a ? a->data.size() : 0, a ? a->root.data() : nullptr, b.ob[k].data(), b.data.size(), b.root.data(), g,
                                 full.data(), full.size(), &found) == 0 && found <= ub - 1, "the provider");
    const std::vector<uint8_t> blob(full.begin(), full.begin() + head + 64 * found);       // (the exact blob)
    CHECK(apply(a, b, k, blob) == 0, "the round trip of %zu bytes, group_log %u", b.data.size(), g);
    if (a && units_of(a->data.size(), g) == ub) {          // in place
      std::vector<uint8_t> mine = a->ob[k];
      int32_t status = 77;
      uint64_t bad = 77;
      CHECK(b3w_bao_outboard_delta_apply(mine.data(), a->data.size(), a->root.data(), b.data.size(), b.root.data(), g, blob.data(), blob.size(), mine.data(), &status,
                                         &bad) == 0 && status == 0 && mine == b.ob[k], "in place");
    }
    // the capacity rule: every extent from the header and bitmap alone to one node short
    for (uint64_t fit = 0; fit < found; fit += 1 + found / 7) {
      std::vector<uint8_t> part(head + 64 * fit + 8 * (fit & 1));
      uint64_t again = 0;
      CHECK(b3w_bao_outboard_delta(a ? a->ob[k].data() : nullptr, a ? a->data.size() : 0, a ? a->root.data() : nullptr, b.ob[k].data(), b.data.size(), b.root.data(), g,
                                   part.data(), part.size(), &again) == 0 && again == found && !memcmp(part.data(), blob.data(), head + 64 * fit), "capacity %llu",
            (unsigned long long)fit);
      CHECK(apply(a, b, k, part) == B3W_BAO_DELTA_MALFORMED, "a short blob passed");
    }
    if (!hostile) continue;
    for (uint64_t cut = head; cut < blob.size(); cut += 8)                      // cut off
      CHECK(apply(a, b, k, std::vector<uint8_t>(blob.begin(), blob.begin() + cut)) == B3W_BAO_DELTA_MALFORMED, "a blob cut at %llu passed", (unsigned long long)cut);
    for (uint64_t at = 0; at < blob.size(); at += 1 + blob.size() / 600) {      // a flipped byte
      std::vector<uint8_t> bad = blob;
      bad[at] ^= (uint8_t)(1u << (rng() & 7));
      CHECK(apply(a, b, k, bad) != 0, "a flipped byte %llu passed", (unsigned long long)at);
    }
    for (int t = 0; t < 40; ++t) {                                               // made-up bitmaps and counts over random nodes
      std::vector<uint8_t> bad = t & 1 ? blob : random_bytes(rng, head + 64 * (rng() % ub));
      memcpy(bad.data(), blob.data(), 8);
      for (uint64_t j = 16; j < head; ++j) if (rng() % 3 == 0) bad[j] = (uint8_t)rng();
      uint64_t count = 0;
      for (uint64_t j = 16; j < head; ++j) count += (uint64_t)__builtin_popcount(bad[j]);
      const uint64_t k_made = t % 4 == 3 ? rng() : count;
      memcpy(bad.data() + 8, &k_made, 8);
      (void)apply(a, b, k, bad);                                                 // (any status, or a pass that is b's outboard: apply checks it)
    }
  }
}

int main() {
  std::mt19937_64 rng(32);
  for (uint64_t n : {1, 2, 3, 4, 5, 64, 65, 66, 129, 1025, 2049})
    for (uint64_t last : {1, 1024}) {
      const Version a(random_bytes(rng, (n - 1) * 1024 + last));
      check_pair(&a, a, rng, false);
      check_pair(nullptr, a, rng, n <= 129);
      for (uint64_t c : {(uint64_t)0, n / 2, n - 1}) {
        std::vector<uint8_t> d = a.data;
        d[std::min<uint64_t>(c * 1024 + 7, d.size() - 1)] ^= 0x20;
        check_pair(&a, Version(d), rng, n <= 129 || c == n / 2);
      }
    }
  // b grown and b shrunk: one is the other's bytes cut off, then with chunk 1 rewritten
  const std::pair<uint64_t, uint64_t> resized[] = {{1, 2}, {2, 3}, {4, 5}, {16, 17}, {17, 33}, {64, 65}, {65, 66}, {64, 128}, {65, 129}, {1024, 1025}, {1025, 2049}, {1040, 2049}};
  for (const auto &r : resized)
    for (uint64_t last : {1, 1024}) {
      const Version longer(random_bytes(rng, (r.second - 1) * 1024 + last));
      std::vector<uint8_t> cut(longer.data.begin(), longer.data.begin() + (r.first * 1024 - (1024 - last)));
      const Version shorter(cut);
      check_pair(&shorter, longer, rng, r.second <= 129);
      check_pair(&longer, shorter, rng, r.second <= 129);
      if (r.first > 1) {
        cut[std::min<size_t>(1024 + 9, cut.size() - 1)] ^= 1;
        check_pair(&longer, Version(cut), rng, false);
      }
    }
  // refusals
  {
    const Version a(random_bytes(rng, 3000));
    std::vector<uint8_t> blob(b3w_bao_outboard_delta_bound(3000, 0)), out(a.ob[0].size(), 0xEE);
    uint64_t k = 77, bad = 77;
    int32_t status = 77;
    const uint64_t huge = ((1ull << 30) + 1) * 1024;
    CHECK(b3w_bao_outboard_delta(a.ob[0].data(), 3000, nullptr, a.ob[0].data(), 3000, a.root.data(), 0, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "a null root of a");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, nullptr, 3000, a.root.data(), 0, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "a null outboard of b");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, nullptr, 0, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "a null root of b");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, a.root.data(), 7, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "group_log 7");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, a.root.data(), 0, nullptr, blob.size(), &k) == B3W_E_BAD_ARGUMENT, "a null blob");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, a.root.data(), 0, blob.data(), 23, &k) == B3W_E_BAD_ARGUMENT, "an extent of 23 bytes");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, a.root.data(), 0, blob.data(), blob.size(), nullptr) == B3W_E_BAD_ARGUMENT, "a null count");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), huge, a.root.data(), 0, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "b of more than 2^30 chunks");
    CHECK(b3w_bao_outboard_delta(a.ob[0].data(), huge, a.root.data(), a.ob[0].data(), 3000, a.root.data(), 0, blob.data(), blob.size(), &k) == B3W_E_BAD_ARGUMENT, "a of more than 2^30 chunks");
    CHECK(k == 77 && std::all_of(blob.begin(), blob.end(), [](uint8_t x) { return x == 0; }), "a refusal wrote");
    CHECK(b3w_bao_outboard_delta(nullptr, 0, nullptr, a.ob[0].data(), 3000, a.root.data(), 0, blob.data(), blob.size(), &k) == 0 && k == 2, "three chunks against nothing");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, nullptr, 0, blob.data(), blob.size(), out.data(), &status, &bad) == B3W_E_BAD_ARGUMENT, "a null root of b");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 0, nullptr, blob.size(), out.data(), &status, &bad) == B3W_E_BAD_ARGUMENT, "a null blob");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 0, blob.data(), 23, out.data(), &status, &bad) == B3W_E_BAD_ARGUMENT, "an extent of 23 bytes");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 0, blob.data(), blob.size(), nullptr, &status, &bad) == B3W_E_BAD_ARGUMENT, "a null output");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 0, blob.data(), blob.size(), out.data(), nullptr, &bad) == B3W_E_BAD_ARGUMENT, "a null status");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 7, blob.data(), blob.size(), out.data(), &status, &bad) == B3W_E_BAD_ARGUMENT, "group_log 7");
    CHECK(status == 77 && bad == 77 && std::all_of(out.begin(), out.end(), [](uint8_t x) { return x == 0xEE; }), "a refusal wrote");
    CHECK(b3w_bao_outboard_delta_apply(nullptr, 0, nullptr, 3000, a.root.data(), 0, blob.data(), blob.size(), out.data(), &status, &bad) == 0 && status == 0 && out == a.ob[0], "the outboard checked against its root");
  }
  printf("bao_delta_host_check: %ld checks passed\n", checks);
  return 0;
}
