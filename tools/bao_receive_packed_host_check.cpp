// bao_receive_packed_host_check.cpp — the host side of the packed receivers (b3w_bao_slice_ingest_packed_device,
// b3w_bao_range_slice_ingest_packed_device, b3w_bao_set_slice_ingest_packed_device) run stand-alone, up to the launch, for a sanitizer
// build of host code that is never loaded into Python:
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -I include -I hot-proofs-blake3-circom_amd/csrc
//       hot-proofs-blake3-circom_amd/csrc/b3w_bao_host.cpp tools/bao_receive_packed_host_check.cpp -o bao_receive_packed_host_check
//       && ./bao_receive_packed_host_check                                                            (one command line)
// Every buffer is exactly as large as the contract says, so a read or write past one is the sanitizer's to report.
//   - THE SLOT BUFFER'S REFUSALS (b3w_int_slots_wrong, the one place the three calls ask): an empty list takes any buffer, a null one
//     included; a list that is not empty refuses a null buffer, one that is not 16-byte aligned, and one a byte short - naming the bytes
//     needed; the pointers are never dereferenced (they point nowhere).  b3w_int_listed_chunks is the sum of the counts, 64 bits wide.
//   - THE SLOTS.  One-chunk slices: slot i.  Range slices: the running sum of the counts, which is the chunk index
//     b3w_sample_rows_ranges packs its per-chunk outputs by.  Set slices: b3w_int_set_list's chunk_first (= b3w_bao_set_slice_batch_layout's
//     set_chunk_first) + the rank.  For every list the slot buffer is filled by the HOST decoders (b3w_bao_slice_decode,
//     b3w_bao_range_slice_decode, b3w_bao_set_slice_decode write at 1024 (c - first) / 1024 rank behind a list entry's first slot) from
//     slices the host encoders make, into a buffer of exactly 1024 x the listed chunks of 0xEE: every slot must hold its chunk's bytes,
//     the rest of a short last chunk's slot the fill, and with one byte of a chunk flipped that slot alone keeps the fill.
//   - One file of 2^30 chunks: the listed chunks and the bytes needed pass 2^32 and 2^40.
// No device call is made and no kernel compiled: b3w_bao_host.cpp is plain C++ and names nothing of another object file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "b3wit.h"
#include "b3w_bao_plan.h"

static long checks = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

typedef unsigned long long ull;
static const uint8_t FILL = 0xEE;

struct File { uint64_t len, n; std::vector<uint8_t> data, ob; uint32_t root[8]; };

static File make_file(uint64_t len, uint32_t seed) {
  File f;
  f.len = len; f.n = len ? (len + 1023) / 1024 : 1;
  f.data.resize(len);
  uint32_t x = seed * 2654435761u + 12345u;
  for (uint64_t i = 0; i < len; ++i) { x = x * 1664525u + 1013904223u; f.data[i] = (uint8_t)(x >> 24); }
  f.ob.assign(b3w_bao_outboard_size(len), 0);
  for (int k = 0; k < 8; ++k) f.ob[k] = (uint8_t)(len >> (8 * k));
  const uint64_t a = 0;
  CHECK(b3w_bao_outboard_update(len ? f.data.data() : nullptr, len, f.ob.data(), 0, &a, &f.n, 1, f.root) == B3W_OK, "outboard of %llu bytes", (ull)len);
  return f;
}
static uint64_t chunk_len(const File &f, uint64_t c) { return f.len - 1024 * c < 1024 ? f.len - 1024 * c : 1024; }

// slot k of `slots` against chunk c of f: its bytes, then the fill; `kept_out`: the whole slot is the fill
static void check_slot(const std::vector<uint8_t> &slots, uint64_t k, const File &f, uint64_t c, bool kept_out, const char *what) {
  const uint64_t bytes = kept_out ? 0 : chunk_len(f, c);
  CHECK(1024 * (k + 1) <= slots.size(), "%s: slot %llu lies in the buffer", what, (ull)k);
  CHECK(!bytes || !memcmp(slots.data() + 1024 * k, f.data.data() + 1024 * c, bytes), "%s: slot %llu is chunk %llu", what, (ull)k, (ull)c);
  for (uint64_t o = bytes; o < 1024; ++o) CHECK(slots[1024 * k + o] == FILL, "%s: slot %llu byte %llu is not written", what, (ull)k, (ull)o);
}

static void check_refusals() {
  uint8_t *const aligned = reinterpret_cast<uint8_t *>(uintptr_t(0x7000000000ull));      // (never dereferenced)
  CHECK(b3w_int_slots_wrong(nullptr, 0, 0).empty() && b3w_int_slots_wrong(aligned, 0, 0).empty(), "an empty list takes any buffer");
  CHECK(b3w_int_slots_wrong(aligned, 3 * 1024, 3).empty() && b3w_int_slots_wrong(aligned, 1ull << 40, 3).empty(), "room enough");
  std::string why = b3w_int_slots_wrong(nullptr, 3 * 1024, 3);
  CHECK(why.find("null d_chunks") != std::string::npos && why.find("3072") != std::string::npos, "null: %s", why.c_str());
  for (uintptr_t off : {1u, 4u, 8u, 15u}) {
    why = b3w_int_slots_wrong(aligned + off, 1 << 20, 3);
    CHECK(why.find("16-byte") != std::string::npos, "misaligned by %u: %s", (unsigned)off, why.c_str());
  }
  why = b3w_int_slots_wrong(aligned, 3 * 1024 - 1, 3);
  CHECK(why.find("chunks_bytes is 3071") != std::string::npos && why.find("3072") != std::string::npos, "a byte short: %s", why.c_str());
  const uint64_t big = (1ull << 30) + 5;
  why = b3w_int_slots_wrong(aligned, (big << 10) - 1, big);
  CHECK(why.find(std::to_string(big << 10)) != std::string::npos && (big << 10) > (1ull << 40), "2^30 chunks: %s", why.c_str());
  CHECK(b3w_int_slots_wrong(aligned, big << 10, big).empty(), "2^30 chunks fit");
  CHECK(!b3w_int_slots_wrong(aligned, ~0ull, 1ull << 54).empty() && !b3w_int_slots_wrong(aligned, ~0ull, ~0ull).empty(), "slots past 64 bits of bytes");
  const uint64_t counts[3] = {1ull << 33, 7, 1ull << 33}, over[2] = {~0ull - 3, 9};
  CHECK(b3w_int_listed_chunks(counts, 3) == (1ull << 34) + 7 && b3w_int_listed_chunks(counts, 0) == 0, "the sum of the counts");
  CHECK(b3w_int_listed_chunks(over, 2) == ~0ull && !b3w_int_slots_wrong(aligned, ~0ull, b3w_int_listed_chunks(over, 2)).empty(), "a sum past 64 bits");
}

// one call's list over `files`: the three kinds' slots, filled by the host decoders
static void check_lists(const std::vector<File> &files) {
  const uint32_t n_files = (uint32_t)files.size();
  std::vector<uint64_t> lens;
  for (const File &f : files) lens.push_back(f.len);
  // ---- ranges: overlapping, repeated, out of file order; the last chunk alone; the whole file
  std::vector<uint32_t> rf;
  std::vector<uint64_t> ra, rk;
  for (uint32_t f = n_files; f-- > 0;) {
    const uint64_t n = files[f].n;
    for (auto r : {std::pair<uint64_t, uint64_t>{n - 1, 1}, {0, n}, {n / 3, n - n / 3}, {n / 3, n - n / 3}, {n / 2, 1}}) { rf.push_back(f); ra.push_back(r.first); rk.push_back(r.second); }
  }
  const uint32_t nr = (uint32_t)rf.size();
  const uint64_t listed = b3w_int_listed_chunks(rk.data(), nr);
  std::vector<uint64_t> rrf((size_t)nr + 1), crf(listed + 1);
  CHECK(b3w_sample_rows_ranges(lens.data(), n_files, rf.data(), ra.data(), rk.data(), nr, rrf.data(), crf.data(), nullptr) >= 0, "the ranges' rows");
  for (int tamper = 0; tamper < 2; ++tamper) {
    std::vector<uint8_t> slots(1024 * listed, FILL);
    uint64_t slot = 0;
    for (uint32_t i = 0; i < nr; ++i) {
      const File &f = files[rf[i]];
      CHECK(crf[slot] == rrf[i], "range %u: its first slot is its first chunk status", i);      // (the planner's per-chunk index: b3wit.h)
      const uint64_t size = b3w_bao_range_slice_size(f.len, ra[i], rk[i]);
      std::vector<uint8_t> sl(size);
      const uint64_t c0 = ra[i], bytes0 = 1024 * c0 < f.len ? f.len - 1024 * c0 : 0, span = bytes0 < 1024 * rk[i] ? bytes0 : 1024 * rk[i];
      std::vector<uint8_t> range_bytes(f.data.begin() + (f.len ? 1024 * c0 : 0), f.data.begin() + (f.len ? 1024 * c0 : 0) + span);
      CHECK(b3w_bao_range_slice(f.ob.data(), f.len, 0, ra[i], rk[i], range_bytes.data(), sl.data(), size) == (int64_t)size, "range %u: the slice", i);
      const uint64_t victim = ra[i] + rk[i] - 1;            // (the range's last chunk: its bytes end the slice)
      const bool hit = tamper && chunk_len(f, victim);
      if (hit) sl[size - 1] ^= 1;
      int32_t st = -1;
      uint64_t fb = 0;
      std::vector<uint8_t> part(1024 * rk[i], FILL);       // (the decoder's out_bytes: room for 1024 n_chunks, exactly)
      CHECK(b3w_bao_range_slice_decode(sl.data(), size, f.len, ra[i], rk[i], f.root, part.data(), &st, &fb) == B3W_OK, "range %u: decode", i);
      CHECK(st == (hit ? 1 : 0) && fb == (hit ? victim : ~0ull), "range %u: status %d first bad %llu", i, st, (ull)fb);
      memcpy(slots.data() + 1024 * slot, part.data(), part.size());
      for (uint64_t c = ra[i]; c < ra[i] + rk[i]; ++c) check_slot(slots, slot + (c - ra[i]), f, c, hit && c == victim, "ranges");
      slot += rk[i];
    }
    CHECK(slot == listed && 1024 * slot == slots.size(), "the ranges fill their slots");
  }
  // ---- one-chunk samples: slot i, repeated samples each their own
  {
    std::vector<uint32_t> sf;
    std::vector<uint64_t> sc;
    for (uint32_t f = 0; f < n_files; ++f)
      for (uint64_t c : {files[f].n - 1, (uint64_t)0, files[f].n / 2, files[f].n - 1}) { sf.push_back(f); sc.push_back(c); }
    const uint32_t ns = (uint32_t)sf.size();
    std::vector<uint64_t> first((size_t)ns + 1);
    CHECK(b3w_bao_slice_batch_layout(lens.data(), n_files, sf.data(), sc.data(), ns, first.data()) > 0, "the samples' slices");
    std::vector<uint8_t> slots(1024 * (uint64_t)ns, FILL);
    for (uint32_t i = 0; i < ns; ++i) {
      const File &f = files[sf[i]];
      uint64_t size = 0;
      CHECK(b3w_bao_slice(f.ob.data(), f.len, sc[i], nullptr, nullptr, &size) == B3W_OK && size == b3w_bao_slice_size(f.len, sc[i]), "sample %u: the size", i);
      std::vector<uint8_t> sl(size);
      CHECK(b3w_bao_slice(f.ob.data(), f.len, sc[i], f.len ? f.data.data() + 1024 * sc[i] : nullptr, sl.data(), &size) == B3W_OK, "sample %u: the slice", i);
      const bool hit = i % 3 == 1 && chunk_len(f, sc[i]);
      if (hit) sl[size - 1] ^= 1;
      int32_t st = -1;
      uint32_t got = 0;
      std::vector<uint8_t> one(chunk_len(f, sc[i]) ? chunk_len(f, sc[i]) : 1, FILL);
      CHECK(b3w_bao_slice_decode(sl.data(), size, f.len, sc[i], f.root, one.data(), &got, &st) == B3W_OK && st == (hit ? 1 : 0), "sample %u: decode", i);
      memcpy(slots.data() + 1024 * (uint64_t)i, one.data(), got);
      check_slot(slots, i, f, sc[i], hit, "samples");
    }
  }
  // ---- sets: a set a file, files ascending; slot = chunk_first + rank
  {
    std::vector<uint32_t> sf;
    std::vector<uint64_t> sa, sk;
    for (uint32_t f = 0; f < n_files; ++f) {
      const uint64_t n = files[f].n;
      if (n < 4) { sf.push_back(f); sa.push_back(n - 1); sk.push_back(1); continue; }
      for (uint64_t c = 1; c + 1 < n; c += n / 3 + 1) { sf.push_back(f); sa.push_back(c); sk.push_back(c + 2 < n ? 2 : 1); }
      if (sa.back() + sk.back() < n) { sf.push_back(f); sa.push_back(n - 1); sk.push_back(1); }
    }
    const uint32_t nr2 = (uint32_t)sf.size();
    SetList list;
    CHECK(b3w_int_set_list(lens.data(), n_files, sf.data(), sa.data(), sk.data(), nr2, list), "the sets: %s", list.why.c_str());
    std::vector<uint64_t> scf((size_t)nr2 + 1);
    uint32_t n_sets = 0;
    CHECK(b3w_bao_set_slice_batch_layout(lens.data(), n_files, sf.data(), sa.data(), sk.data(), nr2, nullptr, nullptr, scf.data(), nullptr, &n_sets) > 0 &&
          n_sets == list.sets.size() && scf[n_sets] == list.chunks && list.chunks == b3w_int_listed_chunks(sk.data(), nr2), "the sets' layout");
    for (int tamper = 0; tamper < 2; ++tamper) {
      std::vector<uint8_t> slots(1024 * list.chunks, FILL);
      for (uint32_t s = 0; s < n_sets; ++s) {
        const SetEnt &e = list.sets[s];
        const File &f = files[e.file];
        const uint32_t k = e.range_end - e.range_first;
        const uint64_t *a = sa.data() + e.range_first, *cnt = sk.data() + e.range_first;
        CHECK(e.chunk_first == scf[s], "set %u: chunk_first", s);
        const uint64_t size = b3w_bao_set_slice_size(f.len, a, cnt, k), wanted = (s + 1 < n_sets ? scf[s + 1] : list.chunks) - scf[s];
        std::vector<uint8_t> sl(size);
        CHECK(b3w_bao_set_slice(f.ob.data(), f.len, 0, a, cnt, k, f.len ? f.data.data() : nullptr, sl.data(), size) == (int64_t)size, "set %u: the slice", s);
        const uint64_t last = a[k - 1] + cnt[k - 1] - 1;    // (the last wanted chunk's bytes end the slice)
        const bool hit = tamper && chunk_len(f, last);
        if (hit) sl[size - 1] ^= 1;
        std::vector<uint8_t> part(1024 * wanted, FILL);
        std::vector<int32_t> cs(wanted, -1);
        int32_t st = -1;
        uint64_t fb = 0;
        CHECK(b3w_bao_set_slice_decode(sl.data(), size, f.len, a, cnt, k, f.root, part.data(), cs.data(), &st, &fb) == B3W_OK, "set %u: decode", s);
        CHECK(st == (hit ? 1 : 0) && fb == (hit ? last : ~0ull) && cs[wanted - 1] == (hit ? 1 : 0), "set %u: status %d", s, st);
        memcpy(slots.data() + 1024 * e.chunk_first, part.data(), part.size());
        uint64_t rank = 0;
        for (uint32_t i = 0; i < k; ++i)
          for (uint64_t c = a[i]; c < a[i] + cnt[i]; ++c, ++rank) check_slot(slots, e.chunk_first + rank, f, c, hit && c == last, "sets");
        CHECK(rank == wanted, "set %u: its wanted chunks", s);
      }
    }
  }
}

int main() {
  check_refusals();
  const uint64_t K = 1024;
  std::vector<File> files;
  uint32_t seed = 1;
  for (uint64_t len : std::vector<uint64_t>{0, 1, 1023, 1024, 1025, 3 * K + 17, 5 * K + 300, 64 * K + 999, 70 * K + 1, 1025 * K, (1ull << 20) + 300}) files.push_back(make_file(len, seed++));
  check_lists(files);
  for (const File &f : files) check_lists({f});              // and a file a call
  // one file of 2^30 chunks: the slots of its whole-file range need 2^40 bytes; nothing is made
  {
    const uint64_t n = 1ull << 30, len = n * K, a = 0;
    const uint32_t file = 0;
    SetList list;
    CHECK(b3w_int_set_list(&len, 1, &file, &a, &n, 1, list) && list.chunks == n && b3w_int_listed_chunks(&n, 1) == n, "2^30 chunks: the list");
    const std::string why = b3w_int_slots_wrong(reinterpret_cast<void *>(uintptr_t(16)), (1ull << 40) - 1, list.chunks);
    CHECK(why.find("1099511627776") != std::string::npos, "2^30 chunks: %s", why.c_str());
  }
  printf("bao_receive_packed_host_check: %ld checks passed, no sanitizer report\n", checks);
  return 0;
}
