// b3w_bao_tree.h — the bao arithmetic that the host calls (b3w_bao_host.cpp), the device entry points and the kernels (b3w_bao.hip,
// b3w_bao_have.hip) share: chunk and unit counts, sizes, places in the pre-order outboard and in a range slice, the packing of small
// files into waves, what a batch launches, and a chunk's and a subtree's CV on the host.  One definition each; compiles as HIP and as
// plain C++ (b3w_blake3_cv.h).  Not installed.  The inline pieces live in an anonymous namespace, a copy a file, as b3w_blake3_dev.h's.
#pragma once
#include <stdint.h>
#include <string.h>

#include "b3w_blake3_cv.h"

namespace {

constexpr uint32_t B3W_TILE = 1024;                      // chunks per tile = items per merge group
constexpr uint64_t RES_TB = (uint64_t)B3W_TILE * 1024;   // a tile's bytes
constexpr uint64_t RS_SHORT = 64;                        // range slices: ranges of at most this many chunks take rows of 64 chunks

inline uint64_t num_chunks(uint64_t len) { return len ? (len + 1023) / 1024 : 1; }
inline uint64_t chunk_bytes(uint64_t len, uint64_t c) { return len - c * 1024 < 1024 ? len - c * 1024 : 1024; }
inline uint32_t chunk_blocks(uint64_t len, uint64_t c) {
  const uint64_t bytes = chunk_bytes(len, c);
  return bytes ? (uint32_t)((bytes + 63) / 64) : 1;
}
// the units of a group outboard (groups of 1 << gl chunks, the last one ragged) and its bytes (b3w_bao_group_outboard_size; gl = 0:
// b3w_bao_outboard_size)
inline uint64_t n_units(uint64_t len, uint32_t gl) { return (num_chunks(len) + ((1ull << gl) - 1)) >> gl; }
inline uint64_t group_outboard_bytes(uint64_t len, uint32_t gl) { return 8 + 64 * (n_units(len, gl) - 1); }
inline uint64_t tiles_of(uint64_t len) { return (num_chunks(len) + B3W_TILE - 1) / B3W_TILE; }

// the chunks of the left subtree of a subtree over m >= 2 chunks: the largest power of two strictly below m
B3W_HD_INLINE uint64_t left_of(uint64_t m) { return 1ull << (63 - __builtin_clzll(m - 1)); }

// path_len with the split from a bit scan: the parent nodes above chunk c of a subtree over m chunks, its root included
B3W_HD_INLINE uint32_t depth_in(uint64_t c, uint64_t m) {
  uint32_t p = 0;
  for (; m > 1; ++p) {
    const uint64_t k = left_of(m);
    if (c < k) m = k; else { c -= k; m -= k; }
  }
  return p;
}

// the slice of chunk c, whose path has P nodes (b3w_bao_slice_size); the next slice start at or behind byte `end`: 8 modulo 16
inline uint64_t slice_bytes(uint64_t len, uint64_t c, uint32_t P) { return 8 + 64ull * P + chunk_bytes(len, c); }
inline uint64_t slice_start(uint64_t end) { return ((end + 7) & ~15ull) + 8; }

// pre-order position, relative to the root of a tree over `total` chunks, of its node over chunks [a, a + size); the host walks use it too
B3W_HD_INLINE uint64_t preorder_pos(uint64_t total, uint64_t a, uint64_t size) {
  uint64_t p = 0, lo = 0, cnt = total;
  while (cnt > 1 && !(lo == a && cnt == size)) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t k = 1ull << (63 - __clzll((long long)(cnt - 1)));
#else
    const uint64_t k = left_of(cnt);
#endif
    if (a < lo + k) { p += 1; cnt = k; } else { p += k; lo += k; cnt -= k; }
  }
  return p;
}

// ---- outboard diff: where the CV of a block of leaves is STORED (b3w_bao_outboard_diff, the diff kernel in b3w_bao_have.hip) ----------
// Leaves [a, a + size) of a tree over total > size leaves (a leaf: a unit of the outboard's own group_log), a a multiple of the power
// of two `full` >= size, size < full only where the block ends the tree: such a block is a subtree, and its CV is one half of its
// parent's node -> 2 * (that node's pre-order position) + (1: the right half).  The walk goes down from the root; from a complete
// subtree of 2^j leaves on the rest is arithmetic: going right from a node of height h skips the 2^(h-1) - 1 nodes of its left
// subtree, so the bits of the local index from the block's height + 1 up add themselves and every zero among them adds one.  32-bit:
// a file has at most 2^30 chunks here.
B3W_HD_INLINE uint32_t stored_half(uint32_t total, uint32_t a, uint32_t size, uint32_t full) {
  uint32_t p = 0, lo = 0, cnt = total;
  for (;;) {
    if (size == full && !(cnt & (cnt - 1)) && cnt > full) {
      const uint32_t t1 = (uint32_t)__builtin_ctz(full) + 1, j = (uint32_t)__builtin_ctz(cnt), up = (a - lo) >> t1;
      return 2 * (p + (up << t1) + (j - t1) - (uint32_t)__builtin_popcount(up)) + (((a - lo) >> (t1 - 1)) & 1);
    }
    const uint32_t k = 1u << (31 - __builtin_clz(cnt - 1));
    const bool left = a < lo + k;
    const uint32_t clo = left ? lo : lo + k, ccnt = left ? k : cnt - k;
    if (clo == a && ccnt == size) return 2 * p + (left ? 0 : 1);
    p += left ? 1 : k;
    lo = clo; cnt = ccnt;
  }
}
// is unit u (2^G chunks, the last one ragged) of a file of nb chunks SAME in a file of na chunks, as far as the counts say: it exists
// there, covers the same chunks, and is the whole file in both or in neither
B3W_HD_INLINE bool diff_unit_comparable(uint32_t na, uint32_t nb, uint32_t u, uint32_t G) {
  const uint64_t s = (uint64_t)u << G, e = s + (1ull << G);
  return s < na && (e < na ? e : na) == (e < nb ? e : nb) && (na <= (1u << G)) == (nb <= (1u << G));
}
// the byte of the outboard (of group_log gl <= G) of a file of n > 2^G chunks at which the CV of its unit u of 2^G chunks is stored
B3W_HD_INLINE uint64_t diff_cv_at(uint32_t n, uint32_t gl, uint32_t u, uint32_t G) {
  const uint32_t total = (n + ((1u << gl) - 1)) >> gl, full = 1u << (G - gl), a = u << (G - gl);
  return 8 + 32ull * stored_half(total, a, total - a < full ? total - a : full, full);
}
constexpr uint64_t DIFF_MAX_CHUNKS = 1ull << 30;         // a file of the diff: its node positions fit 32 bits

// ---- outboard delta: b's parent nodes that a does not hold (b3wit.h "outboard delta"; the delta kernels in b3w_bao_have.hip) -----------
// Both trees are over units of one group_log.  Everything the provider, the replica and their host mirrors decide about a node is
// decided here, once: the kernels and b3w_bao_host.cpp differ only in how they find a node's rank in the blob.
constexpr uint64_t DELTA_OK = ~0ull;                     // the key of a pair without a fault; a fault's key: 4 * node + status, the least wins
constexpr uint32_t DELTA_MALFORMED = 1, DELTA_BAD_HASH = 2, DELTA_NOT_HELD = 3;      // B3W_BAO_DELTA_* of b3wit.h (the entry points assert it)
B3W_HD_INLINE uint64_t delta_key(uint32_t node, uint32_t status) { return 4ull * node + status; }
B3W_HD_INLINE uint64_t delta_words(uint64_t units) { return (units - 1 + 63) / 64; }
B3W_HD_INLINE uint32_t left_of32(uint32_t m) { return 1u << (31 - __builtin_clz(m - 1)); }

B3W_HD_INLINE uint64_t delta_load64(const uint8_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *reinterpret_cast<const uint64_t *>(p);         // (every place of a blob and of an outboard is 8-byte aligned)
#else
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
#endif
}
// 32 bytes as 8 words; words: the place is a root's, 4-byte aligned only
B3W_HD_INLINE void delta_load_cv(const uint8_t *p, uint32_t w[8], bool words) {
#ifdef __HIP_DEVICE_COMPILE__
  if (words) {
    B3W_UNROLL
    for (int k = 0; k < 8; ++k) w[k] = reinterpret_cast<const uint32_t *>(p)[k];
  } else {
    B3W_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint64_t v = reinterpret_cast<const uint64_t *>(p)[k];
      w[2 * k] = (uint32_t)v; w[2 * k + 1] = (uint32_t)(v >> 32);
    }
  }
#else
  (void)words;
  memcpy(w, p, 32);
#endif
}
B3W_HD_INLINE bool delta_cv_is(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
  B3W_UNROLL
  for (int k = 0; k < 8; ++k) d |= a[k] ^ b[k];
  return d == 0;
}
B3W_HD_INLINE bool delta_cv_equal(const uint8_t *a, const uint8_t *b, bool words) {
  uint32_t x[8], y[8];
  delta_load_cv(a, x, words);
  delta_load_cv(b, y, words);
  return delta_cv_is(x, y);
}

// node p < total - 1 of the tree over `total` units: its span [lo, lo + cnt), its parent's position and the half of the parent's node
// that stores its CV (p = 0: neither)
struct DeltaNode { uint32_t lo, cnt, parent, side; };
B3W_HD_INLINE DeltaNode delta_node(uint32_t total, uint32_t p) {
  DeltaNode r{0, total, 0, 0};
  uint32_t pos = 0;
  while (pos != p) {
    const uint32_t k = left_of32(r.cnt);
    r.parent = pos;
    if (p < pos + k) { r.side = 0; pos += 1; r.cnt = k; } else { r.side = 1; pos += k; r.lo += k; r.cnt -= k; }
  }
  return r;
}
// does the tree over `total` units have a parent node over units [lo, lo + cnt), cnt >= 2?  -> its position, and 2 * (its parent's
// position) + (1: the right half) where its CV is stored (the root: 0)
B3W_HD_INLINE bool delta_find(uint32_t total, uint32_t lo, uint32_t cnt, uint32_t &pos, uint32_t &half) {
  uint32_t p = 0, l = 0, c = total;
  half = 0;
  for (;;) {
    if (l == lo && c == cnt) { pos = p; return true; }
    if (c <= cnt) return false;                            // (c > cnt >= 2 below)
    const uint32_t k = left_of32(c);
    half = 2 * p;
    if (lo < l + k) {
      if (lo + cnt > l + k) return false;                  // it straddles the split
      p += 1; c = k;
    } else { half += 1; p += k; l += k; c -= k; }
  }
}
// the byte of a's outboard that stores the CV of a's node over units [lo, lo + cnt), where a (na chunks, ua units) has such a node
// below its root and it covers the same chunks as in b (nb chunks); 0: a holds no such node.  pos_a: the node's position in a.
B3W_HD_INLINE uint64_t delta_held_at(uint32_t na, uint32_t nb, uint32_t ua, uint32_t g, uint32_t lo, uint32_t cnt, uint32_t &pos_a) {
  uint32_t half;
  if (!delta_find(ua, lo, cnt, pos_a, half) || pos_a == 0) return 0;
  const uint64_t end = (uint64_t)(lo + cnt) << g;
  if ((end < na ? end : na) != (end < nb ? end : nb)) return 0;
  return 8 + 32ull * half;
}

// one pair as both calls see it: a's outboard (null: the replica holds nothing), the two roots, the chunk and unit counts
struct DeltaSides {
  const uint8_t *ob_a;
  const uint8_t *root_a, *root_b;                          // (4-byte aligned)
  uint32_t na, nb, ua, ub, g;
};
// is b's root node SAME: equal chunk counts and equal roots
B3W_HD_INLINE bool delta_root_same(const DeltaSides &s) { return s.ob_a && s.na == s.nb && delta_cv_equal(s.root_a, s.root_b, true); }
// the provider's verdict: is node p < ub - 1 of b (outboard ob_b) SAME
B3W_HD_INLINE bool delta_node_same(const DeltaSides &s, const uint8_t *ob_b, uint32_t p) {
  if (p == 0) return delta_root_same(s);
  if (!s.ob_a) return false;
  const DeltaNode nd = delta_node(s.ub, p);
  uint32_t pos_a;
  const uint64_t at_a = delta_held_at(s.na, s.nb, s.ua, s.g, nd.lo, nd.cnt, pos_a);
  return at_a && delta_cv_equal(s.ob_a + at_a, ob_b + 8 + 64ull * nd.parent + 32 * nd.side, false);
}

// the replica's verdict on bit p < 64 * W of a blob (its first byte: blob; cap: the nodes its extent holds behind header and bitmap):
// DELTA_OK or the fault's key.  rank(q): the set bits of the bitmap below bit q.  A node is read only where its rank is below cap;
// a rank at or above cap means k or the bitmap's count is past the extent, which delta_check_head reports at node 0, the least key.
template <class Rank>
B3W_HD_INLINE uint64_t delta_check_node(const DeltaSides &s, const uint8_t *blob, uint64_t cap, uint32_t p, Rank rank) {
  const uint32_t nodes = s.ub - 1;
  const uint8_t *bitmap = blob + 16, *base = bitmap + 8 * delta_words(s.ub);
  const bool present = (delta_load64(bitmap + 8 * (p >> 6)) >> (p & 63)) & 1;
  if (p >= nodes) return present ? delta_key(p, DELTA_MALFORMED) : DELTA_OK;      // a pad bit
  if (!present) return p == 0 && !delta_root_same(s) ? delta_key(0, DELTA_MALFORMED) : DELTA_OK;
  const uint64_t r = rank(p);
  if (r >= cap) return DELTA_OK;
  const DeltaNode nd = delta_node(s.ub, p);
  if (p && !((delta_load64(bitmap + 8 * (nd.parent >> 6)) >> (nd.parent & 63)) & 1)) return delta_key(p, DELTA_MALFORMED);
  uint32_t m[16], h[8], o[8], want[8];
  delta_load_cv(base + 64 * r, m, false);
  delta_load_cv(base + 64 * r + 32, m + 8, false);
  iv(h);
  blake3_cv(h, m, 0, 0, 64, 4u | (p ? 0u : 8u), o);
  if (p) delta_load_cv(base + 64 * rank(nd.parent) + 32 * nd.side, want, false);      // (the parent is present and in front: its rank is below r)
  else delta_load_cv(s.root_b, want, true);
  if (!delta_cv_is(o, want)) return delta_key(p, DELTA_BAD_HASH);
  const uint32_t k = left_of32(nd.cnt);
  uint64_t key = DELTA_OK;
  for (uint32_t side = 0; side < 2; ++side) {              // an absent child that is a parent subtree: a must hold it
    const uint32_t clo = side ? nd.lo + k : nd.lo, ccnt = side ? nd.cnt - k : k, pc = side ? p + k : p + 1;
    if (ccnt < 2 || ((delta_load64(bitmap + 8 * (pc >> 6)) >> (pc & 63)) & 1)) continue;
    uint32_t pos_a, cv_a[8];
    const uint64_t at_a = s.ob_a ? delta_held_at(s.na, s.nb, s.ua, s.g, clo, ccnt, pos_a) : 0;
    bool held = at_a != 0;
    if (held) {
      delta_load_cv(s.ob_a + at_a, cv_a, false);
      held = delta_cv_is(cv_a, m + 8 * side);
    }
    if (!held && delta_key(pc, DELTA_NOT_HELD) < key) key = delta_key(pc, DELTA_NOT_HELD);
  }
  return key;
}
// the blob's header against the call's len_b, the bitmap's count and the extent
B3W_HD_INLINE uint64_t delta_check_head(const uint8_t *blob, uint64_t len_b, uint64_t cap, uint64_t count) {
  const uint64_t k = delta_load64(blob + 8);
  return delta_load64(blob) != len_b || k != count || k > cap ? delta_key(0, DELTA_MALFORMED) : DELTA_OK;
}
// where the replica's outboard takes node p < ub - 1 from when it is absent from the blob: the byte of a's outboard (the pair passed)
B3W_HD_INLINE uint64_t delta_copy_from(const DeltaSides &s, uint32_t p) {
  const DeltaNode nd = delta_node(s.ub, p);
  uint32_t pos_a = 0, half;                                // (a passed pair: every absent node lies in a subtree a holds in the same shape;
  return s.ob_a && delta_find(s.ua, nd.lo, nd.cnt, pos_a, half) ? 8 + 64ull * pos_a : 0;      // 0: it does not, nothing is copied)
}

// ---- range slices: places (the format is described at the range kernels in b3w_bao.hip) ------------------------------------------------
// U(a, c), a <= c < n
B3W_HD inline uint64_t range_nodes(uint64_t n, uint64_t a, uint64_t c) {
  uint64_t u = 0, lo = 0, m = n;
  while (m > 1) {                                          // the nodes above the split: both ends go the same way
    const uint64_t k = left_of(m);
    if (c < lo + k) m = k;
    else if (a >= lo + k) { lo += k; m -= k; }
    else break;
    ++u;
  }
  if (m <= 1) return u;                                    // (a == c: the chunk's path)
  const uint64_t k = left_of(m);
  ++u;                                                     // the split node: a on its left, c on its right
  for (uint64_t l = lo, s = k; s > 1;) {                   // a's path below it: what lies right of a is inside
    const uint64_t kk = left_of(s);
    ++u;
    if (a < l + kk) { u += s - kk - 1; s = kk; } else { l += kk; s -= kk; }
  }
  for (uint64_t l = lo + k, s = m - k; s > 1;) {           // c's path below it: what lies left of c is inside
    const uint64_t kk = left_of(s);
    ++u;
    if (c >= l + kk) { u += kk - 1; l += kk; s -= kk; } else s = kk;
  }
  return u;
}

// the place within the slice of chunks [a, ..) of a file of n chunks of chunk c >= a, and of the node over [lo, lo + size) that meets it
B3W_HD_INLINE uint64_t range_chunk_at(uint64_t n, uint64_t a, uint64_t c) { return 8 + 64 * range_nodes(n, a, c) + 1024 * (c - a); }
B3W_HD_INLINE uint64_t range_node_at(uint64_t n, uint64_t a, uint64_t lo, uint64_t size) {
  const uint64_t c0 = lo > a ? lo : a;
  return range_chunk_at(n, a, c0) - 64ull * depth_in(c0 - lo, size);
}

inline uint64_t range_slice_bytes(uint64_t len, uint64_t n, uint64_t a, uint64_t k) {     // (a + k <= n, k >= 1)
  const uint64_t end = (a + k) * 1024 < len ? (a + k) * 1024 : len;
  return 8 + 64 * range_nodes(n, a, a + k - 1) + (end - a * 1024);
}
// the rows of a range: the blocks of 64 (short ranges) or 1 024 chunks it touches
inline uint64_t range_rows(uint64_t a, uint64_t k) {
  const uint64_t B = k <= RS_SHORT ? 64 : B3W_TILE;
  return (a + k - 1) / B - a / B + 1;
}

// ---- set slices: one slice for the union S of a file's ascending, disjoint runs (the format: b3wit.h "set slices") -------------------
// The nodes a chunk adds to the slice are those of its path that do not hold the wanted chunk p before it: the path below the node where
// the two part.  j = the highest bit in which p < a differ: a's side of that node is the aligned 2^j chunks from s = (a >> j) << j, cut
// off at n, and a's path inside it has j nodes where it is whole.  O(1) but for the cut-off subtrees on the file's right edge.
inline uint32_t new_nodes(uint64_t n, uint64_t p, uint64_t a) {
  const uint32_t j = 63 - (uint32_t)__builtin_clzll(p ^ a);
  const uint64_t s = (a >> j) << j;
  return s + (1ull << j) <= n ? j : depth_in(a - s, n - s);
}
// what the chunks a + 1 .. a + k - 1 of a run add: U(a, a + k - 1) - depth(a).  Chunk c adds ctz(c) nodes behind c - 1 wherever its
// aligned 2^ctz(c) chunks are whole - everywhere in front of the largest power of two at or below n - and the sum of ctz over (a, p] is
// (p - popcount p) - (a - popcount a); a run that reaches further takes the walk.
inline uint64_t run_inner(uint64_t n, uint64_t a, uint64_t k) {
  if (k == 1) return 0;
  const uint64_t p = a + k - 1;
  if (p < (1ull << (63 - __builtin_clzll(n)))) return (p - (uint64_t)__builtin_popcountll(p)) - (a - (uint64_t)__builtin_popcountll(a));
  return range_nodes(n, a, p) - depth_in(a, n);
}
// SetRuns walks one file's runs in order: ufirst = U_S of the run's first chunk, rank = the wanted chunks in front of the run, so
//   U_S(c) = ufirst + run_inner(a, c - a + 1) for c in the run from a;   the next run's ufirst = U_S(p) + new_nodes(p, its first chunk).
// No step a chunk, and O(1) a run away from the file's ragged right edge.
inline uint64_t set_nodes(uint64_t n, uint64_t ufirst, uint64_t a, uint64_t c) { return ufirst + run_inner(n, a, c - a + 1); }
struct SetRuns {
  uint64_t n, ufirst, rank = 0;
  SetRuns(uint64_t n_, uint64_t a0) : n(n_), ufirst(depth_in(a0, n_)) {}
  void next(uint64_t a, uint64_t k, uint64_t a_next) {
    ufirst += run_inner(n, a, k) + new_nodes(n, a + k - 1, a_next);
    rank += k;
  }
};
// is (first, count)[0 .. k) the list of one file of n chunks: no empty run, none past the file, ascending and disjoint (touching allowed)?
// -> null, or what is wrong with run *bad
inline const char *set_runs_wrong(uint64_t n, const uint64_t *first, const uint64_t *count, uint64_t k, uint64_t *bad) {
  for (uint64_t i = 0; i < k; ++i) {
    *bad = i;
    if (count[i] == 0) return "it has no chunk";
    if (first[i] >= n || count[i] > n - first[i]) return "it reaches past its file's chunk count";
    if (i && first[i] < first[i - 1] + count[i - 1]) return first[i] < first[i - 1] ? "the list is not ascending by (file, first chunk)" : "it overlaps the range before it: the list is not disjoint";
  }
  return nullptr;
}
// the bytes of the set slice of these (valid) runs of a file of len bytes; ufirst / rank (may be null): SetRuns' state at every run
inline uint64_t set_slice_bytes(uint64_t len, const uint64_t *first, const uint64_t *count, uint64_t k, uint64_t *ufirst = nullptr, uint64_t *rank = nullptr) {
  const uint64_t n = num_chunks(len);
  SetRuns w(n, first[0]);
  for (uint64_t i = 0;; ++i) {
    if (ufirst) { ufirst[i] = w.ufirst; rank[i] = w.rank; }
    if (i + 1 == k) break;
    w.next(first[i], count[i], first[i + 1]);
  }
  const uint64_t a = first[k - 1], e = a + count[k - 1], chunks = w.rank + count[k - 1];
  return 8 + 64 * set_nodes(n, w.ufirst, a, e - 1) + 1024 * chunks - (e == n ? 1024 - chunk_bytes(len, n - 1) : 0);
}
// the first run of the (valid) list that ends behind chunk c, k for none; S meets [lo, hi) iff that run starts before hi
inline uint64_t set_run_behind(const uint64_t *first, const uint64_t *count, uint64_t k, uint64_t c) {
  uint64_t a = 0, b = k;
  while (a < b) {
    const uint64_t mid = (a + b) / 2;
    if (first[mid] + count[mid] > c) b = mid; else a = mid + 1;
  }
  return a;
}
inline bool set_meets(const uint64_t *first, const uint64_t *count, uint64_t k, uint64_t lo, uint64_t hi) {
  const uint64_t i = set_run_behind(first, count, k, lo);
  return i < k && first[i] < hi;
}
// the rows of a set whose first and last wanted chunks are c0 and c1: one or two of 64 chunks where the two lie in the same or in
// adjacent aligned 64-chunk blocks, else a row of 1 024 per touched tile (counted by the caller: it needs the runs)
inline bool set_is_short(uint64_t c0, uint64_t c1) { return c1 / 64 - c0 / 64 <= 1; }

// ---- step records of a run of chunks: where a chunk's rows start (b3w_sample_rows_ranges, the range planner's table) ------------------
// the sum of depth_in(i, n) over the chunks i < c of a tree over n chunks, c <= n, in the manner of range_nodes: the walk follows chunk
// c's path, and a left subtree of k = 2^j chunks that lies wholly in front of c gives k (d + 1 + j), d the nodes above it: O(depth)
inline uint64_t path_sum(uint64_t n, uint64_t c) {
  uint64_t s = 0;
  for (uint64_t d = 0; c; ++d) {
    if (n == 1) return s + d;                              // (c == 1: the subtree's only chunk)
    const uint64_t k = left_of(n), each = d + 1 + (uint64_t)__builtin_ctzll(k);
    if (c <= k) return s + c * each;
    s += k * each;
    c -= k; n -= k;
  }
  return s;
}
// the record rows of the chunks in front of chunk c <= n of a file of len bytes, n chunks: a row a block (every chunk but the last has
// sixteen) and one a path node, as b3w_sample_rows_batch counts them chunk by chunk
inline uint64_t rows_before(uint64_t len, uint64_t n, uint64_t c) {
  return 16 * (c < n ? c : n - 1) + (c == n ? chunk_blocks(len, n - 1) : 0) + path_sum(n, c);
}
// do the low bits of chunk c's index spell its path through the tree over n chunks (b3w_plan_path_provable, with the split from a bit scan)?
B3W_HD_INLINE bool path_provable(uint64_t c, uint64_t n) {
  const uint32_t P = depth_in(c, n);
  uint64_t cc = c, m = n;
  for (uint32_t j = 0; j < P; ++j) {
    const uint64_t k = left_of(m);
    const bool left = cc < k;
    if (left) m = k; else { cc -= k; m -= k; }
    if (left != (((c >> (P - 1 - j)) & 1) == 0)) return false;
  }
  return true;
}

// ---- files of at most 64 chunks share waves, in file order, as many as fit ----------------------------------------------------------
// add(n): the first lane of a file of n chunks in its wave; `first` (may be null: counting) takes every wave's first file, and
// close() the end of the last wave
struct SmallPack {
  uint64_t files = 0, waves = 0, fill = 64;              // fill: lanes taken in the current wave (none open yet)
  uint32_t *first = nullptr;
  uint32_t add(uint64_t n) {
    if (fill + n > 64) { if (first) first[waves] = (uint32_t)files; waves++; fill = 0; }
    const uint32_t lane = (uint32_t)fill;
    fill += n;
    files++;
    return lane;
  }
  void close() { if (first && files) first[waves] = (uint32_t)files; }
  uint64_t first_bytes() const { return files ? (waves + 1) * 4 : 0; }
};

// what a batch of these lengths launches: the small files' waves; the others take a workgroup per tile (big); files of more than one
// tile a merge workgroup per 1 024 tiles (groups), files of more than 1 024 tiles one more over those (tops)
struct BatchCounts { uint64_t small, waves, big, big_wgs, merged, groups, tops; bool too_long; };
inline BatchCounts batch_counts(const uint64_t *lens, uint32_t n_files) {
  BatchCounts k{};
  SmallPack pack;
  for (uint32_t f = 0; f < n_files; ++f) {
    const uint64_t n = num_chunks(lens[f]);
    if (n <= 64) { (void)pack.add(n); continue; }
    const uint64_t tiles = (n + B3W_TILE - 1) / B3W_TILE, groups = (tiles + B3W_TILE - 1) / B3W_TILE;
    k.big++; k.big_wgs += tiles;
    if (tiles > 1) { k.merged++; k.groups += groups; }
    if (groups > 1) k.tops++;
    if (groups > B3W_TILE) k.too_long = true;
  }
  k.small = pack.files; k.waves = pack.waves;
  return k;
}

// verification's scratch entries: one per tile of the files of more than one tile, one per group of 1 024 tiles of the files of more
// than one group
inline uint64_t verify_entries(const uint64_t *lens, uint32_t n_files, uint64_t *tile_ents) {
  uint64_t tiles_sum = 0, groups_sum = 0;
  for (uint32_t f = 0; f < n_files; ++f) {
    const uint64_t tiles = tiles_of(lens[f]), groups = (tiles + B3W_TILE - 1) / B3W_TILE;
    if (tiles > 1) tiles_sum += tiles;
    if (groups > 1) groups_sum += groups;
  }
  if (tile_ents) *tile_ents = tiles_sum;
  return tiles_sum + groups_sum;
}

// resize: scratch slots of a listed file at its new length: its tiles' CVs, then its spans' past 1 GiB; none for a file of one tile
inline uint64_t resize_slots(uint64_t new_len) {
  const uint64_t tiles = tiles_of(new_len);
  return tiles > 1 ? tiles + (tiles > B3W_TILE ? (tiles + B3W_TILE - 1) / B3W_TILE : 0) : 0;
}

// ---- hashing on the host ------------------------------------------------------------------------------------------------------------
// the CV of a chunk (the kernels' chunk_cv loop over blake3_cv)
inline void host_chunk_cv(const uint8_t *src, uint32_t bytes, uint64_t c, uint32_t root, uint32_t h[8]) {
  const uint32_t nb = bytes ? (bytes + 63) / 64 : 1;
  iv(h);
  for (uint32_t j = 0; j < nb; ++j) {
    const uint32_t bb = bytes - j * 64 < 64 ? bytes - j * 64 : 64;
    uint32_t m[16] = {}, o[8];
    for (uint32_t q = 0; q < bb; ++q) m[q / 4] |= (uint32_t)src[j * 64 + q] << (8 * (q & 3));
    blake3_cv(h, m, (uint32_t)c, (uint32_t)(c >> 32), bb, (j == 0 ? 1u : 0u) | (j == nb - 1 ? 2u | root : 0u), o);
    for (int k = 0; k < 8; ++k) h[k] = o[k];
  }
}

// BLAKE3's tree over the chunks [first, first + cnt) of a file of `len` bytes whose chunk base_chunk lies at `base` (root: they are
// the whole file)
inline void host_subtree_cv(const uint8_t *base, uint64_t base_chunk, uint64_t len, uint64_t first, uint64_t cnt, bool root, uint32_t h[8]) {
  if (cnt == 1) {
    host_chunk_cv(base + (first - base_chunk) * 1024, (uint32_t)chunk_bytes(len, first), first, root ? 8u : 0u, h);
    return;
  }
  const uint64_t k = left_of(cnt);
  uint32_t m[16], ivv[8];
  host_subtree_cv(base, base_chunk, len, first, k, false, m);
  host_subtree_cv(base, base_chunk, len, first + k, cnt - k, false, m + 8);
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, 4u | (root ? 8u : 0u), h);
}

}  // namespace
