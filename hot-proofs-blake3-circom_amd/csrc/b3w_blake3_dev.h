// b3w_blake3_dev.h — BLAKE3 device code shared by the chained-mode planner (b3w_plan.hip) and the bao outboard / sampled-path
// planner (b3w_bao.hip): the compression, the four-lanes-a-chunk compression and BLAKE3's tree shape (path lengths, the right
// spine of an incomplete tree).  Everything lives in an anonymous namespace: each file that includes it gets its own copy of the
// device code, and the planner's kernels compile to the same code as before the move.  The compression itself, iv and path_len
// are in b3w_blake3_cv.h, which host-only files include without this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "b3w_blake3_cv.h"

namespace {

// ---- the leaf planner, four lanes per chunk (r05) ------------------------------------------------------------------
// A chunk's 16 blocks chain through the chaining value: 16 compressions one after the other, 33 us with one thread per chunk — in
// front of the first witness kernel of every pass (7 % of a rank's share of a 1 MiB pass at 8 ranks).  Four lanes share a
// compression the way the witness kernels' TRACE phase does: lane `col` of a quad holds column col of the state, the diagonal
// step is the column step after a quad rotate (DPP), the block's 16 message words lie in LDS and every lane picks the two a G needs
// by the round's schedule.  Same records, a third of the latency.
template <int P0, int P1, int P2, int P3>
__device__ __forceinline__ uint32_t plan_quad_perm(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, P0 | (P1 << 2) | (P2 << 4) | (P3 << 6), 0xF, 0xF, false);
}
__device__ __forceinline__ void plan_g(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t x, uint32_t y) {
  a = a + b + x; d = rotr(d ^ a, 16);
  c = c + d;     b = rotr(b ^ c, 12);
  a = a + b + y; d = rotr(d ^ a, 8);
  c = c + d;     b = rotr(b ^ c, 7);
}
// message schedule of round r, 4 bits per entry: round r uses m[PERM_r[j]] in place of m[j]
__host__ __device__ constexpr uint64_t plan_sched(int r) {
  const int sigma[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  int p[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  for (int i = 0; i < r; i++) {
    int q[16] = {};
    for (int j = 0; j < 16; j++) q[j] = p[sigma[j]];
    for (int j = 0; j < 16; j++) p[j] = q[j];
  }
  uint64_t v = 0;
  for (int j = 0; j < 16; j++) v |= (uint64_t)p[j] << (4 * j);
  return v;
}
template <int R>
__device__ __forceinline__ void plan_quad_round(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, const uint32_t *M, int col) {
  constexpr uint64_t P = plan_sched(R);
  plan_g(a, b, c, d, M[(P >> (8 * col)) & 15], M[(P >> (8 * col + 4)) & 15]);
  b = plan_quad_perm<1, 2, 3, 0>(b); c = plan_quad_perm<2, 3, 0, 1>(c); d = plan_quad_perm<3, 0, 1, 2>(d);
  plan_g(a, b, c, d, M[(P >> (32 + 8 * col)) & 15], M[(P >> (36 + 8 * col)) & 15]);
  b = plan_quad_perm<3, 0, 1, 2>(b); c = plan_quad_perm<2, 3, 0, 1>(c); d = plan_quad_perm<1, 2, 3, 0>(d);
}
// lane col: in h_lo = h[col], h_hi = h[4 + col]; out the same words of the compression's first eight output words
__device__ __forceinline__ void plan_quad_cv(uint32_t &h_lo, uint32_t &h_hi, const uint32_t *M, int col, uint32_t t0, uint32_t t1, uint32_t b, uint32_t dflag) {
  const uint32_t IVc = col == 0 ? 0x6A09E667u : col == 1 ? 0xBB67AE85u : col == 2 ? 0x3C6EF372u : 0xA54FF53Au;
  uint32_t a = h_lo, bb = h_hi, c = IVc, d = col == 0 ? t0 : col == 1 ? t1 : col == 2 ? b : dflag;
  plan_quad_round<0>(a, bb, c, d, M, col); plan_quad_round<1>(a, bb, c, d, M, col); plan_quad_round<2>(a, bb, c, d, M, col);
  plan_quad_round<3>(a, bb, c, d, M, col); plan_quad_round<4>(a, bb, c, d, M, col); plan_quad_round<5>(a, bb, c, d, M, col);
  plan_quad_round<6>(a, bb, c, d, M, col);
  h_lo = a ^ c;
  h_hi = bb ^ d;
}

// ---- parent steps of every chunk path, any chunk count ----------------------------------------------------------
// BLAKE3's tree over n chunks (left subtree = the largest power of two below the count) is a right spine of complete
// subtrees: seg[0] (the largest, chunks 0 ..), seg[1], ... seg[last]; suffix[i] = the node over seg[i] .. seg[last]
// (suffix[0] = the root, suffix[last] = seg[last], suffix[i] = parent(seg[i], suffix[i+1])).  The level arrays of
// b3w_chain_tree_device hold every complete subtree (level t, node index), its scratch chain the suffix nodes.
//
// The step circuit takes left/right at height g from bit g of chunk_idx (Blake3GetDownLeftPath,
// circuits/blake3_nova.circom:47-84), and the reference's driver picks the PathNode's sibling by the same bit
// (blake3_hash.rs:63-78: bit clear -> the node's RIGHT child CV, bit set -> its LEFT child CV).  That is the leaf's true
// sibling exactly when the leaf's real path spells the low bits of its index — always in a complete tree; in an
// incomplete one only for some leaves (those of seg[0], and of later segments whose position happens to agree).  For
// the others the reference hands the circuit the node's other child, i.e. the path child's own CV, and the fold ends in a
// value that is not BLAKE3(input) (tests/golden/incomplete_trees.nova_vesta.json: the reference WASM driven that way).
// This kernel reproduces the reference's records for every leaf — running value computed the way the circuit does —
// and b3w_plan_path_provable says which paths end in the root.
struct B3wSpine {
  uint32_t nseg;                 // segments on the spine (1 = complete tree)
  uint32_t level[64];            // seg i = complete subtree of 2^level[i] chunks
  uint32_t plen[64];             // path length of its chunks
  uint64_t lo[64];               // first chunk
  uint64_t seg_off[64];          // word offset of the segment's CV in the levels buffer
  uint64_t suf_off[64];          // word offset of suffix[i]'s CV (i >= 1)
  uint64_t row_base[64];         // parent-step row of chunk lo[i]'s first parent step (rows of chunk 0 start at 0)
};

__host__ inline uint64_t level_off_words(uint64_t n, uint32_t t) {
  uint64_t off = 0;
  for (uint32_t l = 0; l < t; ++l) off += (n >> l) * 8;
  return off;
}

__host__ inline B3wSpine spine_of(uint64_t n) {
  B3wSpine sp{};
  // pairwise levels: an odd node out at level l is a complete subtree of 2^l chunks that waits (a "carry")
  uint32_t carry_level[64];
  uint64_t carry_node[64];
  uint32_t nc = 0, l = 0;
  uint64_t count = n;
  while (count > 1) {
    if (count & 1) { carry_level[nc] = l; carry_node[nc] = count - 1; nc++; }
    count >>= 1;
    l++;
  }
  sp.nseg = nc + 1;
  sp.level[0] = l; sp.lo[0] = 0; sp.seg_off[0] = level_off_words(n, l);
  for (uint32_t i = 0; i < nc; ++i) {                     // root-down order = decreasing size = reverse carry order
    const uint32_t k = nc - 1 - i;
    sp.level[1 + i] = carry_level[k];
    sp.lo[1 + i] = carry_node[k] << carry_level[k];
    sp.seg_off[1 + i] = level_off_words(n, carry_level[k]) + carry_node[k] * 8;
  }
  const uint32_t last = nc;
  const uint64_t scratch = 2 * n * 8;                     // b3w_chain_tree_device: suffix[last - i] = scratch[i - 1], i = 1 .. last - 1
  for (uint32_t i = 1; i < last; ++i) sp.suf_off[i] = scratch + (uint64_t)(last - i - 1) * 8;
  sp.suf_off[last] = sp.seg_off[last];
  uint64_t row = 0;
  for (uint32_t i = 0; i <= last; ++i) {
    sp.plen[i] = sp.level[i] + (last == 0 ? 0 : (i == last ? last : i + 1));
    sp.row_base[i] = row;
    row += (uint64_t)sp.plen[i] << sp.level[i];
  }
  return sp;
}

__host__ __device__ inline uint32_t seg_of(const B3wSpine &sp, uint64_t c) {
  uint32_t s = 0;
  while (s + 1 < sp.nseg && c >= sp.lo[s + 1]) s++;
  return s;
}

}  // namespace
