// b3w_bao.hip — bao outboards of device-resident preimages, and the step records of challenged chunk paths planned from an
// outboard plus the challenged chunks' bytes alone.
//
// Format (bao 0.12 as the reference's hash_with_path consumes it, rust_fold/src/blake3_hash.rs:17-93; 1 KiB chunks, BLAKE3's tree:
// the left subtree holds the largest power of two of chunks strictly below the count):
//   outboard = 8-byte little-endian content length, then the n_chunks - 1 parent nodes in pre-order, 64 bytes each
//              (left child CV || right child CV, 8 little-endian words each)
//   pre-order: the root is node 0; a node at position p over m chunks (k = largest power of two below m) has its left subtree
//              from p + 1 and its right subtree from p + k
//   slice of chunk c = the header, the path's nodes root first, the chunk's bytes
//
//   b3w_bao_cv_kernel        one lane per chunk: 1 KiB in, its chaining value out (no step records) — the throughput shape
//   b3w_bao_cv_quad_kernel   four lanes per chunk (the leaf planner's quad compression): small chunk counts, where latency counts
//   (the tree)               b3w_chain_tree_device: the chain's own level arrays, spine and root
//   b3w_bao_emit_kernel      one thread per parent node: its two child CVs from the level arrays to its pre-order position
//   b3w_bao_tile_kernel      a batch of files: one workgroup per tile of 1 024 chunks, chunk CVs and the tile's tree in LDS, nodes straight to
//   b3w_bao_merge_kernel     their pre-order places; the tree over the tile CVs, one workgroup per 1 024 of them (see "batches of files")
//   b3w_sample_plan_kernel   one thread per challenged chunk: its leaf records from its bytes, its path verified top down against the
//                            root the way bao's decoder does, its parent records bottom up with the outboard's CVs
//   b3w_bao_*_group_kernel   the three batch kernels writing GROUP outboards: the tree over chunk groups of 1 << gl chunks, every node over at
//                            most a group's chunks computed and not stored ("outboards over chunk groups" in b3wit.h)
//   b3w_sample_plan_group_kernel  a challenged chunk from a group outboard and its group's bytes: a lane per chunk of the group, the group's
//                            tree merged in LDS, the stored part of the path verified across the sample's lanes, the same records
//   b3w_bao_slice_kernel     the bao slices of challenged chunks gathered from full outboards, 16 lanes a sample
//   b3w_bao_slice_group_kernel  the same standard slices from GROUP outboards: the group planner's lanes and LDS merge, every node of the
//                            path inside the group stored whole before its level's merge
//   b3w_sample_plan_slices_kernel  the step records planned from slices alone (no outboard): a sample over several lanes, the path's nodes
//                            checked side by side, the parent records without the running-h chain where that chain is redundant
//   b3w_*_arena_kernel       the batch planner, the group planner and the two slice kernels with the samples' bytes read where the files lie
//                            in the arena (any byte alignment) instead of from a gathered copy: the same bodies, the byte source a parameter
//   b3w_bao_verify_*_kernel  whole files against their outboards: the three batch kernels with every store of a node turned into a check of
//                            the stored node, the storey above the tiles first; a status per chunk or chunk group ("verification")
//   b3w_bao_stream_*_kernel  one file whose bytes arrive in windows of whole tiles: the tile, merge and verify kernels with the file's entry
//                            by value and the tiles' bytes taken from the window ("streamed files")
//   b3w_bao_stream_*_many_*  the windows (and the finishes) of many stream sessions as one grid: the stream kernels with the entry's row
//                            of a table in place of the arguments by value ("many stream sessions in one launch")
//   b3w_bao_stream_open_*    a file whose length is known only at finish: full tiles hashed into tile-local blocks of a staging area, and
//                            the blocks moved to their pre-order places once the length is known ("open-length sessions")
//                            (b3w_bao_stream_open_relocate_many_kernel: the blocks of many sessions moved in one grid)
//   b3w_bao_range_*_kernel   the slice of a RUN of chunks (bao's general slice, every shared node once) extracted from the arena and the
//                            outboards and taken in again, a row per (range, block of 64 or 1 024 chunks) ("range slices", at the end)
//   b3w_sample_plan_range_kernel  the step records of a RUN of challenged chunks planned from its range slice alone, on the same rows:
//                            b3w_sample_plan_slices_kernel's records and statuses for every chunk's projection (behind the range kernels)
//   b3w_bao_*_packed_kernel  the update's and the ranged verification's tile kernels and the range-slice provider for files that are NOT
//                            resident: the same bodies, the listed chunks read slot by slot from a packed buffer that holds them alone,
//                            a lane's place its rank among the listed chunks, its counter and length its chunk's ("sparse calls from
//                            packed chunk bytes" in b3wit.h)
//   b3w_bao_set_*_kernel     the slice of the union of a file's runs, served (from the arena, or packed: b3w_bao_set_slice_packed_kernel)
//                            and taken in, a row per (set, block with a wanted chunk) carrying the mask ("set slices", the last section)
//   b3w_sample_plan_set_kernel    the step records of every wanted chunk planned from the set slice alone, on the set receiver's rows
//
// The routes (batch table, one streamed file by value, a table of sessions, update / ranges / resize rows) differ only in where a file's
// entry comes from.  Each kernel, or its *_body wrapper, finds its entry and calls one of the bodies every route shares:
//   put_cv, header_is, find_first, preorder_pos (host and device), node_pos / node_at       the small pieces
//   lane_chunk_cv / tile_chunk_cvs      a lane's chunk, a tile's chunks, hashed into LDS
//   tree_levels                         the level loop over a tree in LDS; merge_in_lds and verify_in_lds hand it their work on a pair
//                                       (update_in_lds and ranges_in_lds keep the loop written out: it measured slower for them)
//   tile_outboard, merge_storey         a tile's outboard and the storey above the tiles (batch, stream, many)
//   verify_tile, verify_upper           the same two storeys of verification (batch, stream, many)
//   small_lane, small_levels, small_verify   the packed wave of files of at most 64 chunks (outboards, verify, ranged verify)
//   block_piece, move_piece, block_cv   the relocation of a full tile's block (open sessions, many sessions, resize)
//
// Behind the device code comes the host side of the calls that launch it: first what the entry points share (one refusal path, one
// launch epilogue for each staging kind, one builder for the sample table and one for the whole-batch tables, the small-file packer of
// b3w_bao_tree.h), then the entry points, route by route, each route's own helpers in front of it.  The calls that touch no device (sizes, layouts, the host mirrors) are b3w_bao_host.cpp; the
// arithmetic both need (B3W_TILE, preorder_pos, left_of, the places in a range slice) is b3w_bao_tree.h.
#include "b3w_internal.h"
#include "b3w_blake3_dev.h"
#include "b3w_bao_plan.h"

namespace {

// ---- the step records (b3wit.h batch input format) --------------------------------------------------------------------
// The same words b3w_plan_leaf_kernel and plan_path (b3w_plan.hip) write for a chunk: the sampled path's records must equal the
// chain planner's row for row (tests/test_gpu_bao.py), so these restate those loops for one chunk whose sibling CVs come from
// the outboard instead of the level arrays.
// the leaf steps of one chunk of `bytes` bytes (<= 1024) with P parents above it: one record per block into rec (32 words each) and the
// chunk's chaining value into h (with P == 0 it is the ROOT-flagged output: the hash words of a one-chunk input)
__device__ __forceinline__ void plan_leaf_chunk(const uint8_t *src, uint32_t bytes, uint64_t c, uint32_t P, uint32_t *rec, uint32_t h[8]) {
  const uint32_t n_blocks = bytes ? (bytes + 63) / 64 : 1;
  iv(h);
  for (uint32_t j = 0; j < n_blocks; ++j) {
    const uint32_t bb = bytes - j * 64 < 64 ? bytes - j * 64 : 64;
    uint32_t m[16];
    if (bb == 64 && ((uintptr_t)src & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) m[k] = reinterpret_cast<const uint32_t *>(src + j * 64)[k];
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        uint32_t w = 0;
        for (int q = 0; q < 4; ++q) { const uint32_t p = k * 4 + q; if (p < bb) w |= (uint32_t)src[j * 64 + p] << (8 * q); }
        m[k] = w;
      }
    }
    uint32_t *r = rec + j * 32;
    r[0] = n_blocks; r[1] = j;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[2 + k] = h[k];
    r[10] = (uint32_t)c; r[11] = (uint32_t)(c >> 32);
    r[12] = P + 1; r[13] = P + 1; r[14] = P;              // leaf_depth, total_depth, depth (blake3_circuit.rs:83-110)
#pragma unroll
    for (int k = 0; k < 16; ++k) r[15 + k] = m[k];
    r[31] = bb;
    // flags as Blake3GetFlag assigns them (circuits/blake3_nova.circom:122-167)
    const uint32_t last = j == n_blocks - 1;
    const uint32_t d = (j == 0 ? 1u : 0u) | (last ? 2u : 0u) | ((last && P == 0) ? 8u : 0u);
    uint32_t o[8];
    blake3_cv(h, m, (uint32_t)c, (uint32_t)(c >> 32), bb, d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = o[k];
  }
}

// one parent step of chunk c's path (height g: bit_left = bit g of c is clear, depth = plen - 1 - g): its record into r, and h, the
// running value, becomes the step's h_out.  m8 = the CV the reference's driver hands the circuit at that height (blake3_hash.rs:63-78).
__device__ __forceinline__ void plan_parent_step(uint32_t *r, uint32_t h[8], const uint32_t *m8, bool bit_left, uint64_t c, uint32_t n_blocks,
                                                 uint32_t plen, uint32_t depth) {
  r[0] = n_blocks; r[1] = n_blocks;                       // block_count stays at n_blocks on parent steps (blake3_nova.circom:251)
#pragma unroll
  for (int k = 0; k < 8; ++k) r[2 + k] = h[k];
  r[10] = (uint32_t)c; r[11] = (uint32_t)(c >> 32);
  r[12] = plen + 1; r[13] = plen + 1; r[14] = depth;
  uint32_t m[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) { const uint32_t w = m8[k]; r[15 + k] = w; r[23 + k] = 0; m[bit_left ? 8 + k : k] = w; }   // sibling CV, then zeros (blake3_circuit.rs:230-245)
  r[31] = 64;
  // the next step's h = this step's h_out: compress(IV, h || sibling or sibling || h, PARENT [| ROOT at depth 0])
#pragma unroll
  for (int k = 0; k < 8; ++k) m[bit_left ? k : 8 + k] = h[k];
  uint32_t ivv[8], o[8];
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, 4u | (depth == 0 ? 8u : 0u), o);
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = o[k];
}

// ---- chunk chaining values -----------------------------------------------------------------------------------------
// the CV of chunk c (`bytes` bytes from src; root: 8 where the chunk is the whole input, its output then carries ROOT: the hash itself).
// Where the chunk is whole and starts 16-byte aligned every load is a whole 16-byte quarter of a block and the next block's four loads are
// in flight while the current block is compressed.
__device__ __forceinline__ void chunk_cv(const uint8_t *__restrict__ src, uint32_t bytes, uint64_t c, uint32_t root, uint32_t h[8]) {
  uint32_t o[8], m[16];
  iv(h);
  if (bytes == 1024 && ((uintptr_t)src & 15) == 0) {
    const uint4 *p = reinterpret_cast<const uint4 *>(src);
    uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    for (uint32_t j = 0; j < 16; ++j) {
      m[0] = q0.x; m[1] = q0.y; m[2] = q0.z; m[3] = q0.w; m[4] = q1.x; m[5] = q1.y; m[6] = q1.z; m[7] = q1.w;
      m[8] = q2.x; m[9] = q2.y; m[10] = q2.z; m[11] = q2.w; m[12] = q3.x; m[13] = q3.y; m[14] = q3.z; m[15] = q3.w;
      if (j < 15) { q0 = p[4 * j + 4]; q1 = p[4 * j + 5]; q2 = p[4 * j + 6]; q3 = p[4 * j + 7]; }
      const uint32_t d = (j == 0 ? 1u : 0u) | (j == 15 ? 2u | root : 0u);
      blake3_cv(h, m, (uint32_t)c, (uint32_t)(c >> 32), 64, d, o);
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = o[k];
    }
  } else {                                               // a ragged last chunk, or a file that starts off a 16-byte boundary
    const uint32_t nb = bytes ? (bytes + 63) / 64 : 1;
    for (uint32_t j = 0; j < nb; ++j) {
      const uint32_t bb = bytes - j * 64 < 64 ? bytes - j * 64 : 64;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        uint32_t w = 0;
        for (int x = 0; x < 4; ++x) { const uint32_t q = k * 4 + x; if (q < bb) w |= (uint32_t)src[j * 64 + q] << (8 * x); }
        m[k] = w;
      }
      const uint32_t d = (j == 0 ? 1u : 0u) | (j == nb - 1 ? 2u | root : 0u);
      blake3_cv(h, m, (uint32_t)c, (uint32_t)(c >> 32), bb, d, o);
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = o[k];
    }
  }
}

// lane = chunk (neighbouring lanes' blocks lie 1 KiB apart)
__global__ __launch_bounds__(256) void b3w_bao_cv_kernel(const uint8_t *__restrict__ pre, uint64_t len, uint64_t n, uint32_t *__restrict__ cv) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const uint64_t off = c * 1024;
  uint32_t h[8];
  chunk_cv(pre + off, (uint32_t)(len - off < 1024 ? len - off : 1024), c, n == 1 ? 8u : 0u, h);
  uint4 *dst = reinterpret_cast<uint4 *>(cv + c * 8);
  dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
  dst[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

// four lanes per chunk (b3w_plan_leaf_quad_kernel without the records): lane col holds column col of the state
__global__ __launch_bounds__(64) void b3w_bao_cv_quad_kernel(const uint8_t *__restrict__ pre, uint64_t len, uint64_t n, uint32_t *__restrict__ cv) {
  __shared__ uint32_t Ms[16][16];
  const uint32_t q = threadIdx.x >> 2, col = threadIdx.x & 3u;
  const uint64_t i = (uint64_t)blockIdx.x * 16 + q;
  const bool live = i < n;                               // (a dead quad walks the workgroup's first chunk with its store masked: DPP wants whole quads)
  const uint64_t c = live ? i : (uint64_t)blockIdx.x * 16;
  const uint64_t off = c * 1024;
  const uint32_t bytes = (uint32_t)(len - off < 1024 ? len - off : 1024);
  const uint32_t nb = bytes ? (bytes + 63) / 64 : 1;
  const uint32_t root = n == 1 ? 8u : 0u;
  const uint8_t *src = pre + off;
  uint32_t *M = Ms[q];
  uint32_t h_lo = col == 0 ? 0x6A09E667u : col == 1 ? 0xBB67AE85u : col == 2 ? 0x3C6EF372u : 0xA54FF53Au;
  uint32_t h_hi = col == 0 ? 0x510E527Fu : col == 1 ? 0x9B05688Cu : col == 2 ? 0x1F83D9ABu : 0x5BE0CD19u;
  for (uint32_t j = 0; j < nb; ++j) {                    // (uniform over the quad)
    const uint32_t bb = bytes - j * 64 < 64 ? bytes - j * 64 : 64;
    uint32_t m4[4];
    if (bb == 64 && ((uintptr_t)src & 15) == 0) {
      const uint4 v = *reinterpret_cast<const uint4 *>(src + j * 64 + col * 16);
      m4[0] = v.x; m4[1] = v.y; m4[2] = v.z; m4[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t w = 0;
        for (int x = 0; x < 4; ++x) { const uint32_t p = (col * 4 + k) * 4 + x; if (p < bb) w |= (uint32_t)src[j * 64 + p] << (8 * x); }
        m4[k] = w;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) M[col * 4 + k] = m4[k];
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: the quad's words are in LDS)
    const uint32_t d = (j == 0 ? 1u : 0u) | (j == nb - 1 ? 2u | root : 0u);
    plan_quad_cv(h_lo, h_hi, M, (int)col, (uint32_t)c, (uint32_t)(c >> 32), bb, d);
    __builtin_amdgcn_wave_barrier();                     // (every lane has read this block's words before the next block's overwrite them)
  }
  if (live) { cv[c * 8 + col] = h_lo; cv[c * 8 + 4 + col] = h_hi; }
}

// ---- pre-order emission ---------------------------------------------------------------------------------------------
// A node with d ancestors, r of them passed on their right, covering chunks from a, sits at pre-order position d + a - r: the nodes
// before it are its ancestors and the parents of the left subtrees hanging off its path (a chunks in r subtrees: a - r parents).
// Complete subtree node (level t >= 1, index i, chunks from a = i 2^t) inside spine segment s (2^L chunks from lo, its root at depth
// plen - L reached by s right turns): d = plen - t, r = s + popcount((a - lo) >> t).  Spine node suffix[k] (k < last): d = r = k, a = lo[k].
// Threads [0, n - popcount(n)) take the complete nodes level by level, the last `last` threads the spine nodes.  Thread 0 also writes
// the header.  (The nodes sit 8 bytes off a 16-byte boundary: 8-byte stores.)
__global__ __launch_bounds__(256) void b3w_bao_emit_kernel(const uint32_t *__restrict__ levels, uint64_t n, uint64_t len, B3wSpine sp,
                                                           uint8_t *__restrict__ out) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid == 0) *reinterpret_cast<uint2 *>(out) = make_uint2((uint32_t)len, (uint32_t)(len >> 32));
  const uint64_t ncomplete = n - __popcll(n);
  if (tid >= n - 1) return;
  const uint32_t *lc, *rc;
  uint64_t pos;
  if (tid < ncomplete) {
    uint64_t rem = tid, off = 0;                         // off: word offset of level t - 1
    uint32_t t = 1;
    while (rem >= (n >> t)) { rem -= n >> t; off += (n >> (t - 1)) * 8; t++; }
    const uint64_t a = rem << t;
    const uint32_t s = seg_of(sp, a);
    pos = (uint64_t)(sp.plen[s] - t) + a - s - (uint64_t)__popcll((a - sp.lo[s]) >> t);
    lc = levels + off + rem * 16;
    rc = lc + 8;
  } else {
    const uint32_t k = (uint32_t)(tid - ncomplete);
    pos = sp.lo[k];
    lc = levels + sp.seg_off[k];
    rc = levels + sp.suf_off[k + 1];
  }
  uint2 *dst = reinterpret_cast<uint2 *>(out + 8 + pos * 64);
  const uint4 l0 = reinterpret_cast<const uint4 *>(lc)[0], l1 = reinterpret_cast<const uint4 *>(lc)[1];
  const uint4 r0 = reinterpret_cast<const uint4 *>(rc)[0], r1 = reinterpret_cast<const uint4 *>(rc)[1];
  dst[0] = make_uint2(l0.x, l0.y); dst[1] = make_uint2(l0.z, l0.w); dst[2] = make_uint2(l1.x, l1.y); dst[3] = make_uint2(l1.z, l1.w);
  dst[4] = make_uint2(r0.x, r0.y); dst[5] = make_uint2(r0.z, r0.w); dst[6] = make_uint2(r1.x, r1.y); dst[7] = make_uint2(r1.z, r1.w);
}

// ---- batches of files: tiles ------------------------------------------------------------------------------------------
// A tile = up to B3W_TILE consecutive chunks of one file from a multiple of B3W_TILE.  Every tile is a subtree of the file's tree (the left
// subtree of a node over m > B3W_TILE chunks holds a power of two >= B3W_TILE of them), and the tree above the tiles is BLAKE3's tree shape over
// the tile CVs.  The same holds one storey up for groups of 1 024 tiles.  So:
//   b3w_bao_tile_kernel       one workgroup per tile, lane = chunk: the chunk CVs into LDS, merged level by level in LDS, every parent
//                             node straight to its pre-order place in the file's outboard; one CV per tile to `tile_cv`, or the root and
//                             the header for a one-tile file.  Files of more than 64 chunks.
//   b3w_bao_small_kernel      the files of at most 64 chunks, packed several to a wave
//   b3w_bao_merge_kernel      one workgroup per group of up to 1 024 items (tile CVs; for files past 1 GiB a second launch over the groups'
//                             CVs): the same merge over them, ROOT on a file's top merge.
// Merging in place: the CV of the item that starts at slot i stays in slot i, so level l pairs slot (2 j) << l with slot ((2 j) << l) +
// (1 << l) where that one exists, and an odd item out simply waits — which is BLAKE3's tree (tests/test_bao_batch_cpu.py restates it).
struct BatchEnt { uint64_t off, len, ob; uint32_t first, file; };   // tile launches: arena offset; merge launches: first input CV slot

// the last row of rows[lo .. hi) whose `first` is at or before x (rows sorted by first, rows[lo].first <= x): the entry whose workgroups
// include workgroup x, or the small file whose lanes include lane x
template <class Row>
__device__ __forceinline__ uint32_t find_first(const Row *__restrict__ rows, uint32_t lo, uint32_t hi, uint32_t x) {
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (rows[mid].first <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ BatchEnt batch_ent(const BatchEnt *__restrict__ ents, uint32_t n_ents, uint32_t wg) {
  return ents[find_first(ents, 0, n_ents, wg)];
}

// the CV h to slot i of an LDS array of CVs
__device__ __forceinline__ void put_cv(uint32_t *cv, uint32_t i, const uint32_t h[8]) {
  reinterpret_cast<uint4 *>(cv + i * 8)[0] = make_uint4(h[0], h[1], h[2], h[3]);
  reinterpret_cast<uint4 *>(cv + i * 8)[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

// whether the header of the outboard at ob is `len`
__device__ __forceinline__ bool header_is(const uint8_t *ob, uint64_t len) {
  const uint32_t *h = reinterpret_cast<const uint32_t *>(ob);
  return ((uint64_t)h[0] | ((uint64_t)h[1] << 32)) == len;
}

// The barrier of the walks that do not store every node (tree_levels and small_levels with WAIT, the planners' group merges).  In the group instantiation of the tile kernel the compiler (ROCm 7's clang) left
// the level loop's s_barrier without a wait for the LDS stores of the level before (it keeps the wait in the instantiation that stores
// every node), and a 64-chunk subtree's CV now and then came out wrong: the wait is spelled out.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// one parent: the CVs in slots i0 (left) and i1 (right) of cv to the node at dst, their parent's CV to slot i0 (d = PARENT [| ROOT]).
// GRP (group outboards): a null `node` is a node inside a chunk group, which is computed and not stored.
template <bool GRP>
__device__ __forceinline__ void merge_pair(uint32_t *cv, uint32_t i0, uint32_t i1, uint8_t *__restrict__ node, uint32_t d) {
  uint32_t m[16], ivv[8], o[8];
  const uint4 l0 = reinterpret_cast<const uint4 *>(cv + i0 * 8)[0], l1 = reinterpret_cast<const uint4 *>(cv + i0 * 8)[1];
  const uint4 r0 = reinterpret_cast<const uint4 *>(cv + i1 * 8)[0], r1 = reinterpret_cast<const uint4 *>(cv + i1 * 8)[1];
  if (!GRP || node) {
    uint2 *dst = reinterpret_cast<uint2 *>(node);                    // (8 off a 16-byte boundary)
    dst[0] = make_uint2(l0.x, l0.y); dst[1] = make_uint2(l0.z, l0.w); dst[2] = make_uint2(l1.x, l1.y); dst[3] = make_uint2(l1.z, l1.w);
    dst[4] = make_uint2(r0.x, r0.y); dst[5] = make_uint2(r0.z, r0.w); dst[6] = make_uint2(r1.x, r1.y); dst[7] = make_uint2(r1.z, r1.w);
  }
  m[0] = l0.x; m[1] = l0.y; m[2] = l0.z; m[3] = l0.w; m[4] = l1.x; m[5] = l1.y; m[6] = l1.z; m[7] = l1.w;
  m[8] = r0.x; m[9] = r0.y; m[10] = r0.z; m[11] = r0.w; m[12] = r1.x; m[13] = r1.y; m[14] = r1.z; m[15] = r1.w;
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, d, o);
  put_cv(cv, i0, o);                                                 // (slot i0 is read by this thread alone at this level)
}

// pre-order position of the node over chunks [a, a + size) of a tree over `total` chunks.  GRP: in the GROUP outboard (groups of 1 << gl
// chunks; a is a multiple of that), which is the tree over the file's groups; gl = 0 is the full outboard.
template <bool GRP>
__device__ __forceinline__ uint64_t node_pos(uint64_t total, uint64_t a, uint64_t size, uint32_t gl) {
  if (!GRP) return preorder_pos(total, a, size);
  const uint64_t G1 = (1ull << gl) - 1;
  return preorder_pos((total + G1) >> gl, a >> gl, (size + G1) >> gl);
}
// that node's place where `nodes` is the root's.  GRP: null for a node over at most a group's chunks, which is computed and not stored.
template <bool GRP>
__device__ __forceinline__ uint8_t *node_at(uint8_t *__restrict__ nodes, uint64_t total, uint64_t a, uint64_t size, uint32_t gl) {
  if (!GRP) return nodes + preorder_pos(total, a, size) * 64;
  const uint64_t G1 = (1ull << gl) - 1;
  return size > G1 + 1 ? nodes + preorder_pos((total + G1) >> gl, a >> gl, (size + G1) >> gl) * 64 : nullptr;
}

// The level loop of the dense walks over a tree in LDS (merge, verify): cnt items of `unit` chunks each (the last one
// maybe fewer) of a tree over `total` chunks, item i in slot i.  At level l thread j takes the pairs of slots i0 = (2 j) << l and
// i1 = i0 + (1 << l) and hands pair(l, i0, i1, a, size, d) the node over chunks [a, a + size) with d = PARENT [| ROOT on the top pair where
// `root` says so]; the pair's work leaves the node's CV in slot i0.  A barrier before every level and one behind the last.
// WAIT: the barriers are lds_barrier().  Every walk that does not store every node takes it (the group outboards and all of verify, as
// do the sparse walks below); the merge into a full outboard keeps __syncthreads(), behind which the compiler does wait.
// The sparse walks (update_in_lds, ranges_in_lds) keep this loop written out, with their skip test in front of the pair's span: through
// tree_levels the update and the ranged verify of 4 096 scattered blocks of a 1 GiB file took 3.5 % longer (profiles/r21/bao_shared_bodies_ab.json).
template <int BS, bool WAIT, class Pair>
__device__ __forceinline__ void tree_levels(uint32_t cnt, uint64_t unit, uint64_t total, bool root, Pair pair) {
  for (uint32_t l = 0; (1u << l) < cnt; ++l) {
    if (WAIT) lds_barrier(); else __syncthreads();
    const bool top = (2u << l) >= cnt;
    for (uint32_t j = threadIdx.x;; j += BS) {
      const uint32_t i0 = (2 * j) << l, i1 = i0 + (1u << l);
      if (i1 >= cnt) break;
      const uint64_t a = i0 * unit, e = (uint64_t)(i0 + (2u << l)) * unit, size = (e < total ? e : total) - a;
      pair(l, i0, i1, a, size, 4u | (top && root ? 8u : 0u));
    }
  }
  if (WAIT) lds_barrier(); else __syncthreads();
}

// cv: the items of a tree whose nodes go to `nodes` (its root's place; GRP: in the file's group outboard, the tree starts at a multiple
// of the group size).  Leaves the tree's CV in cv[0 .. 8); ends with a barrier.
template <int BS, bool GRP>
__device__ __forceinline__ void merge_in_lds(uint32_t *cv, uint32_t cnt, uint64_t unit, uint64_t total, uint8_t *__restrict__ nodes, bool root,
                                             uint32_t gl) {
  tree_levels<BS, GRP>(cnt, unit, total, root, [&](uint32_t, uint32_t i0, uint32_t i1, uint64_t a, uint64_t size, uint32_t d) {
    merge_pair<GRP>(cv, i0, i1, node_at<GRP>(nodes, total, a, size, gl), d);
  });
}

// this lane's chunk c of a file of len bytes and n chunks, its bytes at base + 1024 at: its CV to the lane's slot.  lone: the file may be
// a single chunk, whose CV carries ROOT (it is the hash itself); no file of more than 64 chunks is, the small and the streamed ones may be.
__device__ __forceinline__ void lane_chunk_cv(uint32_t *cv, const uint8_t *__restrict__ base, uint64_t at, uint64_t len, uint64_t n, uint64_t c, bool lone) {
  const uint64_t off = c * 1024;
  uint32_t h[8];
  chunk_cv(base + at * 1024, (uint32_t)(len - off < 1024 ? len - off : 1024), c, lone && n == 1 ? 8u : 0u, h);
  put_cv(cv, threadIdx.x, h);
}
// lane = chunk: the CVs of the m chunks from a0 on of a file of n chunks into slots [0, m); the tile's bytes start at base + 1024 at (the
// file's first byte and a0, or a window and the tile's place in it)
__device__ __forceinline__ void tile_chunk_cvs(uint32_t *cv, const uint8_t *__restrict__ base, uint64_t at, uint64_t len, uint64_t n, uint64_t a0, uint32_t m,
                                               bool lone) {
  if (threadIdx.x < m) lane_chunk_cv(cv, base, at + threadIdx.x, len, n, a0 + threadIdx.x, lone);
}

// A tile's outboard: the tile of chunks from a0 (its bytes at base + 1024 at) of a file of len bytes and n chunks whose outboard starts
// at ob.  lone: lane_chunk_cv's.  The tile's CV goes to tile_cv, or (a file of this one tile) the root to `root`.  The batch, stream and
// many-session kernels find their file's entry and call this.
template <bool GRP>
__device__ __forceinline__ void tile_outboard(const uint8_t *__restrict__ base, uint64_t at, uint64_t len, uint64_t n, uint64_t a0, bool lone,
                                              uint8_t *__restrict__ ob, uint32_t *root, uint32_t *tile_cv, uint32_t gl) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  const uint32_t m = (uint32_t)(n - a0 < B3W_TILE ? n - a0 : B3W_TILE);
  const bool sole = n <= B3W_TILE;
  tile_chunk_cvs(cv, base, at, len, n, a0, m, lone);
  if (a0 == 0 && threadIdx.x == 0) *reinterpret_cast<uint2 *>(ob) = make_uint2((uint32_t)len, (uint32_t)(len >> 32));
  merge_in_lds<B3W_TILE, GRP>(cv, m, 1, m, ob + 8 + node_pos<GRP>(n, a0, m, gl) * 64, sole, gl);   // (a tile starts at a multiple of every group size)
  if (threadIdx.x < 8) (sole ? root : tile_cv)[threadIdx.x] = cv[threadIdx.x];
}

template <bool GRP>
__device__ __forceinline__ void tile_body(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents, uint32_t n_ents,
                                          uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots, uint32_t *__restrict__ tile_cv, uint32_t gl) {
  const BatchEnt e = batch_ent(ents, n_ents, blockIdx.x);
  const uint64_t a0 = (uint64_t)(blockIdx.x - e.first) * B3W_TILE;
  tile_outboard<GRP>(arena + e.off, a0, e.len, (e.len + 1023) / 1024, a0, false, outboards + e.ob, roots + (uint64_t)e.file * 8,   // (more than 64 chunks)
                     tile_cv + (uint64_t)blockIdx.x * 8, gl);
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_tile_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents, uint32_t n_ents,
                                                                uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots,
                                                                uint32_t *__restrict__ tile_cv) {
  tile_body<false>(arena, ents, n_ents, outboards, roots, tile_cv, 0);
}
// the same into group outboards (groups of 1 << gl chunks, gl <= 6)
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_tile_group_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents, uint32_t n_ents,
                                                                      uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots,
                                                                      uint32_t *__restrict__ tile_cv, uint32_t gl) {
  tile_body<true>(arena, ents, n_ents, outboards, roots, tile_cv, gl);
}

// Files of at most 64 chunks, several to a wave: wave w takes the files [wave_first[w], wave_first[w + 1]) of `rows`, which have at most 64
// chunks together; rows[f].first = the lane of file f's chunk 0.  lane = chunk, every lane busy where the files fill the wave (a wave a
// file would leave 60 of 64 lanes idle on 4 KiB files, and idle lanes cost the same issue cycles).
// This lane's file (Row: BatchEnt or VrSmall), the file's chunk count n, the lane's chunk i of it, and whether the file has such a chunk
// (the lanes behind the last file's chunks do not); a live lane's chunk CV goes to slot `lane` of cv.
template <class Row>
struct SmallLane { Row e; uint32_t n, i; bool live; };
template <class Row>
__device__ __forceinline__ SmallLane<Row> small_lane(uint32_t *cv, const uint8_t *__restrict__ arena, const Row *__restrict__ rows,
                                                     const uint32_t *__restrict__ wave_first) {
  const uint32_t lane = threadIdx.x;
  SmallLane<Row> s;
  s.e = rows[find_first(rows, wave_first[blockIdx.x], wave_first[blockIdx.x + 1], lane)];
  s.n = s.e.len ? (uint32_t)((s.e.len + 1023) / 1024) : 1;
  s.i = lane - s.e.first;
  s.live = s.i < s.n;
  if (s.live) lane_chunk_cv(cv, arena + s.e.off, s.i, s.e.len, s.n, s.i, true);
  return s;
}
// The in-place merge with each file in its own run of slots: at level l the lane of a chunk index that is a multiple of 2 << l takes the
// slot 1 << l further on, and pair(l, size, d) gets the node over the file's chunks [i, i + size).  Barriers as in tree_levels.
template <bool WAIT, class Pair>
__device__ __forceinline__ void small_levels(uint32_t n, uint32_t i, bool live, Pair pair) {
  for (uint32_t l = 0; l < 6; ++l) {
    if (WAIT) lds_barrier(); else __syncthreads();
    if (!__any(live && (1u << l) < n)) break;                         // (uniform: the workgroup is this one wave)
    if (live && (i & ((2u << l) - 1)) == 0 && i + (1u << l) < n)
      pair(l, n - i < (2u << l) ? n - i : (2u << l), 4u | (i == 0 && (2u << l) >= n ? 8u : 0u));
  }
  if (WAIT) lds_barrier(); else __syncthreads();
}

template <bool GRP>
__device__ __forceinline__ void small_body(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents, const uint32_t *__restrict__ wave_first,
                                           uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots, uint32_t gl) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[64 * 8];
  const uint32_t lane = threadIdx.x;
  const SmallLane<BatchEnt> s = small_lane(cv, arena, ents, wave_first);
  const BatchEnt &e = s.e;
  uint8_t *ob = outboards + e.ob;
  if (s.live && s.i == 0) *reinterpret_cast<uint2 *>(ob) = make_uint2((uint32_t)e.len, (uint32_t)(e.len >> 32));
  small_levels<GRP>(s.n, s.i, s.live, [&](uint32_t l, uint32_t size, uint32_t d) {   // (GRP, size > a group: i is a multiple of the group size)
    merge_pair<GRP>(cv, lane, lane + (1u << l), node_at<GRP>(ob + 8, s.n, s.i, size, gl), d);
  });
  if (s.live && s.i == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) roots[(uint64_t)e.file * 8 + k] = cv[lane * 8 + k];
  }
}

__global__ __launch_bounds__(64) void b3w_bao_small_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents,
                                                           const uint32_t *__restrict__ wave_first, uint8_t *__restrict__ outboards,
                                                           uint32_t *__restrict__ roots) {
  small_body<false>(arena, ents, wave_first, outboards, roots, 0);
}
// the same into group outboards: with gl >= 1 a file of at most a group's chunks gets its header alone
__global__ __launch_bounds__(64) void b3w_bao_small_group_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents,
                                                                 const uint32_t *__restrict__ wave_first, uint8_t *__restrict__ outboards,
                                                                 uint32_t *__restrict__ roots, uint32_t gl) {
  small_body<true>(arena, ents, wave_first, outboards, roots, gl);
}

// The merge storey: workgroup g of a file of n chunks (more than one tile) merges up to 1 024 items of `unit` chunks each (B3W_TILE, or
// B3W_TILE^2 for the launch over the groups' CVs), whose CVs lie from `in` on; its CV goes to out_cv, or (the file's top) the root to `root`.
template <bool GRP>
__device__ __forceinline__ void merge_storey(uint64_t n, uint64_t g, uint64_t unit, const uint32_t *__restrict__ in, uint8_t *__restrict__ ob,
                                             uint32_t *root, uint32_t *out_cv, uint32_t gl) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  const uint64_t span = unit * B3W_TILE, a0 = g * span;
  const uint64_t tot = n - a0 < span ? n - a0 : span;
  const uint32_t cnt = (uint32_t)((tot + unit - 1) / unit);
  const bool sole = n <= span;
  const uint4 *src = reinterpret_cast<const uint4 *>(in);
  for (uint32_t i = threadIdx.x; i < cnt * 2; i += 256) reinterpret_cast<uint4 *>(cv)[i] = src[i];
  merge_in_lds<256, GRP>(cv, cnt, unit, tot, ob + 8 + node_pos<GRP>(n, a0, tot, gl) * 64, sole, gl);   // (every node here is over more than a tile: all are stored)
  if (threadIdx.x < 8) (sole ? root : out_cv)[threadIdx.x] = cv[threadIdx.x];
}

// input item i of the file: in_cv slot e.off + i
template <bool GRP>
__device__ __forceinline__ void merge_body(const BatchEnt *__restrict__ ents, uint32_t n_ents, uint64_t unit, const uint32_t *__restrict__ in_cv,
                                           uint32_t *__restrict__ out_cv, uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots, uint32_t gl) {
  const BatchEnt e = batch_ent(ents, n_ents, blockIdx.x);
  const uint64_t n = (e.len + 1023) / 1024, g = blockIdx.x - e.first;
  merge_storey<GRP>(n, g, unit, in_cv + (e.off + g * B3W_TILE) * 8, outboards + e.ob, roots + (uint64_t)e.file * 8,
                    out_cv + (uint64_t)blockIdx.x * 8, gl);
}

__global__ __launch_bounds__(256) void b3w_bao_merge_kernel(const BatchEnt *__restrict__ ents, uint32_t n_ents, uint64_t unit,
                                                            const uint32_t *__restrict__ in_cv, uint32_t *__restrict__ out_cv,
                                                            uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots) {
  merge_body<false>(ents, n_ents, unit, in_cv, out_cv, outboards, roots, 0);
}
__global__ __launch_bounds__(256) void b3w_bao_merge_group_kernel(const BatchEnt *__restrict__ ents, uint32_t n_ents, uint64_t unit,
                                                                  const uint32_t *__restrict__ in_cv, uint32_t *__restrict__ out_cv,
                                                                  uint8_t *__restrict__ outboards, uint32_t *__restrict__ roots, uint32_t gl) {
  merge_body<true>(ents, n_ents, unit, in_cv, out_cv, outboards, roots, gl);
}

// ---- challenged paths ------------------------------------------------------------------------------------------------
struct Root8 { uint32_t w[8]; };

__device__ __forceinline__ bool eq8(const uint32_t *a, const uint32_t *b) {
  uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) x |= a[k] ^ b[k];
  return x == 0;
}

// One challenged chunk: chunk c of a file of len bytes (n chunks) whose outboard starts at ob and whose root words are root8; its records
// from row `row` on.  Returns the status: 0 verified, 1 chunk bytes, 2 a path node or the root, 3 header.
__device__ __forceinline__ int32_t sample_plan_one(uint64_t len, uint64_t n, const uint32_t *__restrict__ ob, const uint32_t *root8, uint64_t c,
                                                   uint64_t row, const uint8_t *__restrict__ cb, uint32_t *__restrict__ recs) {
  const uint32_t P = path_len(c, n);
  const uint64_t off = c * 1024;
  const uint32_t bytes = (uint32_t)(len - off < 1024 ? len - off : 1024);
  const uint32_t n_blocks = bytes ? (bytes + 63) / 64 : 1;
  uint32_t *r = recs + row * 32;
  uint32_t h[8];
  plan_leaf_chunk(cb, bytes, c, P, r, h);
  int32_t st = ((uint64_t)ob[0] | ((uint64_t)ob[1] << 32)) != len ? 3 : 0;
  // top down, as bao's decoder: the root node against the root, every lower node against its half of the node above, the chunk
  // against its half of the lowest node
  uint64_t pos[64];
  uint32_t want[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) want[k] = root8[k];
  uint64_t p = 0, cc = c, m = n;
  for (uint32_t i = 0; i < P; ++i) {
    const uint32_t *node = ob + 2 + p * 16;
    uint32_t mw[16], ivv[8], o[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) mw[k] = node[k];
    iv(ivv);
    blake3_cv(ivv, mw, 0, 0, 64, 4u | (i == 0 ? 8u : 0u), o);
    if (!eq8(o, want) && st == 0) st = 2;
    uint64_t k2 = 1;
    while (k2 * 2 < m) k2 *= 2;
    const bool left = cc < k2;
#pragma unroll
    for (int k = 0; k < 8; ++k) want[k] = left ? mw[k] : mw[8 + k];
    pos[i] = p;
    if (left) { p += 1; m = k2; } else { p += k2; cc -= k2; m -= k2; }
  }
  if (!eq8(h, want) && st == 0) st = 1;                  // (one chunk: its ROOT-flagged output against the root)
  // parent steps bottom up: the CV the reference's driver picks by bit g of the index (blake3_hash.rs:63-78)
  r += (uint64_t)n_blocks * 32;
  for (uint32_t g = 0; g < P; ++g, r += 32) {
    const uint32_t *node = ob + 2 + pos[P - 1 - g] * 16;
    const bool bit_left = ((c >> g) & 1) == 0;
    plan_parent_step(r, h, bit_left ? node + 8 : node, bit_left, c, n_blocks, P, P - 1 - g);
  }
  return st;
}

// desc[2 s] = chunk, desc[2 s + 1] = first row of sample s.  status: 0 verified, 1 chunk bytes, 2 a path node or the root, 3 header.
__global__ __launch_bounds__(64) void b3w_sample_plan_kernel(uint64_t len, uint64_t n, const uint32_t *__restrict__ ob, Root8 root,
                                                             const uint64_t *__restrict__ desc, uint32_t n_samples,
                                                             const uint8_t *__restrict__ chunk_bytes, uint32_t *__restrict__ recs,
                                                             int32_t *__restrict__ status) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_samples) return;
  status[s] = sample_plan_one(len, n, ob, root.w, desc[2 * s], desc[2 * s + 1], chunk_bytes + (uint64_t)s * 1024, recs);
}

// the same over a batch of files: desc[5 s ..] = chunk, first row, the file's length, the byte offset of its outboard in `obs`, the file
// (its root: 8 words of `roots`, on the device)
__global__ __launch_bounds__(64) void b3w_sample_plan_batch_kernel(const uint8_t *__restrict__ obs, const uint32_t *__restrict__ roots,
                                                                   const uint64_t *__restrict__ desc, uint32_t n_samples,
                                                                   const uint8_t *__restrict__ chunk_bytes, uint32_t *__restrict__ recs,
                                                                   int32_t *__restrict__ status) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_samples) return;
  const uint64_t *d = desc + 5 * (uint64_t)s;
  const uint64_t len = d[2];
  uint32_t root[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) root[k] = roots[d[4] * 8 + k];
  status[s] = sample_plan_one(len, len ? (len + 1023) / 1024 : 1, reinterpret_cast<const uint32_t *>(obs + d[3]), root, d[0], d[1],
                              chunk_bytes + (uint64_t)s * 1024, recs);
}

// ARENA (this kernel and the <true> instantiations of the three below): the samples' bytes are read where the files lie.  The table has
// a sixth word per sample, the byte offset of the sample's file in the arena, and a chunk's bytes start at arena + desc[6 s + 5] + 1024 chunk
// instead of at the sample's row of a gathered copy.  A file starts at any byte, so a chunk lies at any of the 16 alignments; no byte outside
// [offset, offset + len) of the sample's own file is read (the hashing reads a chunk's `bytes` bytes and the lanes of the chunks a short
// last group lacks read nothing).
// desc[6 s ..] = chunk, first row, the file's length, the byte offset of its outboard in `obs`, the file, the file's byte offset in `arena`
__global__ __launch_bounds__(64) void b3w_sample_plan_arena_kernel(const uint8_t *__restrict__ obs, const uint32_t *__restrict__ roots,
                                                                   const uint64_t *__restrict__ desc, uint32_t n_samples,
                                                                   const uint8_t *__restrict__ arena, uint32_t *__restrict__ recs,
                                                                   int32_t *__restrict__ status) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_samples) return;
  const uint64_t *d = desc + 6 * (uint64_t)s;
  const uint64_t len = d[2];
  uint32_t root[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) root[k] = roots[d[4] * 8 + k];
  status[s] = sample_plan_one(len, len ? (len + 1023) / 1024 : 1, reinterpret_cast<const uint32_t *>(obs + d[3]), root, d[0], d[1],
                              arena + d[5] + d[0] * 1024, recs);
}

// ---- challenged paths from group outboards ---------------------------------------------------------------------------
// A group outboard (groups of G = 1 << gl chunks) holds the nodes over more than G chunks, which are the parent nodes of BLAKE3's tree
// over the file's groups.  The lower part of a chunk's path, inside its group, is recomputed from the group's bytes.
// One wave takes 64 >> gl samples, lane = one chunk of one sample's group (gl = 6: a sample a wave, gl = 4: four, gl = 0: 64, the
// lane-per-sample planner above), so no lane hashes two chunks of a group:
//   1. every lane its chunk's CV into LDS (2 KiB a wave); the lane of the sampled chunk (the sample's leader) writes the leaf records
//      from the same compressions
//   2. the in-place merge of b3w_bao_small_kernel over each group's run of slots, no node stored; before each level the leader takes the
//      half of its path's node that the reference's driver picks by the index bit
//   3. the stored part of the path top down, node j on lane j mod G of the sample: the root node with ROOT against the root, every other
//      against its half of the node above; the leader holds the group's CV against its half of the lowest stored node (a file of one
//      group: the group's ROOT-flagged output against the root)
//   4. the leader writes the parent records bottom up: the recomputed halves, then the stored nodes'

// the CV of one chunk as chunk_cv computes it, and with rec != NULL the chunk's leaf records (plan_leaf_chunk's words; P = the path length)
__device__ __forceinline__ void group_chunk(const uint8_t *__restrict__ src, uint32_t bytes, uint64_t c, uint32_t P, uint32_t root,
                                            uint32_t *__restrict__ rec, uint32_t h[8]) {
  const uint32_t nb = bytes ? (bytes + 63) / 64 : 1;
  const bool fast = ((uintptr_t)src & 15) == 0;
  uint32_t o[8], m[16];
  iv(h);
  for (uint32_t j = 0; j < nb; ++j) {
    const uint32_t bb = bytes - j * 64 < 64 ? bytes - j * 64 : 64;
    if (bb == 64 && fast) {
      const uint4 *p = reinterpret_cast<const uint4 *>(src + j * 64);
      const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
      m[0] = q0.x; m[1] = q0.y; m[2] = q0.z; m[3] = q0.w; m[4] = q1.x; m[5] = q1.y; m[6] = q1.z; m[7] = q1.w;
      m[8] = q2.x; m[9] = q2.y; m[10] = q2.z; m[11] = q2.w; m[12] = q3.x; m[13] = q3.y; m[14] = q3.z; m[15] = q3.w;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        uint32_t w = 0;
        for (int x = 0; x < 4; ++x) { const uint32_t q = k * 4 + x; if (q < bb) w |= (uint32_t)src[j * 64 + q] << (8 * x); }
        m[k] = w;
      }
    }
    if (rec) {
      uint32_t *r = rec + j * 32;
      r[0] = nb; r[1] = j;
#pragma unroll
      for (int k = 0; k < 8; ++k) r[2 + k] = h[k];
      r[10] = (uint32_t)c; r[11] = (uint32_t)(c >> 32);
      r[12] = P + 1; r[13] = P + 1; r[14] = P;
#pragma unroll
      for (int k = 0; k < 16; ++k) r[15 + k] = m[k];
      r[31] = bb;
    }
    const uint32_t d = (j == 0 ? 1u : 0u) | (j == nb - 1 ? 2u | root : 0u);
    blake3_cv(h, m, (uint32_t)c, (uint32_t)(c >> 32), bb, d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = o[k];
  }
}

// desc as b3w_sample_plan_batch_kernel's, the outboard offsets those of the group layout; group_bytes: 1024 << gl bytes per sample.
// status: 0 verified, 1 the group's bytes (any chunk of the group), 2 a stored node or the root, 3 header.
// ARENA (b3w_sample_plan_arena_kernel): src is the arena, the table has the file's offset in it and lane i reads chunk first + i of its file
// where it lies.  <false>: the gathered bytes (b3w_sample_plan_group_batch_device), <true>: the arena (b3w_sample_plan_arena_device).
template <bool ARENA>
__global__ __launch_bounds__(64) void b3w_sample_plan_group_kernel(const uint8_t *__restrict__ obs, const uint32_t *__restrict__ roots,
                                                                   const uint64_t *__restrict__ desc, uint32_t n_samples, uint32_t gl,
                                                                   const uint8_t *__restrict__ src, uint32_t *__restrict__ recs,
                                                                   int32_t *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[64 * 8];
  const uint32_t lane = threadIdx.x, G = 1u << gl, i = lane & (G - 1), base = lane - i;
  const uint32_t s = blockIdx.x * (64u >> gl) + (lane >> gl);
  const bool valid = s < n_samples;
  const uint64_t *d = desc + (ARENA ? 6 : 5) * (uint64_t)(valid ? s : 0);   // (a wave's lanes past the last sample read sample 0's row and write nothing)
  const uint64_t c = d[0], len = d[2], n = len ? (len + 1023) / 1024 : 1;
  const uint64_t first = (c >> gl) << gl, n_groups = (n + G - 1) >> gl;
  const uint32_t gn = (uint32_t)(n - first < G ? n - first : G), ci = (uint32_t)(c - first);
  const bool live = valid && i < gn, leader = live && i == ci;
  const uint32_t P = path_len(c, n), U = path_len(c >> gl, n_groups);     // the whole path, its stored part
  const uint64_t lc = first + i, off = lc * 1024;
  const uint32_t bytes = live ? (uint32_t)(len - off < 1024 ? len - off : 1024) : 0;
  const uint32_t n_blocks = bytes ? (bytes + 63) / 64 : 1;
  uint32_t *r = recs + d[1] * 32;
  uint32_t h[8];
  if (live) {
    group_chunk(ARENA ? src + d[5] + off : src + ((uint64_t)s << (10 + gl)) + (uint64_t)i * 1024, bytes, lc, P, n == 1 ? 8u : 0u, leader ? r : nullptr, h);
    reinterpret_cast<uint4 *>(cv + lane * 8)[0] = make_uint4(h[0], h[1], h[2], h[3]);
    reinterpret_cast<uint4 *>(cv + lane * 8)[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
  // 2. the group's tree; sib: the leader's picks, bottom up
  uint32_t sib[6 * 8], low = 0;
  for (uint32_t l = 0; l < gl; ++l) {                                     // (uniform: the workgroup is this one wave)
    lds_barrier();
    if (leader) {
      const uint32_t i0 = (ci >> (l + 1)) << (l + 1), i1 = i0 + (1u << l);
      if (i1 < gn) {                                                      // (else the leader's subtree waits at this level)
        const uint32_t *src = cv + (base + (((c >> low) & 1) == 0 ? i1 : i0)) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) sib[low * 8 + k] = src[k];
        low++;
      }
    }
    lds_barrier();
    if (live && (i & ((2u << l) - 1)) == 0 && i + (1u << l) < gn)
      merge_pair<true>(cv, lane, lane + (1u << l), nullptr, 4u | (n_groups == 1 && (2u << l) >= gn ? 8u : 0u));
  }
  lds_barrier();
  // 3. the stored part, top down
  const uint32_t *ob = reinterpret_cast<const uint32_t *>(obs + d[3]);
  uint64_t pos[64], lefts = 0;
  {
    uint64_t p = 0, cc = c >> gl, m = n_groups;
    for (uint32_t j = 0; j < U; ++j) {
      uint64_t k2 = 1;
      while (k2 * 2 < m) k2 *= 2;
      pos[j] = p;
      if (cc < k2) { lefts |= 1ull << j; p += 1; m = k2; } else { p += k2; cc -= k2; m -= k2; }
    }
  }
  bool node_bad = false;
  if (valid) {
    for (uint32_t j = i; j < U; j += G) {
      const uint32_t *node = ob + 2 + pos[j] * 16;
      uint32_t mw[16], ivv[8], o[8];
#pragma unroll
      for (int k = 0; k < 16; ++k) mw[k] = node[k];
      iv(ivv);
      blake3_cv(ivv, mw, 0, 0, 64, 4u | (j == 0 ? 8u : 0u), o);
      const uint32_t *want = j == 0 ? roots + d[4] * 8 : ob + 2 + pos[j - 1] * 16 + (((lefts >> (j - 1)) & 1) ? 0 : 8);
      if (!eq8(o, want)) node_bad = true;
    }
  }
  const uint64_t bad_lanes = __ballot(node_bad);
  if (!leader) return;
  const uint32_t *want = U == 0 ? roots + d[4] * 8 : ob + 2 + pos[U - 1] * 16 + (((lefts >> (U - 1)) & 1) ? 0 : 8);
  int32_t st = 0;
  if (((uint64_t)ob[0] | ((uint64_t)ob[1] << 32)) != len) st = 3;
  else if ((bad_lanes >> base) & (G == 64 ? ~0ull : (1ull << G) - 1)) st = 2;
  else if (!eq8(cv + base * 8, want)) st = 1;
  status[s] = st;
  // 4. the parent records, bottom up: h is the leader's chunk CV
  r += (uint64_t)n_blocks * 32;
  for (uint32_t g = 0; g < P; ++g, r += 32) {
    const bool bit_left = ((c >> g) & 1) == 0;
    const uint32_t *m8;
    if (g < low) m8 = sib + g * 8;
    else { const uint32_t *node = ob + 2 + pos[U - 1 - (g - low)] * 16; m8 = bit_left ? node + 8 : node; }   // (P = low + U)
    plan_parent_step(r, h, m8, bit_left, c, n_blocks, P, P - 1 - g);
  }
}

// ---- bao slices (ABI 1.4) ------------------------------------------------------------------------------------------------
// slice of chunk c = header (8) || the P nodes of c's path root first (64 each) || the chunk's bytes.  Packed slices start at 8 modulo 16
// (b3w_bao_slice_batch_layout), so the nodes and the chunk's bytes, which follow the 8-byte header, lie on 16-byte boundaries.
// desc of the two extraction kernels: desc[5 s ..] = chunk, the slice's byte offset in `slices`, the file's length, the byte offset of its
// outboard in `obs`, the file.

// 16 bytes from src (8-byte aligned: a node's quarter in an outboard, or chunk bytes) to dst (16-byte aligned).
// ANY: src at any alignment (chunk bytes where they lie in an arena).  The load width is the source's natural alignment, so that no load
// straddles its own width and none reaches outside the 16 bytes moved: 16 bytes from a source at 0 modulo 16, 8 at 8, 4 at 4 and 12, single
// bytes from every other one, put together in registers; the store is one 16-byte store either way.
template <bool ANY>
__device__ __forceinline__ void move16(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src) {
  uint4 v;
  if (((uintptr_t)src & 15) == 0) {
    v = *reinterpret_cast<const uint4 *>(src);
  } else if (!ANY || ((uintptr_t)src & 7) == 0) {
    const uint2 a = reinterpret_cast<const uint2 *>(src)[0], b = reinterpret_cast<const uint2 *>(src)[1];
    v = make_uint4(a.x, a.y, b.x, b.y);
  } else if (((uintptr_t)src & 3) == 0) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(src);
    v = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = (uint32_t)src[4 * k] | ((uint32_t)src[4 * k + 1] << 8) | ((uint32_t)src[4 * k + 2] << 16) | ((uint32_t)src[4 * k + 3] << 24);
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  *reinterpret_cast<uint4 *>(dst) = v;
}

// the sampled chunk's `bytes` bytes to dst (16-byte aligned), lane t of T: whole 16-byte pieces where src is 8-byte aligned, the ragged
// tail (or everything, from an odd src) byte-wise.  ANY: whole pieces from a source at any alignment (move16<true>), the tail byte-wise.
template <bool ANY>
__device__ __forceinline__ void move_chunk(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes, uint32_t t, uint32_t T) {
  uint32_t whole = 0;
  if (ANY || ((uintptr_t)src & 7) == 0) {
    whole = bytes & ~15u;
    for (uint32_t o = t * 16; o < whole; o += T * 16) move16<ANY>(dst + o, src + o);
  }
  for (uint32_t o = whole + t; o < bytes; o += T) dst[o] = src[o];
}

// from full outboards: a gather, 16 lanes a sample.  Every lane walks the path (integer work); node j is moved by the four lanes t with
// t / 4 == j mod 4, a quarter each, then all 16 move the chunk's bytes.
constexpr uint32_t SLICE_LANES = 16;
// ARENA: src is the arena and the table has the file's offset in it (b3w_sample_plan_arena_kernel).  <false>: the gathered bytes
// (b3w_bao_slice_batch_device), <true>: the arena (b3w_bao_slice_arena_device).
template <bool ARENA>
__global__ __launch_bounds__(256) void b3w_bao_slice_kernel(const uint8_t *__restrict__ obs, const uint64_t *__restrict__ desc, uint32_t n_samples,
                                                            const uint8_t *__restrict__ src, uint8_t *__restrict__ slices) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, s = tid / SLICE_LANES, t = tid % SLICE_LANES;
  if (s >= n_samples) return;
  const uint64_t *d = desc + (ARENA ? 6 : 5) * (uint64_t)s;
  const uint64_t c = d[0], len = d[2], n = len ? (len + 1023) / 1024 : 1;
  const uint8_t *ob = obs + d[3];
  uint8_t *sl = slices + d[1];
  const uint32_t P = path_len(c, n);
  if (t == 0) *reinterpret_cast<uint2 *>(sl) = *reinterpret_cast<const uint2 *>(ob);          // the header as the outboard has it
  uint64_t p = 0, cc = c, m = n;
  for (uint32_t j = 0; j < P; ++j) {
    if ((j & 3) == (t >> 2)) move16<false>(sl + 8 + 64 * (uint64_t)j + (t & 3) * 16, ob + 8 + p * 64 + (t & 3) * 16);
    uint64_t k2 = 1;
    while (k2 * 2 < m) k2 *= 2;
    if (cc < k2) { p += 1; m = k2; } else { p += k2; cc -= k2; m -= k2; }
  }
  const uint64_t off = c * 1024;
  move_chunk<ARENA>(sl + 8 + 64 * (uint64_t)P, ARENA ? src + d[5] + off : src + (uint64_t)s * 1024, (uint32_t)(len - off < 1024 ? len - off : 1024), t,
                    SLICE_LANES);
}

// from group outboards: phases 1 and 2 of b3w_sample_plan_group_kernel (lane = one chunk of one sample's group, the chunk CVs into LDS, the
// in-place merge).  Before the merge of level l the node of the sampled chunk's path at that level, where it exists, is cv[i0] || cv[i1]:
// the first lanes of the sample store it whole to its place in the slice (the k-th that exists bottom up at node P - 1 - k).  Then the U
// stored nodes from the group outboard to the slice's first U places, the header and the sampled chunk's bytes, over the sample's G lanes.
// ARENA: src is the arena and the table has the file's offset in it (b3w_sample_plan_arena_kernel); gb is where the sample's group starts.
// <false>: the gathered bytes (b3w_bao_slice_batch_device), <true>: the arena (b3w_bao_slice_arena_device).
template <bool ARENA>
__global__ __launch_bounds__(64) void b3w_bao_slice_group_kernel(const uint8_t *__restrict__ obs, const uint64_t *__restrict__ desc, uint32_t n_samples,
                                                                 uint32_t gl, const uint8_t *__restrict__ src, uint8_t *__restrict__ slices) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[64 * 8];
  const uint32_t lane = threadIdx.x, G = 1u << gl, i = lane & (G - 1), base = lane - i;
  const uint32_t s = blockIdx.x * (64u >> gl) + (lane >> gl);
  const bool valid = s < n_samples;
  const uint64_t *d = desc + (ARENA ? 6 : 5) * (uint64_t)(valid ? s : 0);   // (a wave's lanes past the last sample read sample 0's row and write nothing)
  const uint64_t c = d[0], len = d[2], n = len ? (len + 1023) / 1024 : 1;
  const uint64_t first = (c >> gl) << gl, n_groups = (n + G - 1) >> gl;
  const uint32_t gn = (uint32_t)(n - first < G ? n - first : G), ci = (uint32_t)(c - first);
  const bool live = valid && i < gn;
  const uint32_t P = path_len(c, n), U = path_len(c >> gl, n_groups);     // the whole path, its stored part
  const uint64_t lc = first + i, off = lc * 1024;
  const uint32_t bytes = live ? (uint32_t)(len - off < 1024 ? len - off : 1024) : 0;
  const uint8_t *gb = ARENA ? src + d[5] + first * 1024 : src + ((uint64_t)s << (10 + gl));
  uint8_t *sl = slices + d[1];
  if (live) {
    uint32_t h[8];
    group_chunk(gb + (uint64_t)i * 1024, bytes, lc, P, n == 1 ? 8u : 0u, nullptr, h);
    reinterpret_cast<uint4 *>(cv + lane * 8)[0] = make_uint4(h[0], h[1], h[2], h[3]);
    reinterpret_cast<uint4 *>(cv + lane * 8)[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
  uint32_t low = 0;
  for (uint32_t l = 0; l < gl; ++l) {                                     // (uniform: the workgroup is this one wave)
    lds_barrier();
    const uint32_t i0 = (ci >> (l + 1)) << (l + 1), i1 = i0 + (1u << l);
    if (i1 < gn) {                                                        // (else the path's subtree waits at this level: no node)
      if (valid && low < P)
        for (uint32_t q = i; q < 4; q += G)                               // quarter q of the node: the halves of cv[i0], then of cv[i1]
          *reinterpret_cast<uint4 *>(sl + 8 + 64 * (uint64_t)(P - 1 - low) + q * 16) = reinterpret_cast<const uint4 *>(cv + (base + (q < 2 ? i0 : i1)) * 8)[q & 1];
      low++;
    }
    lds_barrier();
    if (live && (i & ((2u << l) - 1)) == 0 && i + (1u << l) < gn)
      merge_pair<true>(cv, lane, lane + (1u << l), nullptr, 4u | (n_groups == 1 && (2u << l) >= gn ? 8u : 0u));
  }
  lds_barrier();
  if (!valid) return;
  const uint8_t *ob = obs + d[3];
  if (i == 0) *reinterpret_cast<uint2 *>(sl) = *reinterpret_cast<const uint2 *>(ob);
  uint64_t p = 0, cc = c >> gl, m = n_groups;
  for (uint32_t j = 0; j < U; ++j) {                                      // (P = low + U: the stored nodes fill the places in front)
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
      if (((j * 4 + q) & (G - 1)) == i) move16<false>(sl + 8 + 64 * (uint64_t)j + q * 16, ob + 8 + p * 64 + q * 16);
    uint64_t k2 = 1;
    while (k2 * 2 < m) k2 *= 2;
    if (cc < k2) { p += 1; m = k2; } else { p += k2; cc -= k2; m -= k2; }
  }
  const uint64_t offc = c * 1024;
  move_chunk<ARENA>(sl + 8 + 64 * (uint64_t)P, gb + (uint64_t)ci * 1024, (uint32_t)(len - offc < 1024 ? len - offc : 1024), i, G);
}

// ---- challenged paths from slices ------------------------------------------------------------------------------------
// The prover's side: the slice is all there is.  K lanes a sample (64 / K samples a wave):
//   1. lane 0 of the sample (the leader) runs the chunk's blocks and writes the leaf records (plan_leaf_chunk on the slice's bytes)
//   2. the P nodes lie side by side, so their checks do not wait for each other: node j on lane j mod K — node 0 with ROOT against the
//      file's root, node j against its half of node j - 1 — and one ballot for the verdict; the leader holds the chunk's CV against its half
//      of node P - 1 (P == 0: its ROOT-flagged output against the root)
//   3. the parent records.  Record g carries the running value h of the reference's fold, which follows the index bits: P more compressions
//      one after the other (plan_parent_step, the leader).  Where the sample verified and its path is provable (the index bits are the
//      tree's own directions) that chain is redundant: every node hashed to its half of the node above, so h at height g IS the on-path
//      half of node P - 1 - g, and the K lanes write record g = t, t + K, ... straight from the nodes.  Any other sample — a failed check,
//      a path of an incomplete tree that is not provable — gets the chained words.
// desc[5 s ..] = chunk, first row, the file's length, the slice's byte offset in `slices`, the file.

// the words of plan_parent_step's record from a known h
__device__ __forceinline__ void parent_record(uint32_t *__restrict__ r, const uint32_t *h, const uint32_t *m8, uint64_t c, uint32_t n_blocks, uint32_t plen,
                                              uint32_t depth) {
  r[0] = n_blocks; r[1] = n_blocks;
#pragma unroll
  for (int k = 0; k < 8; ++k) r[2 + k] = h[k];
  r[10] = (uint32_t)c; r[11] = (uint32_t)(c >> 32);
  r[12] = plen + 1; r[13] = plen + 1; r[14] = depth;
#pragma unroll
  for (int k = 0; k < 8; ++k) { r[15 + k] = m8[k]; r[23 + k] = 0; }
  r[31] = 64;
}

template <int K>
__global__ __launch_bounds__(64) void b3w_sample_plan_slices_kernel(const uint8_t *__restrict__ slices, const uint32_t *__restrict__ roots,
                                                                    const uint64_t *__restrict__ desc, uint32_t n_samples, uint32_t always_chain,
                                                                    uint32_t *__restrict__ recs, int32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x, t = lane & (K - 1), base = lane - t;
  const uint32_t s = blockIdx.x * (64u / K) + lane / K;
  const bool valid = s < n_samples, leader = valid && t == 0;
  const uint64_t *d = desc + 5 * (uint64_t)(valid ? s : 0);              // (lanes past the last sample read sample 0's row and write nothing)
  const uint64_t c = d[0], len = d[2], n = len ? (len + 1023) / 1024 : 1;
  const uint8_t *sl = slices + d[3];
  const uint32_t *nodes = reinterpret_cast<const uint32_t *>(sl + 8);     // (16-byte aligned)
  const uint32_t P = path_len(c, n);
  const uint64_t off = c * 1024;
  const uint32_t bytes = (uint32_t)(len - off < 1024 ? len - off : 1024);
  const uint32_t n_blocks = bytes ? (bytes + 63) / 64 : 1;
  uint32_t *r = recs + d[1] * 32;
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (leader) plan_leaf_chunk(sl + 8 + 64 * (uint64_t)P, bytes, c, P, r, h);
  // the tree's own directions, root first (bit j: left at node j), and whether the index bits spell them (b3w_plan_path_provable)
  uint64_t lefts = 0;
  bool provable = true;
  {
    uint64_t cc = c, m = n;
    for (uint32_t j = 0; j < P; ++j) {
      uint64_t k2 = 1;
      while (k2 * 2 < m) k2 *= 2;
      const bool left = cc < k2;
      if (left) { lefts |= 1ull << j; m = k2; } else { cc -= k2; m -= k2; }
      if (left != (((c >> (P - 1 - j)) & 1) == 0)) provable = false;
    }
  }
  const uint32_t *root8 = roots + d[4] * 8;
  bool node_bad = false;
  if (valid) {
    for (uint32_t j = t; j < P; j += K) {
      const uint4 *q = reinterpret_cast<const uint4 *>(nodes + j * 16);
      const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      const uint32_t mw[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
      uint32_t ivv[8], o[8];
      iv(ivv);
      blake3_cv(ivv, mw, 0, 0, 64, 4u | (j == 0 ? 8u : 0u), o);
      const uint32_t *want = j == 0 ? root8 : nodes + (j - 1) * 16 + (((lefts >> (j - 1)) & 1) ? 0 : 8);
      if (!eq8(o, want)) node_bad = true;
    }
  }
  const uint64_t bad_lanes = __ballot(node_bad);
  int32_t st = 0;
  if (leader) {
    const uint32_t *want = P == 0 ? root8 : nodes + (P - 1) * 16 + (((lefts >> (P - 1)) & 1) ? 0 : 8);
    const uint32_t *hd = reinterpret_cast<const uint32_t *>(sl);
    if (((uint64_t)hd[0] | ((uint64_t)hd[1] << 32)) != len) st = 3;
    else if ((bad_lanes >> base) & ((1ull << K) - 1)) st = 2;
    else if (!eq8(h, want)) st = 1;                                       // (one chunk: its ROOT-flagged output against the root)
    status[s] = st;
  }
  if (K > 1) st = __shfl(st, (int)base);
  r += (uint64_t)n_blocks * 32;
  if (always_chain || st != 0 || !provable) {
    if (!leader) return;
    for (uint32_t g = 0; g < P; ++g, r += 32) {
      const uint32_t *node = nodes + (P - 1 - g) * 16;
      const bool bit_left = ((c >> g) & 1) == 0;
      plan_parent_step(r, h, bit_left ? node + 8 : node, bit_left, c, n_blocks, P, P - 1 - g);
    }
    return;
  }
  if (!valid) return;
  for (uint32_t g = t; g < P; g += K) {                                   // (g == 0 is the leader's: h is the chunk's CV)
    const uint32_t *node = nodes + (P - 1 - g) * 16;
    const bool bit_left = ((c >> g) & 1) == 0;
    parent_record(r + (uint64_t)g * 32, g == 0 ? h : (bit_left ? node : node + 8), bit_left ? node + 8 : node, c, n_blocks, P, P - 1 - g);
  }
}

// ---- slices taken in: the receiver's side ------------------------------------------------------------------------------
// The mirror image of b3w_bao_slice_kernel<true>: the slice is verified as b3w_sample_plan_slices_kernel verifies it (no records), and
// ONLY THEN its parts go to their places — the chunk's bytes into the file where it lies in the arena, the stored nodes of its path to
// their pre-order places in the file's outboard (gl = 0: all P; gl > 0: the first U = path_len(c >> gl, n_groups), the walk of
// b3w_bao_slice_group_kernel; the nodes inside the group are verified and dropped), the header in front.  K lanes a sample:
//   1. the sample's lane 0 (the leader) hashes the chunk from the slice (chunk_cv: 16-byte loads, the slice's bytes lie on a 16-byte
//      boundary); node j on lane j mod K against its half of node j - 1 (node 0 with ROOT against the root); one ballot; the leader's
//      verdict to the sample's K lanes by shuffle.  The leader-only stretch keeps 64 / K lanes of the wave busy, so the host takes K = 4
//      unless the batch's longest path is long enough to want sixteen lanes (b3w_bao_slice_ingest_device).
//   2. a sample whose verdict is not 0 has written its status and ends here.  The others: quarter q of stored node j by lane
//      (4 j + q) mod K, two 8-byte stores (an outboard's nodes lie 8 off a 16-byte boundary); then the chunk in 16-byte pieces, each
//      loaded whole from the slice and stored at the width the DESTINATION is aligned to (put16), the ragged tail byte-wise.
// Samples that name the same chunk, or share path nodes, store the same verified values to the same places.
// desc: the arena calls' row, {chunk, the slice's byte offset in `slices`, length, outboard offset, file, the file's arena offset}.

// 16 bytes from src (16-byte aligned) to dst at any alignment: the reverse of move16<true>.  The store width is the destination's natural
// alignment, so that no store straddles its own width and none reaches outside the 16 bytes moved: one 16-byte store to a destination at
// 0 modulo 16, two of 8 at 8, four of 4 at 4 and 12, single bytes to every other one.
__device__ __forceinline__ void put16(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src) {
  const uint4 v = *reinterpret_cast<const uint4 *>(src);
  if (((uintptr_t)dst & 15) == 0) {
    *reinterpret_cast<uint4 *>(dst) = v;
  } else if (((uintptr_t)dst & 7) == 0) {
    reinterpret_cast<uint2 *>(dst)[0] = make_uint2(v.x, v.y);
    reinterpret_cast<uint2 *>(dst)[1] = make_uint2(v.z, v.w);
  } else if (((uintptr_t)dst & 3) == 0) {
    uint32_t *w = reinterpret_cast<uint32_t *>(dst);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

// HAVE: a verified sample also ORs its chunk's bit into the arrival bitmap (b3w_bao_have_layout: chunk c of file f is bit c & 63 of word
// word_first[f] + (c >> 6)), one atomicOr by the sample's leader behind its stores; the word offsets lie behind the rows of `desc`.
// PACKED (b3w_bao_slice_ingest_packed_device): `arena` is a slot buffer and sample s's chunk goes to slot s of 1 024 bytes (16-byte
// aligned: put16 takes its widest store); a row has no arena offset (five words); `obs` may be null: nothing but the slot, the status
// and the bit is written (decode).
template <int K, bool HAVE = false, bool PACKED = false>
__global__ __launch_bounds__(64) void b3w_bao_slice_ingest_kernel(const uint8_t *__restrict__ slices, const uint32_t *__restrict__ roots,
                                                                  const uint64_t *__restrict__ desc, uint32_t n_samples, uint32_t gl,
                                                                  uint8_t *__restrict__ arena, uint8_t *__restrict__ obs, int32_t *__restrict__ status,
                                                                  unsigned long long *__restrict__ have) {
  const uint32_t lane = threadIdx.x, t = lane & (K - 1), base = lane - t;
  const uint32_t s = blockIdx.x * (64u / K) + lane / K;
  const bool valid = s < n_samples, leader = valid && t == 0;
  constexpr uint32_t W = PACKED ? 5 : 6;                                  // the words of a row
  const uint64_t *d = desc + W * (uint64_t)(valid ? s : 0);              // (lanes past the last sample read sample 0's row and write nothing)
  const uint64_t c = d[0], len = d[2], n = len ? (len + 1023) / 1024 : 1;
  const uint8_t *sl = slices + d[1];
  const uint32_t *nodes = reinterpret_cast<const uint32_t *>(sl + 8);     // (16-byte aligned)
  const uint32_t P = path_len(c, n);
  const uint64_t off = c * 1024;
  const uint32_t bytes = (uint32_t)(len - off < 1024 ? len - off : 1024);
  const uint8_t *body = sl + 8 + 64 * (uint64_t)P;
  // 1. the verdict
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (leader) chunk_cv(body, bytes, c, n == 1 ? 8u : 0u, h);
  uint64_t lefts = 0;                                                     // the tree's own directions, root first (bit j: left at node j)
  {
    uint64_t cc = c, m = n;
    for (uint32_t j = 0; j < P; ++j) {
      uint64_t k2 = 1;
      while (k2 * 2 < m) k2 *= 2;
      if (cc < k2) { lefts |= 1ull << j; m = k2; } else { cc -= k2; m -= k2; }
    }
  }
  const uint32_t *root8 = roots + d[4] * 8;
  bool node_bad = false;
  if (valid) {
    for (uint32_t j = t; j < P; j += K) {
      const uint4 *q = reinterpret_cast<const uint4 *>(nodes + j * 16);
      const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      const uint32_t mw[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
      uint32_t ivv[8], o[8];
      iv(ivv);
      blake3_cv(ivv, mw, 0, 0, 64, 4u | (j == 0 ? 8u : 0u), o);
      const uint32_t *want = j == 0 ? root8 : nodes + (j - 1) * 16 + (((lefts >> (j - 1)) & 1) ? 0 : 8);
      if (!eq8(o, want)) node_bad = true;
    }
  }
  const uint64_t bad_lanes = __ballot(node_bad);
  int32_t st = 0;
  if (leader) {
    const uint32_t *want = P == 0 ? root8 : nodes + (P - 1) * 16 + (((lefts >> (P - 1)) & 1) ? 0 : 8);
    const uint32_t *hd = reinterpret_cast<const uint32_t *>(sl);
    if (((uint64_t)hd[0] | ((uint64_t)hd[1] << 32)) != len) st = 3;
    else if ((bad_lanes >> base) & ((1ull << K) - 1)) st = 2;
    else if (!eq8(h, want)) st = 1;                                       // (one chunk: its ROOT-flagged output against the root)
    status[s] = st;
  }
  if (K > 1) st = __shfl(st, (int)base);
  if (!valid || st != 0) return;                                          // nothing unverified is written
  // 2. the places
  if (!PACKED || obs) {
    uint8_t *ob = obs + d[3];
    if (t == 0) *reinterpret_cast<uint2 *>(ob) = *reinterpret_cast<const uint2 *>(sl);          // the header (it is the length: just checked)
    const uint64_t n_groups = (n + (1ull << gl) - 1) >> gl;
    const uint32_t U = path_len(c >> gl, n_groups);                         // (gl = 0: P)
    uint64_t p = 0, cc = c >> gl, m = n_groups;
    for (uint32_t j = 0; j < U; ++j) {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (((j * 4 + q) & (K - 1)) == t) {
          const uint4 v = *reinterpret_cast<const uint4 *>(sl + 8 + 64 * (uint64_t)j + q * 16);
          uint2 *node = reinterpret_cast<uint2 *>(ob + 8 + p * 64 + q * 16);
          node[0] = make_uint2(v.x, v.y);
          node[1] = make_uint2(v.z, v.w);
        }
      uint64_t k2 = 1;
      while (k2 * 2 < m) k2 *= 2;
      if (cc < k2) { p += 1; m = k2; } else { p += k2; cc -= k2; m -= k2; }
    }
  }
  uint8_t *dst;
  if constexpr (PACKED) dst = arena + 1024 * (uint64_t)s; else dst = arena + d[5] + off;
  const uint32_t whole = bytes & ~15u;
  for (uint32_t o = t * 16; o < whole; o += K * 16) put16(dst + o, body + o);
  for (uint32_t o = whole + t; o < bytes; o += K) dst[o] = body[o];
  if (HAVE && t == 0) atomicOr(have + desc[W * (uint64_t)n_samples + d[4]] + (c >> 6), 1ull << (c & 63));
}

// ---- verification: whole files against their outboards ---------------------------------------------------------------------
// Bao's decoder applied to every UNIT of every file at once (a unit: a chunk, or with group outboards a group of 1 << gl chunks).  The
// mirror image of the three batch kernels: where those store a node, these load the stored node from the same pre-order place, hold the
// two CVs in their LDS slots (what the children claim to be) against the node's halves, and leave hash(stored node) in slot i0 — so
// above the lowest level a slot holds what the STORED child node hashes to, and every check is stored data against stored data: a bad
// chunk marks its own unit, a bad node the units below it.  Inside a group there is no stored node: merge_pair<true> computes up to the
// group's CV and the comparison starts there.
//   b3w_bao_verify_upper_kernel  the storey above the tiles, which needs no file bytes and runs BEFORE the tile kernel: one workgroup
//                                per 1 024 tiles (and, for files past 1 GiB, first one per 1 024 of those), the stored nodes over them
//                                checked bottom up in LDS; leaves per tile the CV its tile must have (the stored half in the lowest node
//                                above it) and a "path above is bad" flag in the scratch; a file's top workgroup initialises the file's
//                                status and first bad unit
//   b3w_bao_verify_tile_kernel   one workgroup per tile, lane = chunk: chunk CVs, the tile's stored nodes, the tile's CV against the
//                                scratch (one-tile file: its ROOT-hashed root node against the root); every unit's final status, one
//                                byte a lane; the per-file outputs by reduction (one-tile file) or atomicMax / atomicMin (others)
//   b3w_bao_verify_small_kernel  the files of at most 64 chunks, several to a wave, everything in the wave
// Mismatch flags, one word per slot: bit l = the subtree of 1 << l items that starts at this slot (a child at level l) is not the half
// its stored parent holds for it; bit VER_TOP = the whole tile / file (slot 0) is not what is expected from above; VER_UNIT = the same
// for a subtree that is a single unit, whose claim comes from the file's bytes (status 1, not 2).  An item's path is bad where bit l of
// slot (item >> l) << l is set for some l: that slot starts the item's subtree at level l, whether it was paired there or waited.
struct VerFile { uint64_t ufirst, slot, gslot; };         // a file's first unit in the packed statuses; its first tile's / group's scratch entry
constexpr uint32_t VER_UNIT = 1u << 31, VER_TOP = 1u << 10;

__device__ __forceinline__ void load_node(const uint8_t *__restrict__ node, uint32_t m[16]) {   // (8 off a 16-byte boundary)
  const uint2 *s = reinterpret_cast<const uint2 *>(node);
#pragma unroll
  for (int k = 0; k < 8; ++k) { const uint2 v = s[k]; m[2 * k] = v.x; m[2 * k + 1] = v.y; }
}

// one stored parent at level l: slots i0 (left) and i1 (right) against the halves of the node at `node`, hash(node) to slot i0.  A child
// over at most `leaf` chunks is a single unit (CLAIM: its slot holds its CV from the bytes) or a single item with no claim yet (!CLAIM:
// its half goes to exp_out, the CV expected of it); sl, sr: the children's chunk counts.
template <bool CLAIM>
__device__ __forceinline__ void check_pair(uint32_t *cv, uint32_t *flags, uint32_t i0, uint32_t i1, uint32_t l, const uint8_t *__restrict__ node,
                                           uint32_t d, uint64_t sl, uint64_t sr, uint64_t leaf, uint32_t *__restrict__ exp_out) {
  uint32_t m[16], ivv[8], o[8];
  load_node(node, m);
  if (sl <= leaf) {
    if (CLAIM) { if (!eq8(cv + i0 * 8, m)) flags[i0] |= VER_UNIT; }
    else {
#pragma unroll
      for (int k = 0; k < 8; ++k) exp_out[(uint64_t)i0 * 8 + k] = m[k];
    }
  } else if (!eq8(cv + i0 * 8, m)) flags[i0] |= 1u << l;
  if (sr <= leaf) {
    if (CLAIM) { if (!eq8(cv + i1 * 8, m + 8)) flags[i1] |= VER_UNIT; }
    else {
#pragma unroll
      for (int k = 0; k < 8; ++k) exp_out[(uint64_t)i1 * 8 + k] = m[8 + k];
    }
  } else if (!eq8(cv + i1 * 8, m + 8)) flags[i1] |= 1u << l;
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, d, o);
  put_cv(cv, i0, o);                                                 // (slot i0 is this thread's alone at this level)
}

// merge_in_lds with the stores turned into checks: cnt items of `unit` chunks of a tree over `total` chunks whose root's place in the
// file's outboard (groups of 1 << gl chunks; gl = 0: the full outboard) is `nodes`.  Leaves hash(the tree's stored root node) in cv[0 .. 8)
// (cnt == 1: the item's own slot untouched) and the children's flags in `flags` (zeroed by the caller); ends with a barrier.
template <int BS, bool CLAIM>
__device__ __forceinline__ void verify_in_lds(uint32_t *cv, uint32_t *flags, uint32_t cnt, uint64_t unit, uint64_t total,
                                              const uint8_t *__restrict__ nodes, bool root, uint32_t gl, uint32_t *__restrict__ exp_out) {
  const uint64_t G = 1ull << gl, leaf = CLAIM ? G : unit;
  tree_levels<BS, true>(cnt, unit, total, root, [&](uint32_t l, uint32_t i0, uint32_t i1, uint64_t a, uint64_t size, uint32_t d) {
    if (CLAIM && size <= G) { merge_pair<true>(cv, i0, i1, nullptr, d); return; }               // inside a group: computed
    const uint64_t sl = ((uint64_t)unit) << l;
    check_pair<CLAIM>(cv, flags, i0, i1, l, nodes + node_pos<true>(total, a, size, gl) * 64, d, sl, size - sl, leaf, exp_out);
  });
}

// the OR of the node flags on item t's path
__device__ __forceinline__ bool path_bad(const uint32_t *flags, uint32_t t) {
  uint32_t x = 0;
#pragma unroll
  for (uint32_t l = 0; l <= 10; ++l) x |= flags[(t >> l) << l] & (1u << l);
  return x != 0;
}

// The storey above the tiles of one file (len bytes, more than one tile, its outboard at ob): workgroup g takes up to 1 024 items of `unit`
// chunks each (B3W_TILE: the items are tiles; B3W_TILE^2, the launch for files past 1 GiB, which runs first: groups of tiles).
// Scratch entries: an expected CV of 8 words and a "path above is bad" word.  exp_in / bad_in: the workgroup's own entry, left by the
// launch before (unused by the file's top workgroup, which takes `root`); exp_out / bad_out: the entry of its first item.
__device__ __forceinline__ void verify_upper(uint64_t len, uint64_t g, uint64_t unit, const uint8_t *__restrict__ ob, const uint32_t *root,
                                             const uint32_t *exp_in, const uint32_t *bad_in, uint32_t *exp_out, uint32_t *bad_out, uint32_t gl,
                                             int32_t *file_status, unsigned long long *first_bad) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t flags[B3W_TILE];
  const uint64_t n = (len + 1023) / 1024;
  const uint64_t span = unit * B3W_TILE, a0 = g * span;
  const uint64_t tot = n - a0 < span ? n - a0 : span;
  const uint32_t cnt = (uint32_t)((tot + unit - 1) / unit);
  const bool sole = n <= span;                                        // the file's top workgroup
  const uint32_t *want = sole ? root : exp_in;
  bool above = sole ? false : *bad_in != 0;
  if (sole && threadIdx.x == 0) {                                     // (the tile kernel, which runs after this one, adds to these)
    const bool hdr = !header_is(ob, len);
    *file_status = hdr ? 3 : 0;
    *first_bad = hdr ? 0ull : ~0ull;
  }
  if (cnt == 1) {                                                     // a lone last tile (or group) hangs straight off the storey above
    if (threadIdx.x < 8) exp_out[threadIdx.x] = want[threadIdx.x];
    if (threadIdx.x == 0) *bad_out = above;
    return;
  }
  for (uint32_t i = threadIdx.x; i < cnt; i += 256) flags[i] = 0;
  verify_in_lds<256, false>(cv, flags, cnt, unit, tot, ob + 8 + node_pos<true>(n, a0, tot, gl) * 64, sole, gl, exp_out);
  above = above || !eq8(cv, want);
  for (uint32_t t = threadIdx.x; t < cnt; t += 256) bad_out[t] = above || path_bad(flags, t);
}

// Scratch entries: the tiles' first (n_tile_ents of them), then the groups'.
__global__ __launch_bounds__(256) void b3w_bao_verify_upper_kernel(const BatchEnt *__restrict__ ents, uint32_t n_ents, uint64_t unit,
                                                                   const VerFile *__restrict__ vf, uint64_t n_tile_ents,
                                                                   const uint8_t *__restrict__ outboards, const uint32_t *__restrict__ roots,
                                                                   uint32_t *__restrict__ exp_cv, uint32_t *__restrict__ bad, uint32_t gl,
                                                                   int32_t *__restrict__ file_status, unsigned long long *__restrict__ first_bad) {
  const BatchEnt e = batch_ent(ents, n_ents, blockIdx.x);
  const VerFile v = vf[e.file];
  const uint64_t g = blockIdx.x - e.first;
  const uint64_t out0 = unit == B3W_TILE ? v.slot + g * B3W_TILE : n_tile_ents + v.gslot, in = n_tile_ents + v.gslot + g;
  verify_upper(e.len, g, unit, outboards + e.ob, roots + (uint64_t)e.file * 8, exp_cv + in * 8, bad + in, exp_cv + out0 * 8, bad + out0, gl,
               file_status + e.file, first_bad + e.file);
}

// One tile against the file's outboard: the tile of chunks from a0 (its bytes at base + 1024 at) of a file of len bytes and n chunks.  exp / bad:
// the tile's scratch entry from the storey above (unused by a file of this one tile, which takes `root`); unit_status: the status byte of
// the file's unit 0; lone: lane_chunk_cv's.  The per-file outputs by reduction (one-tile file) or atomicMax / atomicMin (others).
__device__ __forceinline__ void verify_tile(const uint8_t *__restrict__ base, uint64_t at, uint64_t len, uint64_t n, uint64_t a0, bool lone,
                                            const uint8_t *__restrict__ ob, const uint32_t *root, const uint32_t *exp, const uint32_t *bad,
                                            uint32_t gl, uint8_t *unit_status, int32_t *file_status, unsigned long long *first_bad) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t flags[B3W_TILE];
  __shared__ uint32_t worst, first;
  const uint32_t t = threadIdx.x, G = 1u << gl;
  const uint32_t m = (uint32_t)(n - a0 < B3W_TILE ? n - a0 : B3W_TILE);
  const bool sole = n <= B3W_TILE;
  tile_chunk_cvs(cv, base, at, len, n, a0, m, lone);
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; }
  const bool hdr = !header_is(ob, len);
  verify_in_lds<B3W_TILE, true>(cv, flags, m, 1, m, ob + 8 + node_pos<true>(n, a0, m, gl) * 64, sole, gl, nullptr);
  if (t == 0 && !eq8(cv, sole ? root : exp)) flags[0] |= m <= G ? VER_UNIT : VER_TOP;
  const bool above = sole ? false : *bad != 0;
  lds_barrier();
  if (t < m && (t & (G - 1)) == 0) {                                  // a unit's first chunk: its status
    const uint32_t st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    unit_status[(a0 + t) >> gl] = (uint8_t)st;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t >> gl); }    // (LDS; a clean tile issues none)
  }
  __syncthreads();
  if (t != 0) return;
  if (sole) {
    *file_status = (int32_t)worst;
    *first_bad = worst ? (unsigned long long)first : ~0ull;
  } else if (worst) {                                                 // (initialised by the file's top workgroup of the storey above)
    atomicMax(file_status, (int32_t)worst);
    atomicMin(first_bad, (unsigned long long)((a0 >> gl) + first));
  }
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_verify_tile_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents, uint32_t n_ents,
                                                                       const VerFile *__restrict__ vf, const uint8_t *__restrict__ outboards,
                                                                       const uint32_t *__restrict__ roots, const uint32_t *__restrict__ exp_cv,
                                                                       const uint32_t *__restrict__ bad, uint32_t gl, uint8_t *__restrict__ unit_status,
                                                                       int32_t *__restrict__ file_status, unsigned long long *__restrict__ first_bad) {
  const BatchEnt e = batch_ent(ents, n_ents, blockIdx.x);
  const VerFile v = vf[e.file];
  const uint32_t tile = blockIdx.x - e.first;
  const uint64_t a0 = (uint64_t)tile * B3W_TILE, ent = v.slot + tile;
  verify_tile(arena + e.off, a0, e.len, (e.len + 1023) / 1024, a0, false, outboards + e.ob, roots + (uint64_t)e.file * 8,   // (more than 64 chunks)
              exp_cv + ent * 8, bad + ent, gl, unit_status + v.ufirst, file_status + e.file, first_bad + e.file);
}

// small_body's wave with every stored node of a file checked by the lane that would have stored it (cv: the chunk CVs from small_lane;
// `first`: the lane of the file's chunk 0).  Returns the status of the unit whose first chunk the lane holds, in `is_unit` whether it
// holds one.
__device__ __forceinline__ uint32_t small_verify(uint32_t *cv, uint32_t *flags, uint64_t len, uint32_t first, uint32_t n, uint32_t i, bool live,
                                                 const uint8_t *__restrict__ ob, const uint32_t *root, uint32_t gl, bool &is_unit) {
  const uint32_t lane = threadIdx.x, G = 1u << gl;
  flags[lane] = 0;
  const bool hdr = !header_is(ob, len);
  small_levels<true>(n, i, live, [&](uint32_t l, uint32_t size, uint32_t d) {
    if (size <= G) merge_pair<true>(cv, lane, lane + (1u << l), nullptr, d);
    else check_pair<true>(cv, flags, lane, lane + (1u << l), l, ob + 8 + node_pos<true>(n, i, size, gl) * 64, d, 1u << l, size - (1u << l), G, nullptr);
  });
  // the file's top (its ROOT-flagged CV, or what its stored root node hashes to with ROOT) against the root; bit 6: above every level here
  if (live && i == 0 && !eq8(cv + lane * 8, root)) flags[lane] |= n <= G ? VER_UNIT : 1u << 6;
  lds_barrier();
  is_unit = live && (i & (G - 1)) == 0;
  if (!is_unit) return 0;
  uint32_t x = 0;
#pragma unroll
  for (uint32_t l = 0; l <= 6; ++l) x |= flags[first + ((i >> l) << l)] & (1u << l);
  return hdr ? 3u : x ? 2u : (flags[lane] & VER_UNIT) ? 1u : 0u;
}

// the files of at most 64 chunks; the per-file outputs from ballots over the file's lanes
__global__ __launch_bounds__(64) void b3w_bao_verify_small_kernel(const uint8_t *__restrict__ arena, const BatchEnt *__restrict__ ents,
                                                                  const uint32_t *__restrict__ wave_first, const VerFile *__restrict__ vf,
                                                                  const uint8_t *__restrict__ outboards, const uint32_t *__restrict__ roots, uint32_t gl,
                                                                  uint8_t *__restrict__ unit_status, int32_t *__restrict__ file_status,
                                                                  unsigned long long *__restrict__ first_bad) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[64 * 8];
  __shared__ uint32_t flags[64];
  const SmallLane<BatchEnt> s = small_lane(cv, arena, ents, wave_first);
  const BatchEnt &e = s.e;
  bool is_unit;
  const uint32_t st = small_verify(cv, flags, e.len, e.first, s.n, s.i, s.live, outboards + e.ob, roots + (uint64_t)e.file * 8, gl, is_unit);
  if (is_unit) unit_status[vf[e.file].ufirst + (s.i >> gl)] = (uint8_t)st;
  const uint64_t mine = (s.n == 64 ? ~0ull : (1ull << s.n) - 1) << e.first;
  const uint64_t b1 = __ballot(st >= 1) & mine, b2 = __ballot(st >= 2) & mine, b3 = __ballot(st >= 3) & mine;
  if (s.live && s.i == 0) {
    file_status[e.file] = b3 ? 3 : b2 ? 2 : b1 ? 1 : 0;
    first_bad[e.file] = b1 ? (unsigned long long)((__ffsll((unsigned long long)b1) - 1 - e.first) >> gl) : ~0ull;
  }
}

// ---- streamed files: one file of known length whose bytes arrive in windows of whole tiles -------------------------------------
// A tile is a subtree of the file's tree whatever else is known of the file, and the place of every node below its root follows from
// the file's length and the tile's ABSOLUTE index alone.  So the kernels of a window are the tile kernels with the file's entry by value
// (no table in device memory: a push uploads nothing) and the tile's bytes taken from the window, not from arena + offset:
//   b3w_bao_stream_tile[_group]_kernel   a workgroup per tile of the window: tile_outboard, the tile's CV to scratch slot `tile`.
//                                        A file of one tile, down to one chunk (ROOT on the chunk) or no byte at all, ends here too:
//                                        its root and header, the bytes the small kernel writes for it
//   b3w_bao_stream_merge[_group]_kernel  finish: merge_storey over the tile CVs in scratch (files past 1 GiB: once more over the groups')
//   b3w_bao_stream_upper_kernel          verification, at begin: verify_upper for the one file, from the stored nodes alone
//   b3w_bao_stream_verify_kernel         a workgroup per tile of the window: verify_tile, exp_cv / bad read at `tile`
// Every one of these bodies is the batch kernels' own (one definition, above); a stream kernel only says where the one file's fields are.
// window: the bytes of the file from tile `tile0` on; workgroup w takes tile tile0 + w
template <bool GRP>
__device__ __forceinline__ void stream_tile_body(const uint8_t *__restrict__ window, uint32_t w, uint64_t len, uint32_t tile0, uint8_t *__restrict__ ob,
                                                 uint32_t *__restrict__ root, uint32_t *__restrict__ tile_cv, uint32_t gl) {
  const uint64_t n = len ? (len + 1023) / 1024 : 1, tile = (uint64_t)tile0 + w;
  tile_outboard<GRP>(window, (uint64_t)w * B3W_TILE, len, n, tile * B3W_TILE, true, ob, root, tile_cv + tile * 8, gl);
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_tile_kernel(const uint8_t *__restrict__ window, uint64_t len, uint32_t tile0,
                                                                       uint8_t *__restrict__ ob, uint32_t *__restrict__ root,
                                                                       uint32_t *__restrict__ tile_cv) {
  stream_tile_body<false>(window, blockIdx.x, len, tile0, ob, root, tile_cv, 0);
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_tile_group_kernel(const uint8_t *__restrict__ window, uint64_t len, uint32_t tile0,
                                                                             uint8_t *__restrict__ ob, uint32_t *__restrict__ root,
                                                                             uint32_t *__restrict__ tile_cv, uint32_t gl) {
  stream_tile_body<true>(window, blockIdx.x, len, tile0, ob, root, tile_cv, gl);
}

// the merge storey of the one file (more than one tile): workgroup g merges items [1 024 g, ...) of in_cv, its CV to out_cv slot g or the root
__global__ __launch_bounds__(256) void b3w_bao_stream_merge_kernel(uint64_t len, uint64_t unit, const uint32_t *__restrict__ in_cv,
                                                                   uint32_t *__restrict__ out_cv, uint8_t *__restrict__ ob, uint32_t *__restrict__ root) {
  const uint64_t g = blockIdx.x;
  merge_storey<false>((len + 1023) / 1024, g, unit, in_cv + g * B3W_TILE * 8, ob, root, out_cv + g * 8, 0);
}
__global__ __launch_bounds__(256) void b3w_bao_stream_merge_group_kernel(uint64_t len, uint64_t unit, const uint32_t *__restrict__ in_cv,
                                                                         uint32_t *__restrict__ out_cv, uint8_t *__restrict__ ob,
                                                                         uint32_t *__restrict__ root, uint32_t gl) {
  const uint64_t g = blockIdx.x;
  merge_storey<true>((len + 1023) / 1024, g, unit, in_cv + g * B3W_TILE * 8, ob, root, out_cv + g * 8, gl);
}

// verify_upper for the one file (more than one tile).  Scratch entries as in the batch: the tiles' (n_tile_ents), then the groups'.
__global__ __launch_bounds__(256) void b3w_bao_stream_upper_kernel(uint64_t len, uint64_t unit, uint64_t n_tile_ents, const uint8_t *__restrict__ ob8,
                                                                   const uint32_t *__restrict__ root, uint32_t *__restrict__ exp_cv,
                                                                   uint32_t *__restrict__ bad, uint32_t gl, int32_t *__restrict__ file_status,
                                                                   unsigned long long *__restrict__ first_bad) {
  const uint64_t g = blockIdx.x, out0 = unit == B3W_TILE ? g * B3W_TILE : n_tile_ents, in = n_tile_ents + g;
  verify_upper(len, g, unit, ob8, root, exp_cv + in * 8, bad + in, exp_cv + out0 * 8, bad + out0, gl, file_status, first_bad);
}

// verify_tile for tile tile0 + w of a window, exp_cv / bad read at the tile's index; a file of one tile, down to one chunk or no byte at
// all, is settled here whole
__device__ __forceinline__ void stream_verify_body(const uint8_t *__restrict__ window, uint32_t w, uint64_t len, uint32_t tile0, const uint8_t *__restrict__ ob,
                                                   const uint32_t *root, const uint32_t *exp_cv, const uint32_t *bad, uint32_t gl, uint8_t *unit_status,
                                                   int32_t *file_status, unsigned long long *first_bad) {
  const uint64_t n = len ? (len + 1023) / 1024 : 1, tile = (uint64_t)tile0 + w;
  verify_tile(window, (uint64_t)w * B3W_TILE, len, n, tile * B3W_TILE, true, ob, root, exp_cv + tile * 8, bad + tile, gl,
              unit_status, file_status, first_bad);
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_verify_kernel(const uint8_t *__restrict__ window, uint64_t len, uint32_t tile0,
                                                                         const uint8_t *__restrict__ ob8, const uint32_t *__restrict__ root,
                                                                         const uint32_t *__restrict__ exp_cv, const uint32_t *__restrict__ bad,
                                                                         uint32_t gl, uint8_t *__restrict__ unit_status,
                                                                         int32_t *__restrict__ file_status, unsigned long long *__restrict__ first_bad) {
  stream_verify_body(window, blockIdx.x, len, tile0, ob8, root, exp_cv, bad, gl, unit_status, file_status, first_bad);
}

// ---- many stream sessions in one launch ----------------------------------------------------------------------------------------------
// The windows of many sessions, each a file of its own, as ONE grid: what the stream kernels take by value, or from blockIdx.x, comes from
// a table with a row per (session, window) entry, found by bisection over the rows' first workgroups as batch_ent finds a file.  The
// work on a tile is the stream kernels' own bodies, called with the row's fields, so the bytes are theirs.
//   b3w_bao_stream_tile_many[_group]_kernel   stream_tile_body per workgroup.  The group kernel takes gl from the row, and at gl = 0 it
//                                             stores every node where the plain kernel does (a parent is over 2 chunks or more): a call
//                                             that mixes full and group outboards is one launch of the group kernel
//   b3w_bao_stream_verify_many_kernel         verify_tile's work, restated (it measured slower through the shared body)
//   b3w_bao_stream_merge_many[_group]_kernel  merge_storey; a row per session of more than one tile (unit = B3W_TILE) or of more
//                                             than 1 024 tiles (unit = B3W_TILE^2)
// cv / aux: tile kernels: the session's tile CVs / unused; verify: exp_cv / bad; merge: the input CVs / the output CVs
struct ManyRow {
  uint64_t len;
  const uint8_t *window;                                 // the bytes of the file from tile `tile0` on
  uint8_t *ob;
  uint32_t *root, *cv, *aux;
  uint8_t *unit_status;
  int32_t *file_status;
  unsigned long long *first_bad;
  uint32_t first, tile0, gl, pad;                        // first: the entry's first workgroup
};

// p as a pointer the compiler knows to be device memory (by way of an integer: it folds a cast there and straight back away)
template <class P>
__device__ __forceinline__ P *as_global(P *p) { return (P *)(__attribute__((address_space(1))) P *)(uintptr_t)p; }

__device__ __forceinline__ ManyRow many_row(const ManyRow *__restrict__ rows, uint32_t n_rows, uint32_t wg) {
  ManyRow r = rows[find_first(rows, 0, n_rows, wg)];
  // (a pointer loaded from memory is a generic one to the compiler, and its loads and stores would be flat ones, which count against the
  // LDS counter too; these are device memory, as the stream kernels' arguments are known to be)
  r.window = as_global(r.window); r.ob = as_global(r.ob); r.root = as_global(r.root); r.cv = as_global(r.cv); r.aux = as_global(r.aux);
  r.unit_status = as_global(r.unit_status); r.file_status = as_global(r.file_status); r.first_bad = as_global(r.first_bad);
  return r;
}

template <bool GRP>
__device__ __forceinline__ void many_tile_body(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  const ManyRow r = many_row(rows, n_rows, blockIdx.x);
  stream_tile_body<GRP>(r.window, blockIdx.x - r.first, r.len, r.tile0, r.ob, r.root, r.cv, GRP ? r.gl : 0);
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_tile_many_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  many_tile_body<false>(rows, n_rows);
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_tile_many_group_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  many_tile_body<true>(rows, n_rows);
}

// workgroup g of a row merges items [1 024 g, ...) of the row's input CVs, its CV to output slot g or the root
template <bool GRP>
__device__ __forceinline__ void many_merge_body(const ManyRow *__restrict__ rows, uint32_t n_rows, uint64_t unit) {
  const ManyRow r = many_row(rows, n_rows, blockIdx.x);
  const uint64_t n = (r.len + 1023) / 1024, g = blockIdx.x - r.first;
  merge_storey<GRP>(n, g, unit, r.cv + g * B3W_TILE * 8, r.ob, r.root, r.aux + g * 8, GRP ? r.gl : 0);
}

__global__ __launch_bounds__(256) void b3w_bao_stream_merge_many_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows, uint64_t unit) {
  many_merge_body<false>(rows, n_rows, unit);
}
__global__ __launch_bounds__(256) void b3w_bao_stream_merge_many_group_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows, uint64_t unit) {
  many_merge_body<true>(rows, n_rows, unit);
}

// verify_in_lds<B3W_TILE, true> with tree_levels's loop written out, for the kernel below alone
__device__ __forceinline__ void verify_many_walk(uint32_t *cv, uint32_t *flags, uint32_t cnt, uint64_t unit, uint64_t total,
                                                 const uint8_t *__restrict__ nodes, bool root, uint32_t gl) {
  const uint64_t G = 1ull << gl, G1 = G - 1, leaf = G;
  for (uint32_t l = 0; (1u << l) < cnt; ++l) {
    lds_barrier();
    const bool top = (2u << l) >= cnt;
    for (uint32_t j = threadIdx.x;; j += B3W_TILE) {
      const uint32_t i0 = (2 * j) << l, i1 = i0 + (1u << l);
      if (i1 >= cnt) break;
      const uint64_t a = i0 * unit, e = (uint64_t)(i0 + (2u << l)) * unit, size = (e < total ? e : total) - a;
      const uint32_t d = 4u | (top && root ? 8u : 0u);
      if (size <= G) { merge_pair<true>(cv, i0, i1, nullptr, d); continue; }                   // inside a group: computed
      const uint64_t sl = ((uint64_t)unit) << l;
      check_pair<true>(cv, flags, i0, i1, l, nodes + preorder_pos((total + G1) >> gl, a >> gl, (size + G1) >> gl) * 64, d, sl, size - sl, leaf, nullptr);
    }
  }
  lds_barrier();
}

// verify_tile and its walk restated with the row's fields: through verify_tile this kernel measured 0.02 to 0.2 % slower at gl = 0 (profiles/r21/bao_shared_bodies_ab.json)
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_verify_many_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t flags[B3W_TILE];
  __shared__ uint32_t worst, first;
  const ManyRow r = many_row(rows, n_rows, blockIdx.x);
  const uint32_t w = blockIdx.x - r.first, gl = r.gl;
  const uint64_t len = r.len, n = len ? (len + 1023) / 1024 : 1;
  const uint32_t t = threadIdx.x, G = 1u << gl;
  const uint64_t tile = (uint64_t)r.tile0 + w, a0 = tile * B3W_TILE;
  const uint32_t m = (uint32_t)(n - a0 < B3W_TILE ? n - a0 : B3W_TILE);
  const bool sole = n <= B3W_TILE;
  tile_chunk_cvs(cv, r.window, (uint64_t)w * B3W_TILE, len, n, a0, m, true);
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; }
  const uint32_t *ob = reinterpret_cast<const uint32_t *>(r.ob);
  const bool hdr = ((uint64_t)ob[0] | ((uint64_t)ob[1] << 32)) != len;
  const uint64_t G1 = G - 1;
  verify_many_walk(cv, flags, m, 1, m, r.ob + 8 + preorder_pos((n + G1) >> gl, a0 >> gl, (m + G1) >> gl) * 64, sole, gl);
  if (t == 0 && !eq8(cv, sole ? r.root : r.cv + tile * 8)) flags[0] |= m <= G ? VER_UNIT : VER_TOP;
  const bool above = sole ? false : r.aux[tile] != 0;
  lds_barrier();
  if (t < m && (t & (G - 1)) == 0) {                                  // a unit's first chunk: its status
    const uint32_t st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    r.unit_status[(a0 + t) >> gl] = (uint8_t)st;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t >> gl); }    // (LDS; a clean tile issues none)
  }
  __syncthreads();
  if (t != 0) return;
  if (sole) {
    *r.file_status = (int32_t)worst;
    *r.first_bad = worst ? (unsigned long long)first : ~0ull;
  } else if (worst) {                                                 // (initialised at begin by the file's top workgroup of the storey above)
    atomicMax(r.file_status, (int32_t)worst);
    atomicMin(r.first_bad, (unsigned long long)((a0 >> gl) + first));
  }
}

// ---- updates in place: outboards of resident files after writes to some of their chunks ------------------------------------------------
// A stored node is left CV || right CV, so the CV of every clean sibling on a dirty chunk's path is in the outboard already: only the dirty
// chunks are hashed from bytes, and only the nodes with a dirty unit below them are written, each dirty half alone (b3wit.h "updates in
// place").  The storeys are the batch kernels': a workgroup per DIRTY tile, then one per span of 1 024 tiles that holds a dirty tile (and
// once more over the spans' CVs for files past 1 GiB).  Files of at most 64 chunks are rehashed whole by b3w_bao_small[_group]_kernel.
//   b3w_bao_update_tile[_group]_kernel    lane = chunk; the lanes of dirty chunks hash; the sparse merge; the tile's CV to its compact
//                                         scratch slot, or (a one-tile file) the ROOT-flagged top merge to the file's root
//   b3w_bao_update_merge[_group]_kernel   the same merge over the tiles of a span (unit = B3W_TILE) or the spans of a file (B3W_TILE^2): the
//                                         dirty items' CVs from consecutive scratch slots (the rows are sorted: slot = base + dirty items below)
// A row per workgroup, indexed by blockIdx.x.  mask: bit i = item i of the workgroup (a chunk of the tile, a tile of the span, a span of the
// file) is dirty; the host expands chunk masks to whole groups, so inside a dirty group every chunk is hashed and nothing is loaded.
struct UpdRow {
  uint64_t len;
  const uint8_t *data;                                   // the file's first byte (tile rows; packed: the slot of the tile's first dirty chunk)
  uint8_t *ob;                                           // the file's outboard, header first
  uint32_t *root;
  uint32_t *in;                                          // merge rows: the scratch slot of the workgroup's first dirty item
  uint32_t *out;                                         // the workgroup's own scratch slot (unused where its top merge is the file's)
  uint32_t idx, gl;                                      // the tile within the file / the span within the file (0 one storey up)
  uint32_t mask[B3W_TILE / 32];
};

// one parent of the sparse merge: a dirty half from its LDS slot, a clean half from the stored node; the dirty halves alone are stored,
// the parent's CV goes to slot i0.  GRP: a null `node` is a node inside a (dirty) chunk group: both halves are in LDS, nothing is stored.
template <bool GRP>
__device__ __forceinline__ void update_pair(uint32_t *cv, uint32_t i0, uint32_t i1, bool d0, bool d1, uint8_t *__restrict__ node, uint32_t d) {
  uint32_t m[16], ivv[8], o[8];
  uint2 *nd = reinterpret_cast<uint2 *>(node);                       // (8 off a 16-byte boundary)
  const bool inside = GRP && !node;
  if (d0 || inside) {
    const uint4 l0 = reinterpret_cast<const uint4 *>(cv + i0 * 8)[0], l1 = reinterpret_cast<const uint4 *>(cv + i0 * 8)[1];
    m[0] = l0.x; m[1] = l0.y; m[2] = l0.z; m[3] = l0.w; m[4] = l1.x; m[5] = l1.y; m[6] = l1.z; m[7] = l1.w;
    if (!inside) { nd[0] = make_uint2(m[0], m[1]); nd[1] = make_uint2(m[2], m[3]); nd[2] = make_uint2(m[4], m[5]); nd[3] = make_uint2(m[6], m[7]); }
  } else {
    const uint2 a = nd[0], b = nd[1], c = nd[2], e = nd[3];
    m[0] = a.x; m[1] = a.y; m[2] = b.x; m[3] = b.y; m[4] = c.x; m[5] = c.y; m[6] = e.x; m[7] = e.y;
  }
  if (d1 || inside) {
    const uint4 r0 = reinterpret_cast<const uint4 *>(cv + i1 * 8)[0], r1 = reinterpret_cast<const uint4 *>(cv + i1 * 8)[1];
    m[8] = r0.x; m[9] = r0.y; m[10] = r0.z; m[11] = r0.w; m[12] = r1.x; m[13] = r1.y; m[14] = r1.z; m[15] = r1.w;
    if (!inside) { nd[4] = make_uint2(m[8], m[9]); nd[5] = make_uint2(m[10], m[11]); nd[6] = make_uint2(m[12], m[13]); nd[7] = make_uint2(m[14], m[15]); }
  } else {
    const uint2 a = nd[4], b = nd[5], c = nd[6], e = nd[7];
    m[8] = a.x; m[9] = a.y; m[10] = b.x; m[11] = b.y; m[12] = c.x; m[13] = c.y; m[14] = e.x; m[15] = e.y;
  }
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, d, o);
  put_cv(cv, i0, o);                                                 // (slot i0 is this thread's alone at this level)
}

// merge_in_lds over the dirty items alone: dirty[i] says whether slot i holds a CV (an item with a dirty chunk below it).  A pair with no
// dirty child is skipped; any other one leaves its CV in slot i0 and marks it; an odd item out waits and keeps its flag.  The arguments are
// merge_in_lds's; ends with a barrier, the tree's CV in cv[0 .. 8) where the tree holds a dirty item.  (tree_levels's loop written out: see there.)
template <int BS, bool GRP>
__device__ __forceinline__ void update_in_lds(uint32_t *cv, uint32_t *dirty, uint32_t cnt, uint64_t unit, uint64_t total, uint8_t *__restrict__ nodes,
                                              bool root, uint32_t gl) {
  for (uint32_t l = 0; (1u << l) < cnt; ++l) {
    lds_barrier();
    const bool top = (2u << l) >= cnt;
    for (uint32_t j = threadIdx.x;; j += BS) {
      const uint32_t i0 = (2 * j) << l, i1 = i0 + (1u << l);
      if (i1 >= cnt) break;
      const bool d0 = dirty[i0] != 0, d1 = dirty[i1] != 0;
      if (!d0 && !d1) continue;
      const uint64_t a = i0 * unit, e = (uint64_t)(i0 + (2u << l)) * unit, size = (e < total ? e : total) - a;
      update_pair<GRP>(cv, i0, i1, d0, d1, node_at<GRP>(nodes, total, a, size, gl), 4u | (top && root ? 8u : 0u));
      dirty[i0] = 1;
    }
  }
  lds_barrier();
}

// the items of a row's mask below item t: where the rows are sorted, the place of item t among the workgroup's listed ones
__device__ __forceinline__ uint32_t mask_rank(const uint32_t *mask, uint32_t t) {
  uint32_t below = __popc(mask[t >> 5] & ((1u << (t & 31)) - 1));
  for (uint32_t k = 0; k < (t >> 5); ++k) below += __popc(mask[k]);
  return below;
}

// PACKED (b3w_bao_outboard_update_packed_device): r->data is the slot of the tile's first dirty chunk in the packed buffer and a dirty
// chunk lies behind the tile's dirty chunks below it; its counter and its length stay those of chunk a0 + t
template <bool GRP, bool PACKED>
__device__ __forceinline__ void update_tile_body(const UpdRow *__restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t dirty[B3W_TILE];
  const UpdRow *__restrict__ r = rows + blockIdx.x;
  const uint32_t t = threadIdx.x, gl = GRP ? r->gl : 0;
  const uint64_t len = r->len, n = (len + 1023) / 1024;               // (more than 64 chunks)
  const uint64_t a0 = (uint64_t)r->idx * B3W_TILE;
  const uint32_t m = (uint32_t)(n - a0 < B3W_TILE ? n - a0 : B3W_TILE);
  const bool sole = n <= B3W_TILE;
  const bool mine = t < m && ((r->mask[t >> 5] >> (t & 31)) & 1u);
  dirty[t] = mine ? 1u : 0u;
  if (mine) lane_chunk_cv(cv, as_global(r->data), PACKED ? mask_rank(r->mask, t) : a0 + t, len, n, a0 + t, false);
  update_in_lds<B3W_TILE, GRP>(cv, dirty, m, 1, m, as_global(r->ob) + 8 + node_pos<GRP>(n, a0, m, gl) * 64, sole, gl);   // (a tile starts at a multiple of every group size)
  if (t < 8) as_global(sole ? r->root : r->out)[t] = cv[t];            // (the row's mask is not empty: slot 0 holds the tile's CV)
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_update_tile_kernel(const UpdRow *__restrict__ rows) { update_tile_body<false, false>(rows); }
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_update_tile_group_kernel(const UpdRow *__restrict__ rows) { update_tile_body<true, false>(rows); }
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_update_tile_packed_kernel(const UpdRow *__restrict__ rows) { update_tile_body<false, true>(rows); }
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_update_tile_packed_group_kernel(const UpdRow *__restrict__ rows) { update_tile_body<true, true>(rows); }

// unit = chunks per input item, as in merge_storey; the workgroup's items are [1 024 idx, ...) of the file's
template <bool GRP>
__device__ __forceinline__ void update_merge_body(const UpdRow *__restrict__ rows, uint64_t unit) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t dirty[B3W_TILE];
  const UpdRow *__restrict__ r = rows + blockIdx.x;
  const uint32_t gl = GRP ? r->gl : 0;
  const uint64_t n = (r->len + 1023) / 1024;                          // (more than one tile)
  const uint64_t span = unit * B3W_TILE, a0 = (uint64_t)r->idx * span;
  const uint64_t tot = n - a0 < span ? n - a0 : span;
  const uint32_t cnt = (uint32_t)((tot + unit - 1) / unit);
  const bool sole = n <= span;
  const uint32_t *__restrict__ in = as_global(r->in);
  for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
    const uint32_t w = r->mask[i >> 5], bit = 1u << (i & 31);
    dirty[i] = (w & bit) ? 1u : 0u;
    if (w & bit) {                                                    // its CV: the slot behind those of the dirty items below it
      uint32_t below = __popc(w & (bit - 1));
      for (uint32_t k = 0; k < (i >> 5); ++k) below += __popc(r->mask[k]);
      const uint4 *src = reinterpret_cast<const uint4 *>(in + (uint64_t)below * 8);
      reinterpret_cast<uint4 *>(cv + i * 8)[0] = src[0];
      reinterpret_cast<uint4 *>(cv + i * 8)[1] = src[1];
    }
  }
  update_in_lds<256, GRP>(cv, dirty, cnt, unit, tot, as_global(r->ob) + 8 + node_pos<GRP>(n, a0, tot, gl) * 64, sole, gl);   // (every node here is over more than a tile: all are stored)
  if (threadIdx.x < 8) as_global(sole ? r->root : r->out)[threadIdx.x] = cv[threadIdx.x];
}

__global__ __launch_bounds__(256) void b3w_bao_update_merge_kernel(const UpdRow *__restrict__ rows, uint64_t unit) { update_merge_body<false>(rows, unit); }
__global__ __launch_bounds__(256) void b3w_bao_update_merge_group_kernel(const UpdRow *__restrict__ rows, uint64_t unit) { update_merge_body<true>(rows, unit); }

// ---- ranged verification: listed chunk ranges of resident files against their outboards ------------------------------------------------
// The update's sparse walk with check_pair where the update has its sparse merge (b3wit.h "verification of listed chunk ranges"): only
// the LISTED units are hashed from bytes, only the stored nodes with a listed unit below them are loaded, and what is checked of such a
// node is what verify_in_lds checks of it — its listed halves against the claims in LDS, its own hash against its half of the node
// above.  A clean half is no claim and is not looked at.  The storeys run top down as in the whole-file call:
//   b3w_bao_verify_ranges_upper_kernel   a workgroup per span of 1 024 tiles that holds a listed tile (unit = B3W_TILE; before it, for
//                                        files past 1 GiB, one per file over its listed spans, unit = B3W_TILE^2): leaves, for each
//                                        LISTED item, the CV it must have and the flags of the path above in the item's compact
//                                        scratch entry (entry = the workgroup's base + the listed items below it: the rows are sorted)
//   b3w_bao_verify_ranges_tile_kernel    a workgroup per listed tile, lane = chunk, the lanes of listed units alone hash: the status byte
//                                        of every listed unit and of no other
//   b3w_bao_verify_ranges_small_kernel   the listed files of at most 64 chunks, verified whole: b3w_bao_verify_small_kernel's wave with
//                                        the entry by row (no per-file table, no per-file outputs)
//   b3w_bao_verify_ranges_reduce_kernel  a workgroup per range AS THE CALLER GAVE IT: the largest status byte and the first non-zero
//                                        one among the units the range touches, written plainly (nothing to clear, no global atomic)
// A row per workgroup, indexed by blockIdx.x; mask as in UpdRow (expanded to whole groups by the host).  The word an upper workgroup
// leaves beside an expected CV: VR_PATH = a stored node above fails, VR_HDR = the header is not the length (read once, by the file's top
// workgroup; a one-tile file's tile reads it itself).
struct VrRow {
  uint64_t len;
  const uint8_t *data;                                   // the file's first byte (tile rows; packed: the slot of the tile's first listed chunk)
  const uint8_t *ob;                                     // the file's outboard, header first
  const uint32_t *root;
  const uint32_t *want;                                  // the workgroup's own scratch entry: 8 words of CV ... (unused by a file's top workgroup)
  const uint32_t *above;                                 // ... and its word
  uint32_t *out_cv, *out_word;                           // upper rows: the entry of the workgroup's first listed item
  uint8_t *unit_status;                                  // tile rows: the status byte of the file's unit 0
  uint32_t idx, gl;                                      // the tile within the file / the span within the file (0 one storey up)
  uint32_t mask[B3W_TILE / 32];
};
struct VrSmall { uint64_t off, len; const uint8_t *ob; const uint32_t *root; uint8_t *unit_status; uint32_t first, pad; };
struct VrRange { const uint8_t *units; uint64_t first, count; };      // status bytes [first, first + count) of the file whose unit 0 is at `units`
constexpr uint32_t VR_PATH = 1u, VR_HDR = 2u;

// check_pair over the listed halves alone (d0, d1: the half has a listed unit below it).  !CLAIM: rank[i] = the listed items below item i,
// its entry behind exp_out.
template <bool CLAIM>
__device__ __forceinline__ void ranges_pair(uint32_t *cv, uint32_t *flags, const uint32_t *rank, uint32_t i0, uint32_t i1, bool d0, bool d1, uint32_t l,
                                            const uint8_t *__restrict__ node, uint32_t d, uint64_t sl, uint64_t sr, uint64_t leaf,
                                            uint32_t *__restrict__ exp_out) {
  uint32_t m[16], ivv[8], o[8];
  load_node(node, m);
  if (d0) {
    if (sl <= leaf) {
      if (CLAIM) { if (!eq8(cv + i0 * 8, m)) flags[i0] |= VER_UNIT; }
      else {
        const uint64_t at = (uint64_t)rank[i0] * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) exp_out[at + k] = m[k];
      }
    } else if (!eq8(cv + i0 * 8, m)) flags[i0] |= 1u << l;
  }
  if (d1) {
    if (sr <= leaf) {
      if (CLAIM) { if (!eq8(cv + i1 * 8, m + 8)) flags[i1] |= VER_UNIT; }
      else {
        const uint64_t at = (uint64_t)rank[i1] * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) exp_out[at + k] = m[8 + k];
      }
    } else if (!eq8(cv + i1 * 8, m + 8)) flags[i1] |= 1u << l;
  }
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, d, o);
  put_cv(cv, i0, o);                                                 // (slot i0 is this thread's alone at this level)
}

// verify_in_lds over the listed items alone: listed[i] says whether slot i holds a claim (CLAIM) or has a listed item below it.  A pair
// with no listed child is skipped: nothing loaded, nothing checked.  Any other one leaves hash(stored node) in slot i0 and marks it; an
// odd item out waits and keeps its mark.  Inside a (listed) group both halves are in LDS and nothing is loaded.  Ends with a barrier.
// (tree_levels's loop written out: see there.)
template <int BS, bool CLAIM>
__device__ __forceinline__ void ranges_in_lds(uint32_t *cv, uint32_t *flags, uint32_t *listed, const uint32_t *rank, uint32_t cnt, uint64_t unit,
                                              uint64_t total, const uint8_t *__restrict__ nodes, bool root, uint32_t gl, uint32_t *__restrict__ exp_out) {
  const uint64_t G = 1ull << gl, leaf = CLAIM ? G : unit;
  for (uint32_t l = 0; (1u << l) < cnt; ++l) {
    lds_barrier();
    const bool top = (2u << l) >= cnt;
    for (uint32_t j = threadIdx.x;; j += BS) {
      const uint32_t i0 = (2 * j) << l, i1 = i0 + (1u << l);
      if (i1 >= cnt) break;
      const bool d0 = listed[i0] != 0, d1 = listed[i1] != 0;
      if (!d0 && !d1) continue;
      const uint64_t a = i0 * unit, e = (uint64_t)(i0 + (2u << l)) * unit, size = (e < total ? e : total) - a;
      const uint32_t d = 4u | (top && root ? 8u : 0u);
      if (CLAIM && size <= G) { merge_pair<true>(cv, i0, i1, nullptr, d); continue; }          // inside a listed group: computed
      const uint64_t sl = ((uint64_t)unit) << l;
      ranges_pair<CLAIM>(cv, flags, rank, i0, i1, d0, d1, l, nodes + node_pos<true>(total, a, size, gl) * 64, d, sl, size - sl, leaf, exp_out);
      listed[i0] = 1;
    }
  }
  lds_barrier();
}

// unit = chunks per item, as in b3w_bao_verify_upper_kernel; the workgroup's items are [1 024 idx, ...) of the file's
__global__ __launch_bounds__(256) void b3w_bao_verify_ranges_upper_kernel(const VrRow *__restrict__ rows, uint64_t unit) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t flags[B3W_TILE], listed[B3W_TILE], rank[B3W_TILE];
  const VrRow *__restrict__ r = rows + blockIdx.x;
  const uint32_t gl = r->gl;
  const uint64_t len = r->len, n = (len + 1023) / 1024;               // (more than one tile)
  const uint64_t span = unit * B3W_TILE, a0 = (uint64_t)r->idx * span;
  const uint64_t tot = n - a0 < span ? n - a0 : span;
  const uint32_t cnt = (uint32_t)((tot + unit - 1) / unit);
  const bool sole = n <= span;                                        // the file's top workgroup
  const uint8_t *__restrict__ ob = as_global(r->ob);
  const uint32_t *__restrict__ want = as_global(sole ? r->root : r->want);
  uint32_t *__restrict__ out_cv = as_global(r->out_cv), *__restrict__ out_word = as_global(r->out_word);
  uint32_t above = sole ? (header_is(ob, len) ? 0u : VR_HDR) : *as_global(r->above);
  if (cnt == 1) {                                                    // a lone last tile (or span) hangs straight off the storey above
    if (threadIdx.x < 8) out_cv[threadIdx.x] = want[threadIdx.x];
    if (threadIdx.x == 0) out_word[0] = above;
    return;
  }
  for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
    const uint32_t w = r->mask[i >> 5], bit = 1u << (i & 31);
    uint32_t below = __popc(w & (bit - 1));
    for (uint32_t k = 0; k < (i >> 5); ++k) below += __popc(r->mask[k]);
    flags[i] = 0; listed[i] = (w & bit) ? 1u : 0u; rank[i] = below;
  }
  ranges_in_lds<256, false>(cv, flags, listed, rank, cnt, unit, tot, ob + 8 + node_pos<true>(n, a0, tot, gl) * 64, sole, gl, out_cv);
  if (!eq8(cv, want)) above |= VR_PATH;
  for (uint32_t t = threadIdx.x; t < cnt; t += 256)
    if ((r->mask[t >> 5] >> (t & 31)) & 1u) out_word[rank[t]] = above | (path_bad(flags, t) ? VR_PATH : 0u);
}

// PACKED (b3w_bao_verify_ranges_packed_device): as in update_tile_body
template <bool PACKED>
__device__ __forceinline__ void verify_ranges_tile_body(const VrRow *__restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  __shared__ uint32_t flags[B3W_TILE], listed[B3W_TILE];
  const VrRow *__restrict__ r = rows + blockIdx.x;
  const uint32_t t = threadIdx.x, gl = r->gl, G = 1u << gl;
  const uint64_t len = r->len, n = (len + 1023) / 1024;               // (more than 64 chunks)
  const uint64_t a0 = (uint64_t)r->idx * B3W_TILE;
  const uint32_t m = (uint32_t)(n - a0 < B3W_TILE ? n - a0 : B3W_TILE);
  const bool sole = n <= B3W_TILE;
  const bool mine = t < m && ((r->mask[t >> 5] >> (t & 31)) & 1u);
  const uint8_t *__restrict__ ob = as_global(r->ob);
  listed[t] = mine ? 1u : 0u;
  flags[t] = 0;
  if (mine) lane_chunk_cv(cv, as_global(r->data), PACKED ? mask_rank(r->mask, t) : a0 + t, len, n, a0 + t, false);
  const uint32_t above = sole ? (header_is(ob, len) ? 0u : VR_HDR) : *as_global(r->above);
  ranges_in_lds<B3W_TILE, true>(cv, flags, listed, nullptr, m, 1, m, ob + 8 + node_pos<true>(n, a0, m, gl) * 64, sole, gl, nullptr);
  // (the row's mask is not empty: slot 0 holds what the tile's stored root node hashes to, or the CV of a tile that is one unit)
  if (t == 0 && !eq8(cv, as_global(sole ? r->root : r->want))) flags[0] |= m <= G ? VER_UNIT : VER_TOP;
  lds_barrier();
  if (mine && (t & (G - 1)) == 0) {                                   // a listed unit's first chunk: its status
    const uint32_t st = (above & VR_HDR) ? 3u : (above & VR_PATH) || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    as_global(r->unit_status)[(a0 + t) >> gl] = (uint8_t)st;
  }
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_verify_ranges_tile_kernel(const VrRow *__restrict__ rows) { verify_ranges_tile_body<false>(rows); }
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_verify_ranges_tile_packed_kernel(const VrRow *__restrict__ rows) { verify_ranges_tile_body<true>(rows); }

// b3w_bao_verify_small_kernel with a row per file: wave w takes the rows [wave_first[w], wave_first[w + 1]), r.first = the lane of the
// file's chunk 0; every unit byte of the file is written, with the whole-file call's value; no per-file outputs
__global__ __launch_bounds__(64) void b3w_bao_verify_ranges_small_kernel(const uint8_t *__restrict__ arena, const VrSmall *__restrict__ rows,
                                                                         const uint32_t *__restrict__ wave_first, uint32_t gl) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[64 * 8];
  __shared__ uint32_t flags[64];
  const SmallLane<VrSmall> s = small_lane(cv, arena, rows, wave_first);
  const VrSmall &e = s.e;
  bool is_unit;
  const uint32_t st = small_verify(cv, flags, e.len, e.first, s.n, s.i, s.live, as_global(e.ob), as_global(e.root), gl, is_unit);
  if (is_unit) as_global(e.unit_status)[s.i >> gl] = (uint8_t)st;
}

// range_status / range_first_bad of range blockIdx.x from the status bytes the launches before this one wrote (16 at a time between
// the first and the last 16-byte boundary of the run)
__global__ __launch_bounds__(256) void b3w_bao_verify_ranges_reduce_kernel(const VrRange *__restrict__ ranges, int32_t *__restrict__ range_status,
                                                                           unsigned long long *__restrict__ range_first_bad) {
  __shared__ uint32_t worst;
  __shared__ unsigned long long first;
  const VrRange r = ranges[blockIdx.x];
  const uint8_t *__restrict__ u = as_global(r.units);
  if (threadIdx.x == 0) { worst = 0; first = ~0ull; }
  __syncthreads();
  uint32_t w = 0;
  unsigned long long f = ~0ull;
  const uint64_t lo = r.first, hi = r.first + r.count;
  const uint64_t mis = (16 - ((uintptr_t)(u + lo) & 15)) & 15;
  const uint64_t b0 = lo + (mis < r.count ? mis : r.count), b1 = b0 + ((hi - b0) & ~15ull);
  for (uint64_t i = lo + threadIdx.x; i < b0; i += 256) {
    const uint32_t s = u[i];
    if (s) { w = w > s ? w : s; f = f < i ? f : i; }
  }
  for (uint64_t i = b0 + (uint64_t)threadIdx.x * 16; i < b1; i += 256 * 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(u + i);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    if (v.x | v.y | v.z | v.w) {
#pragma unroll
      for (int k = 3; k >= 0; --k)
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          const uint32_t s = (q[k] >> (8 * b)) & 255u;
          if (s) { w = w > s ? w : s; const uint64_t at = i + 4 * k + b; f = f < at ? f : at; }
        }
    }
  }
  for (uint64_t i = b1 + threadIdx.x; i < hi; i += 256) {
    const uint32_t s = u[i];
    if (s) { w = w > s ? w : s; f = f < i ? f : i; }
  }
  if (w) { atomicMax(&worst, w); atomicMin(&first, f); }              // (LDS; a clean range issues none)
  __syncthreads();
  if (threadIdx.x == 0) {
    range_status[blockIdx.x] = (int32_t)worst;
    range_first_bad[blockIdx.x] = first;
  }
}

// ---- open-length sessions: full tiles hashed before the file's length is known -----------------------------------------------------------
// A FULL tile of 1 024 chunks is a complete subtree whatever the file's length turns out to be: its (1 024 >> gl) - 1 stored nodes are
// contiguous in the file's pre-order outboard, in the order merge_in_lds gives them relative to the tile's root, and only the START of that
// run depends on the total.  Its CV is never ROOT-flagged by the tile (a file of exactly one full tile: see the relocation kernel).  So:
//   b3w_bao_stream_open_tile[_group]_kernel       a workgroup per full tile of the window: chunk CVs into LDS, merge_in_lds with `nodes` at
//                                                 the tile's BLOCK of a staging area (block t = the nodes of tile t, tile-local order),
//                                                 the tile's CV to scratch slot `tile`.  No header, no root, no length.
//   b3w_bao_stream_open_tile_many[_group]_kernel  the same with the window, tile0, staging and scratch from a ManyRow (ob = the blocks)
//   b3w_bao_stream_open_relocate_kernel           at finish, the length known: every block to ob + 8 + 64 preorder_pos(...), and the header
//   b3w_bao_stream_open_relocate_many_kernel      the same for the sessions of a ManyRow table (window = the blocks, tile0 = the full tiles)
// The tile of the file's tail goes through b3w_bao_stream_tile[_group]_kernel and the storeys above through b3w_bao_stream_merge[_group]_kernel
// as they are.  Blocks start 8 bytes off a 16-byte boundary (the staging is 16-byte aligned and block 0 starts at byte 8), which is where
// the nodes of a 16-byte-aligned outboard lie: merge_pair's 8-byte stores are aligned, and the relocation moves an 8-byte head, a body of
// aligned 16-byte pieces and an 8-byte tail.
constexpr uint32_t OPEN_PIECE = 16384;                   // the most bytes of blocks one relocation workgroup moves
constexpr uint32_t OPEN_PAD = B3W_BAO_STREAM_OPEN_STAGING_PAD;                       // staging bytes that are no block's: 8 in front of block 0, 8 behind the last one
struct OpenShape { uint32_t bb, ppb, tpw_log; };         // a block's bytes; workgroups per block; log2 of the blocks per workgroup
__host__ __device__ __forceinline__ OpenShape open_shape(uint32_t gl) {
  OpenShape s;
  s.bb = ((B3W_TILE >> gl) - 1) * 64;                    // 65 472 (gl = 0) ... 960 (gl = 6)
  s.ppb = (s.bb + OPEN_PIECE - 1) / OPEN_PIECE;          // 4, 2, 1, 1, ...
  s.tpw_log = 0;                                         // 1, 1, 1, 2, 4, 8, 16 blocks
  while (s.tpw_log < 4 && (s.bb << (s.tpw_log + 1)) <= OPEN_PIECE) s.tpw_log++;
  return s;
}

// blocks: block 0's first byte; w: the tile's place in the window.  (Every chunk is whole and the file's length is not known: the lanes
// call chunk_cv with 1 024 bytes where the other tile bodies call tile_chunk_cvs with the length.)
template <bool GRP>
__device__ __forceinline__ void open_tile_body(const uint8_t *__restrict__ window, uint32_t w, uint64_t tile, uint8_t *__restrict__ blocks,
                                               uint32_t *__restrict__ tile_cv, uint32_t gl) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B3W_TILE * 8];
  uint32_t h[8];
  chunk_cv(window + ((uint64_t)w * B3W_TILE + threadIdx.x) * 1024, 1024, tile * B3W_TILE + threadIdx.x, 0, h);
  put_cv(cv, threadIdx.x, h);
  merge_in_lds<B3W_TILE, GRP>(cv, B3W_TILE, 1, B3W_TILE, blocks + tile * (((B3W_TILE >> gl) - 1) * 64), false, gl);
  if (threadIdx.x < 8) tile_cv[tile * 8 + threadIdx.x] = cv[threadIdx.x];
}

__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_open_tile_kernel(const uint8_t *__restrict__ window, uint32_t tile0,
                                                                            uint8_t *__restrict__ blocks, uint32_t *__restrict__ tile_cv) {
  open_tile_body<false>(window, blockIdx.x, (uint64_t)tile0 + blockIdx.x, blocks, tile_cv, 0);
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_open_tile_group_kernel(const uint8_t *__restrict__ window, uint32_t tile0,
                                                                                  uint8_t *__restrict__ blocks, uint32_t *__restrict__ tile_cv,
                                                                                  uint32_t gl) {
  open_tile_body<true>(window, blockIdx.x, (uint64_t)tile0 + blockIdx.x, blocks, tile_cv, gl);
}
// rows as the tile kernels of many sessions take them, with ob = the session's blocks (len, root and the rest unused)
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_open_tile_many_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  const ManyRow r = many_row(rows, n_rows, blockIdx.x);
  const uint32_t w = blockIdx.x - r.first;
  open_tile_body<false>(r.window, w, (uint64_t)r.tile0 + w, r.ob, r.cv, 0);
}
__global__ __launch_bounds__(B3W_TILE) void b3w_bao_stream_open_tile_many_group_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  const ManyRow r = many_row(rows, n_rows, blockIdx.x);
  const uint32_t w = blockIdx.x - r.first;
  open_tile_body<true>(r.window, w, (uint64_t)r.tile0 + w, r.ob, r.cv, r.gl);
}

// What one lane of relocation workgroup wg (of those of one file, open_shape(gl)) moves.  A workgroup takes a piece of at most OPEN_PIECE
// bytes of one block (gl <= 2) or 2 .. 16 whole blocks, L = 256 >> tpw_log lanes a block: bytes [at, at + nb) of the block of `tile`, as
// lane `lane` of L.  pos_tile: the tile whose pre-order place the lane needs — the workgroup's first where the workgroup has one block,
// so that the place is found once per workgroup.
struct BlockPiece { uint32_t tile, pos_tile, piece, lane, L, at, nb, bb; };
__device__ __forceinline__ BlockPiece block_piece(uint32_t gl, uint32_t wg) {
  const OpenShape s = open_shape(gl);
  BlockPiece p;
  p.L = 256u >> s.tpw_log; p.lane = threadIdx.x & (p.L - 1);
  const uint32_t wg_tile = (wg / s.ppb) << s.tpw_log;
  p.piece = wg % s.ppb;
  p.tile = wg_tile + (threadIdx.x >> (8 - s.tpw_log));
  p.pos_tile = s.tpw_log == 0 ? wg_tile : p.tile;
  p.bb = s.bb; p.at = p.piece * OPEN_PIECE;
  p.nb = s.bb - p.at < OPEN_PIECE ? s.bb - p.at : OPEN_PIECE;         // (a multiple of 64)
  return p;
}

// nb bytes of a block from src to dst by L lanes.  Source and destination are different buffers and no two workgroups share a byte of
// either.  Both at 8 modulo 16 (the blocks' phase in a staging area and in a 16-byte-aligned outboard): an 8-byte head, 16-byte pieces,
// an 8-byte tail; any other pair of phases: 8 bytes at a time.
__device__ __forceinline__ void move_piece(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nb, uint32_t lane, uint32_t L) {
  if (((uintptr_t)dst & 15) == 8 && ((uintptr_t)src & 15) == 8) {
    uint2 head = make_uint2(0, 0), tail = make_uint2(0, 0);
    if (lane == 0) { head = *reinterpret_cast<const uint2 *>(src); tail = *reinterpret_cast<const uint2 *>(src + nb - 8); }
    // the body: (nb - 16) / 16 <= 4 L pieces whatever gl is (nb <= OPEN_PIECE >> tpw_log, L = 256 >> tpw_log), so a lane has at most
    // four; all four loads are issued before the first store (the compiler cannot know that dst and src never meet), a lane with
    // fewer pieces loading the piece's first bytes again in place of a branch around the load.  The empty asm keeps the compiler
    // from sinking each load into the branch of its store, where every one would be waited for alone.
    uint4 v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) { const uint32_t o = 8 + (lane + k * L) * 16; v[k] = *reinterpret_cast<const uint4 *>(src + (o < nb - 8 ? o : 8)); }
    asm volatile("" : "+v"(v[0].x), "+v"(v[0].y), "+v"(v[0].z), "+v"(v[0].w), "+v"(v[1].x), "+v"(v[1].y), "+v"(v[1].z), "+v"(v[1].w),
                      "+v"(v[2].x), "+v"(v[2].y), "+v"(v[2].z), "+v"(v[2].w), "+v"(v[3].x), "+v"(v[3].y), "+v"(v[3].z), "+v"(v[3].w),
                      "+v"(head.x), "+v"(head.y), "+v"(tail.x), "+v"(tail.y));
    if (lane == 0) { *reinterpret_cast<uint2 *>(dst) = head; *reinterpret_cast<uint2 *>(dst + nb - 8) = tail; }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) { const uint32_t o = 8 + (lane + k * L) * 16; if (o < nb - 8) *reinterpret_cast<uint4 *>(dst + o) = v[k]; }
  } else {                                                // nb / 8 <= 8 L pieces
    uint2 v[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) { const uint32_t o = (lane + k * L) * 8; v[k] = *reinterpret_cast<const uint2 *>(src + (o < nb ? o : 0)); }
    asm volatile("" : "+v"(v[0].x), "+v"(v[0].y), "+v"(v[1].x), "+v"(v[1].y), "+v"(v[2].x), "+v"(v[2].y), "+v"(v[3].x), "+v"(v[3].y),
                      "+v"(v[4].x), "+v"(v[4].y), "+v"(v[5].x), "+v"(v[5].y), "+v"(v[6].x), "+v"(v[6].y), "+v"(v[7].x), "+v"(v[7].y));
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) { const uint32_t o = (lane + k * L) * 8; if (o < nb) *reinterpret_cast<uint2 *>(dst + o) = v[k]; }
  }
}

// the CV of a full tile from its block's first node (left CV || right CV of the tile's top merge, stored for every gl <= 6) to `out`;
// root: 8 where the file is EXACTLY this one tile, which has no storey above: the compression is ROOT-flagged and is the file's root
__device__ __forceinline__ void block_cv(const uint8_t *__restrict__ block, uint32_t root, uint32_t *__restrict__ out) {
  uint32_t m[16], ivv[8], o[8];
  load_node(block, m);
  iv(ivv);
  blake3_cv(ivv, m, 0, 0, 64, 4u | root, o);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = o[k];
}

// The blocks of the `tiles` full tiles of a file of `len` bytes (tiles MiB <= len) to their places in its outboard, and the header; wg:
// the workgroup's index among the file's.  Which tile a lane moves comes from wg by division (block_piece), the place from preorder_pos.
// A file of exactly one full tile has no tail either: workgroup 0 computes its root here.
__device__ __forceinline__ void open_relocate_body(const uint8_t *__restrict__ blocks, uint64_t len, uint32_t tiles, uint32_t gl, uint8_t *__restrict__ ob,
                                                   uint32_t *__restrict__ root, uint32_t wg) {
  if (wg == 0 && threadIdx.x == 0) {
    *reinterpret_cast<uint2 *>(ob) = make_uint2((uint32_t)len, (uint32_t)(len >> 32));
    if (len == (uint64_t)B3W_TILE * 1024) block_cv(blocks, 8u, root);
  }
  const BlockPiece p = block_piece(gl, wg);
  if (p.tile >= tiles) return;
  const uint64_t G1 = (1ull << gl) - 1, ng = (((len + 1023) / 1024) + G1) >> gl;
  const uint32_t sh = 10 - gl;                            // a tile is 1 << sh groups
  const uint64_t pos = preorder_pos(ng, (uint64_t)p.pos_tile << sh, 1ull << sh);
  move_piece(ob + 8 + pos * 64 + p.at, blocks + (uint64_t)p.tile * p.bb + p.at, p.nb, p.lane, p.L);
}

__global__ __launch_bounds__(256) void b3w_bao_stream_open_relocate_kernel(const uint8_t *__restrict__ blocks, uint64_t len, uint32_t tiles,
                                                                           uint32_t gl, uint8_t *__restrict__ ob, uint32_t *__restrict__ root) {
  open_relocate_body(blocks, len, tiles, gl, ob, root, blockIdx.x);
}

// The same for a table of sessions, one grid: a row per file of one full tile or more, with window = the session's blocks, ob and root
// the file's, len its now-known length, tile0 = its count of full tiles and gl its group_log.  A row has
// ((tile0 + 2^tpw_log - 1) >> tpw_log) * ppb workgroups of open_shape(gl), which differs from row to row; a workgroup lies in one row,
// so its outboard's phase, and with it the choice between the 16-byte and the 8-byte moves, is one for all its lanes.
__global__ __launch_bounds__(256) void b3w_bao_stream_open_relocate_many_kernel(const ManyRow *__restrict__ rows, uint32_t n_rows) {
  const ManyRow row = many_row(rows, n_rows, blockIdx.x);
  open_relocate_body(row.window, row.len, row.tile0, row.gl, row.ob, row.root, blockIdx.x - row.first);
}

// ---- resident files after appends and truncations: the kept blocks from the outboard of the old length to that of the new ----------------
// A change of length moves the nodes of a pre-order outboard and changes none below a tile that is full before and after: the block of
// such a tile is the same run of bytes at another place (see "open-length sessions"), and the tile's CV is the parent compression of the
// block's first node.  So the kernel is b3w_bao_stream_open_relocate_many_kernel with an outboard of the OLD length as the source, and it
// leaves the kept tiles' CVs where the merge storeys look for them (b3wit.h "resident files after appends and truncations").
//   b3w_bao_resize_relocate_kernel   a row per file with at least one kept tile; workgroups of open_shape(gl) as above.  A workgroup moves
//                                    a piece of a block (or 2 .. 16 whole blocks) from old_ob + 8 + 64 preorder_pos(old units, ...) to
//                                    new_ob + 8 + 64 preorder_pos(new units, ...); the lane that moves a block's first node computes the
//                                    tile's CV into slot `tile` of the row's CVs, or (a file that is now exactly one full tile) the
//                                    ROOT-flagged one into the root; one lane per row writes the header.
// The tiles behind the kept ones go through b3w_bao_stream_tile_many[_group]_kernel and the storeys above through
// b3w_bao_stream_merge_many[_group]_kernel as they are.  The 16-byte moves need BOTH places at 8 modulo 16 (both outboards 16-byte
// aligned); any other pair of phases takes the 8-byte moves.  The old outboard is only read.
struct ResRow {
  uint64_t old_len, new_len;
  const uint8_t *old_ob;                                 // the file's outboard for old_len, header first
  uint8_t *new_ob;                                       // where its outboard for new_len goes
  uint32_t *cv;                                          // the file's tile CVs (unused where new_len is exactly one tile)
  uint32_t *root;
  uint32_t first, tiles, gl, pad;                        // first: the row's first workgroup; tiles: the kept ones
};

__global__ __launch_bounds__(256) void b3w_bao_resize_relocate_kernel(const ResRow *__restrict__ rows, uint32_t n_rows) {
  const ResRow row = rows[find_first(rows, 0, n_rows, blockIdx.x)];
  const uint8_t *__restrict__ old_ob = as_global(row.old_ob);
  uint8_t *__restrict__ new_ob = as_global(row.new_ob);
  const uint64_t len = row.new_len;
  const uint32_t gl = row.gl, wg = blockIdx.x - row.first;
  if (wg == 0 && threadIdx.x == 0) *reinterpret_cast<uint2 *>(new_ob) = make_uint2((uint32_t)len, (uint32_t)(len >> 32));
  const BlockPiece p = block_piece(gl, wg);
  if (p.tile >= row.tiles) return;
  const uint64_t G1 = (1ull << gl) - 1;
  const uint64_t ng_old = (((row.old_len + 1023) / 1024) + G1) >> gl, ng_new = (((len + 1023) / 1024) + G1) >> gl;
  const uint32_t sh = 10 - gl;                            // a tile is 1 << sh groups
  const uint64_t a = (uint64_t)p.pos_tile << sh;
  const uint8_t *__restrict__ src = old_ob + 8 + preorder_pos(ng_old, a, 1ull << sh) * 64 + p.at;
  move_piece(new_ob + 8 + preorder_pos(ng_new, a, 1ull << sh) * 64 + p.at, src, p.nb, p.lane, p.L);
  // the kept tile's CV, by the lane that moves the block's first node
  if (p.piece == 0 && p.lane == 0) {
    const bool sole = len == (uint64_t)B3W_TILE * 1024;
    block_cv(src, sole ? 8u : 0u, sole ? as_global(row.root) : as_global(row.cv) + (uint64_t)p.tile * 8);
  }
}

}  // namespace

// ---- the host side: what the device entry points share ---------------------------------------------------------------------------------
namespace {

// ---- refusals: every bad argument of every call ends in refuse (b3w_internal.h, with group_log_ok) ---------------------------------------
std::string entry_text(uint32_t i) { return "entry " + std::to_string(i) + ": "; }

int32_t nova_ok(b3w_ctx *ctx) {
  return ctx->desc.kind == B3W_KIND_COMP ? refuse(ctx, nullptr, "sampled paths plan the nova step circuits' records") : B3W_OK;
}
// every sample names a file of the batch and a chunk of that file
int32_t samples_ok(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples) {
  for (uint32_t s = 0; s < n_samples; ++s) {
    if (host_files[s] >= n_files) return refuse(ctx, nullptr, "a sampled file index is not below the file count");
    if (host_chunks[s] >= num_chunks(host_lens[host_files[s]])) return refuse(ctx, nullptr, "a sampled chunk index is not below its file's chunk count");
  }
  return B3W_OK;
}
// the arena calls: the samples' indices, and every sampled file inside [0, arena_bytes)
int32_t arena_samples_ok(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                         uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples) {
  B3W_TRY(samples_ok(ctx, host_lens, n_files, host_files, host_chunks, n_samples));
  for (uint32_t s = 0; s < n_samples; ++s) {
    const uint64_t off = host_offsets[host_files[s]], len = host_lens[host_files[s]];
    if (len && !d_arena) return refuse(ctx, nullptr, "a null arena with a sampled file that is not empty");
    if (off > arena_bytes || len > arena_bytes - off) return refuse(ctx, nullptr, "a sampled file reaches past arena_bytes");
  }
  return B3W_OK;
}
// the whole-batch calls: no file too long for the grids, the scratch large enough and aligned, an arena where a file has bytes
int32_t batch_ok(b3w_ctx *ctx, const char *call, const BatchCounts &k, const uint8_t *d_arena, const uint64_t *host_lens, uint32_t n_files, const void *d_scratch,
                 uint64_t scratch_bytes, uint64_t need, const char *too_small) {
  if (k.too_long || k.big_wgs > 0x7fffffffull) return refuse(ctx, call, "a file of more than 2^30 chunks, or more than 2^31 tiles");
  if (scratch_bytes < need) return refuse(ctx, call, too_small);
  if (need && (!d_scratch || ((uintptr_t)d_scratch & 15))) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  if (!d_arena)
    for (uint32_t f = 0; f < n_files; ++f)
      if (host_lens[f]) return refuse(ctx, call, "a null arena with a file that is not empty");
  return B3W_OK;
}

// ---- launches: which kernel, and what follows the last one -------------------------------------------------------------------------------
// a kernel template over the lanes a sample (1, 4 or 16): f(K) launches the instantiation, lanes_grid its grid of waves
template <class F>
void with_lanes(int lanes, F f) {
  if (lanes == 1) f(std::integral_constant<int, 1>{});
  else if (lanes == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 16>{});
}
template <int K>
dim3 lanes_grid(uint32_t n_samples) { return dim3((n_samples + 64 / K - 1) / (64 / K)); }

// a kernel, or with `grp` its group instantiation, which takes group_log behind the same arguments
template <class P, class G, class... A>
void launch_pair(bool grp, P plain, G group, uint32_t group_log, dim3 grid, dim3 block, hipStream_t st, A... args) {
  if (grp) hipLaunchKernelGGL(group, grid, block, 0, st, args..., group_log);
  else hipLaunchKernelGGL(plain, grid, block, 0, st, args...);
}

// a file's merge storeys over the tile CVs of a streamed file: a workgroup per 1 024 tiles, one more over those past 1 GiB
void stream_merge(uint64_t len, uint64_t groups, uint32_t gl, const uint32_t *tile_cv, uint32_t *group_cv, uint8_t *ob, uint32_t *root, hipStream_t st) {
  const uint64_t T = B3W_TILE;
  launch_pair(gl != 0, b3w_bao_stream_merge_kernel, b3w_bao_stream_merge_group_kernel, gl, dim3((uint32_t)groups), dim3(256), st, len, T, tile_cv, group_cv, ob, root);
  if (groups > 1)
    launch_pair(gl != 0, b3w_bao_stream_merge_kernel, b3w_bao_stream_merge_group_kernel, gl, dim3(1), dim3(256), st, len, T * T, (const uint32_t *)group_cv, (uint32_t *)nullptr, ob, root);
}
// the same two storeys over the rows of a table of files: n1 rows in wg1 workgroups, then n2 rows behind them
void many_merge(bool grp, const ManyRow *d_one, uint32_t n1, uint32_t wg1, const ManyRow *d_two, uint32_t n2, hipStream_t st) {
  const uint64_t T = B3W_TILE;
  const auto kernel = grp ? b3w_bao_stream_merge_many_group_kernel : b3w_bao_stream_merge_many_kernel;
  if (n1) hipLaunchKernelGGL(kernel, dim3(wg1), dim3(256), 0, st, d_one, n1, T);
  if (n2) hipLaunchKernelGGL(kernel, dim3(n2), dim3(256), 0, st, d_two, n2, T * T);
}

// behind the launches of a call whose table went through the batch staging: the event is not recorded after a failed launch
int32_t batch_launched(b3w_ctx *ctx, hipStream_t st, const char *what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, what);
  HIP_TRY(ctx, hipEventRecord(ctx->batch_done, st));
  return B3W_OK;
}

// the context's staging for the batch calls' tables: waits for the previous batch call, grows both buffers to `bytes`
int32_t batch_staging(b3w_ctx *ctx, uint64_t bytes) {
  if (ctx->batch_done) HIP_TRY(ctx, hipEventSynchronize(ctx->batch_done));
  else HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->batch_done, hipEventDisableTiming));
  if (ctx->batch_cap < bytes) {
    if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
    if (ctx->d_batch) (void)hipFree(ctx->d_batch);
    ctx->h_batch = nullptr; ctx->d_batch = nullptr; ctx->batch_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_batch, (size_t)bytes, hipHostMallocDefault));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_batch, (size_t)bytes));
    ctx->batch_cap = bytes;
  }
  return B3W_OK;
}

// ---- the sample table of the sampled-path, slice and ingest calls -------------------------------------------------------------------------
// A row is {chunk, word 1, length, word 3, file[, the file's arena offset]}.  The rows go into the batch staging and on to the device;
// behind them, on the host, lies the files' outboard layout the rows are filled from (none where word 3 is the slice's offset).
struct SampleRows {
  uint32_t words;                                        // 5, or 6: with the file's arena offset
  bool w1_slice, w3_slice;                               // word 1: the sample's slice offset, not its first record row; word 3: the same, not its file's outboard offset
  bool have;                                             // the have layout takes the outboard layout's place once the rows are filled, and is uploaded with them
};
// -> the table on the device and the batch's longest path.  The call is host work a sample before it is anything else, so the path is
// walked once a sample, with the split from a bit scan (depth_in), and serves the record rows, the slice's size and the longest path;
// and the rows' kind is a template argument, so that a call's loop computes only what its rows hold (with the kind a run-time value the
// ingest call at 65 536 slices took 3.6 % longer than the parent's own loop: profiles/r24/bao_host_ab.json, "first_build").
template <uint32_t WORDS, bool W1_SLICE, bool W3_SLICE, bool HAVE>
int32_t sample_table(b3w_ctx *ctx, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                     const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, hipStream_t st, const uint64_t **d_desc,
                     uint32_t *longest = nullptr) {
  constexpr SampleRows k{WORDS, W1_SLICE, W3_SLICE, HAVE};
  const uint64_t desc_bytes = (uint64_t)n_samples * k.words * 8, layout_bytes = k.w3_slice ? 0 : ((uint64_t)n_files + 1) * 8;
  B3W_TRY(batch_staging(ctx, desc_bytes + layout_bytes));
  uint64_t *desc = reinterpret_cast<uint64_t *>(ctx->h_batch), *ob_first = desc + (uint64_t)k.words * n_samples;
  if (!k.w3_slice) (void)b3w_bao_group_batch_layout(host_lens, n_files, group_log, ob_first);        // (group_log 0: b3w_bao_batch_layout's)
  uint64_t row = 0, at = slice_start(0);
  uint32_t most = 0;
  for (uint32_t s = 0; s < n_samples; ++s) {
    const uint32_t f = host_files[s];
    const uint64_t len = host_lens[f], c = host_chunks[s];
    const uint32_t P = depth_in(c, num_chunks(len));
    uint64_t *d = desc + (uint64_t)k.words * s;
    d[0] = c; d[1] = k.w1_slice ? at : row; d[2] = len; d[3] = k.w3_slice ? at : ob_first[f]; d[4] = f;
    if (k.words == 6) d[5] = host_offsets[f];
    row += chunk_blocks(len, c) + P;
    at = slice_start(at + slice_bytes(len, c, P));
    if (P > most) most = P;
  }
  if (k.have) (void)b3w_bao_have_layout(host_lens, n_files, ob_first);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)(desc_bytes + (k.have ? layout_bytes : 0)), hipMemcpyHostToDevice, st));
  *d_desc = reinterpret_cast<const uint64_t *>(ctx->d_batch);
  if (longest) *longest = most;
  return B3W_OK;
}

// ---- the tables of the two whole-batch calls (outboards, verification) --------------------------------------------------------------------
// one behind the other in the staging, uploaded in one copy: small | big | merged | tops | [verification: a VerFile a file |] the small
// waves' first files
struct BatchTables { BatchEnt *small, *big, *merged, *tops; VerFile *files; uint32_t *waves; };
BatchTables batch_tables_at(uint8_t *base, const BatchCounts &k, uint32_t n_ver_files) {
  BatchTables t;
  t.small = reinterpret_cast<BatchEnt *>(base); t.big = t.small + k.small; t.merged = t.big + k.big; t.tops = t.merged + k.merged;
  t.files = reinterpret_cast<VerFile *>(t.tops + k.tops);
  t.waves = reinterpret_cast<uint32_t *>(t.files + n_ver_files);
  return t;
}
// -> the tables on the device.  The outboard calls' merged and top entries start with their first input CV slot (big_wgs, groups);
// verification's with 0, and it adds the files' rows {first unit, first tile's scratch entry, first group's}
int32_t batch_tables(b3w_ctx *ctx, const BatchCounts &k, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files, uint32_t gl, bool verify,
                     hipStream_t st, BatchTables *d) {
  const uint32_t n_ver = verify ? n_files : 0;
  const uint64_t n_ents = k.small + k.big + k.merged + k.tops;
  const uint64_t table_bytes = n_ents * sizeof(BatchEnt) + (uint64_t)n_ver * sizeof(VerFile) + (k.small ? (k.waves + 1) * 4 : 0);
  B3W_TRY(batch_staging(ctx, table_bytes));
  const BatchTables h = batch_tables_at(ctx->h_batch, k, n_ver);
  SmallPack pack;
  pack.first = h.waves;
  uint32_t i_big = 0, i_merged = 0, i_tops = 0, big_wgs = 0, groups = 0;
  uint64_t ob = 0, units = 0, slot = 0, gslot = 0;
  for (uint32_t f = 0; f < n_files; ++f) {
    const uint64_t len = host_lens[f], n = num_chunks(len);
    if (verify) h.files[f] = VerFile{units, slot, gslot};
    if (n <= 64) {
      const uint32_t lane = pack.add(n);
      h.small[pack.files - 1] = BatchEnt{host_offsets[f], len, ob, lane, f};
    } else {
      const uint32_t tiles = (uint32_t)((n + B3W_TILE - 1) / B3W_TILE), grp = (tiles + B3W_TILE - 1) / B3W_TILE;
      h.big[i_big++] = BatchEnt{host_offsets[f], len, ob, big_wgs, f};
      if (tiles > 1) h.merged[i_merged++] = BatchEnt{verify ? 0 : big_wgs, len, ob, groups, f};
      if (grp > 1) { h.tops[i_tops] = BatchEnt{verify ? 0 : groups, len, ob, i_tops, f}; i_tops++; }
      big_wgs += tiles;
      if (tiles > 1) { groups += grp; slot += tiles; }
      if (grp > 1) gslot += grp;
    }
    ob += group_outboard_bytes(len, gl);
    units += n_units(len, gl);
  }
  pack.close();
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)table_bytes, hipMemcpyHostToDevice, st));
  *d = batch_tables_at(ctx->d_batch, k, n_ver);
  return B3W_OK;
}

// ---- the bodies of entry points that come in pairs ------------------------------------------------------------------------------------------
// b3w_sample_plan_batch_device (the kernel of ABI 1.2 over full outboards) and b3w_sample_plan_group_batch_device
int32_t sample_plan_batch(b3w_ctx *ctx, const char *call, const uint64_t *host_lens, uint32_t n_files, bool grp, uint32_t group_log, const uint8_t *d_outboards,
                                 const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_bytes,
                                 uint32_t *d_records, int32_t *d_sample_status, void *stream, const char *launch) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_samples) return B3W_OK;
  if (!host_lens || !d_outboards || !d_roots || !host_files || !host_chunks || !d_bytes || !d_records || !d_sample_status) return refuse(ctx, call, "a null pointer");
  B3W_TRY(samples_ok(ctx, host_lens, n_files, host_files, host_chunks, n_samples));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  B3W_TRY(sample_table<5, false, false, false>(ctx, nullptr, host_lens, n_files, group_log, host_files, host_chunks, n_samples, st, &d_desc));
  const uint32_t per_wave = 64u >> group_log;
  if (grp) hipLaunchKernelGGL(b3w_sample_plan_group_kernel<false>, dim3((n_samples + per_wave - 1) / per_wave), dim3(64), 0, st, d_outboards, d_roots, d_desc, n_samples, group_log, d_bytes, d_records, d_sample_status);
  else hipLaunchKernelGGL(b3w_sample_plan_batch_kernel, dim3((n_samples + 63) / 64), dim3(64), 0, st, d_outboards, d_roots, d_desc, n_samples, d_bytes, d_records, d_sample_status);
  return batch_launched(ctx, st, launch);
}

// grp false: full outboards, the kernels of ABI 1.2; true: group outboards (group_log 0 included), their group instantiations
int32_t outboard_batch(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files, bool grp, uint32_t gl,
                              uint8_t *d_outboards, uint32_t *d_roots, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao batch";
  if (!n_files) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !d_roots) return refuse(ctx, call, "a null pointer (offsets, lengths, outboards or roots)");
  if ((uintptr_t)d_outboards & 7) return refuse(ctx, call, "d_outboards is not 8-byte aligned");
  const BatchCounts k = batch_counts(host_lens, n_files);
  B3W_TRY(batch_ok(ctx, call, k, d_arena, host_lens, n_files, d_scratch, scratch_bytes, (k.big_wgs + k.groups) * 32,
                   "the scratch is smaller than b3w_bao_batch_scratch_bytes says"));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  BatchTables d;
  B3W_TRY(batch_tables(ctx, k, host_offsets, host_lens, n_files, gl, false, st, &d));
  uint32_t *tile_cv = reinterpret_cast<uint32_t *>(d_scratch), *group_cv = tile_cv + k.big_wgs * 8;
  const uint64_t T = B3W_TILE;
  if (k.small) launch_pair(grp, b3w_bao_small_kernel, b3w_bao_small_group_kernel, gl, dim3((uint32_t)k.waves), dim3(64), st, d_arena, (const BatchEnt *)d.small, (const uint32_t *)d.waves, d_outboards, d_roots);
  if (k.big) launch_pair(grp, b3w_bao_tile_kernel, b3w_bao_tile_group_kernel, gl, dim3((uint32_t)k.big_wgs), dim3(B3W_TILE), st, d_arena, (const BatchEnt *)d.big, (uint32_t)k.big, d_outboards, d_roots, tile_cv);
  if (k.merged) launch_pair(grp, b3w_bao_merge_kernel, b3w_bao_merge_group_kernel, gl, dim3((uint32_t)k.groups), dim3(256), st, (const BatchEnt *)d.merged, (uint32_t)k.merged, T, (const uint32_t *)tile_cv, group_cv, d_outboards, d_roots);
  if (k.tops) launch_pair(grp, b3w_bao_merge_kernel, b3w_bao_merge_group_kernel, gl, dim3((uint32_t)k.tops), dim3(256), st, (const BatchEnt *)d.tops, (uint32_t)k.tops, T * T, (const uint32_t *)group_cv, (uint32_t *)nullptr, d_outboards, d_roots);
  return batch_launched(ctx, st, grp ? "bao group batch launch" : "bao batch launch");
}

// the slices of the samples gathered from the outboards: 16 lanes a sample from full outboards, a lane a chunk of the group from group
// outboards; ARENA: the bytes read where the files lie
template <bool ARENA>
void launch_slices(uint32_t group_log, uint32_t n_samples, hipStream_t st, const uint8_t *d_outboards, const uint64_t *d_desc, const uint8_t *d_bytes, uint8_t *d_slices) {
  const uint32_t per_wg = 256 / SLICE_LANES, per_wave = 64u >> group_log;
  if (group_log == 0) hipLaunchKernelGGL(b3w_bao_slice_kernel<ARENA>, dim3((n_samples + per_wg - 1) / per_wg), dim3(256), 0, st, d_outboards, d_desc, n_samples, d_bytes, d_slices);
  else hipLaunchKernelGGL(b3w_bao_slice_group_kernel<ARENA>, dim3((n_samples + per_wave - 1) / per_wave), dim3(64), 0, st, d_outboards, d_desc, n_samples, group_log, d_bytes, d_slices);
}

// the slot buffer of the packed receivers (1 024 bytes a listed chunk): b3w_int_slots_wrong's refusal through the one refusal path
int32_t slots_ok(b3w_ctx *ctx, const char *call, const uint8_t *d_chunks, uint64_t chunks_bytes, uint64_t listed) {
  const std::string why = b3w_int_slots_wrong(d_chunks, chunks_bytes, listed);
  return why.empty() ? B3W_OK : refuse(ctx, call, why);
}

// b3w_bao_slice_ingest_device (HAVE false: d_have is not looked at) and b3w_bao_slice_ingest_have_device; PACKED:
// b3w_bao_slice_ingest_packed_device, (d_arena, arena_bytes) its slot buffer, no offsets, d_outboards may be null
template <bool HAVE, bool PACKED = false>
int32_t slice_ingest(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                            uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                            const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status, uint64_t *d_have, void *stream) {
  const char *call = PACKED ? "bao slice ingest packed" : "bao slice ingest";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (HAVE && (!d_have || ((uintptr_t)d_have & 7))) return refuse(ctx, call, "d_have is null or not 8-byte aligned");
  if (!n_samples) return B3W_OK;
  if ((!PACKED && (!host_offsets || !d_outboards)) || !host_lens || !d_roots || !host_files || !host_chunks || !d_slices || !d_sample_status) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  if (PACKED) {
    B3W_TRY(samples_ok(ctx, host_lens, n_files, host_files, host_chunks, n_samples));
    B3W_TRY(slots_ok(ctx, call, d_arena, arena_bytes, n_samples));
  } else {
    B3W_TRY(arena_samples_ok(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_chunks, n_samples));
  }
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  uint32_t longest = 0;
  B3W_TRY((sample_table<PACKED ? 5 : 6, true, false, HAVE>(ctx, host_offsets, host_lens, n_files, group_log, host_files, host_chunks, n_samples, st, &d_desc, &longest)));
  // lanes a sample, from the batch's longest path P: node j is checked by lane j mod K, ceil(P / K) rounds beside the chunk's sixteen blocks,
  // and every lane fewer a sample is a leader more a wave in the stretch only leaders run.  Measured at P = 20: four lanes
  // (five rounds) beat sixteen (two) at 4 096 and at 65 536 slices, so four up to six rounds; sixteen for the longer paths (files past
  // 16 GiB; not measured).  B3W_SLICE_INGEST_LANES=1 / 4 / 16: measurements
  const char *env = getenv("B3W_SLICE_INGEST_LANES");
  unsigned long long *have = HAVE ? reinterpret_cast<unsigned long long *>(d_have) : nullptr;
  with_lanes(env ? atoi(env) : (longest <= 24 ? 4 : 16), [&](auto K) {
    constexpr int LANES = decltype(K)::value;
    hipLaunchKernelGGL((b3w_bao_slice_ingest_kernel<LANES, HAVE, PACKED>), lanes_grid<LANES>(n_samples), dim3(64), 0, st, d_slices, d_roots, d_desc, n_samples, group_log, d_arena,
                       d_outboards, d_sample_status, have);
  });
  return batch_launched(ctx, st, PACKED ? "bao slice ingest packed launch" : "bao slice ingest launch");
}

}  // namespace

// b3w_bao_have.hip's way to the staging of the batch calls and to their epilogue
int32_t b3w_int_batch_staging(b3w_ctx *ctx, uint64_t bytes) { return batch_staging(ctx, bytes); }
int32_t b3w_int_batch_launched(b3w_ctx *ctx, hipStream_t st, const char *what) { return batch_launched(ctx, st, what); }

// ---- the device entry points (the calls that touch no device: b3w_bao_host.cpp) ----------------------------------------------------------
extern "C" {

int32_t b3w_bao_outboard_device(b3w_ctx *ctx, const uint8_t *d_preimage, uint64_t len, uint8_t *d_outboard, uint32_t *d_levels, uint32_t *d_root,
                                void *stream) {
  if (!ctx || (!d_preimage && len) || !d_outboard || !d_levels || !d_root) return B3W_E_BAD_ARGUMENT;
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n = num_chunks(len);
  // four lanes per chunk up to 64 Ki chunks (latency), one lane per chunk above (throughput); B3W_BAO_QUAD=0 / 1: measurements
  const char *env = getenv("B3W_BAO_QUAD");
  const bool quad = env ? atoi(env) != 0 : n <= 65536u;
  if (quad) hipLaunchKernelGGL(b3w_bao_cv_quad_kernel, dim3((uint32_t)((n + 15) / 16)), dim3(64), 0, st, d_preimage, len, n, d_levels);
  else hipLaunchKernelGGL(b3w_bao_cv_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_preimage, len, n, d_levels);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "bao chunk CV launch");
  B3W_TRY(b3w_chain_tree_device(ctx, d_levels, n, d_root, stream));
  const B3wSpine sp = n > 1 ? spine_of(n) : B3wSpine{};
  hipLaunchKernelGGL(b3w_bao_emit_kernel, dim3((uint32_t)(n > 1 ? (n - 1 + 255) / 256 : 1)), dim3(256), 0, st, d_levels, n, len, sp, d_outboard);
  e = hipGetLastError();
  return e != hipSuccess ? hip_fail(ctx, e, "bao emit launch") : B3W_OK;
}

// ---- challenged paths: the record rows (here, where b3w_plan_path_len links) and the planners ------------------------------------------
int64_t b3w_sample_rows(uint64_t len, const uint64_t *host_chunks, uint32_t n_samples, uint64_t *row_first) {
  if ((!host_chunks && n_samples) || !row_first) return -B3W_E_BAD_ARGUMENT;
  const uint64_t n = num_chunks(len);
  for (uint32_t s = 0; s < n_samples; ++s)
    if (host_chunks[s] >= n) return -B3W_E_BAD_ARGUMENT;
  uint64_t row = 0;
  for (uint32_t s = 0; s < n_samples; ++s) {
    row_first[s] = row;
    row += chunk_blocks(len, host_chunks[s]) + b3w_plan_path_len(host_chunks[s], n);
  }
  row_first[n_samples] = row;
  return (int64_t)row;
}

int64_t b3w_sample_rows_batch(const uint64_t *host_lens, uint32_t n_files, const uint32_t *host_files, const uint64_t *host_chunks,
                              uint32_t n_samples, uint64_t *row_first) {
  if (!row_first || (n_samples && (!host_lens || !host_files || !host_chunks))) return -B3W_E_BAD_ARGUMENT;
  for (uint32_t s = 0; s < n_samples; ++s)
    if (host_files[s] >= n_files || host_chunks[s] >= num_chunks(host_lens[host_files[s]])) return -B3W_E_BAD_ARGUMENT;
  uint64_t row = 0;
  for (uint32_t s = 0; s < n_samples; ++s) {
    const uint64_t len = host_lens[host_files[s]];
    row_first[s] = row;
    row += chunk_blocks(len, host_chunks[s]) + b3w_plan_path_len(host_chunks[s], num_chunks(len));
  }
  row_first[n_samples] = row;
  return (int64_t)row;
}

// (its own staging and event, h_samples / d_samples / samples_done: on the batch staging it would wait for the batch calls)
int32_t b3w_sample_plan_device(b3w_ctx *ctx, uint64_t len, const uint8_t *d_outboard, const uint32_t *root, const uint64_t *host_chunks,
                               uint32_t n_samples, const uint8_t *d_chunk_bytes, uint32_t *d_records, int32_t *d_sample_status, void *stream) {
  if (!ctx || !d_outboard || !root || (n_samples && (!host_chunks || !d_chunk_bytes || !d_records || !d_sample_status))) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  const uint64_t n = num_chunks(len);
  for (uint32_t s = 0; s < n_samples; ++s)
    if (host_chunks[s] >= n) return refuse(ctx, nullptr, "a sampled chunk index is not below the chunk count");
  if (!n_samples) return B3W_OK;
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  // the per-sample {chunk, first row} table goes through the context's pinned staging buffer; the event of the previous call says
  // when that call's copy and kernel are done with both buffers
  if (ctx->samples_done) HIP_TRY(ctx, hipEventSynchronize(ctx->samples_done));
  else HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->samples_done, hipEventDisableTiming));
  if (ctx->samples_cap < n_samples) {
    if (ctx->h_samples) (void)hipHostFree(ctx->h_samples);
    if (ctx->d_samples) (void)hipFree(ctx->d_samples);
    ctx->h_samples = nullptr; ctx->d_samples = nullptr; ctx->samples_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_samples, (size_t)n_samples * 16, hipHostMallocDefault));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_samples, (size_t)n_samples * 16));
    ctx->samples_cap = n_samples;
  }
  uint64_t row = 0;
  for (uint32_t s = 0; s < n_samples; ++s) {
    ctx->h_samples[2 * s] = host_chunks[s];
    ctx->h_samples[2 * s + 1] = row;
    row += chunk_blocks(len, host_chunks[s]) + b3w_plan_path_len(host_chunks[s], n);
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_samples, ctx->h_samples, (size_t)n_samples * 16, hipMemcpyHostToDevice, st));
  Root8 r8;
  for (int k = 0; k < 8; ++k) r8.w[k] = root[k];
  hipLaunchKernelGGL(b3w_sample_plan_kernel, dim3((n_samples + 63) / 64), dim3(64), 0, st, len, n, reinterpret_cast<const uint32_t *>(d_outboard), r8,
                     ctx->d_samples, n_samples, d_chunk_bytes, d_records, d_sample_status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "sample plan launch");
  HIP_TRY(ctx, hipEventRecord(ctx->samples_done, st));
  return B3W_OK;
}

int32_t b3w_sample_plan_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint8_t *d_outboards, const uint32_t *d_roots,
                                     const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_chunk_bytes,
                                     uint32_t *d_records, int32_t *d_sample_status, void *stream) {
  return sample_plan_batch(ctx, "sample plan batch", host_lens, n_files, false, 0, d_outboards, d_roots, host_files, host_chunks, n_samples, d_chunk_bytes, d_records,
                           d_sample_status, stream, "sample plan batch launch");
}

int32_t b3w_sample_plan_group_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                           const uint8_t *d_group_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                           const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_group_bytes, uint32_t *d_records,
                                           int32_t *d_sample_status, void *stream) {
  return sample_plan_batch(ctx, "sample plan group batch", host_lens, n_files, true, group_log, d_group_outboards, d_roots, host_files, host_chunks, n_samples,
                           d_group_bytes, d_records, d_sample_status, stream, "sample plan group batch launch");
}

// ---- outboards of a batch of files ---------------------------------------------------------------------------------------------------
int32_t b3w_bao_outboard_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens,
                                      uint32_t n_files, uint8_t *d_outboards, uint32_t *d_roots, void *d_scratch, uint64_t scratch_bytes,
                                      void *stream) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  return outboard_batch(ctx, d_arena, host_offsets, host_lens, n_files, false, 0, d_outboards, d_roots, d_scratch, scratch_bytes, stream);
}

int32_t b3w_bao_group_outboard_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens,
                                            uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, uint32_t *d_roots, void *d_scratch,
                                            uint64_t scratch_bytes, void *stream) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, "bao group batch", group_log));
  return outboard_batch(ctx, d_arena, host_offsets, host_lens, n_files, true, group_log, d_outboards, d_roots, d_scratch, scratch_bytes, stream);
}

// ---- verification: whole files against their outboards -----------------------------------------------------------------------------------
int32_t b3w_bao_verify_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files,
                                    uint32_t group_log, const uint8_t *d_outboards, const uint32_t *d_roots, uint8_t *d_unit_status,
                                    int32_t *d_file_status, uint64_t *d_first_bad, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao verify";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_files) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !d_roots || !d_unit_status || !d_file_status || !d_first_bad)
    return refuse(ctx, call, "a null pointer (offsets, lengths, outboards, roots or an output)");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_first_bad & 7) || ((uintptr_t)d_file_status & 3) || ((uintptr_t)d_roots & 3))
    return refuse(ctx, call, "d_outboards or d_first_bad is not 8-byte aligned, or d_file_status or d_roots not 4-byte aligned");
  const BatchCounts k = batch_counts(host_lens, n_files);
  uint64_t tile_ents = 0;
  const uint64_t n_scr = verify_entries(host_lens, n_files, &tile_ents);
  B3W_TRY(batch_ok(ctx, call, k, d_arena, host_lens, n_files, d_scratch, scratch_bytes, (n_scr * 36 + 15) & ~15ull,
                   "the scratch is smaller than b3w_bao_verify_scratch_bytes says"));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  BatchTables d;
  B3W_TRY(batch_tables(ctx, k, host_offsets, host_lens, n_files, group_log, true, st, &d));
  uint32_t *exp_cv = reinterpret_cast<uint32_t *>(d_scratch), *bad = exp_cv + n_scr * 8;
  unsigned long long *fb = reinterpret_cast<unsigned long long *>(d_first_bad);
  const uint64_t T = B3W_TILE;
  // top down: the storeys above the tiles first (stored nodes alone), then the kernels that read the files
  if (k.tops) hipLaunchKernelGGL(b3w_bao_verify_upper_kernel, dim3((uint32_t)k.tops), dim3(256), 0, st, d.tops, (uint32_t)k.tops, T * T, d.files, tile_ents, d_outboards, d_roots, exp_cv, bad, group_log, d_file_status, fb);
  if (k.merged) hipLaunchKernelGGL(b3w_bao_verify_upper_kernel, dim3((uint32_t)k.groups), dim3(256), 0, st, d.merged, (uint32_t)k.merged, T, d.files, tile_ents, d_outboards, d_roots, exp_cv, bad, group_log, d_file_status, fb);
  if (k.small) hipLaunchKernelGGL(b3w_bao_verify_small_kernel, dim3((uint32_t)k.waves), dim3(64), 0, st, d_arena, d.small, d.waves, d.files, d_outboards, d_roots, group_log, d_unit_status, d_file_status, fb);
  if (k.big) hipLaunchKernelGGL(b3w_bao_verify_tile_kernel, dim3((uint32_t)k.big_wgs), dim3(B3W_TILE), 0, st, d_arena, d.big, (uint32_t)k.big, d.files, d_outboards, d_roots, exp_cv, bad, group_log, d_unit_status, d_file_status, fb);
  return batch_launched(ctx, st, "bao verify launch");
}

// ---- bao slices, and challenged paths planned from them alone ------------------------------------------------------------------------------
int32_t b3w_bao_slice_batch_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards,
                                   const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_bytes,
                                   uint8_t *d_slices, void *stream) {
  const char *call = "bao slice batch";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_samples) return B3W_OK;
  if (!host_lens || !d_outboards || !host_files || !host_chunks || !d_bytes || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  B3W_TRY(samples_ok(ctx, host_lens, n_files, host_files, host_chunks, n_samples));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  B3W_TRY(sample_table<5, true, false, false>(ctx, nullptr, host_lens, n_files, group_log, host_files, host_chunks, n_samples, st, &d_desc));
  launch_slices<false>(group_log, n_samples, st, d_outboards, d_desc, d_bytes, d_slices);
  return batch_launched(ctx, st, "bao slice batch launch");
}

int32_t b3w_sample_plan_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots, const uint32_t *host_files,
                                      const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices, uint32_t *d_records,
                                      int32_t *d_sample_status, void *stream) {
  const char *call = "sample plan slices";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  if (!n_samples) return B3W_OK;
  if (!host_lens || !d_roots || !host_files || !host_chunks || !d_slices || !d_records || !d_sample_status) return refuse(ctx, call, "a null pointer");
  if ((uintptr_t)d_slices & 15) return refuse(ctx, call, "d_slices is not 16-byte aligned");
  B3W_TRY(samples_ok(ctx, host_lens, n_files, host_files, host_chunks, n_samples));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  B3W_TRY(sample_table<5, false, true, false>(ctx, nullptr, host_lens, n_files, 0, host_files, host_chunks, n_samples, st, &d_desc));
  // lanes a sample: 16; B3W_SLICE_PLAN_LANES=1 / 4 and B3W_SLICE_PLAN_CHAIN=1 (the running-h chain for every sample): measurements
  const char *env = getenv("B3W_SLICE_PLAN_LANES"), *env_chain = getenv("B3W_SLICE_PLAN_CHAIN");
  const uint32_t chain = env_chain && atoi(env_chain) != 0;
  with_lanes(env ? atoi(env) : 16, [&](auto K) {
    constexpr int LANES = decltype(K)::value;
    hipLaunchKernelGGL(b3w_sample_plan_slices_kernel<LANES>, lanes_grid<LANES>(n_samples), dim3(64), 0, st, d_slices, d_roots, d_desc, n_samples, chain, d_records, d_sample_status);
  });
  return batch_launched(ctx, st, "sample plan slices launch");
}

// ---- challenged paths and slices read in place from the arena --------------------------------------------------------------------------------
int32_t b3w_sample_plan_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                     uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *d_roots,
                                     const uint32_t *host_files, const uint64_t *host_chunks, uint32_t n_samples, uint32_t *d_records,
                                     int32_t *d_sample_status, void *stream) {
  const char *call = "sample plan arena";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_samples) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !d_roots || !host_files || !host_chunks || !d_records || !d_sample_status) return refuse(ctx, call, "a null pointer");
  if ((uintptr_t)d_outboards & 7) return refuse(ctx, call, "d_outboards is not 8-byte aligned");
  B3W_TRY(arena_samples_ok(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_chunks, n_samples));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  B3W_TRY(sample_table<6, false, false, false>(ctx, host_offsets, host_lens, n_files, group_log, host_files, host_chunks, n_samples, st, &d_desc));
  const uint32_t per_wave = 64u >> group_log;
  if (group_log == 0) hipLaunchKernelGGL(b3w_sample_plan_arena_kernel, dim3((n_samples + 63) / 64), dim3(64), 0, st, d_outboards, d_roots, d_desc, n_samples, d_arena, d_records, d_sample_status);
  else hipLaunchKernelGGL(b3w_sample_plan_group_kernel<true>, dim3((n_samples + per_wave - 1) / per_wave), dim3(64), 0, st, d_outboards, d_roots, d_desc, n_samples, group_log, d_arena, d_records, d_sample_status);
  return batch_launched(ctx, st, "sample plan arena launch");
}

int32_t b3w_bao_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                   uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files,
                                   const uint64_t *host_chunks, uint32_t n_samples, uint8_t *d_slices, void *stream) {
  const char *call = "bao slice arena";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_samples) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !host_files || !host_chunks || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  B3W_TRY(arena_samples_ok(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_chunks, n_samples));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *d_desc = nullptr;
  B3W_TRY(sample_table<6, true, false, false>(ctx, host_offsets, host_lens, n_files, group_log, host_files, host_chunks, n_samples, st, &d_desc));
  launch_slices<true>(group_log, n_samples, st, d_outboards, d_desc, d_arena, d_slices);
  return batch_launched(ctx, st, "bao slice arena launch");
}

// ---- slices taken in --------------------------------------------------------------------------------------------------------------------
int32_t b3w_bao_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                    uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                    const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status, void *stream) {
  return slice_ingest<false>(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_chunks, n_samples,
                             d_slices, d_sample_status, nullptr, stream);
}

int32_t b3w_bao_slice_ingest_have_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                         uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                         const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status,
                                         uint64_t *d_have, void *stream) {
  return slice_ingest<true>(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_chunks, n_samples,
                            d_slices, d_sample_status, d_have, stream);
}

// the same body with the slot buffer for the arena; the bitmap is optional, so one name serves both
int32_t b3w_bao_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                           uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                           const uint64_t *host_chunks, uint32_t n_samples, const uint8_t *d_slices, int32_t *d_sample_status,
                                           uint64_t *d_have, void *stream) {
  if (d_have)
    return slice_ingest<true, true>(ctx, d_chunks, chunks_bytes, nullptr, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_chunks, n_samples,
                                    d_slices, d_sample_status, d_have, stream);
  return slice_ingest<false, true>(ctx, d_chunks, chunks_bytes, nullptr, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_chunks, n_samples,
                                   d_slices, d_sample_status, nullptr, stream);
}

}  // extern "C"

// ---- stream sessions: outboards and verification of a file pushed in windows ---------------------------------------------------
// A host object: the file's shape, the caller's device pointers, a bit per tile pushed and (verification) the event behind which the
// storeys above the tiles have left what each tile must hash to.  No device memory of its own.
struct b3w_bao_stream {
  b3w_ctx *ctx = nullptr;
  uint32_t kind = 0, gl = 0;
  uint64_t len = 0, tiles = 0, groups = 0, pushed = 0;
  uint8_t *ob = nullptr;
  uint32_t *root = nullptr;
  uint8_t *unit_status = nullptr;
  int32_t *file_status = nullptr;
  unsigned long long *first_bad = nullptr;
  uint32_t *scratch = nullptr;
  hipEvent_t begun = nullptr;
  bool finished = false;
  std::vector<uint64_t> seen;
  uint64_t capacity = 0;                                 // open sessions: the bound given at begin (len is set by open_finish) ...
  uint8_t *blocks = nullptr;                             // ... and block 0 of the staging
};

namespace {

// the session's kernel over `count` tiles from tile `tile0`, their bytes at `window`
void stream_launch_tiles(const b3w_bao_stream *s, const uint8_t *window, uint32_t tile0, uint32_t count, hipStream_t st) {
  if (s->kind == B3W_BAO_STREAM_VERIFY) {
    const uint64_t n_scr = (s->tiles > 1 ? s->tiles : 0) + (s->groups > 1 ? s->groups : 0);
    hipLaunchKernelGGL(b3w_bao_stream_verify_kernel, dim3(count), dim3(B3W_TILE), 0, st, window, s->len, tile0, (const uint8_t *)s->ob, (const uint32_t *)s->root,
                       (const uint32_t *)s->scratch, (const uint32_t *)(s->scratch + n_scr * 8), s->gl, s->unit_status, s->file_status, s->first_bad);
  } else {
    launch_pair(s->gl != 0, b3w_bao_stream_tile_kernel, b3w_bao_stream_tile_group_kernel, s->gl, dim3(count), dim3(B3W_TILE), st, window, s->len, tile0, s->ob, s->root, s->scratch);
  }
}

int32_t stream_begin_checks(b3w_ctx *ctx, uint64_t len, uint32_t group_log, const void *d_outboard, const void *d_root, const void *d_scratch,
                            uint64_t scratch_bytes, uint64_t need, b3w_bao_stream **out) {
  if (!out) return refuse(ctx, "bao stream", "a null session pointer");
  *out = nullptr;
  B3W_TRY(group_log_ok(ctx, "bao stream", group_log));
  if (num_chunks(len) > (1ull << 30)) return refuse(ctx, "bao stream", "a file of more than 2^30 chunks");
  if (!d_outboard || !d_root) return refuse(ctx, "bao stream", "a null pointer (outboard or root)");
  if (((uintptr_t)d_outboard & 7) || ((uintptr_t)d_root & 3)) return refuse(ctx, "bao stream", "d_outboard is not 8-byte aligned, or d_root not 4-byte aligned");
  if (scratch_bytes < need) return refuse(ctx, "bao stream", "the scratch is smaller than b3w_bao_stream_scratch_bytes says");
  if (need && (!d_scratch || ((uintptr_t)d_scratch & 15))) return refuse(ctx, "bao stream", "the scratch is null or not 16-byte aligned");
  return B3W_OK;
}

b3w_bao_stream *stream_new(b3w_ctx *ctx, uint32_t kind, uint64_t len, uint32_t gl, void *d_scratch) {
  b3w_bao_stream *s = new b3w_bao_stream;
  s->ctx = ctx; s->kind = kind; s->gl = gl; s->len = len;
  s->tiles = tiles_of(len);
  s->groups = (s->tiles + B3W_TILE - 1) / B3W_TILE;
  s->scratch = reinterpret_cast<uint32_t *>(d_scratch);
  s->seen.assign((size_t)((s->tiles + 63) / 64), 0);
  return s;
}
// the session's tiles [t0, t0 + cnt) have been launched
void stream_mark(b3w_bao_stream *s, uint64_t t0, uint64_t cnt) {
  for (uint64_t t = t0; t < t0 + cnt; ++t) s->seen[t >> 6] |= 1ull << (t & 63);
  s->pushed += cnt;
}

// the per-window rules of a session of known length (whole tiles or up to the file's end, each tile once): the reason, or nullptr
const char *window_refusal(const b3w_bao_stream *s, uint64_t offset, const uint8_t *d_window, uint64_t bytes, std::string *twice) {
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  if (s->finished) return "the session is finished";
  if (offset % TB) return "the offset is not a multiple of 1 MiB";
  if (!bytes || !d_window) return "an empty window or a null pointer";
  if (offset > s->len || bytes > s->len - offset) return "the window reaches past the file's end";
  if (bytes % TB && offset + bytes != s->len) return "the window is not whole tiles of 1 MiB and does not end at the file's end";
  for (uint64_t t = offset / TB; t < (offset + bytes + TB - 1) / TB; ++t)
    if (s->seen[t >> 6] >> (t & 63) & 1) { *twice = "tile " + std::to_string(t) + " was pushed before"; return twice->c_str(); }
  return nullptr;
}

// ---- open-length sessions: the host side ---------------------------------------------------------------------------------------------
// an open session's group CVs: behind the tile CVs of its capacity in the scratch, the tail's tile included
uint32_t *open_group_cv(const b3w_bao_stream *s) { return s->scratch + tiles_of(s->capacity) * 8; }
// the relocation workgroups of T full tiles
uint64_t open_move_wgs(uint64_t T, uint32_t gl) {
  const OpenShape sh = open_shape(gl);
  return ((T + (1ull << sh.tpw_log) - 1) >> sh.tpw_log) * sh.ppb;
}
// the rules of finishing an open session with this tail into this outboard: the reason, or "" and the file's length
std::string open_finish_refusal(const b3w_bao_stream *s, const uint8_t *d_tail, uint64_t tail_bytes, const uint8_t *d_outboard, uint64_t outboard_bytes,
                                const uint32_t *d_root, uint64_t *out_len) {
  const uint64_t TB = (uint64_t)B3W_TILE * 1024, T = s->pushed;
  if (s->kind != B3W_BAO_STREAM_OPEN) return "not an open session";
  if (s->finished) return "the session is finished";
  for (uint64_t t = 0; t < T; ++t)
    if (!(s->seen[t >> 6] >> (t & 63) & 1)) return "tile " + std::to_string(t) + " has not been pushed and a later one has (" + std::to_string(T) + " tiles were pushed)";
  if (tail_bytes >= TB) return "a tail of 1 MiB or more (whole tiles are pushed)";
  if (tail_bytes && !d_tail) return "a null tail with bytes";
  const uint64_t len = T * TB + tail_bytes;
  if (len > s->capacity) return "the file (" + std::to_string(len) + " bytes) is longer than the session's capacity";
  if (!d_outboard || !d_root) return "a null pointer (outboard or root)";
  if (((uintptr_t)d_outboard & 7) || ((uintptr_t)d_root & 3)) return "d_outboard is not 8-byte aligned, or d_root not 4-byte aligned";
  if (outboard_bytes < group_outboard_bytes(len, s->gl)) return "the outboard is smaller than b3w_bao_group_outboard_size of the file's length";
  *out_len = len;
  return std::string();
}

// the per-window rules of an open session (whole tiles only, inside the capacity, each tile once): the reason, or nullptr
const char *open_window_refusal(const b3w_bao_stream *s, uint64_t offset, const uint8_t *d_window, uint64_t bytes, std::string *twice) {
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  if (s->finished) return "the session is finished";
  if (offset % TB) return "the offset is not a multiple of 1 MiB";
  if (!bytes || !d_window) return "an empty window or a null pointer";
  if (bytes % TB) return "the window of an open session is not whole tiles of 1 MiB (what does not fill a tile goes to b3w_bao_stream_open_finish)";
  if (offset > s->capacity || bytes > s->capacity - offset) return "the window reaches past the session's capacity";
  for (uint64_t t = offset / TB; t < (offset + bytes) / TB; ++t)
    if (s->seen[t >> 6] >> (t & 63) & 1) { *twice = "tile " + std::to_string(t) + " was pushed before"; return twice->c_str(); }
  return nullptr;
}

int32_t open_push(b3w_bao_stream *s, uint64_t offset, const uint8_t *d_window, uint64_t bytes, void *stream) {
  b3w_ctx *ctx = s->ctx;
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  std::string twice;
  if (const char *why = open_window_refusal(s, offset, d_window, bytes, &twice)) return refuse(ctx, "bao stream push", why);
  const uint64_t t0 = offset / TB, cnt = bytes / TB;
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  launch_pair(s->gl != 0, b3w_bao_stream_open_tile_kernel, b3w_bao_stream_open_tile_group_kernel, s->gl, dim3((uint32_t)cnt), dim3(B3W_TILE), st, d_window, (uint32_t)t0, s->blocks, s->scratch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "bao stream push launch (open session)");
  stream_mark(s, t0, cnt);
  return B3W_OK;
}

}  // namespace

extern "C" {

// ---- stream sessions: outboards and verification of a file pushed in windows ---------------------------------------------------
int32_t b3w_bao_stream_outboard_begin(b3w_ctx *ctx, uint64_t len, uint32_t group_log, uint8_t *d_outboard, uint32_t *d_root, void *d_scratch,
                                      uint64_t scratch_bytes, b3w_bao_stream **out_session) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(stream_begin_checks(ctx, len, group_log, d_outboard, d_root, d_scratch, scratch_bytes,
                                         b3w_bao_stream_scratch_bytes(len, B3W_BAO_STREAM_OUTBOARD), out_session));
  b3w_bao_stream *s = stream_new(ctx, B3W_BAO_STREAM_OUTBOARD, len, group_log, d_scratch);
  s->ob = d_outboard; s->root = d_root;
  *out_session = s;
  return B3W_OK;
}

int32_t b3w_bao_stream_verify_begin(b3w_ctx *ctx, uint64_t len, uint32_t group_log, const uint8_t *d_outboard, const uint32_t *d_root,
                                    uint8_t *d_unit_status, int32_t *d_file_status, uint64_t *d_first_bad, void *d_scratch, uint64_t scratch_bytes,
                                    void *stream, b3w_bao_stream **out_session) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(stream_begin_checks(ctx, len, group_log, d_outboard, d_root, d_scratch, scratch_bytes,
                                         b3w_bao_stream_scratch_bytes(len, B3W_BAO_STREAM_VERIFY), out_session));
  if (!d_unit_status || !d_file_status || !d_first_bad) return refuse(ctx, "bao stream", "a null output (unit status, file status or first bad)");
  if (((uintptr_t)d_first_bad & 7) || ((uintptr_t)d_file_status & 3)) return refuse(ctx, "bao stream", "d_first_bad is not 8-byte aligned, or d_file_status not 4-byte aligned");
  ON_DEVICE(ctx);
  b3w_bao_stream *s = stream_new(ctx, B3W_BAO_STREAM_VERIFY, len, group_log, d_scratch);
  s->ob = const_cast<uint8_t *>(d_outboard); s->root = const_cast<uint32_t *>(d_root);
  s->unit_status = d_unit_status; s->file_status = d_file_status; s->first_bad = reinterpret_cast<unsigned long long *>(d_first_bad);
  if (s->tiles > 1) {                                                 // top down over the stored nodes alone, as the batch call begins
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n_scr = s->tiles + (s->groups > 1 ? s->groups : 0);
    uint32_t *exp_cv = s->scratch, *bad = exp_cv + n_scr * 8;
    hipError_t e = hipEventCreateWithFlags(&s->begun, hipEventDisableTiming);
    if (e != hipSuccess) { delete s; return hip_fail(ctx, e, "bao stream: hipEventCreateWithFlags"); }
    if (s->groups > 1) hipLaunchKernelGGL(b3w_bao_stream_upper_kernel, dim3(1), dim3(256), 0, st, len, (uint64_t)B3W_TILE * B3W_TILE, s->tiles, d_outboard, d_root, exp_cv, bad, group_log, d_file_status, s->first_bad);
    hipLaunchKernelGGL(b3w_bao_stream_upper_kernel, dim3((uint32_t)s->groups), dim3(256), 0, st, len, (uint64_t)B3W_TILE, s->tiles, d_outboard, d_root, exp_cv, bad, group_log, d_file_status, s->first_bad);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s->begun, st);
    if (e != hipSuccess) { (void)hipEventDestroy(s->begun); delete s; return hip_fail(ctx, e, "bao stream verify begin"); }
  }
  *out_session = s;
  return B3W_OK;
}

int32_t b3w_bao_stream_push(b3w_bao_stream *s, uint64_t offset, const uint8_t *d_window, uint64_t bytes, void *stream) {
  if (!s) return B3W_E_BAD_ARGUMENT;
  b3w_ctx *ctx = s->ctx;
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  if (s->kind == B3W_BAO_STREAM_OPEN) return open_push(s, offset, d_window, bytes, stream);
  std::string twice;
  if (const char *why = window_refusal(s, offset, d_window, bytes, &twice)) return refuse(ctx, "bao stream push", why);
  const uint64_t t0 = offset / TB, cnt = (bytes + TB - 1) / TB;
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  if (s->begun) HIP_TRY(ctx, hipStreamWaitEvent(st, s->begun, 0));    // (on the device: the host waits for nothing)
  stream_launch_tiles(s, d_window, (uint32_t)t0, (uint32_t)cnt, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "bao stream push launch");
  stream_mark(s, t0, cnt);
  return B3W_OK;
}

int32_t b3w_bao_stream_finish(b3w_bao_stream *s, void *stream) {
  if (!s) return B3W_E_BAD_ARGUMENT;
  b3w_ctx *ctx = s->ctx;
  if (s->kind == B3W_BAO_STREAM_OPEN) return refuse(ctx, "bao stream finish", "an open session is finished by b3w_bao_stream_open_finish");
  if (s->finished) return refuse(ctx, "bao stream finish", "the session is finished");
  if (s->len && s->pushed != s->tiles) return refuse(ctx, "bao stream finish", std::to_string(s->tiles - s->pushed) + " of " + std::to_string(s->tiles) + " tiles have not been pushed");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  if (!s->len) stream_launch_tiles(s, nullptr, 0, 1, st);             // no byte, no push: the empty chunk's ROOT output, here
  else if (s->kind == B3W_BAO_STREAM_OUTBOARD && s->tiles > 1) stream_merge(s->len, s->groups, s->gl, s->scratch, s->scratch + s->tiles * 8, s->ob, s->root, st);
  // (verification: the windows' kernels have left the per-file outputs final)
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "bao stream finish launch");
  s->finished = true;
  return B3W_OK;
}

void b3w_bao_stream_free(b3w_bao_stream *s) {
  if (!s) return;
  if (s->begun) (void)hipEventDestroy(s->begun);
  delete s;
}

}  // extern "C"

namespace {

// ---- many stream sessions in one launch ----------------------------------------------------------------------------------------------
// A staging slot of the context's ring with room for `bytes` of rows: the first one, from many_next on, whose event has passed.  The
// host waits (for the oldest slot) only where every slot is still in flight; hipHostMalloc / hipMalloc only where the slot has to grow.
int32_t many_staging(b3w_ctx *ctx, uint64_t bytes, b3w_ctx::ManySlot **out) {
  const uint32_t N = b3w_ctx::B3W_MANY_SLOTS;
  b3w_ctx::ManySlot *m = nullptr;
  for (uint32_t k = 0; k < N && !m; ++k) {
    b3w_ctx::ManySlot &c = ctx->many_slots[(ctx->many_next + k) % N];
    if (c.busy) {
      const hipError_t e = hipEventQuery(c.done);
      if (e == hipErrorNotReady) continue;
      if (e != hipSuccess) return hip_fail(ctx, e, "bao stream many: hipEventQuery");
      c.busy = false;
    }
    m = &c;
    ctx->many_next = (ctx->many_next + k + 1) % N;
  }
  if (!m) {
    m = &ctx->many_slots[ctx->many_next];
    ctx->many_next = (ctx->many_next + 1) % N;
    HIP_TRY(ctx, hipEventSynchronize(m->done));
    m->busy = false;
  }
  if (!m->done) HIP_TRY(ctx, hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
  if (m->cap < bytes) {
    uint64_t cap = 4096;
    while (cap < bytes) cap *= 2;
    if (m->h) (void)hipHostFree(m->h);
    if (m->d) (void)hipFree(m->d);
    m->h = nullptr; m->d = nullptr; m->cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void **)&m->h, (size_t)cap, hipHostMallocDefault));
    HIP_TRY(ctx, hipMalloc((void **)&m->d, (size_t)cap));
    m->cap = cap;
  }
  *out = m;
  return B3W_OK;
}

// the rows to a slot and on to the device, on `st`; the caller launches behind the copy and then calls many_release
int32_t many_upload(b3w_ctx *ctx, const std::vector<ManyRow> &rows, hipStream_t st, b3w_ctx::ManySlot **slot) {
  const uint64_t bytes = rows.size() * sizeof(ManyRow);
  B3W_TRY(many_staging(ctx, bytes, slot));
  memcpy((*slot)->h, rows.data(), (size_t)bytes);
  HIP_TRY(ctx, hipMemcpyAsync((*slot)->d, (*slot)->h, (size_t)bytes, hipMemcpyHostToDevice, st));
  return B3W_OK;
}
// (called whether or not the launches went well: the copy is enqueued and reads the slot)
void many_release(b3w_ctx::ManySlot *slot, hipStream_t st) {
  if (hipEventRecord(slot->done, st) != hipSuccess) (void)hipStreamSynchronize(st);
  slot->busy = true;
}
// behind the launches of a call whose table went through a slot: the slot is released even when a launch failed
int32_t many_launched(b3w_ctx *ctx, b3w_ctx::ManySlot *slot, hipStream_t st, const char *what) {
  const hipError_t e = hipGetLastError();
  many_release(slot, st);
  return e != hipSuccess ? hip_fail(ctx, e, what) : B3W_OK;
}

ManyRow many_tile_row(const b3w_bao_stream *s, const uint8_t *window, uint32_t tile0, uint32_t first) {
  ManyRow r{};
  r.len = s->len; r.window = window; r.ob = s->ob; r.root = s->root; r.cv = s->scratch;
  r.first = first; r.tile0 = tile0; r.gl = s->gl;
  if (s->kind == B3W_BAO_STREAM_VERIFY) {
    const uint64_t n_scr = (s->tiles > 1 ? s->tiles : 0) + (s->groups > 1 ? s->groups : 0);
    r.aux = s->scratch + n_scr * 8;
    r.unit_status = s->unit_status; r.file_status = s->file_status; r.first_bad = s->first_bad;
  }
  return r;
}

// the tile kernel of the rows' kind over `rows` (on the device) with `wgs` workgroups in all
void many_launch_tiles(uint32_t kind, bool grp, const ManyRow *d_rows, uint32_t n_rows, uint32_t wgs, hipStream_t st) {
  if (kind == B3W_BAO_STREAM_VERIFY) hipLaunchKernelGGL(b3w_bao_stream_verify_many_kernel, dim3(wgs), dim3(B3W_TILE), 0, st, d_rows, n_rows);
  else if (grp) hipLaunchKernelGGL(b3w_bao_stream_tile_many_group_kernel, dim3(wgs), dim3(B3W_TILE), 0, st, d_rows, n_rows);
  else hipLaunchKernelGGL(b3w_bao_stream_tile_many_kernel, dim3(wgs), dim3(B3W_TILE), 0, st, d_rows, n_rows);
}

// entry i of a push pushes the session's tiles [t0, t0 + cnt)
struct Span { b3w_bao_stream *s; uint64_t t0, cnt; uint32_t i; };
// `total` tiles fit a grid and no tile is named twice -> the spans by (session, first tile)
int32_t spans_ok(b3w_ctx *ctx, const char *call, const std::vector<Span> &spans, uint64_t total, std::vector<Span> *by_tile) {
  if (total > 0x7fffffffull) return refuse(ctx, call, std::to_string(total) + " tiles in one call do not fit a 32-bit grid");
  *by_tile = spans;
  std::sort(by_tile->begin(), by_tile->end(), [](const Span &a, const Span &b) { return a.s != b.s ? std::less<const void *>()(a.s, b.s) : a.t0 != b.t0 ? a.t0 < b.t0 : a.i < b.i; });
  for (size_t k = 1; k < by_tile->size(); ++k) {
    const Span &a = (*by_tile)[k - 1], &b = (*by_tile)[k];
    if (a.s == b.s && a.t0 + a.cnt > b.t0)
      return refuse(ctx, call, entry_text(a.i > b.i ? a.i : b.i) + "tile " + std::to_string(b.t0) + " is named twice in the call (entry " + std::to_string(a.i < b.i ? a.i : b.i) + " has it too)");
  }
  return B3W_OK;
}
// no session is named twice in a finish
int32_t sessions_once(b3w_ctx *ctx, const char *call, b3w_bao_stream *const *sessions, uint32_t n) {
  std::vector<std::pair<const b3w_bao_stream *, uint32_t>> by_ptr(n);
  for (uint32_t i = 0; i < n; ++i) by_ptr[i] = {sessions[i], i};
  std::sort(by_ptr.begin(), by_ptr.end(), [](const auto &a, const auto &b) { return a.first != b.first ? std::less<const void *>()(a.first, b.first) : a.second < b.second; });
  for (uint32_t k = 1; k < n; ++k)
    if (by_ptr[k - 1].first == by_ptr[k].first)
      return refuse(ctx, call, entry_text(by_ptr[k].second) + "the session appears twice in the call (entry " + std::to_string(by_ptr[k - 1].second) + " is the same)");
  return B3W_OK;
}

// b3w_bao_stream_push_many for a call whose entry 0 is an open session: every session open, the open per-window rules, one launch
int32_t open_push_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, const uint64_t *offsets, const uint8_t *const *d_windows, const uint64_t *bytes,
                       uint32_t n, void *stream) {
  const char *call = "bao stream push_many";
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  std::vector<Span> spans(n), by_tile;
  uint64_t total = 0;
  bool grp = false;
  for (uint32_t i = 0; i < n; ++i) {                                  // every entry is checked before anything is launched or marked
    b3w_bao_stream *s = sessions[i];
    if (!s) return refuse(ctx, call, entry_text(i) + "a null session");
    if (s->ctx != ctx) return refuse(ctx, call, entry_text(i) + "the session belongs to another context");
    if (s->kind != B3W_BAO_STREAM_OPEN) return refuse(ctx, call, entry_text(i) + "the session is not of the kind of entry 0 (open sessions do not mix with sessions of known length)");
    std::string twice;
    if (const char *why = open_window_refusal(s, offsets[i], d_windows[i], bytes[i], &twice)) return refuse(ctx, call, entry_text(i) + why);
    spans[i] = Span{s, offsets[i] / TB, bytes[i] / TB, i};
    total += bytes[i] / TB;
    grp = grp || s->gl != 0;
  }
  B3W_TRY(spans_ok(ctx, call, spans, total, &by_tile));
  std::vector<ManyRow> rows(n);
  uint32_t first = 0;
  for (uint32_t i = 0; i < n; ++i) {
    ManyRow r{};
    r.window = d_windows[i]; r.ob = spans[i].s->blocks; r.cv = spans[i].s->scratch;
    r.first = first; r.tile0 = (uint32_t)spans[i].t0; r.gl = spans[i].s->gl;
    rows[i] = r;
    first += (uint32_t)spans[i].cnt;
  }
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_upload(ctx, rows, st, &slot));
  hipLaunchKernelGGL(grp ? b3w_bao_stream_open_tile_many_group_kernel : b3w_bao_stream_open_tile_many_kernel, dim3(first), dim3(B3W_TILE), 0, st,
                     reinterpret_cast<const ManyRow *>(slot->d), n);
  B3W_TRY(many_launched(ctx, slot, st, "bao stream push_many launch (open sessions)"));
  for (const Span &sp : spans) stream_mark(sp.s, sp.t0, sp.cnt);
  return B3W_OK;
}

}  // namespace

extern "C" {

// ---- many stream sessions in one launch ----------------------------------------------------------------------------------------------
int32_t b3w_bao_stream_push_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, const uint64_t *offsets, const uint8_t *const *d_windows,
                                 const uint64_t *bytes, uint32_t n, void *stream) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  if (!n) return B3W_OK;
  const char *call = "bao stream push_many";
  if (!sessions || !offsets || !d_windows || !bytes) return refuse(ctx, call, "a null array");
  if (sessions[0] && sessions[0]->kind == B3W_BAO_STREAM_OPEN) return open_push_many(ctx, sessions, offsets, d_windows, bytes, n, stream);
  const uint64_t TB = (uint64_t)B3W_TILE * 1024;
  std::vector<Span> spans(n), by_tile;
  uint64_t total = 0;
  bool grp = false;
  for (uint32_t i = 0; i < n; ++i) {                                  // every entry is checked before anything is launched or marked
    b3w_bao_stream *s = sessions[i];
    if (!s) return refuse(ctx, call, entry_text(i) + "a null session");
    if (s->ctx != ctx) return refuse(ctx, call, entry_text(i) + "the session belongs to another context");
    if (s->kind != sessions[0]->kind) return refuse(ctx, call, entry_text(i) + "the session is not of the kind of entry 0 (outboard and verification sessions do not mix)");
    std::string twice;
    if (const char *why = window_refusal(s, offsets[i], d_windows[i], bytes[i], &twice)) return refuse(ctx, call, entry_text(i) + why);
    const uint64_t t0 = offsets[i] / TB, cnt = (bytes[i] + TB - 1) / TB;
    spans[i] = Span{s, t0, cnt, i};
    total += cnt;
    grp = grp || s->gl != 0;
  }
  B3W_TRY(spans_ok(ctx, call, spans, total, &by_tile));
  std::vector<ManyRow> rows(n);
  uint32_t first = 0;
  for (uint32_t i = 0; i < n; ++i) {
    rows[i] = many_tile_row(spans[i].s, d_windows[i], (uint32_t)spans[i].t0, first);
    first += (uint32_t)spans[i].cnt;
  }
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  for (uint32_t k = 0; k < n; ++k)                                    // (on the device: the host waits for nothing)
    if (by_tile[k].s->begun && (k == 0 || by_tile[k - 1].s != by_tile[k].s)) HIP_TRY(ctx, hipStreamWaitEvent(st, by_tile[k].s->begun, 0));
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_upload(ctx, rows, st, &slot));
  many_launch_tiles(sessions[0]->kind, grp, reinterpret_cast<const ManyRow *>(slot->d), n, first, st);
  B3W_TRY(many_launched(ctx, slot, st, "bao stream push_many launch"));
  for (const Span &sp : spans) stream_mark(sp.s, sp.t0, sp.cnt);
  return B3W_OK;
}

int32_t b3w_bao_stream_finish_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, uint32_t n, void *stream) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  if (!n) return B3W_OK;
  const char *call = "bao stream finish_many";
  if (!sessions) return refuse(ctx, call, "a null array");
  uint64_t wgs = 0;
  bool grp = false;
  for (uint32_t i = 0; i < n; ++i) {
    const b3w_bao_stream *s = sessions[i];
    if (!s) return refuse(ctx, call, entry_text(i) + "a null session");
    if (s->ctx != ctx) return refuse(ctx, call, entry_text(i) + "the session belongs to another context");
    if (s->kind == B3W_BAO_STREAM_OPEN) return refuse(ctx, call, entry_text(i) + "an open session is finished by b3w_bao_stream_open_finish");
    if (s->kind != sessions[0]->kind) return refuse(ctx, call, entry_text(i) + "the session is not of the kind of entry 0 (outboard and verification sessions do not mix)");
    if (s->finished) return refuse(ctx, call, entry_text(i) + "the session is finished");
    if (s->len && s->pushed != s->tiles)
      return refuse(ctx, call, entry_text(i) + std::to_string(s->tiles - s->pushed) + " of " + std::to_string(s->tiles) + " tiles have not been pushed");
    wgs += s->groups;
    grp = grp || s->gl != 0;
  }
  if (wgs > 0x7fffffffull) return refuse(ctx, call, std::to_string(wgs) + " workgroups in one call do not fit a 32-bit grid");
  B3W_TRY(sessions_once(ctx, call, sessions, n));
  // one table, three runs of rows: the first merge storey (a workgroup per 1 024 tiles), the second (files past 1 GiB), the files of no bytes
  const bool outboard = sessions[0]->kind == B3W_BAO_STREAM_OUTBOARD;
  std::vector<ManyRow> rows;
  uint32_t n1 = 0, n2 = 0, n3 = 0, wg1 = 0;
  if (outboard) {
    for (uint32_t i = 0; i < n; ++i) {
      const b3w_bao_stream *s = sessions[i];
      if (!s->len || s->tiles <= 1) continue;
      ManyRow r = many_tile_row(s, nullptr, 0, wg1);
      r.aux = s->scratch + s->tiles * 8;
      rows.push_back(r); n1++; wg1 += (uint32_t)s->groups;
    }
    for (uint32_t i = 0; i < n; ++i) {
      const b3w_bao_stream *s = sessions[i];
      if (!s->len || s->groups <= 1) continue;
      ManyRow r = many_tile_row(s, nullptr, 0, n2);
      r.cv = s->scratch + s->tiles * 8; r.aux = nullptr;
      rows.push_back(r); n2++;
    }
  }
  for (uint32_t i = 0; i < n; ++i)
    if (!sessions[i]->len) { rows.push_back(many_tile_row(sessions[i], nullptr, 0, n3)); n3++; }
  if (!rows.empty()) {
    ON_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    b3w_ctx::ManySlot *slot = nullptr;
    B3W_TRY(many_upload(ctx, rows, st, &slot));
    const ManyRow *d_rows = reinterpret_cast<const ManyRow *>(slot->d);
    many_merge(grp, d_rows, n1, wg1, d_rows + n1, n2, st);
    if (n3) many_launch_tiles(sessions[0]->kind, grp, d_rows + n1 + n2, n3, n3, st);
    B3W_TRY(many_launched(ctx, slot, st, "bao stream finish_many launch"));
  }
  for (uint32_t i = 0; i < n; ++i) sessions[i]->finished = true;
  return B3W_OK;
}

// ---- open-length sessions (b3wit.h "outboards of streamed files whose length is not known up front") ---------------------------
uint64_t b3w_bao_stream_open_staging_bytes(uint64_t capacity_bytes, uint32_t group_log) {
  if (group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  return (capacity_bytes / ((uint64_t)B3W_TILE * 1024)) * open_shape(group_log).bb + OPEN_PAD;
}

int32_t b3w_bao_stream_open_begin(b3w_ctx *ctx, uint64_t capacity_bytes, uint32_t group_log, void *d_staging, uint64_t staging_bytes, void *d_scratch,
                                  uint64_t scratch_bytes, b3w_bao_stream **out_session) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  if (!out_session) return refuse(ctx, "bao stream open", "a null session pointer");
  *out_session = nullptr;
  B3W_TRY(group_log_ok(ctx, "bao stream open", group_log));
  if (num_chunks(capacity_bytes) > (1ull << 30)) return refuse(ctx, "bao stream open", "a capacity of more than 2^30 chunks");
  if (!d_staging || !d_scratch) return refuse(ctx, "bao stream open", "a null pointer (staging or scratch)");
  if (((uintptr_t)d_staging & 15) || ((uintptr_t)d_scratch & 15)) return refuse(ctx, "bao stream open", "the staging or the scratch is not 16-byte aligned");
  if (staging_bytes < b3w_bao_stream_open_staging_bytes(capacity_bytes, group_log)) return refuse(ctx, "bao stream open", "the staging is smaller than b3w_bao_stream_open_staging_bytes says");
  if (scratch_bytes < b3w_bao_stream_open_scratch_bytes(capacity_bytes)) return refuse(ctx, "bao stream open", "the scratch is smaller than b3w_bao_stream_open_scratch_bytes says");
  b3w_bao_stream *s = new b3w_bao_stream;
  s->ctx = ctx; s->kind = B3W_BAO_STREAM_OPEN; s->gl = group_log; s->capacity = capacity_bytes;
  s->tiles = capacity_bytes / ((uint64_t)B3W_TILE * 1024);             // (the tiles a push may name; open_finish sets len, tiles and groups)
  s->scratch = reinterpret_cast<uint32_t *>(d_scratch);
  s->blocks = reinterpret_cast<uint8_t *>(d_staging) + OPEN_PAD / 2;
  s->seen.assign((size_t)((s->tiles + 63) / 64), 0);
  *out_session = s;
  return B3W_OK;
}

int32_t b3w_bao_stream_open_finish(b3w_bao_stream *s, const uint8_t *d_tail, uint64_t tail_bytes, uint8_t *d_outboard, uint64_t outboard_bytes,
                                   uint32_t *d_root, void *stream, uint64_t *out_len) {
  if (!s) return B3W_E_BAD_ARGUMENT;
  b3w_ctx *ctx = s->ctx;
  const uint64_t T = s->pushed;
  uint64_t len = 0;
  const std::string why = open_finish_refusal(s, d_tail, tail_bytes, d_outboard, outboard_bytes, d_root, &len);
  if (!why.empty()) return refuse(ctx, "bao stream open_finish", why);
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t tiles = T + (tail_bytes || !T ? 1 : 0), groups = (tiles + B3W_TILE - 1) / B3W_TILE;
  uint32_t *tile_cv = s->scratch;
  // at most four launches: the tail's tile (for T = 0 the whole file, rooted; header and all), the blocks to their places, the storeys
  if (tail_bytes || !T)
    launch_pair(s->gl != 0, b3w_bao_stream_tile_kernel, b3w_bao_stream_tile_group_kernel, s->gl, dim3(1), dim3(B3W_TILE), st, d_tail, len, (uint32_t)T, d_outboard, d_root, tile_cv);
  if (T) hipLaunchKernelGGL(b3w_bao_stream_open_relocate_kernel, dim3((uint32_t)open_move_wgs(T, s->gl)), dim3(256), 0, st, (const uint8_t *)s->blocks, len, (uint32_t)T, s->gl, d_outboard, d_root);   // (at most 2^22)
  if (tiles > 1) stream_merge(len, groups, s->gl, tile_cv, open_group_cv(s), d_outboard, d_root, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(ctx, e, "bao stream open_finish launch");
  s->len = len; s->ob = d_outboard; s->root = d_root;
  s->finished = true;
  if (out_len) *out_len = len;
  return B3W_OK;
}

// b3w_bao_stream_open_finish for n sessions in at most four launches: one table through the staging ring in four runs of rows (the
// tails' tiles, the relocations, the first merge storey, the second), each run the rows of one grid.  The runs write disjoint bytes of
// every file (the storeys only nodes above tiles, the tail's tile only nodes below its own root, the blocks neither), so their order on
// the one stream is free.
int32_t b3w_bao_stream_open_finish_many(b3w_ctx *ctx, b3w_bao_stream *const *sessions, const uint8_t *const *d_tails, const uint64_t *tail_bytes,
                                        uint8_t *const *d_outboards, const uint64_t *outboard_bytes, uint32_t *const *d_roots, uint32_t n, void *stream,
                                        uint64_t *out_lens) {
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  if (!n) return B3W_OK;
  const char *call = "bao stream open_finish_many";
  if (!sessions || !d_tails || !tail_bytes || !d_outboards || !outboard_bytes || !d_roots) return refuse(ctx, call, "a null array");
  const uint64_t TB = (uint64_t)B3W_TILE * 1024, LIMIT = 0x7fffffffull;
  std::vector<uint64_t> lens(n);
  uint64_t wg_tail = 0, wg_move = 0, wg_one = 0, wg_two = 0;
  bool grp = false;
  for (uint32_t i = 0; i < n; ++i) {                                  // every entry is checked before anything is launched or marked
    const b3w_bao_stream *s = sessions[i];
    if (!s) return refuse(ctx, call, entry_text(i) + "a null session");
    if (s->ctx != ctx) return refuse(ctx, call, entry_text(i) + "the session belongs to another context");
    const std::string why = open_finish_refusal(s, d_tails[i], tail_bytes[i], d_outboards[i], outboard_bytes[i], d_roots[i], &lens[i]);
    if (!why.empty()) return refuse(ctx, call, entry_text(i) + why);
    const uint64_t T = s->pushed;
    const bool tail = tail_bytes[i] || !T;
    const uint64_t tiles = T + (tail ? 1 : 0);
    wg_tail += tail ? 1 : 0;
    wg_move += open_move_wgs(T, s->gl);
    wg_one += tiles > 1 ? (tiles + B3W_TILE - 1) / B3W_TILE : 0;
    wg_two += tiles > B3W_TILE ? 1 : 0;
    if (wg_tail > LIMIT || wg_move > LIMIT || wg_one > LIMIT || wg_two > LIMIT)
      return refuse(ctx, call, entry_text(i) + "with this entry one of the call's four grids has more than 2^31 - 1 workgroups");
    grp = grp || s->gl != 0;
  }
  B3W_TRY(sessions_once(ctx, call, sessions, n));
  // the row of entry i for one of the runs: the file's length, outboard, root and group_log; the run sets the rest
  auto row = [&](uint32_t i, uint32_t first) {
    ManyRow r{};
    r.len = lens[i]; r.ob = d_outboards[i]; r.root = d_roots[i]; r.gl = sessions[i]->gl; r.tile0 = (uint32_t)sessions[i]->pushed; r.first = first;
    return r;
  };
  std::vector<ManyRow> rows;
  rows.reserve((size_t)n * 2);
  uint32_t n_tail = 0, n_move = 0, n_one = 0, n_two = 0, first = 0;
  for (uint32_t i = 0; i < n; ++i) {                                  // the tails' tiles (for T = 0 the whole file, rooted; header and all)
    if (!tail_bytes[i] && sessions[i]->pushed) continue;
    ManyRow r = row(i, n_tail);
    r.window = d_tails[i]; r.cv = sessions[i]->scratch;
    rows.push_back(r); n_tail++;
  }
  for (uint32_t i = 0; i < n; ++i) {                                  // the blocks to their places, and the headers
    const uint64_t T = sessions[i]->pushed;
    if (!T) continue;
    ManyRow r = row(i, first);
    r.window = sessions[i]->blocks;
    rows.push_back(r); n_move++;
    first += (uint32_t)open_move_wgs(T, sessions[i]->gl);
  }
  first = 0;
  for (uint32_t i = 0; i < n; ++i) {                                  // the first merge storey: a workgroup per 1 024 tiles
    const uint64_t tiles = (lens[i] + TB - 1) / TB;
    if (tiles <= 1) continue;
    ManyRow r = row(i, first);
    r.cv = sessions[i]->scratch; r.aux = open_group_cv(sessions[i]);
    rows.push_back(r); n_one++;
    first += (uint32_t)((tiles + B3W_TILE - 1) / B3W_TILE);
  }
  for (uint32_t i = 0; i < n; ++i) {                                  // the second: files past 1 GiB
    if ((lens[i] + TB - 1) / TB <= B3W_TILE) continue;
    ManyRow r = row(i, n_two);
    r.cv = open_group_cv(sessions[i]);
    rows.push_back(r); n_two++;
  }
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_upload(ctx, rows, st, &slot));
  const ManyRow *d_tail = reinterpret_cast<const ManyRow *>(slot->d), *d_move = d_tail + n_tail, *d_one = d_move + n_move, *d_two = d_one + n_one;
  if (n_tail) many_launch_tiles(B3W_BAO_STREAM_OUTBOARD, grp, d_tail, n_tail, n_tail, st);
  if (n_move) hipLaunchKernelGGL(b3w_bao_stream_open_relocate_many_kernel, dim3((uint32_t)wg_move), dim3(256), 0, st, d_move, n_move);
  many_merge(grp, d_one, n_one, (uint32_t)wg_one, d_two, n_two, st);
  B3W_TRY(many_launched(ctx, slot, st, "bao stream open_finish_many launch"));
  for (uint32_t i = 0; i < n; ++i) {
    b3w_bao_stream *s = sessions[i];
    s->len = lens[i]; s->ob = d_outboards[i]; s->root = d_roots[i];
    s->finished = true;
    if (out_lens) out_lens[i] = lens[i];
  }
  return B3W_OK;
}

}  // extern "C"

namespace {

// ---- the sparse calls (update, ranged verification, resize) and the range slices ------------------------------------------------------
std::string update_range_text(uint32_t i, uint32_t file, uint64_t first, uint64_t count) {
  return "range " + std::to_string(i) + " (file " + std::to_string(file) + ", chunks " + std::to_string(first) + " + " + std::to_string(count) + ")";
}
// Where a sparse call finds its chunks: file f's bytes at base + offsets[f] of an arena of `bytes` bytes, or (null offsets) the listed
// chunks alone, slot by slot, in a packed buffer of `bytes` bytes (b3wit.h "sparse calls from packed chunk bytes")
struct SparseSrc {
  const uint8_t *base; uint64_t bytes; const uint64_t *offsets;
  bool packed() const { return !offsets; }
};
// the packed calls' own two refusals
int32_t packed_ok(b3w_ctx *ctx, const char *call, const SparseSrc &src, const PkLayout &pk) {
  if (pk.bytes && !src.base) return refuse(ctx, call, "a null d_packed with " + std::to_string(pk.bytes) + " bytes of listed chunks (b3w_bao_packed_layout's total_bytes)");
  if (src.bytes < pk.bytes)
    return refuse(ctx, call, "packed_bytes is " + std::to_string(src.bytes) + ", the listed chunks take " + std::to_string(pk.bytes) + " (b3w_bao_packed_layout's total_bytes)");
  return B3W_OK;
}
// the first item of a row's mask (not empty)
uint32_t mask_first(const uint32_t *mask) {
  uint32_t w = 0;
  while (!mask[w]) ++w;
  return w * 32 + (uint32_t)__builtin_ctz(mask[w]);
}
// the update and ranged-verification calls: every range is checked before anything is launched or written (null host_offsets: a packed
// call, which has no arena to look at)
int32_t sparse_ranges_ok(b3w_ctx *ctx, const char *call, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                         uint32_t n_files, const uint64_t *host_ob_first, const uint32_t *host_files, const uint64_t *host_first_chunk, const uint64_t *host_n_chunks,
                         uint32_t n_ranges, const char *null_arena) {
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint32_t f = host_files[i];
    const uint64_t a = host_first_chunk[i], c = host_n_chunks[i];
    if (f >= n_files) return refuse(ctx, call, update_range_text(i, f, a, c) + ": the file index is not below the file count " + std::to_string(n_files));
    const uint64_t len = host_lens[f], n = num_chunks(len);
    if (n > (1ull << 30)) return refuse(ctx, call, update_range_text(i, f, a, c) + ": a file of more than 2^30 chunks");
    if (a > n || c > n - a) return refuse(ctx, call, update_range_text(i, f, a, c) + " reaches past the file's " + std::to_string(n) + " chunks");
    if (host_offsets && (host_offsets[f] > arena_bytes || len > arena_bytes - host_offsets[f])) return refuse(ctx, call, update_range_text(i, f, a, c) + ": the file reaches past arena_bytes");
    if (host_offsets && len && !d_arena) return refuse(ctx, call, update_range_text(i, f, a, c) + null_arena);
    if (host_ob_first[f] & 7) return refuse(ctx, call, update_range_text(i, f, a, c) + ": the file's outboard offset is not a multiple of 8");
  }
  return B3W_OK;
}
// the waves these small files pack into
SmallPack small_waves(const uint64_t *lens, const std::vector<uint32_t> &files) {
  SmallPack pack;
  for (uint32_t f : files) (void)pack.add(num_chunks(lens[f]));
  return pack;
}
std::string resize_entry_text(uint32_t i, uint32_t file) { return "entry " + std::to_string(i) + " (file " + std::to_string(file) + ")"; }

}  // namespace

extern "C" {

}  // extern "C"

namespace {

// ---- updates in place, ranged verification, appends and truncations (b3wit.h) -----------------------------------------------------------
// b3w_bao_outboard_update_batch_device and b3w_bao_outboard_update_packed_device: one plan, one table, the same launches; the two differ in
// where a tile row's and a small file's bytes lie and in the tile kernel that reads them
int32_t update_call(b3w_ctx *ctx, const char *call, const SparseSrc src, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                    const uint64_t *host_ob_first, uint8_t *d_outboards, uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first_chunk,
                    const uint64_t *host_n_chunks, uint32_t n_ranges, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const uint8_t *const d_arena = src.base;
  const uint64_t *const host_offsets = src.offsets;
  if (!host_lens || !host_ob_first || !d_outboards || !d_roots || !host_files || !host_first_chunk || !host_n_chunks)
    return refuse(ctx, call, "a null pointer (offsets, lengths, outboard offsets, outboards, roots or a range array)");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_roots & 3)) return refuse(ctx, call, "d_outboards is not 8-byte aligned, or d_roots not 4-byte aligned");
  B3W_TRY(sparse_ranges_ok(ctx, call, d_arena, src.bytes, host_offsets, host_lens, n_files, host_ob_first, host_files, host_first_chunk, host_n_chunks, n_ranges,
                           ": a null arena with a dirty file that is not empty"));
  const std::vector<UpdRange> merged = b3w_int_update_ranges(host_lens, host_files, host_first_chunk, host_n_chunks, n_ranges);
  const UpdPlan p = b3w_int_update_plan(host_lens, merged, group_log);
  PkLayout pk;
  if (src.packed()) { pk = b3w_int_packed_layout(host_lens, merged, group_log); B3W_TRY(packed_ok(ctx, call, src, pk)); }
  const uint64_t need = (p.tile_slots + p.span_slots) * 32;
  if (scratch_bytes < need) return refuse(ctx, call, "the scratch is smaller than b3w_bao_update_scratch_bytes says (" + std::to_string(need) + " bytes)");
  if (need && (!d_scratch || ((uintptr_t)d_scratch & 15))) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  if (p.tiles.size() > 0x7fffffffull) return refuse(ctx, call, "more than 2^31 - 1 dirty tiles in one call");
  const uint64_t waves = small_waves(host_lens, p.small).waves;        // the small files' waves, as the batch call packs them
  if (p.small.empty() && p.tiles.empty()) return B3W_OK;              // (every range was empty)
  // one table: tile rows | span rows | top rows | the small files' entries | their waves' first files
  const uint64_t n_rows = p.tiles.size() + p.spans.size() + p.tops.size();
  const uint64_t bytes = n_rows * sizeof(UpdRow) + p.small.size() * sizeof(BatchEnt) + (p.small.empty() ? 0 : (waves + 1) * 4);
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_staging(ctx, bytes, &slot));
  uint32_t *scratch = reinterpret_cast<uint32_t *>(d_scratch), *span_cv = scratch + p.tile_slots * 8;
  UpdRow *h_rows = reinterpret_cast<UpdRow *>(slot->h);
  BatchEnt *h_small = reinterpret_cast<BatchEnt *>(h_rows + n_rows);
  uint32_t *h_waves = reinterpret_cast<uint32_t *>(h_small + p.small.size());
  auto row = [&](const UpdWg &w, uint32_t *in, uint32_t *out) {
    UpdRow r{};
    const uint32_t f = w.file;
    r.len = host_lens[f]; r.ob = d_outboards + host_ob_first[f]; r.root = d_roots + (uint64_t)f * 8;
    r.in = in; r.out = out; r.idx = w.idx; r.gl = group_log;
    memcpy(r.mask, w.mask, sizeof r.mask);
    return r;
  };
  UpdRow *at = h_rows;
  for (const UpdWg &w : p.tiles) {
    UpdRow r = row(w, nullptr, scratch + w.out * 8);
    r.data = src.packed() ? d_arena + 1024 * pk.slot_of(w.file, (uint64_t)w.idx * B3W_TILE + mask_first(w.mask)) : d_arena + host_offsets[w.file];
    *at++ = r;
  }
  for (const UpdWg &w : p.spans) *at++ = row(w, scratch + w.in * 8, span_cv + w.out * 8);
  for (const UpdWg &w : p.tops) *at++ = row(w, span_cv + w.in * 8, nullptr);
  SmallPack pack;
  pack.first = h_waves;
  for (uint32_t f : p.small) {
    const uint32_t lane = pack.add(num_chunks(host_lens[f]));
    h_small[pack.files - 1] = BatchEnt{src.packed() ? 1024 * pk.slot_of(f, 0) : host_offsets[f], host_lens[f], host_ob_first[f], lane, f};
  }
  pack.close();
  const hipError_t ec = hipMemcpyAsync(slot->d, slot->h, (size_t)bytes, hipMemcpyHostToDevice, st);
  if (ec != hipSuccess) return hip_fail(ctx, ec, "bao update: table upload");
  const UpdRow *d_tiles = reinterpret_cast<const UpdRow *>(slot->d), *d_spans = d_tiles + p.tiles.size(), *d_tops = d_spans + p.spans.size();
  const BatchEnt *d_small = reinterpret_cast<const BatchEnt *>(d_tops + p.tops.size());
  const uint32_t *d_waves = reinterpret_cast<const uint32_t *>(d_small + p.small.size());
  const uint64_t U = B3W_TILE;
  const bool grp = group_log != 0;
  const auto tile_kernel = src.packed() ? (grp ? b3w_bao_update_tile_packed_group_kernel : b3w_bao_update_tile_packed_kernel)
                                        : (grp ? b3w_bao_update_tile_group_kernel : b3w_bao_update_tile_kernel);
  const auto merge_kernel = grp ? b3w_bao_update_merge_group_kernel : b3w_bao_update_merge_kernel;
  if (pack.files) launch_pair(grp, b3w_bao_small_kernel, b3w_bao_small_group_kernel, group_log, dim3((uint32_t)waves), dim3(64), st, d_arena, d_small, d_waves, d_outboards, d_roots);
  if (!p.tiles.empty()) hipLaunchKernelGGL(tile_kernel, dim3((uint32_t)p.tiles.size()), dim3(B3W_TILE), 0, st, d_tiles);
  if (!p.spans.empty()) hipLaunchKernelGGL(merge_kernel, dim3((uint32_t)p.spans.size()), dim3(256), 0, st, d_spans, U);
  if (!p.tops.empty()) hipLaunchKernelGGL(merge_kernel, dim3((uint32_t)p.tops.size()), dim3(256), 0, st, d_tops, U * U);
  return many_launched(ctx, slot, st, (std::string(call) + " launch").c_str());
}

// b3w_bao_verify_ranges_batch_device and b3w_bao_verify_ranges_packed_device, as update_call
int32_t verify_ranges_call(b3w_ctx *ctx, const char *call, const SparseSrc src, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                           const uint64_t *host_ob_first, const uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                           const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges, const uint64_t *host_unit_first,
                           uint8_t *d_unit_status, int32_t *d_range_status, uint64_t *d_range_first_bad, void *d_scratch, uint64_t scratch_bytes,
                           void *stream) {
  const uint8_t *const d_arena = src.base;
  const uint64_t *const host_offsets = src.offsets;
  if (!host_lens || !host_ob_first || !d_outboards || !d_roots || !host_files || !host_first_chunk || !host_n_chunks || !host_unit_first)
    return refuse(ctx, call, "a null pointer (offsets, lengths, outboard offsets, unit offsets, outboards, roots or a range array)");
  if (!d_unit_status || !d_range_status || !d_range_first_bad) return refuse(ctx, call, "a null output pointer (unit statuses, range statuses or first bad units)");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_roots & 3)) return refuse(ctx, call, "d_outboards is not 8-byte aligned, or d_roots not 4-byte aligned");
  if (((uintptr_t)d_range_first_bad & 7) || ((uintptr_t)d_range_status & 3))
    return refuse(ctx, call, "d_range_first_bad is not 8-byte aligned, or d_range_status not 4-byte aligned");
  if (n_ranges > 0x7fffffffu) return refuse(ctx, call, "more than 2^31 - 1 ranges in one call");
  B3W_TRY(sparse_ranges_ok(ctx, call, d_arena, src.bytes, host_offsets, host_lens, n_files, host_ob_first, host_files, host_first_chunk, host_n_chunks, n_ranges,
                           ": a null arena with a listed file that is not empty"));
  const std::vector<UpdRange> merged = b3w_int_update_ranges(host_lens, host_files, host_first_chunk, host_n_chunks, n_ranges);
  const UpdPlan p = b3w_int_update_plan(host_lens, merged, group_log);
  PkLayout pk;
  if (src.packed()) { pk = b3w_int_packed_layout(host_lens, merged, group_log); B3W_TRY(packed_ok(ctx, call, src, pk)); }
  const uint64_t n_scr = p.tile_slots + p.span_slots, need = (n_scr * 36 + 15) & ~15ull;
  if (scratch_bytes < need) return refuse(ctx, call, "the scratch is smaller than b3w_bao_verify_ranges_scratch_bytes says (" + std::to_string(need) + " bytes)");
  if (need && (!d_scratch || ((uintptr_t)d_scratch & 15))) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  if (p.tiles.size() > 0x7fffffffull) return refuse(ctx, call, "more than 2^31 - 1 listed tiles in one call");
  const uint64_t waves = small_waves(host_lens, p.small).waves;        // the small files' waves, as the batch call packs them
  // one table: tile rows | span rows | top rows | the ranges as given | the small files' rows | their waves' first files
  const uint64_t n_rows = p.tiles.size() + p.spans.size() + p.tops.size();
  const uint64_t bytes = n_rows * sizeof(VrRow) + (uint64_t)n_ranges * sizeof(VrRange) + p.small.size() * sizeof(VrSmall) + (p.small.empty() ? 0 : (waves + 1) * 4);
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_staging(ctx, bytes, &slot));
  // scratch: the expected CVs of the listed tiles, then of the listed spans, then their words in the same order
  uint32_t *tile_cv = reinterpret_cast<uint32_t *>(d_scratch), *span_cv = tile_cv + p.tile_slots * 8, *tile_word = tile_cv + n_scr * 8,
           *span_word = tile_word + p.tile_slots;
  VrRow *h_rows = reinterpret_cast<VrRow *>(slot->h);
  VrRange *h_ranges = reinterpret_cast<VrRange *>(h_rows + n_rows);
  VrSmall *h_small = reinterpret_cast<VrSmall *>(h_ranges + n_ranges);
  uint32_t *h_waves = reinterpret_cast<uint32_t *>(h_small + p.small.size());
  auto row = [&](const UpdWg &w) {
    VrRow r{};
    const uint32_t f = w.file;
    r.len = host_lens[f]; r.ob = d_outboards + host_ob_first[f]; r.root = d_roots + (uint64_t)f * 8;
    r.unit_status = d_unit_status + host_unit_first[f];
    r.idx = w.idx; r.gl = group_log;
    memcpy(r.mask, w.mask, sizeof r.mask);
    return r;
  };
  VrRow *at = h_rows;
  for (const UpdWg &w : p.tiles) {
    VrRow r = row(w);
    r.data = src.packed() ? d_arena + 1024 * pk.slot_of(w.file, (uint64_t)w.idx * B3W_TILE + mask_first(w.mask)) : d_arena + host_offsets[w.file];
    r.want = tile_cv + w.out * 8; r.above = tile_word + w.out;
    *at++ = r;
  }
  for (const UpdWg &w : p.spans) {
    VrRow r = row(w);
    r.want = span_cv + w.out * 8; r.above = span_word + w.out; r.out_cv = tile_cv + w.in * 8; r.out_word = tile_word + w.in;
    *at++ = r;
  }
  for (const UpdWg &w : p.tops) { VrRow r = row(w); r.out_cv = span_cv + w.in * 8; r.out_word = span_word + w.in; *at++ = r; }
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint64_t a = host_first_chunk[i], c = host_n_chunks[i];
    h_ranges[i] = VrRange{d_unit_status + host_unit_first[host_files[i]], a >> group_log, c ? ((a + c - 1) >> group_log) - (a >> group_log) + 1 : 0};
  }
  SmallPack pack;
  pack.first = h_waves;
  for (uint32_t f : p.small) {
    const uint32_t lane = pack.add(num_chunks(host_lens[f]));
    h_small[pack.files - 1] = VrSmall{src.packed() ? 1024 * pk.slot_of(f, 0) : host_offsets[f], host_lens[f], d_outboards + host_ob_first[f], d_roots + (uint64_t)f * 8, d_unit_status + host_unit_first[f], lane, 0};
  }
  pack.close();
  const hipError_t ec = hipMemcpyAsync(slot->d, slot->h, (size_t)bytes, hipMemcpyHostToDevice, st);
  if (ec != hipSuccess) return hip_fail(ctx, ec, "bao verify ranges: table upload");
  const VrRow *d_tiles = reinterpret_cast<const VrRow *>(slot->d), *d_spans = d_tiles + p.tiles.size(), *d_tops = d_spans + p.spans.size();
  const VrRange *d_ranges = reinterpret_cast<const VrRange *>(d_tops + p.tops.size());
  const VrSmall *d_small = reinterpret_cast<const VrSmall *>(d_ranges + n_ranges);
  const uint32_t *d_waves = reinterpret_cast<const uint32_t *>(d_small + p.small.size());
  const uint64_t U = B3W_TILE;
  // top down: the storeys above the tiles first (stored nodes alone), then the kernels that read the files, then the ranges' reduction
  if (pack.files) hipLaunchKernelGGL(b3w_bao_verify_ranges_small_kernel, dim3((uint32_t)waves), dim3(64), 0, st, d_arena, d_small, d_waves, group_log);
  if (!p.tops.empty()) hipLaunchKernelGGL(b3w_bao_verify_ranges_upper_kernel, dim3((uint32_t)p.tops.size()), dim3(256), 0, st, d_tops, U * U);
  if (!p.spans.empty()) hipLaunchKernelGGL(b3w_bao_verify_ranges_upper_kernel, dim3((uint32_t)p.spans.size()), dim3(256), 0, st, d_spans, U);
  if (!p.tiles.empty())
    hipLaunchKernelGGL(src.packed() ? b3w_bao_verify_ranges_tile_packed_kernel : b3w_bao_verify_ranges_tile_kernel, dim3((uint32_t)p.tiles.size()), dim3(B3W_TILE), 0, st,
                       d_tiles);
  hipLaunchKernelGGL(b3w_bao_verify_ranges_reduce_kernel, dim3(n_ranges), dim3(256), 0, st, d_ranges, d_range_status,
                     reinterpret_cast<unsigned long long *>(d_range_first_bad));
  return many_launched(ctx, slot, st, (std::string(call) + " launch").c_str());
}

}  // namespace

extern "C" {

int32_t b3w_bao_outboard_update_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                             const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint64_t *host_ob_first,
                                             uint8_t *d_outboards, uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first_chunk,
                                             const uint64_t *host_n_chunks, uint32_t n_ranges, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao update";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_offsets) return refuse(ctx, call, "a null pointer (offsets, lengths, outboard offsets, outboards, roots or a range array)");
  return update_call(ctx, call, SparseSrc{d_arena, arena_bytes, host_offsets}, host_lens, n_files, group_log, host_ob_first, d_outboards, d_roots, host_files,
                     host_first_chunk, host_n_chunks, n_ranges, d_scratch, scratch_bytes, stream);
}

int32_t b3w_bao_outboard_update_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens, uint32_t n_files,
                                              uint32_t group_log, const uint64_t *host_ob_first, uint8_t *d_outboards, uint32_t *d_roots,
                                              const uint32_t *host_files, const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges,
                                              void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao update packed";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  return update_call(ctx, call, SparseSrc{d_packed, packed_bytes, nullptr}, host_lens, n_files, group_log, host_ob_first, d_outboards, d_roots, host_files,
                     host_first_chunk, host_n_chunks, n_ranges, d_scratch, scratch_bytes, stream);
}

int32_t b3w_bao_verify_ranges_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                           const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint64_t *host_ob_first,
                                           const uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                           const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges,
                                           const uint64_t *host_unit_first, uint8_t *d_unit_status, int32_t *d_range_status,
                                           uint64_t *d_range_first_bad, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao verify ranges";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_offsets) return refuse(ctx, call, "a null pointer (offsets, lengths, outboard offsets, unit offsets, outboards, roots or a range array)");
  return verify_ranges_call(ctx, call, SparseSrc{d_arena, arena_bytes, host_offsets}, host_lens, n_files, group_log, host_ob_first, d_outboards, d_roots, host_files,
                            host_first_chunk, host_n_chunks, n_ranges, host_unit_first, d_unit_status, d_range_status, d_range_first_bad, d_scratch, scratch_bytes,
                            stream);
}

int32_t b3w_bao_verify_ranges_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens, uint32_t n_files,
                                            uint32_t group_log, const uint64_t *host_ob_first, const uint8_t *d_outboards, const uint32_t *d_roots,
                                            const uint32_t *host_files, const uint64_t *host_first_chunk, const uint64_t *host_n_chunks, uint32_t n_ranges,
                                            const uint64_t *host_unit_first, uint8_t *d_unit_status, int32_t *d_range_status, uint64_t *d_range_first_bad,
                                            void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao verify ranges packed";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  return verify_ranges_call(ctx, call, SparseSrc{d_packed, packed_bytes, nullptr}, host_lens, n_files, group_log, host_ob_first, d_outboards, d_roots, host_files,
                            host_first_chunk, host_n_chunks, n_ranges, host_unit_first, d_unit_status, d_range_status, d_range_first_bad, d_scratch, scratch_bytes,
                            stream);
}

// At most five launches: one table through the staging ring in runs of rows, each run the rows of one grid (the tiles behind the kept
// ones, the relocations, the first merge storey, the second), then the small files' entries and their waves.  The runs write disjoint
// bytes of every file, as those of b3w_bao_stream_open_finish_many do; the storeys read the CVs the two launches before them leave.
int32_t b3w_bao_outboard_resize_batch_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets,
                                             const uint64_t *host_old_lens, const uint64_t *host_new_lens, uint32_t n_files, uint32_t group_log,
                                             const uint64_t *host_old_ob_first, const uint8_t *d_old_outboards, const uint64_t *host_new_ob_first,
                                             uint8_t *d_new_outboards, uint32_t *d_roots, const uint32_t *host_files, uint32_t n_resized, void *d_scratch,
                                             uint64_t scratch_bytes, void *stream) {
  const char *call = "bao resize";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_resized) return B3W_OK;
  if (!host_offsets || !host_old_lens || !host_new_lens || !host_old_ob_first || !d_old_outboards || !host_new_ob_first || !d_new_outboards || !d_roots || !host_files)
    return refuse(ctx, call, "a null pointer (offsets, lengths, outboard offsets, outboards, roots or the file list)");
  if (((uintptr_t)d_old_outboards & 7) || ((uintptr_t)d_new_outboards & 7) || ((uintptr_t)d_roots & 3))
    return refuse(ctx, call, "d_old_outboards or d_new_outboards is not 8-byte aligned, or d_roots not 4-byte aligned");
  const uint64_t LIMIT = 0x7fffffffull;
  SmallPack count;
  uint64_t n_tile = 0, wg_tile = 0, n_move = 0, wg_move = 0, n_one = 0, wg_one = 0, n_two = 0, need = 0;
  for (uint32_t i = 0; i < n_resized; ++i) {                          // every entry is checked before anything is launched or written
    const uint32_t f = host_files[i];
    if (f >= n_files) return refuse(ctx, call, resize_entry_text(i, f) + ": the file index is not below the file count " + std::to_string(n_files));
    const uint64_t old_len = host_old_lens[f], len = host_new_lens[f], n = num_chunks(len);
    if (n > (1ull << 30) || num_chunks(old_len) > (1ull << 30)) return refuse(ctx, call, resize_entry_text(i, f) + ": a file of more than 2^30 chunks at its old or new length");
    if (host_offsets[f] > arena_bytes || len > arena_bytes - host_offsets[f]) return refuse(ctx, call, resize_entry_text(i, f) + ": the file reaches past arena_bytes at its new length");
    const uint64_t kept = b3w_bao_resize_kept_tiles(old_len, len), tiles = tiles_of(len);
    if (len > kept * RES_TB && !d_arena) return refuse(ctx, call, resize_entry_text(i, f) + ": a null arena with a file whose bytes have to be read");
    if ((host_old_ob_first[f] & 7) || (host_new_ob_first[f] & 7)) return refuse(ctx, call, resize_entry_text(i, f) + ": an outboard offset of the file is not a multiple of 8");
    const uintptr_t a0 = (uintptr_t)d_old_outboards + host_old_ob_first[f], a1 = a0 + group_outboard_bytes(old_len, group_log);
    const uintptr_t b0 = (uintptr_t)d_new_outboards + host_new_ob_first[f], b1 = b0 + group_outboard_bytes(len, group_log);
    if (a0 < b1 && b0 < a1) return refuse(ctx, call, resize_entry_text(i, f) + ": the file's old and new outboards overlap");
    need += resize_slots(len) * 32;
    if (n <= 64) (void)count.add(n);
    else {
      if (tiles > kept) { n_tile++; wg_tile += tiles - kept; }
      if (kept) { n_move++; wg_move += open_move_wgs(kept, group_log); }
      if (tiles > 1) { n_one++; wg_one += (tiles + B3W_TILE - 1) / B3W_TILE; }
      if (tiles > B3W_TILE) n_two++;
    }
    if (count.waves > LIMIT || wg_tile > LIMIT || wg_move > LIMIT || wg_one > LIMIT || n_two > LIMIT)
      return refuse(ctx, call, resize_entry_text(i, f) + ": with this entry one of the call's five grids has more than 2^31 - 1 workgroups");
  }
  {
    std::vector<std::pair<uint32_t, uint32_t>> by_file(n_resized);
    for (uint32_t i = 0; i < n_resized; ++i) by_file[i] = {host_files[i], i};
    std::sort(by_file.begin(), by_file.end());
    for (uint32_t k = 1; k < n_resized; ++k)
      if (by_file[k - 1].first == by_file[k].first)
        return refuse(ctx, call, resize_entry_text(by_file[k].second, by_file[k].first) + ": the file is listed twice (entry " + std::to_string(by_file[k - 1].second) + " is the same)");
  }
  if (scratch_bytes < need) return refuse(ctx, call, "the scratch is smaller than b3w_bao_resize_scratch_bytes says (" + std::to_string(need) + " bytes)");
  if (need && (!d_scratch || ((uintptr_t)d_scratch & 15))) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  // one table: tile rows | relocation rows | first storey | second storey | the small files' entries | their waves' first files
  const uint64_t n_small = count.files;
  const uint64_t bytes = (n_tile + n_one + n_two) * sizeof(ManyRow) + n_move * sizeof(ResRow) + n_small * sizeof(BatchEnt) + count.first_bytes();
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_staging(ctx, bytes, &slot));
  ManyRow *h_tile = reinterpret_cast<ManyRow *>(slot->h), *h_one = h_tile + n_tile, *h_two = h_one + n_one;
  ResRow *h_move = reinterpret_cast<ResRow *>(h_two + n_two);
  BatchEnt *h_small = reinterpret_cast<BatchEnt *>(h_move + n_move);
  uint32_t *h_waves = reinterpret_cast<uint32_t *>(h_small + n_small);
  uint32_t *at = reinterpret_cast<uint32_t *>(d_scratch);
  uint32_t i_tile = 0, i_move = 0, i_one = 0, i_two = 0, f_tile = 0, f_move = 0, f_one = 0;
  SmallPack pack;
  pack.first = h_waves;
  for (uint32_t i = 0; i < n_resized; ++i) {
    const uint32_t f = host_files[i];
    const uint64_t old_len = host_old_lens[f], len = host_new_lens[f], n = num_chunks(len);
    if (n <= 64) {
      const uint32_t lane = pack.add(n);
      h_small[pack.files - 1] = BatchEnt{host_offsets[f], len, host_new_ob_first[f], lane, f};
      continue;
    }
    const uint64_t kept = b3w_bao_resize_kept_tiles(old_len, len), tiles = tiles_of(len);
    uint32_t *tile_cv = tiles > 1 ? at : nullptr, *span_cv = tiles > B3W_TILE ? at + tiles * 8 : nullptr;
    at += resize_slots(len) * 8;
    ManyRow r{};
    r.len = len; r.ob = d_new_outboards + host_new_ob_first[f]; r.root = d_roots + (uint64_t)f * 8; r.gl = group_log;
    if (tiles > kept) {                                               // the tiles behind the kept ones (kept = 0: every tile, the header with tile 0)
      ManyRow t = r;
      t.window = d_arena + host_offsets[f] + kept * RES_TB; t.cv = tile_cv; t.tile0 = (uint32_t)kept; t.first = f_tile;
      h_tile[i_tile++] = t;
      f_tile += (uint32_t)(tiles - kept);
    }
    if (kept) {                                                       // the kept blocks to their new places, the header, the kept tiles' CVs
      ResRow m{};
      m.old_len = old_len; m.new_len = len; m.old_ob = d_old_outboards + host_old_ob_first[f]; m.new_ob = r.ob; m.cv = tile_cv; m.root = r.root;
      m.first = f_move; m.tiles = (uint32_t)kept; m.gl = group_log;
      h_move[i_move++] = m;
      f_move += (uint32_t)open_move_wgs(kept, group_log);
    }
    if (tiles > 1) {                                                  // the first merge storey: a workgroup per 1 024 tiles
      ManyRow t = r;
      t.cv = tile_cv; t.aux = span_cv; t.first = f_one;
      h_one[i_one++] = t;
      f_one += (uint32_t)((tiles + B3W_TILE - 1) / B3W_TILE);
    }
    if (tiles > B3W_TILE) {                                           // the second: files past 1 GiB
      ManyRow t = r;
      t.cv = span_cv; t.first = i_two;
      h_two[i_two++] = t;
    }
  }
  pack.close();
  const hipError_t ec = hipMemcpyAsync(slot->d, slot->h, (size_t)bytes, hipMemcpyHostToDevice, st);
  if (ec != hipSuccess) return hip_fail(ctx, ec, "bao resize: table upload");
  const ManyRow *d_tile = reinterpret_cast<const ManyRow *>(slot->d), *d_one = d_tile + n_tile, *d_two = d_one + n_one;
  const ResRow *d_move = reinterpret_cast<const ResRow *>(d_two + n_two);
  const BatchEnt *d_small = reinterpret_cast<const BatchEnt *>(d_move + n_move);
  const uint32_t *d_waves = reinterpret_cast<const uint32_t *>(d_small + n_small);
  const bool grp = group_log != 0;
  if (n_small) launch_pair(grp, b3w_bao_small_kernel, b3w_bao_small_group_kernel, group_log, dim3((uint32_t)count.waves), dim3(64), st, d_arena, d_small, d_waves, d_new_outboards, d_roots);
  if (n_move) hipLaunchKernelGGL(b3w_bao_resize_relocate_kernel, dim3((uint32_t)wg_move), dim3(256), 0, st, d_move, (uint32_t)n_move);
  if (n_tile) many_launch_tiles(B3W_BAO_STREAM_OUTBOARD, grp, d_tile, (uint32_t)n_tile, (uint32_t)wg_tile, st);
  many_merge(grp, d_one, (uint32_t)n_one, (uint32_t)wg_one, d_two, (uint32_t)n_two, st);
  return many_launched(ctx, slot, st, "bao resize launch");
}

}  // extern "C"

// ---- range slices: the slice of a run of chunks, extracted and taken in (still ABI 1.4: new names only) ----------------------------------
// The slice of chunks [a, a + k) of a file of n chunks = the header, then the tree in pre-order restricted to the range: a parent node
// whose span meets the range gives its 64 bytes, then its left subtree where that meets the range, then its right one; a chunk of the
// range gives its bytes (b3wit.h "range slices").  Every shared node is carried once.  Places:
//   U(a, c)      the parent nodes whose span meets [a, c] (range_nodes: the common path, the split node, then the two boundary paths, on
//                which a sibling subtree of s chunks wholly inside the range adds s - 1 and one outside adds nothing: O(depth))
//   chunk c      at 8 + 64 U(a, c) + 1024 (c - a)
//   node X       over [lo, lo + size) that meets the range, c0 = max(lo, a): at place(c0) - 64 (the nodes of c0's path at or below X) —
//                between X and the first chunk of the range below it the slice holds that chunk's path alone
// Slices are packed at 8 modulo 16 (b3w_bao_range_slice_batch_layout), so nodes lie 8 off a 16-byte boundary and chunks on one.
// A ROW is (range, block): a block is B aligned chunks of the file, which is a subtree of the file's tree (full, or the ragged last one).
// Ranges of at most 64 chunks take rows of B = 64 (a wave each: one or two rows a range), longer ones rows of B = 1 024 (a workgroup per
// touched tile); the two kinds are one template and one launch each.  No workgroup waits for another and nothing is handed between them:
//   b3w_bao_range_slice_kernel<B>    the provider: the chunks' bytes from the arena and the nodes from the outboard to their places; with
//                                    group outboards the chunks of every touched group are hashed and the nodes inside the groups stored
//                                    from LDS before their level's merge (merge_pair<true> with a place), as b3w_bao_slice_group_kernel
//                                    does for one chunk.  A node above the block is moved by the row that holds the first chunk of the
//                                    range below it, the header by the row that holds chunk a: every byte has one writer.
//   b3w_bao_range_ingest_kernel<B>   the receiver: lane = chunk, the lanes of the range hash their chunk from the slice; the block's tree
//                                    is walked as ranges_in_lds walks it, the nodes loaded from the slice (ranges_pair<true>, a chunk the
//                                    leaf at every group_log: the nodes inside a group are in the slice and are verified); the D nodes
//                                    above the block are checked side by side by the first D lanes, each against its half of the node
//                                    above it (the root: against the file's root), as b3w_bao_slice_ingest_kernel checks a path — D <= 22
//                                    compressions a row for files up to 4 GiB, and every node of the block hashed once.  The verdicts go
//                                    down through the LDS flags (path_bad).  ONLY THEN the writes: the verified chunks' bytes by all
//                                    lanes in 16-byte pieces (put16), the stored nodes with a verified chunk below them (a second walk
//                                    that ORs "verified" upwards, no hashing), the nodes above the block and the header where the block
//                                    has a verified chunk, one atomicOr of a wave's 64 verdicts into the bitmap word.  The row's largest
//                                    status and first bad chunk go to the scratch.
//   b3w_bao_range_reduce_kernel      a wave per range: the largest status and the first bad chunk over the range's rows.
namespace {

// a range's entry and a workgroup's row of the two device calls' table (the planner's entry: `off` is the range's first chunk status)
struct RsRange { uint64_t len, off, ob, slice, first, count, have; uint32_t file, row0; };   // have: the file's first bitmap word; row0: its first row
struct RsRow { uint32_t range, block; };

__device__ __forceinline__ void copy_node(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src) {   // (both 8-byte aligned)
  const uint2 *s = reinterpret_cast<const uint2 *>(src);
  uint2 *d = reinterpret_cast<uint2 *>(dst);
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = s[k];
}

// The nodes above the block [a0, a0 + m) of a file of n chunks, root first: their number, lane t's own (the t-th) with the node above it
// and the side it hangs on, and the lowest one with the side the block hangs on.
struct RsAbove { uint64_t lo, cnt, plo, pcnt, last_lo, last_cnt; uint32_t depth; bool left, last_left; };
__device__ __forceinline__ RsAbove range_above(uint64_t n, uint64_t a0, uint64_t m, uint32_t t) {
  RsAbove r{};
  uint64_t lo = 0, cnt = n;
  uint32_t j = 0;
  for (; cnt > 1 && !(lo == a0 && cnt == m); ++j) {
    const uint64_t k = left_of(cnt);
    const bool left = a0 < lo + k;
    if (j == t) { r.lo = lo; r.cnt = cnt; }
    if (j + 1 == t) { r.plo = lo; r.pcnt = cnt; r.left = left; }
    r.last_lo = lo; r.last_cnt = cnt; r.last_left = left;
    if (left) cnt = k; else { lo += k; cnt -= k; }
  }
  r.depth = j;
  return r;
}

// what a row's lanes share: the block's place in the file and the part of the range inside it, [lo, hi) in the block's own lanes
struct RsBlock { uint64_t len, n, a, a0; uint32_t m, lo, hi; bool sole; };
template <int B>
__device__ __forceinline__ RsBlock range_block(const RsRange &r, uint32_t block) {
  RsBlock b;
  b.len = r.len; b.n = r.len ? (r.len + 1023) / 1024 : 1; b.a = r.first; b.a0 = (uint64_t)block * B;
  b.m = (uint32_t)(b.n - b.a0 < B ? b.n - b.a0 : B);
  const uint64_t e = r.first + r.count, top = b.a0 + b.m;
  b.lo = (uint32_t)((b.a > b.a0 ? b.a : b.a0) - b.a0);
  b.hi = (uint32_t)((e < top ? e : top) - b.a0);
  b.sole = b.n <= B;
  return b;
}
__device__ __forceinline__ uint32_t range_chunk_bytes(uint64_t len, uint64_t c) { return (uint32_t)(len - c * 1024 < 1024 ? len - c * 1024 : 1024); }
// the node over the block's lanes [i0, i0 + size): its place in the slice (before[]: U(a, c) of the range's lanes)
__device__ __forceinline__ uint64_t range_block_node_at(const RsBlock &b, const uint32_t *before, uint32_t i0, uint32_t size) {
  const uint32_t c0 = i0 > b.lo ? i0 : b.lo;
  return 8 + 64ull * before[c0] + 1024 * (b.a0 + c0 - b.a) - 64ull * depth_in(c0 - i0, size);
}

// PACKED (b3w_bao_range_slice_packed_device): `arena` is the packed buffer and r.off the place of the range's first LISTED chunk in it —
// the first chunk of the group that holds chunk a, or chunk 0 of a file of at most 64 chunks (b3w_bao_packed_layout's range_first) —
// and the chunks the range lists follow it slot by slot
template <int B, bool PACKED>
__device__ __forceinline__ void range_slice_body(const RsRange *__restrict__ ranges, const RsRow *__restrict__ rows, uint32_t gl,
                                                 const uint8_t *__restrict__ arena, const uint8_t *__restrict__ obs, uint8_t *__restrict__ slices) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ uint32_t before[B];
  const RsRow row = rows[blockIdx.x];
  const RsRange r = ranges[row.range];
  const RsBlock b = range_block<B>(r, row.block);
  const uint32_t t = threadIdx.x, G = 1u << gl;
  const uint8_t *__restrict__ data = arena + r.off, *__restrict__ ob = obs + r.ob;
  const uint64_t base = !PACKED || b.n <= 64 ? 0 : b.a & ~(uint64_t)(G - 1);   // the chunk of the file that lies at `data`
  uint8_t *__restrict__ sl = slices + r.slice;
  if (t >= b.lo && t < b.hi) before[t] = (uint32_t)range_nodes(b.n, b.a, b.a0 + t);
  // group outboards: the chunks of the touched groups, hashed (no byte behind the file's last one is read)
  const uint32_t gs = t & ~(G - 1);
  const bool touched = gl != 0 && t < b.m && gs < b.hi && gs + G > b.lo;
  if (touched) lane_chunk_cv(cv, data, b.a0 + t - base, b.len, b.n, b.a0 + t, true);
  for (uint32_t l = 0; (1u << l) < b.m; ++l) {
    if (l <= gl) lds_barrier();                            // (before[] and the level below inside a group; above the groups nothing is handed on)
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= b.m) continue;
    const uint32_t end = i0 + (2u << l), size = (end < b.m ? end : b.m) - i0;
    const bool meets = i0 < b.hi && i0 + size > b.lo;
    uint8_t *place = meets ? sl + range_block_node_at(b, before, i0, size) : nullptr;
    if (l < gl) {                                          // inside a group: computed, and stored where the range wants it
      const uint32_t g0 = i0 & ~(G - 1);
      if (g0 < b.hi && g0 + G > b.lo) merge_pair<true>(cv, i0, i1, place, 4u | (b.sole && (2u << l) >= b.m ? 8u : 0u));
    } else if (meets) {
      copy_node(place, ob + 8 + node_pos<true>(b.n, b.a0 + i0, size, gl) * 64);
    }
  }
  if (b.m == 1) lds_barrier();                             // (before[] for the bytes below; any other block has passed a barrier)
  // the nodes above the block whose first chunk of the range lies in it, and the header in front of chunk a
  const RsAbove up = range_above(b.n, b.a0, b.m, t);
  if (t < up.depth) {
    const uint64_t c0 = up.lo > b.a ? up.lo : b.a;
    if (c0 >= b.a0 && c0 < b.a0 + b.m) copy_node(sl + range_node_at(b.n, b.a, up.lo, up.cnt), ob + 8 + node_pos<true>(b.n, up.lo, up.cnt, gl) * 64);
  }
  if (t == 0 && b.a >= b.a0) *reinterpret_cast<uint2 *>(sl) = *reinterpret_cast<const uint2 *>(ob);
  for (uint32_t p = t; p < (b.hi - b.lo) * 64; p += B) {
    const uint32_t ch = b.lo + (p >> 6), q = (p & 63) * 16;
    const uint64_t c = b.a0 + ch;
    const uint32_t bytes = range_chunk_bytes(b.len, c);
    uint8_t *dst = sl + 8 + 64ull * before[ch] + 1024 * (c - b.a);
    const uint8_t *src = data + (c - base) * 1024;
    if (q + 16 <= bytes) move16<true>(dst + q, src + q);
    else for (uint32_t o = q; o < bytes; ++o) dst[o] = src[o];
  }
}
template <int B>
__global__ __launch_bounds__(B) void b3w_bao_range_slice_kernel(const RsRange *__restrict__ ranges, const RsRow *__restrict__ rows, uint32_t gl,
                                                                const uint8_t *__restrict__ arena, const uint8_t *__restrict__ obs,
                                                                uint8_t *__restrict__ slices) {
  range_slice_body<B, false>(ranges, rows, gl, arena, obs, slices);
}
template <int B>
__global__ __launch_bounds__(B) void b3w_bao_range_slice_packed_kernel(const RsRange *__restrict__ ranges, const RsRow *__restrict__ rows, uint32_t gl,
                                                                       const uint8_t *__restrict__ packed, const uint8_t *__restrict__ obs,
                                                                       uint8_t *__restrict__ slices) {
  range_slice_body<B, true>(ranges, rows, gl, packed, obs, slices);
}

// PACKED (b3w_bao_range_slice_ingest_packed_device): `arena` is a slot buffer and r.off the place of the range's first slot in it
// (1 024 bytes a listed chunk, the ranges one behind the other as given: chunk c of the range at r.off + 1024 (c - a)); `obs` may be
// null: no node and no header is stored (decode).
template <int B, bool PACKED = false>
__global__ __launch_bounds__(B) void b3w_bao_range_ingest_kernel(const RsRange *__restrict__ ranges, const RsRow *__restrict__ rows, uint32_t gl,
                                                                 const uint8_t *__restrict__ slices, const uint32_t *__restrict__ roots,
                                                                 uint8_t *__restrict__ arena, uint8_t *__restrict__ obs,
                                                                 unsigned long long *__restrict__ have, uint4 *__restrict__ results) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ uint32_t flags[B], listed[B], before[B];
  __shared__ uint32_t worst, first, above;
  const RsRow row = rows[blockIdx.x];
  const RsRange r = ranges[row.range];
  const RsBlock b = range_block<B>(r, row.block);
  const uint32_t t = threadIdx.x;
  const bool mine = t >= b.lo && t < b.hi;
  const uint8_t *__restrict__ sl = slices + r.slice;
  const uint32_t *__restrict__ root = roots + (uint64_t)r.file * 8;
  listed[t] = mine ? 1u : 0u;
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; above = 0; }
  __syncthreads();
  // 1. the verdicts: the range's chunks, the block's nodes bottom up, the nodes above the block side by side
  if (mine) {
    const uint64_t c = b.a0 + t, u = range_nodes(b.n, b.a, c);
    uint32_t h[8];
    before[t] = (uint32_t)u;
    chunk_cv(sl + 8 + 64 * u + 1024 * (c - b.a), range_chunk_bytes(b.len, c), c, b.n == 1 ? 8u : 0u, h);   // (16-byte aligned)
    put_cv(cv, t, h);
  }
  const RsAbove up = range_above(b.n, b.a0, b.m, t);
  if (t < up.depth) {
    uint32_t mw[16], ivv[8], o[8];
    load_node(sl + range_node_at(b.n, b.a, up.lo, up.cnt), mw);
    iv(ivv);
    blake3_cv(ivv, mw, 0, 0, 64, 4u | (t == 0 ? 8u : 0u), o);
    const uint32_t *want = t == 0 ? root : reinterpret_cast<const uint32_t *>(sl + range_node_at(b.n, b.a, up.plo, up.pcnt) + (up.left ? 0 : 32));
    if (!eq8(o, want)) atomicOr(&above, 1u);
  }
  for (uint32_t l = 0; (1u << l) < b.m; ++l) {             // (ranges_in_lds's loop: the node's place is the slice's)
    lds_barrier();
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= b.m) continue;
    const bool d0 = listed[i0] != 0, d1 = listed[i1] != 0;
    if (!d0 && !d1) continue;
    const uint32_t end = i0 + (2u << l), size = (end < b.m ? end : b.m) - i0;
    ranges_pair<true>(cv, flags, nullptr, i0, i1, d0, d1, l, sl + range_block_node_at(b, before, i0, size), 4u | (b.sole && (2u << l) >= b.m ? 8u : 0u),
                      1ull << l, size - (1u << l), 1, nullptr);
    listed[i0] = 1;
  }
  lds_barrier();
  if (t == 0) {                                            // slot 0: what the block's stored root node hashes to, or the CV of a block of one chunk
    const uint32_t *want = up.depth ? reinterpret_cast<const uint32_t *>(sl + range_node_at(b.n, b.a, up.last_lo, up.last_cnt) + (up.last_left ? 0 : 32)) : root;
    if (!eq8(cv, want)) flags[0] |= b.m == 1 ? VER_UNIT : VER_TOP;
  }
  lds_barrier();
  const uint2 hd = *reinterpret_cast<const uint2 *>(sl);
  const bool hdr = ((uint64_t)hd.x | ((uint64_t)hd.y << 32)) != b.len;
  uint32_t st = 0;
  if (mine) {
    st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t); }          // (LDS; a clean row issues none)
  }
  const bool ok = mine && st == 0;
  __syncthreads();
  listed[t] = ok ? 1u : 0u;                                // from here on: a verified chunk (below this slot)
  __syncthreads();
  if (t == 0) results[blockIdx.x] = make_uint4(worst, 0, first == ~0u ? ~0u : (uint32_t)(b.a0 + first), first == ~0u ? ~0u : (uint32_t)((b.a0 + first) >> 32));
  // 2. the places: nothing unverified is written
  uint8_t *__restrict__ data = arena + r.off, *__restrict__ ob = obs + r.ob;
  for (uint32_t p = t; p < (b.hi - b.lo) * 64; p += B) {
    const uint32_t ch = b.lo + (p >> 6), q = (p & 63) * 16;
    if (!listed[ch]) continue;
    const uint64_t c = b.a0 + ch;
    const uint32_t bytes = range_chunk_bytes(b.len, c);
    const uint8_t *src = sl + 8 + 64ull * before[ch] + 1024 * (c - b.a);
    uint8_t *dst;
    if constexpr (PACKED) dst = data + (c - b.a) * 1024; else dst = data + c * 1024;
    if (q + 16 <= bytes) put16(dst + q, src + q);
    else for (uint32_t o = q; o < bytes; ++o) dst[o] = src[o];
  }
  if (!PACKED || obs) {
    for (uint32_t l = 0; (1u << l) < b.m; ++l) {             // the stored nodes with a verified chunk below them
      lds_barrier();
      const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
      if (i1 >= b.m || !(listed[i0] | listed[i1])) continue;
      const uint32_t end = i0 + (2u << l), size = (end < b.m ? end : b.m) - i0;
      uint8_t *node = node_at<true>(ob + 8, b.n, b.a0 + i0, size, gl);
      if (node) copy_node(node, sl + range_block_node_at(b, before, i0, size));
      listed[i0] = 1;
    }
    lds_barrier();
    if (listed[0]) {
      if (t < up.depth) {
        uint8_t *node = node_at<true>(ob + 8, b.n, up.lo, up.cnt, gl);
        if (node) copy_node(node, sl + range_node_at(b.n, b.a, up.lo, up.cnt));
      }
      if (t == 0) *reinterpret_cast<uint2 *>(ob) = hd;       // the header (it is the length: just checked)
    }
  }
  if (have) {                                              // a wave's lanes are the chunks of one word (a block starts at a multiple of 64)
    const unsigned long long mask = __ballot(ok);
    if ((t & 63) == 0 && mask) atomicOr(have + r.have + ((b.a0 + t) >> 6), mask);
  }
}

// a wave per range: the largest status and the first bad chunk of its rows (results: a row's {status, -, first bad chunk low, high})
__global__ __launch_bounds__(256) void b3w_bao_range_reduce_kernel(const RsRange *__restrict__ ranges, uint32_t n_ranges, const uint4 *__restrict__ results,
                                                                   int32_t *__restrict__ range_status, unsigned long long *__restrict__ range_first_bad) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n_ranges) return;
  const uint64_t a = ranges[i].first, k = ranges[i].count, B = k <= RS_SHORT ? 64 : B3W_TILE;
  const uint32_t n_rows = (uint32_t)((a + k - 1) / B - a / B + 1);
  const uint4 *__restrict__ res = results + ranges[i].row0;
  uint32_t w = 0;
  unsigned long long f = ~0ull;
  for (uint32_t j = lane; j < n_rows; j += 64) {
    const uint4 v = res[j];
    const unsigned long long at = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    w = w > v.x ? w : v.x;
    f = f < at ? f : at;
  }
#pragma unroll
  for (int d = 32; d >= 1; d /= 2) {
    const uint32_t ow = __shfl_xor(w, d);
    const unsigned long long of = __shfl_xor(f, d);
    w = w > ow ? w : ow;
    f = f < of ? f : of;
  }
  if (lane == 0) { range_status[i] = (int32_t)w; range_first_bad[i] = f; }
}

// ---- step records from range slices: the prover's side -----------------------------------------------------------------------------------
// b3w_sample_plan_slices_kernel's records and statuses for the projection of the range slice onto every chunk of the range, on the row
// shape of the receiver (b3w_bao_range_ingest_kernel<B>: lane = chunk, every node of the block hashed once):
//   0. where a lane's rows start: the row's base (a 64-bit field of its table entry, from the host's closed form rows_before) plus the
//      prefix sum over the block's lanes of blocks + path nodes (a wave's by shuffles, the waves' totals through LDS)
//   1. the range's lanes run plan_leaf_chunk on their chunk's bytes in the slice: the leaf records in place, the chunk's CV to LDS
//   2. - 4. the receiver's verdicts: the block's tree with ranges_pair<true>, the nodes above the block side by side (their places kept in
//      LDS for step 5), the verdicts down through the flags (path_bad); the chunk's status out, the row's result to the scratch
//   5. the parent records, bottom up, each from the slice's own node: a verified chunk with a provable path gets parent_record from the
//      on-path and sibling halves; any other the plan_parent_step chain on its lane.
// Every row of 128 bytes is written by the lane that owns the chunk.  `off` of the range's entry is its first chunk status.
struct RpRow { uint32_t range, block; uint64_t row; };    // row: the first record row of the block's first chunk of the range

template <int B>
__global__ __launch_bounds__(B) void b3w_sample_plan_range_kernel(const RsRange *__restrict__ ranges, const RpRow *__restrict__ rows,
                                                                  const uint8_t *__restrict__ slices, const uint32_t *__restrict__ roots,
                                                                  uint32_t *__restrict__ recs, int32_t *__restrict__ chunk_status,
                                                                  uint4 *__restrict__ results) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ uint32_t flags[B], listed[B], before[B];
  __shared__ uint64_t above_at[64];
  __shared__ uint32_t wave_rows[B / 64], worst, first, above;
  const RpRow row = rows[blockIdx.x];
  const RsRange r = ranges[row.range];
  const RsBlock b = range_block<B>(r, row.block);
  const uint32_t t = threadIdx.x;
  const bool mine = t >= b.lo && t < b.hi;
  const uint8_t *__restrict__ sl = slices + r.slice;
  const uint32_t *__restrict__ root = roots + (uint64_t)r.file * 8;
  const uint64_t c = b.a0 + t;
  const uint32_t P = mine ? depth_in(c, b.n) : 0, bytes = mine ? range_chunk_bytes(b.len, c) : 0, n_blocks = bytes ? (bytes + 63) / 64 : 1;
  listed[t] = mine ? 1u : 0u;
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; above = 0; }
  // 0. the lane's first row
  const uint32_t own = mine ? n_blocks + P : 0;
  uint32_t upto = own;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const uint32_t o = __shfl_up(upto, d);
    if ((t & 63) >= (uint32_t)d) upto += o;
  }
  if ((t & 63) == 63) wave_rows[t >> 6] = upto;
  __syncthreads();
  uint32_t ahead = upto - own;
  for (uint32_t w = 0; w < (t >> 6); ++w) ahead += wave_rows[w];
  uint32_t *__restrict__ rec = recs + (row.row + ahead) * 32;
  // 1. the leaf records and the chunks' CVs
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mine) {
    const uint64_t u = range_nodes(b.n, b.a, c);
    before[t] = (uint32_t)u;
    plan_leaf_chunk(sl + 8 + 64 * u + 1024 * (c - b.a), bytes, c, P, rec, h);   // (16-byte aligned; P == 0: the ROOT-flagged output)
    put_cv(cv, t, h);
  }
  // 2. - 4. the verdicts, as the receiver reaches them
  const RsAbove up = range_above(b.n, b.a0, b.m, t);
  if (t < up.depth) {
    uint32_t mw[16], ivv[8], o[8];
    const uint64_t at = range_node_at(b.n, b.a, up.lo, up.cnt);
    above_at[t] = at;
    load_node(sl + at, mw);
    iv(ivv);
    blake3_cv(ivv, mw, 0, 0, 64, 4u | (t == 0 ? 8u : 0u), o);
    const uint32_t *want = t == 0 ? root : reinterpret_cast<const uint32_t *>(sl + range_node_at(b.n, b.a, up.plo, up.pcnt) + (up.left ? 0 : 32));
    if (!eq8(o, want)) atomicOr(&above, 1u);
  }
  for (uint32_t l = 0; (1u << l) < b.m; ++l) {
    lds_barrier();
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= b.m) continue;
    const bool d0 = listed[i0] != 0, d1 = listed[i1] != 0;
    if (!d0 && !d1) continue;
    const uint32_t end = i0 + (2u << l), size = (end < b.m ? end : b.m) - i0;
    ranges_pair<true>(cv, flags, nullptr, i0, i1, d0, d1, l, sl + range_block_node_at(b, before, i0, size), 4u | (b.sole && (2u << l) >= b.m ? 8u : 0u),
                      1ull << l, size - (1u << l), 1, nullptr);
    listed[i0] = 1;
  }
  lds_barrier();
  if (t == 0) {
    const uint32_t *want = up.depth ? reinterpret_cast<const uint32_t *>(sl + range_node_at(b.n, b.a, up.last_lo, up.last_cnt) + (up.last_left ? 0 : 32)) : root;
    if (!eq8(cv, want)) flags[0] |= b.m == 1 ? VER_UNIT : VER_TOP;
  }
  lds_barrier();
  const uint2 hd = *reinterpret_cast<const uint2 *>(sl);
  const bool hdr = ((uint64_t)hd.x | ((uint64_t)hd.y << 32)) != b.len;
  uint32_t st = 0;
  if (mine) {
    st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    chunk_status[r.off + (c - b.a)] = (int32_t)st;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t); }
  }
  __syncthreads();
  if (t == 0) results[blockIdx.x] = make_uint4(worst, 0, first == ~0u ? ~0u : (uint32_t)(b.a0 + first), first == ~0u ? ~0u : (uint32_t)((b.a0 + first) >> 32));
  if (!mine) return;
  // 5. the parent records: the block's nodes on the lane's path bottom up, then the nodes above the block
  const bool chain = st != 0 || !path_provable(c, b.n);
  uint32_t g = 0;
  rec += (uint64_t)n_blocks * 32;
  const auto step = [&](uint64_t at) {
    uint32_t mw[16], on[8], sib[8];
    load_node(sl + at, mw);
    const bool bit_left = ((c >> g) & 1) == 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { on[k] = bit_left ? mw[k] : mw[8 + k]; sib[k] = bit_left ? mw[8 + k] : mw[k]; }
    if (chain) plan_parent_step(rec, h, sib, bit_left, c, n_blocks, P, P - 1 - g);
    else {
      if (g) {                                             // (every node hashed to its half of the node above: h at height g is that half)
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = on[k];
      }
      parent_record(rec, h, sib, c, n_blocks, P, P - 1 - g);
    }
    rec += 32; ++g;
  };
  for (uint32_t l = 0; (1u << l) < b.m; ++l) {
    const uint32_t i0 = (t >> (l + 1)) << (l + 1), i1 = i0 + (1u << l);
    if (i1 >= b.m) continue;
    const uint32_t end = i0 + (2u << l), size = (end < b.m ? end : b.m) - i0;
    step(range_block_node_at(b, before, i0, size));
  }
  for (uint32_t j = up.depth; j-- > 0;) step(above_at[j]);
}

struct RangeRows { uint64_t big, small; };                // rows of 1 024 chunks, rows of 64

// every refusal the range calls share that concerns the ranges; counts the rows.  The planner has no arena (null host_offsets: the arena
// is not looked at) and a longest file (most_chunks; 0: none).
int32_t range_list_ok(b3w_ctx *ctx, const char *what, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                      uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, RangeRows &rows,
                      uint64_t most_chunks = 0) {
  rows = RangeRows{};
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const char *why = nullptr;
    const uint32_t f = host_files[i];
    if (f >= n_files) why = "its file index is not below the file count";
    else {
      const uint64_t n = num_chunks(host_lens[f]), off = host_offsets ? host_offsets[f] : 0, len = host_lens[f];
      if (host_count[i] == 0) why = "it has no chunk";
      else if (host_first[i] >= n || host_count[i] > n - host_first[i]) why = "it reaches past its file's chunk count";
      else if (most_chunks && n > most_chunks) why = "its file has more than 2^30 chunks";
      else if (!host_offsets) why = nullptr;
      else if (len && !d_arena) why = "a null arena with a file that is not empty";
      else if (off > arena_bytes || len > arena_bytes - off) why = "its file reaches past arena_bytes";
    }
    if (why) return refuse(ctx, what, "range " + std::to_string(i) + ": " + why);
    (host_count[i] <= RS_SHORT ? rows.small : rows.big) += range_rows(host_first[i], host_count[i]);
  }
  if (rows.big > 0x7fffffffull || rows.small > 0x7fffffffull) return refuse(ctx, what, "more than 2^31 - 1 rows of one kind");
  return B3W_OK;
}

// the table into the staging and on its way: the ranges' entries, the rows of 1 024 chunks, the rows of 64 (behind them, host only, the
// files' outboard offsets and bitmap words).  The call says what a range's `off` is (off_of(i, file), asked once a range, in order, before
// the range's rows) and makes its own kind of row (make_row(i, block, B)).
template <class Row, class Off, class Make>
int32_t range_table(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint32_t *host_files,
                    const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, RangeRows rows, hipStream_t st, const RsRange *&d_ranges,
                    const Row *&d_big, const Row *&d_small, Off off_of, Make make_row) {
  const uint64_t up_bytes = (uint64_t)n_ranges * sizeof(RsRange) + (rows.big + rows.small) * sizeof(Row);
  B3W_TRY(batch_staging(ctx, up_bytes + 2 * ((uint64_t)n_files + 1) * 8));
  RsRange *rg = reinterpret_cast<RsRange *>(ctx->h_batch);
  Row *big = reinterpret_cast<Row *>(rg + n_ranges), *small = big + rows.big;
  uint64_t *ob_first = reinterpret_cast<uint64_t *>(small + rows.small), *word_first = ob_first + n_files + 1;
  (void)b3w_bao_group_batch_layout(host_lens, n_files, group_log, ob_first);        // (group_log 0: b3w_bao_batch_layout's)
  (void)b3w_bao_have_layout(host_lens, n_files, word_first);
  uint64_t at = slice_start(0), nb = 0, ns = 0;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    const uint32_t f = host_files[i];
    const uint64_t len = host_lens[f], a = host_first[i], k = host_count[i];
    const bool shrt = k <= RS_SHORT;
    const uint64_t B = shrt ? 64 : B3W_TILE, b0 = a / B, b1 = (a + k - 1) / B;
    rg[i] = RsRange{len, off_of(i, f), ob_first[f], at, a, k, word_first[f], f, (uint32_t)(shrt ? rows.big + ns : nb)};
    Row *out = shrt ? small + ns : big + nb;
    for (uint64_t blk = b0; blk <= b1; ++blk) *out++ = make_row(i, blk, B);
    (shrt ? ns : nb) += b1 - b0 + 1;
    at = slice_start(at + range_slice_bytes(len, num_chunks(len), a, k));
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)up_bytes, hipMemcpyHostToDevice, st));
  d_ranges = reinterpret_cast<const RsRange *>(ctx->d_batch);
  d_big = reinterpret_cast<const Row *>(d_ranges + n_ranges);
  d_small = d_big + rows.big;
  return B3W_OK;
}
// the provider's and the receiver's table: `off` is the file's place in the arena, a row its range and block
int32_t range_table(b3w_ctx *ctx, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint32_t *host_files,
                    const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, RangeRows rows, hipStream_t st, const RsRange *&d_ranges,
                    const RsRow *&d_big, const RsRow *&d_small) {
  return range_table<RsRow>(ctx, host_lens, n_files, group_log, host_files, host_first, host_count, n_ranges, rows, st, d_ranges, d_big, d_small,
                            [&](uint32_t, uint32_t f) { return host_offsets[f]; }, [](uint32_t i, uint64_t blk, uint64_t) { return RsRow{i, (uint32_t)blk}; });
}

// b3w_bao_range_slice_ingest_device, and PACKED: b3w_bao_range_slice_ingest_packed_device - (d_arena, arena_bytes) its slot buffer, no
// offsets, d_outboards may be null; a range's `off` is the place of its first slot, 1 024 bytes times the running sum of the counts
template <bool PACKED>
int32_t range_slice_ingest(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files,
                           uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first,
                           const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_range_status, uint64_t *d_range_first_bad,
                           uint64_t *d_have, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = PACKED ? "bao range slice ingest packed" : "bao range slice ingest";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if ((uintptr_t)d_have & 7) return refuse(ctx, call, "d_have is not 8-byte aligned");
  if (!n_ranges) return B3W_OK;
  if ((!PACKED && (!host_offsets || !d_outboards)) || !host_lens || !d_roots || !host_files || !host_first || !host_count || !d_slices || !d_range_status || !d_range_first_bad) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  if (((uintptr_t)d_range_status & 3) || ((uintptr_t)d_range_first_bad & 7)) return refuse(ctx, call, "d_range_status is not 4-byte or d_range_first_bad not 8-byte aligned");
  RangeRows rows;
  B3W_TRY(range_list_ok(ctx, call, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_first, host_count, n_ranges, rows));
  if (PACKED) B3W_TRY(slots_ok(ctx, call, d_arena, arena_bytes, b3w_int_listed_chunks(host_count, n_ranges)));
  if (scratch_bytes < (rows.big + rows.small) * 16) return refuse(ctx, call, "the scratch is smaller than b3w_bao_range_slice_ingest_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 15)) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const RsRange *d_ranges = nullptr;
  const RsRow *d_big = nullptr, *d_small = nullptr;
  uint64_t next_slot = 0;
  B3W_TRY(range_table<RsRow>(ctx, host_lens, n_files, group_log, host_files, host_first, host_count, n_ranges, rows, st, d_ranges, d_big, d_small,
                             [&](uint32_t i, uint32_t f) {
                               if (!PACKED) return host_offsets[f];
                               const uint64_t slot = next_slot;
                               next_slot += host_count[i];
                               return 1024 * slot;
                             },
                             [](uint32_t i, uint64_t blk, uint64_t) { return RsRow{i, (uint32_t)blk}; }));
  uint4 *res = reinterpret_cast<uint4 *>(d_scratch);
  unsigned long long *have = reinterpret_cast<unsigned long long *>(d_have);
  if (rows.big)
    hipLaunchKernelGGL((b3w_bao_range_ingest_kernel<(int)B3W_TILE, PACKED>), dim3((uint32_t)rows.big), dim3(B3W_TILE), 0, st, d_ranges, d_big, group_log, d_slices, d_roots,
                       d_arena, d_outboards, have, res);
  if (rows.small)
    hipLaunchKernelGGL((b3w_bao_range_ingest_kernel<64, PACKED>), dim3((uint32_t)rows.small), dim3(64), 0, st, d_ranges, d_small, group_log, d_slices, d_roots, d_arena,
                       d_outboards, have, res + rows.big);
  hipLaunchKernelGGL(b3w_bao_range_reduce_kernel, dim3((n_ranges + 3) / 4), dim3(256), 0, st, d_ranges, n_ranges, res, d_range_status,
                     reinterpret_cast<unsigned long long *>(d_range_first_bad));
  return batch_launched(ctx, st, PACKED ? "bao range slice ingest packed launch" : "bao range slice ingest launch");
}

}  // namespace

extern "C" {

// ---- range slices --------------------------------------------------------------------------------------------------------------------
int32_t b3w_bao_range_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                         uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files,
                                         const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices, void *stream) {
  const char *call = "bao range slice arena";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !host_files || !host_first || !host_count || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  RangeRows rows;
  B3W_TRY(range_list_ok(ctx, call, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_first, host_count, n_ranges, rows));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const RsRange *d_ranges = nullptr;
  const RsRow *d_big = nullptr, *d_small = nullptr;
  B3W_TRY(range_table(ctx, host_offsets, host_lens, n_files, group_log, host_files, host_first, host_count, n_ranges, rows, st, d_ranges, d_big, d_small));
  if (rows.big) hipLaunchKernelGGL(b3w_bao_range_slice_kernel<(int)B3W_TILE>, dim3((uint32_t)rows.big), dim3(B3W_TILE), 0, st, d_ranges, d_big, group_log, d_arena, d_outboards, d_slices);
  if (rows.small) hipLaunchKernelGGL(b3w_bao_range_slice_kernel<64>, dim3((uint32_t)rows.small), dim3(64), 0, st, d_ranges, d_small, group_log, d_arena, d_outboards, d_slices);
  return batch_launched(ctx, st, "bao range slice arena launch");
}

// the same table and grids; a range's `off` is the place of its first listed chunk in the packed buffer
int32_t b3w_bao_range_slice_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens, uint32_t n_files,
                                          uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files, const uint64_t *host_first,
                                          const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices, void *stream) {
  const char *call = "bao range slice packed";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_lens || !d_outboards || !host_files || !host_first || !host_count || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  RangeRows rows;
  B3W_TRY(range_list_ok(ctx, call, nullptr, 0, nullptr, host_lens, n_files, host_files, host_first, host_count, n_ranges, rows));
  const PkLayout pk = b3w_int_packed_layout(host_lens, b3w_int_update_ranges(host_lens, host_files, host_first, host_count, n_ranges), group_log);
  B3W_TRY(packed_ok(ctx, call, SparseSrc{d_packed, packed_bytes, nullptr}, pk));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const RsRange *d_ranges = nullptr;
  const RsRow *d_big = nullptr, *d_small = nullptr;
  B3W_TRY(range_table<RsRow>(ctx, host_lens, n_files, group_log, host_files, host_first, host_count, n_ranges, rows, st, d_ranges, d_big, d_small,
                             [&](uint32_t i, uint32_t f) {
                               uint64_t first, count;
                               b3w_int_packed_range(host_lens[f], group_log, host_first[i], host_count[i], &first, &count);
                               return 1024 * pk.slot_of(f, first);
                             },
                             [](uint32_t i, uint64_t blk, uint64_t) { return RsRow{i, (uint32_t)blk}; }));
  if (rows.big) hipLaunchKernelGGL(b3w_bao_range_slice_packed_kernel<(int)B3W_TILE>, dim3((uint32_t)rows.big), dim3(B3W_TILE), 0, st, d_ranges, d_big, group_log, d_packed, d_outboards, d_slices);
  if (rows.small) hipLaunchKernelGGL(b3w_bao_range_slice_packed_kernel<64>, dim3((uint32_t)rows.small), dim3(64), 0, st, d_ranges, d_small, group_log, d_packed, d_outboards, d_slices);
  return batch_launched(ctx, st, "bao range slice packed launch");
}

int32_t b3w_bao_range_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                          uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                          const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                          int32_t *d_range_status, uint64_t *d_range_first_bad, uint64_t *d_have, void *d_scratch, uint64_t scratch_bytes,
                                          void *stream) {
  return range_slice_ingest<false>(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_first, host_count,
                                   n_ranges, d_slices, d_range_status, d_range_first_bad, d_have, d_scratch, scratch_bytes, stream);
}

int32_t b3w_bao_range_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                                 uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                                 const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                                 int32_t *d_range_status, uint64_t *d_range_first_bad, uint64_t *d_have, void *d_scratch,
                                                 uint64_t scratch_bytes, void *stream) {
  return range_slice_ingest<true>(ctx, d_chunks, chunks_bytes, nullptr, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_first, host_count,
                                  n_ranges, d_slices, d_range_status, d_range_first_bad, d_have, d_scratch, scratch_bytes, stream);
}

// ---- step records of challenged chunk runs from range slices --------------------------------------------------------------------------
int32_t b3w_sample_plan_range_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots, const uint32_t *host_files,
                                            const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                            uint32_t *d_records, int32_t *d_chunk_status, int32_t *d_range_status, uint64_t *d_range_first_bad,
                                            void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "sample plan range slices";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  if (!n_ranges) return B3W_OK;
  if (!host_lens || !d_roots || !host_files || !host_first || !host_count || !d_slices || !d_records || !d_chunk_status || !d_range_status || !d_range_first_bad)
    return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_slices & 15) || ((uintptr_t)d_roots & 3)) return refuse(ctx, call, "d_slices is not 16-byte or d_roots not 4-byte aligned");
  if (((uintptr_t)d_records & 3) || ((uintptr_t)d_chunk_status & 3)) return refuse(ctx, call, "d_records or d_chunk_status is not 4-byte aligned");
  if (((uintptr_t)d_range_status & 3) || ((uintptr_t)d_range_first_bad & 7)) return refuse(ctx, call, "d_range_status is not 4-byte or d_range_first_bad not 8-byte aligned");
  RangeRows rows;
  B3W_TRY(range_list_ok(ctx, call, nullptr, 0, nullptr, host_lens, n_files, host_files, host_first, host_count, n_ranges, rows, 1ull << 30));
  if (scratch_bytes < (rows.big + rows.small) * 16) return refuse(ctx, call, "the scratch is smaller than b3w_bao_range_slice_ingest_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 15)) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const RsRange *d_ranges = nullptr;
  const RpRow *d_big = nullptr, *d_small = nullptr;
  // a range's `off` is its first chunk status; a row carries the first record row of its first chunk of the range (rows_before: O(depth))
  uint64_t next_row = 0, next_chunk = 0, range_row = 0;
  B3W_TRY(range_table<RpRow>(ctx, host_lens, n_files, 0, host_files, host_first, host_count, n_ranges, rows, st, d_ranges, d_big, d_small,
                             [&](uint32_t i, uint32_t f) {
                               const uint64_t len = host_lens[f], n = num_chunks(len), chunk0 = next_chunk;
                               range_row = next_row;
                               next_row += rows_before(len, n, host_first[i] + host_count[i]) - rows_before(len, n, host_first[i]);
                               next_chunk += host_count[i];
                               return chunk0;
                             },
                             [&](uint32_t i, uint64_t blk, uint64_t B) {
                               const uint64_t len = host_lens[host_files[i]], n = num_chunks(len), a = host_first[i], c0 = blk * B > a ? blk * B : a;
                               return RpRow{i, (uint32_t)blk, range_row + rows_before(len, n, c0) - rows_before(len, n, a)};
                             }));
  uint4 *res = reinterpret_cast<uint4 *>(d_scratch);
  if (rows.big)
    hipLaunchKernelGGL(b3w_sample_plan_range_kernel<(int)B3W_TILE>, dim3((uint32_t)rows.big), dim3(B3W_TILE), 0, st, d_ranges, d_big, d_slices, d_roots, d_records,
                       d_chunk_status, res);
  if (rows.small)
    hipLaunchKernelGGL(b3w_sample_plan_range_kernel<64>, dim3((uint32_t)rows.small), dim3(64), 0, st, d_ranges, d_small, d_slices, d_roots, d_records, d_chunk_status,
                       res + rows.big);
  hipLaunchKernelGGL(b3w_bao_range_reduce_kernel, dim3((n_ranges + 3) / 4), dim3(256), 0, st, d_ranges, n_ranges, res, d_range_status,
                     reinterpret_cast<unsigned long long *>(d_range_first_bad));
  return batch_launched(ctx, st, "sample plan range slices launch");
}

}  // extern "C"

// ---- set slices: one slice for the union S of a file's runs, extracted and taken in (still ABI 1.4: new names only) ----------------------
// The format and the places are b3wit.h's "set slices"; the arithmetic the host shares is b3w_bao_tree.h's.  The kernels are the range
// kernels' siblings: a ROW is (set, block of B aligned chunks with a wanted chunk), `mine` is the row's mask bit where the range kernels
// ask t in [lo, hi), and a node's place follows from the first wanted chunk at or behind its first lane.  The device never sees the runs:
//   lv[0]      the row's mask, 64 lanes a word
//   lv[l]      the mask OR-folded by 2^l: bit j says that S meets lanes [j << l, (j + 1) << l) - the `meets` of the node of that span
//   rel[t]     of a wanted lane: 64 (U_S(c) - U_S(cf)) + 1024 (the wanted lanes below t), cf the row's first wanted lane; the node of
//              level l over index j is a parent iff (j << l) + 2^(l-1) < m, so U_S(c) - U_S(cf) = the sum over l of the set bits of
//              lv[l] at the parents of index <= t >> l, less the nodes of cf's own path (full tile: popcount(L_l[0 .. c >> l]) - 1 a level)
//   lane_of[r] the r-th wanted lane: the byte movers walk the wanted chunks alone
// The table carries, a row, the place and rank of cf and the places of the nodes above the block (SET_UP of them at most); the row that
// holds the first wanted chunk below such a node finds its place equal to place(cf) - 64 (the nodes of cf's path at or below it).
namespace {

constexpr uint32_t SET_UP = 24;                           // nodes above a block of 64 chunks of a file of at most 2^30 chunks
struct SetDev { uint64_t len, off, ob, slice, have, chunk_first; uint32_t file, row0, n_rows, pad; };   // row0: its first row's result
template <int B>
struct SetRow { uint32_t set, block; uint64_t place0, rank0, up[SET_UP]; uint32_t mask[B / 32]; };
template <int B>
struct SetLds { unsigned long long lv[B == 64 ? 7 : 11][B / 64]; uint32_t rel[B]; uint16_t lane_of[B]; };
struct SetLanes { uint32_t cf, cnt, rank; bool mine; };   // the first wanted lane, their number; this lane's rank among them

__device__ __forceinline__ bool set_bit(const unsigned long long *w, uint32_t i) { return (w[i >> 6] >> (i & 63)) & 1ull; }
// the set bits of w at indices 0 .. idx
__device__ __forceinline__ uint32_t set_prefix(const unsigned long long *w, uint32_t idx) {
  uint32_t r = 0;
  for (uint32_t k = 0; k < (idx >> 6); ++k) r += (uint32_t)__popcll(w[k]);
  return r + (uint32_t)__popcll(w[idx >> 6] & ((2ull << (idx & 63)) - 1));
}
// the first set bit at or behind i0 (the caller knows there is one below the words' end)
template <int B>
__device__ __forceinline__ uint32_t set_first_at(const unsigned long long *w, uint32_t i0) {
  uint32_t k = i0 >> 6;
  unsigned long long x = w[k] & (~0ull << (i0 & 63));
  while (!x && k + 1 < B / 64) x = w[++k];
  return x ? k * 64 + (uint32_t)__ffsll((long long)x) - 1 : B - 1;
}

// the row's masks, rel[] and lane_of[] into LDS (ends with a barrier); m: the block's chunks
template <int B>
__device__ __forceinline__ SetLanes set_lanes(const SetRow<B> *__restrict__ row, uint32_t m, uint32_t t, SetLds<B> &s) {
  constexpr uint32_t LOG = B == 64 ? 6 : 10;
  if (t < B / 64) s.lv[0][t] = (unsigned long long)row->mask[2 * t] | ((unsigned long long)row->mask[2 * t + 1] << 32);
  lds_barrier();
#pragma unroll
  for (uint32_t l = 1; l <= LOG; ++l) {
    bool bit = false;
    if (t < (B >> l)) {
      if (l <= 6) {
        const unsigned long long word = s.lv[0][(t << l) >> 6] >> ((t << l) & 63);
        bit = (l == 6 ? word : word & ((1ull << (1u << l)) - 1)) != 0;
      } else {
        for (uint32_t k = 0; k < (1u << (l - 6)); ++k) bit |= s.lv[0][(t << (l - 6)) + k] != 0;
      }
    }
    const unsigned long long b = __ballot(bit);
    if ((t & 63) == 0 && t < (B >> l)) s.lv[l][t >> 6] = b;
  }
  lds_barrier();
  SetLanes w;
  w.cf = set_first_at<B>(s.lv[0], 0);
  w.cnt = set_prefix(s.lv[0], B - 1);
  w.mine = set_bit(s.lv[0], t);
  w.rank = 0;
  if (w.mine) {
    w.rank = set_prefix(s.lv[0], t) - 1;
    uint32_t u = 0;
#pragma unroll
    for (uint32_t l = 1; l <= LOG; ++l) {
      const uint32_t half = 1u << (l - 1);
      if (m <= half) break;
      const uint32_t parents = (m - half + (1u << l) - 1) >> l, idx = t >> l;
      u += set_prefix(s.lv[l], idx < parents ? idx : parents - 1);
    }
    s.rel[t] = 64 * (u - depth_in(w.cf, m)) + 1024 * w.rank;
    s.lane_of[w.rank] = (uint16_t)t;
  }
  lds_barrier();
  return w;
}
// the node over the block's lanes [i0, i0 + size), which meets S: its place in the slice behind the row's place0
template <int B>
__device__ __forceinline__ uint64_t set_block_node_at(const SetRow<B> *__restrict__ row, const SetLds<B> &s, uint32_t i0, uint32_t size) {
  const uint32_t c0 = set_first_at<B>(s.lv[0], i0);
  return row->place0 + s.rel[c0] - 64ull * depth_in(c0 - i0, size);
}

// PACKED (b3w_bao_set_slice_packed_device): slot[row] is the slot of the block's first LISTED chunk in the packed buffer, and the
// block's listed lanes follow it slot by slot.  Listed are all lanes of a file of at most 64 chunks, else the lanes of the groups
// the set touches (lv[gl]; at gl 0 the mask itself): a lane reads at its rank among them and keeps c = a0 + t for counter and length.
template <int B>
__device__ __forceinline__ uint32_t set_listed_rank(const SetLds<B> &s, uint32_t gl, bool all, uint32_t t) {
  return all ? t : ((set_prefix(s.lv[gl], t >> gl) - 1) << gl) + (t & ((1u << gl) - 1));
}

// THE PROVIDER (range_slice_body with the mask for the interval)
template <int B>
__global__ __launch_bounds__(B) void b3w_bao_set_slice_kernel(const SetDev *__restrict__ sets, const SetRow<B> *__restrict__ rows, uint32_t gl,
                                                              const uint8_t *__restrict__ arena, const uint8_t *__restrict__ obs,
                                                              uint8_t *__restrict__ slices) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ SetLds<B> s;
  const SetRow<B> *__restrict__ row = rows + blockIdx.x;
  const SetDev r = sets[row->set];
  const uint32_t t = threadIdx.x;
  const uint64_t n = r.len ? (r.len + 1023) / 1024 : 1, a0 = (uint64_t)row->block * B;
  const uint32_t m = (uint32_t)(n - a0 < B ? n - a0 : B);
  const bool sole = n <= B;
  const uint8_t *__restrict__ data = arena + r.off, *__restrict__ ob = obs + r.ob;
  uint8_t *__restrict__ sl = slices + r.slice;
  const SetLanes w = set_lanes<B>(row, m, t, s);
  // group outboards: the chunks of the touched groups, hashed (no byte behind the file's last one is read)
  if (gl != 0 && t < m && set_bit(s.lv[gl], t >> gl)) lane_chunk_cv(cv, data, a0 + t, r.len, n, a0 + t, true);
  for (uint32_t l = 0; (1u << l) < m; ++l) {
    if (l <= gl) lds_barrier();                            // (the level below inside a group; above the groups nothing is handed on)
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= m) continue;
    const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
    const bool meets = set_bit(s.lv[l + 1], t);
    uint8_t *place = meets ? sl + set_block_node_at<B>(row, s, i0, size) : nullptr;
    if (l < gl) {                                          // inside a group: computed, and stored where the set wants it
      if (set_bit(s.lv[gl], i0 >> gl)) merge_pair<true>(cv, i0, i1, place, 4u | (sole && (2u << l) >= m ? 8u : 0u));
    } else if (meets) {
      copy_node(place, ob + 8 + node_pos<true>(n, a0 + i0, size, gl) * 64);
    }
  }
  // the nodes above the block whose first wanted chunk lies in it, and the header in front of min S
  const RsAbove up = range_above(n, a0, m, t);
  const uint64_t own = row->place0 - 64ull * (up.depth + depth_in(w.cf, m));     // the place of the root, if this row holds min S
  if (t < up.depth && row->up[t] == own + 64ull * t) copy_node(sl + row->up[t], ob + 8 + node_pos<true>(n, up.lo, up.cnt, gl) * 64);
  if (t == 0 && own == 8) *reinterpret_cast<uint2 *>(sl) = *reinterpret_cast<const uint2 *>(ob);
  for (uint32_t p = t; p < w.cnt * 64; p += B) {
    const uint32_t ch = s.lane_of[p >> 6], q = (p & 63) * 16;
    const uint64_t c = a0 + ch;
    const uint32_t bytes = range_chunk_bytes(r.len, c);
    uint8_t *dst = sl + row->place0 + s.rel[ch];
    const uint8_t *src = data + c * 1024;
    if (q + 16 <= bytes) move16<true>(dst + q, src + q);
    else for (uint32_t o = q; o < bytes; ++o) dst[o] = src[o];
  }
}

// THE PROVIDER FROM PACKED BYTES: b3w_bao_set_slice_kernel with the chunks read at their slots.  A kernel of its own: as two
// instantiations of one body the arena kernel did not keep its ISA text (two operand pairs swapped), and its text is the yardstick.
template <int B>
__global__ __launch_bounds__(B) void b3w_bao_set_slice_packed_kernel(const SetDev *__restrict__ sets, const SetRow<B> *__restrict__ rows,
                                                                     const uint64_t *__restrict__ slot, uint32_t gl, const uint8_t *__restrict__ packed,
                                                                     const uint8_t *__restrict__ obs, uint8_t *__restrict__ slices) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ SetLds<B> s;
  const SetRow<B> *__restrict__ row = rows + blockIdx.x;
  const SetDev r = sets[row->set];
  const uint32_t t = threadIdx.x;
  const uint64_t n = r.len ? (r.len + 1023) / 1024 : 1, a0 = (uint64_t)row->block * B;
  const uint32_t m = (uint32_t)(n - a0 < B ? n - a0 : B);
  const bool sole = n <= B, all = n <= 64;
  const uint8_t *__restrict__ data = packed + 1024 * slot[blockIdx.x], *__restrict__ ob = obs + r.ob;
  uint8_t *__restrict__ sl = slices + r.slice;
  const SetLanes w = set_lanes<B>(row, m, t, s);
  // group outboards: the chunks of the touched groups, hashed (no byte behind the file's last one is read)
  if (gl != 0 && t < m && set_bit(s.lv[gl], t >> gl)) lane_chunk_cv(cv, data, set_listed_rank<B>(s, gl, all, t), r.len, n, a0 + t, true);
  for (uint32_t l = 0; (1u << l) < m; ++l) {
    if (l <= gl) lds_barrier();                            // (the level below inside a group; above the groups nothing is handed on)
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= m) continue;
    const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
    const bool meets = set_bit(s.lv[l + 1], t);
    uint8_t *place = meets ? sl + set_block_node_at<B>(row, s, i0, size) : nullptr;
    if (l < gl) {                                          // inside a group: computed, and stored where the set wants it
      if (set_bit(s.lv[gl], i0 >> gl)) merge_pair<true>(cv, i0, i1, place, 4u | (sole && (2u << l) >= m ? 8u : 0u));
    } else if (meets) {
      copy_node(place, ob + 8 + node_pos<true>(n, a0 + i0, size, gl) * 64);
    }
  }
  // the nodes above the block whose first wanted chunk lies in it, and the header in front of min S
  const RsAbove up = range_above(n, a0, m, t);
  const uint64_t own = row->place0 - 64ull * (up.depth + depth_in(w.cf, m));     // the place of the root, if this row holds min S
  if (t < up.depth && row->up[t] == own + 64ull * t) copy_node(sl + row->up[t], ob + 8 + node_pos<true>(n, up.lo, up.cnt, gl) * 64);
  if (t == 0 && own == 8) *reinterpret_cast<uint2 *>(sl) = *reinterpret_cast<const uint2 *>(ob);
  for (uint32_t p = t; p < w.cnt * 64; p += B) {
    const uint32_t ch = s.lane_of[p >> 6], q = (p & 63) * 16;
    const uint32_t bytes = range_chunk_bytes(r.len, a0 + ch);
    uint8_t *dst = sl + row->place0 + s.rel[ch];
    const uint8_t *src = data + set_listed_rank<B>(s, gl, all, ch) * 1024;
    if (q + 16 <= bytes) move16<true>(dst + q, src + q);
    else for (uint32_t o = q; o < bytes; ++o) dst[o] = src[o];
  }
}

// THE RECEIVER (b3w_bao_range_ingest_kernel with the mask for the interval, and a status a wanted chunk)
// PACKED (b3w_bao_set_slice_ingest_packed_device): `arena` is a slot buffer, 1 024 bytes a wanted chunk in the order of chunk_status:
// the copy loop's lane group p >> 6 is the wanted lane's rank in the row, so its slot is r.chunk_first + row->rank0 + (p >> 6); `obs`
// may be null: no node and no header is stored (decode).
// STREAM (b3w_bao_set_slice_stream_push): `slices` is a WINDOW of the set's slice that starts at slice offset r.slice, a cut, so the
// row's places keep their values and every chunk and block node is read where the one-shot kernel reads it.  The only places in front of
// the cut are the header (r.pad says so) and nodes above the block: the host marks those up[] entries SET_CARRIED | the node's offset in
// `carry`, the session's carried area - one select a node load, none a chunk byte.  Nothing carried is trusted: it is hashed as a slice
// node is.
constexpr uint64_t SET_CARRIED = 1ull << 63;
template <bool STREAM>
__device__ __forceinline__ const uint8_t *set_up_at(const uint8_t *__restrict__ sl, const uint8_t *__restrict__ carry, uint64_t up) {
  if constexpr (STREAM) return (up & SET_CARRIED) ? carry + (up & ~SET_CARRIED) : sl + up;
  else return sl + up;
}
template <int B, bool PACKED = false, bool STREAM = false>
__global__ __launch_bounds__(B) void b3w_bao_set_ingest_kernel(const SetDev *__restrict__ sets, const SetRow<B> *__restrict__ rows, uint32_t gl,
                                                               const uint8_t *__restrict__ slices, const uint32_t *__restrict__ roots,
                                                               uint8_t *__restrict__ arena, uint8_t *__restrict__ obs, int32_t *__restrict__ chunk_status,
                                                               unsigned long long *__restrict__ have, uint4 *__restrict__ results,
                                                               const uint8_t *__restrict__ carry = nullptr) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ uint32_t flags[B], listed[B];
  __shared__ SetLds<B> s;
  __shared__ uint32_t worst, first, above;
  const SetRow<B> *__restrict__ row = rows + blockIdx.x;
  const SetDev r = sets[row->set];
  const uint32_t t = threadIdx.x;
  const uint64_t n = r.len ? (r.len + 1023) / 1024 : 1, a0 = (uint64_t)row->block * B;
  const uint32_t m = (uint32_t)(n - a0 < B ? n - a0 : B);
  const bool sole = n <= B;
  const uint8_t *__restrict__ sl = STREAM ? slices - r.slice : slices + r.slice;
  const uint32_t *__restrict__ root = roots + (uint64_t)r.file * 8;
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; above = 0; }
  const SetLanes w = set_lanes<B>(row, m, t, s);
  const bool mine = w.mine;
  listed[t] = mine ? 1u : 0u;
  // 1. the verdicts: the wanted chunks, the block's nodes bottom up, the nodes above the block side by side
  if (mine) {
    const uint64_t c = a0 + t;
    uint32_t h[8];
    chunk_cv(sl + row->place0 + s.rel[t], range_chunk_bytes(r.len, c), c, n == 1 ? 8u : 0u, h);   // (16-byte aligned)
    put_cv(cv, t, h);
  }
  const RsAbove up = range_above(n, a0, m, t);
  if (t < up.depth) {
    uint32_t mw[16], ivv[8], o[8];
    load_node(set_up_at<STREAM>(sl, carry, row->up[t]), mw);
    iv(ivv);
    blake3_cv(ivv, mw, 0, 0, 64, 4u | (t == 0 ? 8u : 0u), o);
    const uint32_t *want = t == 0 ? root : reinterpret_cast<const uint32_t *>(set_up_at<STREAM>(sl, carry, row->up[t - 1]) + (up.left ? 0 : 32));
    if (!eq8(o, want)) atomicOr(&above, 1u);
  }
  for (uint32_t l = 0; (1u << l) < m; ++l) {
    lds_barrier();
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= m) continue;
    const bool d0 = listed[i0] != 0, d1 = listed[i1] != 0;
    if (!d0 && !d1) continue;
    const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
    ranges_pair<true>(cv, flags, nullptr, i0, i1, d0, d1, l, sl + set_block_node_at<B>(row, s, i0, size), 4u | (sole && (2u << l) >= m ? 8u : 0u), 1ull << l,
                      size - (1u << l), 1, nullptr);
    listed[i0] = 1;
  }
  lds_barrier();
  if (t == 0) {                                            // slot 0: what the block's stored root node hashes to, or the CV of a block of one chunk
    const uint32_t *want = up.depth ? reinterpret_cast<const uint32_t *>(set_up_at<STREAM>(sl, carry, row->up[up.depth - 1]) + (up.last_left ? 0 : 32)) : root;
    if (!eq8(cv, want)) flags[0] |= m == 1 ? VER_UNIT : VER_TOP;
  }
  lds_barrier();
  const uint2 hd = *reinterpret_cast<const uint2 *>(STREAM && r.pad ? carry : sl);
  const bool hdr = ((uint64_t)hd.x | ((uint64_t)hd.y << 32)) != r.len;
  uint32_t st = 0;
  if (mine) {
    st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t); }          // (LDS; a clean row issues none)
    if (chunk_status) chunk_status[r.chunk_first + row->rank0 + w.rank] = (int32_t)st;
  }
  const bool ok = mine && st == 0;
  __syncthreads();
  listed[t] = ok ? 1u : 0u;                                // from here on: a verified chunk (below this slot)
  __syncthreads();
  if (t == 0) results[blockIdx.x] = make_uint4(worst, 0, first == ~0u ? ~0u : (uint32_t)(a0 + first), first == ~0u ? ~0u : (uint32_t)((a0 + first) >> 32));
  // 2. the places: nothing unverified is written
  uint8_t *__restrict__ data = arena + r.off, *__restrict__ ob = obs + r.ob;
  for (uint32_t p = t; p < w.cnt * 64; p += B) {
    const uint32_t ch = s.lane_of[p >> 6], q = (p & 63) * 16;
    if (!listed[ch]) continue;
    const uint64_t c = a0 + ch;
    const uint32_t bytes = range_chunk_bytes(r.len, c);
    const uint8_t *src = sl + row->place0 + s.rel[ch];
    uint8_t *dst;
    if constexpr (PACKED) dst = arena + (r.chunk_first + row->rank0 + (p >> 6)) * 1024; else dst = data + c * 1024;
    if (q + 16 <= bytes) put16(dst + q, src + q);
    else for (uint32_t o = q; o < bytes; ++o) dst[o] = src[o];
  }
  if (!PACKED || obs) {
    for (uint32_t l = 0; (1u << l) < m; ++l) {               // the stored nodes with a verified chunk below them
      lds_barrier();
      const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
      if (i1 >= m || !(listed[i0] | listed[i1])) continue;
      const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
      uint8_t *node = node_at<true>(ob + 8, n, a0 + i0, size, gl);
      if (node) copy_node(node, sl + set_block_node_at<B>(row, s, i0, size));
      listed[i0] = 1;
    }
    lds_barrier();
    if (listed[0]) {                                         // (every row with a verified chunk stores the nodes above it: the same verified bytes)
      if (t < up.depth) {
        uint8_t *node = node_at<true>(ob + 8, n, up.lo, up.cnt, gl);
        if (node) copy_node(node, set_up_at<STREAM>(sl, carry, row->up[t]));
      }
      if (t == 0) *reinterpret_cast<uint2 *>(ob) = hd;       // the header (it is the length: just checked)
    }
  }
  if (have) {                                              // a wave's lanes are the chunks of one word (a block starts at a multiple of 64)
    const unsigned long long mask = __ballot(ok);
    if ((t & 63) == 0 && mask) atomicOr(have + r.have + ((a0 + t) >> 6), mask);
  }
}

// a wave per set: b3w_bao_range_reduce_kernel's body over the set's rows
__global__ __launch_bounds__(256) void b3w_bao_set_reduce_kernel(const SetDev *__restrict__ sets, uint32_t n_sets, const uint4 *__restrict__ results,
                                                                 int32_t *__restrict__ set_status, unsigned long long *__restrict__ set_first_bad) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n_sets) return;
  const uint32_t n_rows = sets[i].n_rows;
  const uint4 *__restrict__ res = results + sets[i].row0;
  uint32_t w = 0;
  unsigned long long f = ~0ull;
  for (uint32_t j = lane; j < n_rows; j += 64) {
    const uint4 v = res[j];
    const unsigned long long at = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    w = w > v.x ? w : v.x;
    f = f < at ? f : at;
  }
#pragma unroll
  for (int d = 32; d >= 1; d /= 2) {
    const uint32_t ow = __shfl_xor(w, d);
    const unsigned long long of = __shfl_xor(f, d);
    w = w > ow ? w : ow;
    f = f < of ? f : of;
  }
  if (lane == 0) { set_status[i] = (int32_t)w; set_first_bad[i] = f; }
}

// the tail of a streamed push, one workgroup: wave 0 folds the window's rows' results INTO the set's two outputs (the largest status,
// the least first bad chunk; the pushes of a session are ordered, so a plain read and write), waves 1 .. 2 move what later windows
// need into the carried area - behind the window's rows, which read it: the node at src[t] of the window to depth slot t (16 bytes a
// lane), and the header if the window holds it.  Vector loads and stores only.
struct SetStreamFold { uint64_t src[SET_UP]; uint32_t n_rows, header; };   // src[t]: the node's offset in the window, ~0: keep what is carried
__global__ __launch_bounds__(256) void b3w_bao_set_stream_fold_kernel(const SetStreamFold f, const uint8_t *__restrict__ window,
                                                                      const uint4 *__restrict__ results, int32_t *__restrict__ set_status,
                                                                      unsigned long long *__restrict__ set_first_bad, uint8_t *__restrict__ carry) {
  const uint32_t t = threadIdx.x;
  if (t < 64) {
    uint32_t w = 0;
    unsigned long long fb = ~0ull;
    for (uint32_t j = t; j < f.n_rows; j += 64) {
      const uint4 v = results[j];
      const unsigned long long at = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
      w = w > v.x ? w : v.x;
      fb = fb < at ? fb : at;
    }
#pragma unroll
    for (int d = 32; d >= 1; d /= 2) {
      const uint32_t ow = __shfl_xor(w, d);
      const unsigned long long of = __shfl_xor(fb, d);
      w = w > ow ? w : ow;
      fb = fb < of ? fb : of;
    }
    if (t == 0) {
      const int32_t was = *set_status;
      const unsigned long long first = *set_first_bad;
      if ((int32_t)w > was) *set_status = (int32_t)w;
      if (fb < first) *set_first_bad = fb;
    }
  } else if (t < 64 + SET_UP * 4) {
    const uint32_t q = t - 64, depth = q >> 2, part = q & 3;
    const uint64_t src = f.src[depth];
    if (src != ~0ull) reinterpret_cast<uint4 *>(carry + 16)[q] = *reinterpret_cast<const uint4 *>(window + src + 16 * part);
  } else if (t == 64 + SET_UP * 4 && f.header) {
    *reinterpret_cast<uint2 *>(carry) = *reinterpret_cast<const uint2 *>(window);
  }
}

// THE PLANNER (b3w_sample_plan_range_kernel on the set receiver's rows): b3w_sample_plan_slices_kernel's records and statuses for the
// projection of the set slice onto every wanted chunk.  The range planner's steps with the mask for the interval:
//   0. where a lane's rows start: the row's base (row_base[], 8 bytes a row beside the table: the host's closed form over the set's runs,
//      b3w_int_set_row_base) plus the prefix sum over the WANTED lanes of blocks + path nodes
//   1. plan_leaf_chunk on the chunk where it lies in the slice (place0 + rel[t]): the leaf records in place, the chunk's CV to LDS
//   2. - 4. the set receiver's verdicts as they stand; the chunk's status at chunk_first + rank0 + rank, the row's result to the scratch
//   5. the parent records bottom up: the block's nodes at set_block_node_at, the nodes above it at row->up[]
// Every row of 128 bytes is written by the lane that owns the chunk.
template <int B>
__global__ __launch_bounds__(B) void b3w_sample_plan_set_kernel(const SetDev *__restrict__ sets, const SetRow<B> *__restrict__ rows,
                                                                const uint64_t *__restrict__ row_base, const uint8_t *__restrict__ slices,
                                                                const uint32_t *__restrict__ roots, uint32_t *__restrict__ recs,
                                                                int32_t *__restrict__ chunk_status, uint4 *__restrict__ results) {
  __shared__ __attribute__((aligned(16))) uint32_t cv[B * 8];
  __shared__ uint32_t flags[B], listed[B];
  __shared__ SetLds<B> s;
  __shared__ uint32_t wave_rows[B / 64], worst, first, above;
  const SetRow<B> *__restrict__ row = rows + blockIdx.x;
  const SetDev r = sets[row->set];
  const uint32_t t = threadIdx.x;
  const uint64_t n = r.len ? (r.len + 1023) / 1024 : 1, a0 = (uint64_t)row->block * B, c = a0 + t;
  const uint32_t m = (uint32_t)(n - a0 < B ? n - a0 : B);
  const bool sole = n <= B;
  const uint8_t *__restrict__ sl = slices + r.slice;
  const uint32_t *__restrict__ root = roots + (uint64_t)r.file * 8;
  flags[t] = 0;
  if (t == 0) { worst = 0; first = ~0u; above = 0; }
  const SetLanes w = set_lanes<B>(row, m, t, s);
  const bool mine = w.mine;
  listed[t] = mine ? 1u : 0u;
  const uint32_t P = mine ? depth_in(c, n) : 0, bytes = mine ? range_chunk_bytes(r.len, c) : 0, n_blocks = bytes ? (bytes + 63) / 64 : 1;
  // 0. the lane's first row
  const uint32_t own = mine ? n_blocks + P : 0;
  uint32_t upto = own;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const uint32_t o = __shfl_up(upto, d);
    if ((t & 63) >= (uint32_t)d) upto += o;
  }
  if ((t & 63) == 63) wave_rows[t >> 6] = upto;
  __syncthreads();
  uint32_t ahead = upto - own;
  for (uint32_t wv = 0; wv < (t >> 6); ++wv) ahead += wave_rows[wv];
  uint32_t *__restrict__ rec = recs + (row_base[blockIdx.x] + ahead) * 32;
  // 1. the leaf records and the chunks' CVs
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mine) {
    plan_leaf_chunk(sl + row->place0 + s.rel[t], bytes, c, P, rec, h);   // (16-byte aligned; P == 0: the ROOT-flagged output)
    put_cv(cv, t, h);
  }
  // 2. - 4. the verdicts, as the set receiver reaches them
  const RsAbove up = range_above(n, a0, m, t);
  if (t < up.depth) {
    uint32_t mw[16], ivv[8], o[8];
    load_node(sl + row->up[t], mw);
    iv(ivv);
    blake3_cv(ivv, mw, 0, 0, 64, 4u | (t == 0 ? 8u : 0u), o);
    const uint32_t *want = t == 0 ? root : reinterpret_cast<const uint32_t *>(sl + row->up[t - 1] + (up.left ? 0 : 32));
    if (!eq8(o, want)) atomicOr(&above, 1u);
  }
  for (uint32_t l = 0; (1u << l) < m; ++l) {
    lds_barrier();
    const uint32_t i0 = (2 * t) << l, i1 = i0 + (1u << l);
    if (i1 >= m) continue;
    const bool d0 = listed[i0] != 0, d1 = listed[i1] != 0;
    if (!d0 && !d1) continue;
    const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
    ranges_pair<true>(cv, flags, nullptr, i0, i1, d0, d1, l, sl + set_block_node_at<B>(row, s, i0, size), 4u | (sole && (2u << l) >= m ? 8u : 0u), 1ull << l,
                      size - (1u << l), 1, nullptr);
    listed[i0] = 1;
  }
  lds_barrier();
  if (t == 0) {
    const uint32_t *want = up.depth ? reinterpret_cast<const uint32_t *>(sl + row->up[up.depth - 1] + (up.last_left ? 0 : 32)) : root;
    if (!eq8(cv, want)) flags[0] |= m == 1 ? VER_UNIT : VER_TOP;
  }
  lds_barrier();
  const uint2 hd = *reinterpret_cast<const uint2 *>(sl);
  const bool hdr = ((uint64_t)hd.x | ((uint64_t)hd.y << 32)) != r.len;
  uint32_t st = 0;
  if (mine) {
    st = hdr ? 3u : above || path_bad(flags, t) ? 2u : (flags[t] & VER_UNIT) ? 1u : 0u;
    chunk_status[r.chunk_first + row->rank0 + w.rank] = (int32_t)st;
    if (st) { atomicMax(&worst, st); atomicMin(&first, t); }
  }
  __syncthreads();
  if (t == 0) results[blockIdx.x] = make_uint4(worst, 0, first == ~0u ? ~0u : (uint32_t)(a0 + first), first == ~0u ? ~0u : (uint32_t)((a0 + first) >> 32));
  if (!mine) return;
  // 5. the parent records: the block's nodes on the lane's path bottom up, then the nodes above the block
  const bool chain = st != 0 || !path_provable(c, n);
  uint32_t g = 0;
  rec += (uint64_t)n_blocks * 32;
  const auto step = [&](uint64_t at) {
    uint32_t mw[16], on[8], sib[8];
    load_node(sl + at, mw);
    const bool bit_left = ((c >> g) & 1) == 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { on[k] = bit_left ? mw[k] : mw[8 + k]; sib[k] = bit_left ? mw[8 + k] : mw[k]; }
    if (chain) plan_parent_step(rec, h, sib, bit_left, c, n_blocks, P, P - 1 - g);
    else {
      if (g) {                                             // (every node hashed to its half of the node above: h at height g is that half)
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = on[k];
      }
      parent_record(rec, h, sib, c, n_blocks, P, P - 1 - g);
    }
    rec += 32; ++g;
  };
  for (uint32_t l = 0; (1u << l) < m; ++l) {
    const uint32_t i0 = (t >> (l + 1)) << (l + 1), i1 = i0 + (1u << l);
    if (i1 >= m) continue;
    const uint32_t end = i0 + (2u << l), size = (end < m ? end : m) - i0;
    step(set_block_node_at<B>(row, s, i0, size));
  }
  for (uint32_t j = up.depth; j-- > 0;) step(row->up[j]);
}

// what the set calls refuse about the list and the arena (null host_offsets: the arena is not looked at); the sets, their rows and the
// slices' places
int32_t set_list_ok(b3w_ctx *ctx, const char *what, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                    uint32_t n_files, const uint32_t *host_files, const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, SetList &list) {
  if (!b3w_int_set_list(host_lens, n_files, host_files, host_first, host_count, n_ranges, list)) return refuse(ctx, what, list.why);
  for (const SetEnt &e : list.sets) {
    const uint64_t len = host_lens[e.file], off = host_offsets ? host_offsets[e.file] : 0;
    const char *why = nullptr;
    if (num_chunks(len) > (1ull << 30)) why = "its file has more than 2^30 chunks";
    else if (!host_offsets) why = nullptr;
    else if (len && !d_arena) why = "a null arena with a file that is not empty";
    else if (off > arena_bytes || len > arena_bytes - off) why = "its file reaches past arena_bytes";
    if (why) return refuse(ctx, what, "range " + std::to_string(e.range_first) + ": " + why);
  }
  if (list.big > 0x7fffffffull || list.small > 0x7fffffffull) return refuse(ctx, what, "more than 2^31 - 1 rows of one kind");
  return B3W_OK;
}

// one row of the table: its block's mask from the runs [i0, i1) of the set that touch it, the place and rank of its first wanted chunk,
// the places of the nodes above the block.  ufirst[] / rank[]: SetRuns' state at every run of the set
template <int B>
bool set_make_row(SetRow<B> &row, uint32_t set, uint64_t blk, uint64_t len, const uint64_t *first, const uint64_t *count, uint64_t k,
                  const uint64_t *ufirst, const uint64_t *rank) {
  const uint64_t n = num_chunks(len), a0 = blk * B, m = n - a0 < B ? n - a0 : B;
  memset(&row, 0, sizeof row);
  row.set = set; row.block = (uint32_t)blk;
  auto place = [&](uint64_t i, uint64_t c) { return 8 + 64 * set_nodes(n, ufirst[i], first[i], c) + 1024 * (rank[i] + (c - first[i])); };
  uint64_t i = set_run_behind(first, count, k, a0);       // the first run that reaches into the block
  const uint64_t cf = first[i] > a0 ? first[i] : a0;
  row.place0 = place(i, cf);
  row.rank0 = rank[i] + (cf - first[i]);
  for (; i < k && first[i] < a0 + m; ++i) {
    const uint64_t lo = (first[i] > a0 ? first[i] : a0) - a0, hi = (first[i] + count[i] < a0 + m ? first[i] + count[i] : a0 + m) - a0;
    for (uint64_t wd = lo >> 5; wd <= (hi - 1) >> 5; ++wd) {
      const uint32_t from = wd == lo >> 5 ? (uint32_t)lo & 31 : 0, to = wd == (hi - 1) >> 5 ? (uint32_t)((hi - 1) & 31) + 1 : 32;
      row.mask[wd] |= (to == 32 ? ~0u : (1u << to) - 1) & ~((1u << from) - 1);
    }
  }
  uint64_t lo = 0, cnt = n;
  for (uint32_t j = 0; cnt > 1 && !(lo == a0 && cnt == m); ++j) {
    if (j == SET_UP) return false;                         // (never with at most 2^30 chunks: the kernels read up[] as far as the block lies deep)
    const uint64_t r = set_run_behind(first, count, k, lo), c0 = first[r] > lo ? first[r] : lo;
    row.up[j] = place(r, c0) - 64ull * depth_in(c0 - lo, cnt);
    const uint64_t half = left_of(cnt);
    if (a0 < lo + half) cnt = half; else { lo += half; cnt -= half; }
  }
  return true;
}

// the table into the staging and on its way: the sets' entries, the rows of 1 024 chunks, the rows of 64 and, where the call has one
// (AUX), a 64-bit value a row in the rows' order behind them: d_aux for the tile rows, d_aux + list.big for the rows of 64.  The call
// says what a set's `off` is (off_of(file)) and what a row carries beside the table (aux_of(set, block, B)).
template <bool AUX, class Off, class Aux>
int32_t set_table(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint64_t *host_first, const uint64_t *host_count,
                  const SetList &list, hipStream_t st, const SetDev *&d_sets, const SetRow<(int)B3W_TILE> *&d_big, const SetRow<64> *&d_small,
                  const uint64_t *&d_aux, Off off_of, Aux aux_of) {
  using Big = SetRow<(int)B3W_TILE>;
  using Small = SetRow<64>;
  const uint64_t n_sets = list.sets.size();
  const uint64_t up_bytes = n_sets * sizeof(SetDev) + list.big * sizeof(Big) + list.small * sizeof(Small) + (AUX ? (list.big + list.small) * 8 : 0);
  B3W_TRY(batch_staging(ctx, up_bytes + 2 * ((uint64_t)n_files + 1) * 8));
  SetDev *sd = reinterpret_cast<SetDev *>(ctx->h_batch);
  Big *big = reinterpret_cast<Big *>(sd + n_sets);
  Small *small = reinterpret_cast<Small *>(big + list.big);
  uint64_t *aux = reinterpret_cast<uint64_t *>(small + list.small);
  uint64_t *ob_first = aux + (AUX ? list.big + list.small : 0), *word_first = ob_first + n_files + 1;
  (void)b3w_bao_group_batch_layout(host_lens, n_files, group_log, ob_first);
  (void)b3w_bao_have_layout(host_lens, n_files, word_first);
  uint64_t nb = 0, ns = 0;
  for (uint64_t s = 0; s < n_sets; ++s) {
    const SetEnt &e = list.sets[s];
    const uint64_t len = host_lens[e.file], k = e.range_end - e.range_first;
    const uint64_t *first = host_first + e.range_first, *count = host_count + e.range_first;
    sd[s] = SetDev{len, off_of(e.file), ob_first[e.file], e.slice, word_first[e.file], e.chunk_first, e.file,
                   (uint32_t)(e.shrt ? list.big + ns : nb), (uint32_t)e.rows, 0};
    const uint64_t *ufirst = list.ufirst.data() + e.range_first, *rank = list.rank.data() + e.range_first;
    const uint64_t B = e.shrt ? 64 : B3W_TILE;
    uint64_t last = ~0ull, made = 0;
    for (uint64_t i = 0; i < k; ++i)
      for (uint64_t blk = first[i] / B; blk <= (first[i] + count[i] - 1) / B; ++blk) {
        if (blk == last) continue;
        last = blk;
        if (made++ == e.rows) return refuse(ctx, "bao set slice table", "the rows do not add up");   // (never: b3w_int_set_list counted them)
        if (AUX) aux[e.shrt ? list.big + ns : nb] = aux_of(s, blk, B);
        if (!(e.shrt ? set_make_row<64>(small[ns++], (uint32_t)s, blk, len, first, count, k, ufirst, rank)
                     : set_make_row<(int)B3W_TILE>(big[nb++], (uint32_t)s, blk, len, first, count, k, ufirst, rank)))
          return refuse(ctx, "bao set slice table", "a block lies deeper than the table's places");
      }
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)up_bytes, hipMemcpyHostToDevice, st));
  d_sets = reinterpret_cast<const SetDev *>(ctx->d_batch);
  d_big = reinterpret_cast<const Big *>(d_sets + n_sets);
  d_small = reinterpret_cast<const Small *>(d_big + list.big);
  d_aux = reinterpret_cast<const uint64_t *>(d_small + list.small);
  return B3W_OK;
}
// the arena provider's and the receiver's table: `off` is the file's place in the arena, nothing beside the rows
int32_t set_table(b3w_ctx *ctx, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, const uint64_t *host_first,
                  const uint64_t *host_count, const SetList &list, hipStream_t st, const SetDev *&d_sets, const SetRow<(int)B3W_TILE> *&d_big,
                  const SetRow<64> *&d_small) {
  const uint64_t *none = nullptr;
  return set_table<false>(ctx, host_lens, n_files, group_log, host_first, host_count, list, st, d_sets, d_big, d_small, none,
                          [&](uint32_t f) { return host_offsets ? host_offsets[f] : 0; }, [](uint64_t, uint64_t, uint64_t) { return 0ull; });
}

// b3w_bao_set_slice_ingest_device, and PACKED: b3w_bao_set_slice_ingest_packed_device - (d_arena, arena_bytes) its slot buffer, no
// offsets, d_outboards may be null; the table is the arena call's (a set's `off` 0): the kernel finds a slot from chunk_first and rank0
template <bool PACKED>
int32_t set_slice_ingest(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens, uint32_t n_files,
                         uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files, const uint64_t *host_first,
                         const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices, int32_t *d_set_status, uint64_t *d_set_first_bad,
                         int32_t *d_chunk_status, uint64_t *d_have, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = PACKED ? "bao set slice ingest packed" : "bao set slice ingest";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (((uintptr_t)d_have & 7) || ((uintptr_t)d_chunk_status & 3)) return refuse(ctx, call, "d_have is not 8-byte or d_chunk_status not 4-byte aligned");
  if (!n_ranges) return B3W_OK;
  if ((!PACKED && (!host_offsets || !d_outboards)) || !host_lens || !d_roots || !host_files || !host_first || !host_count || !d_slices || !d_set_status || !d_set_first_bad) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  if (((uintptr_t)d_set_status & 3) || ((uintptr_t)d_set_first_bad & 7)) return refuse(ctx, call, "d_set_status is not 4-byte or d_set_first_bad not 8-byte aligned");
  SetList list;
  B3W_TRY(set_list_ok(ctx, call, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_first, host_count, n_ranges, list));
  if (PACKED) B3W_TRY(slots_ok(ctx, call, d_arena, arena_bytes, list.chunks));
  if (scratch_bytes < (list.big + list.small) * 16) return refuse(ctx, call, "the scratch is smaller than b3w_bao_set_slice_ingest_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 15)) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const SetDev *d_sets = nullptr;
  const SetRow<(int)B3W_TILE> *d_big = nullptr;
  const SetRow<64> *d_small = nullptr;
  B3W_TRY(set_table(ctx, host_offsets, host_lens, n_files, group_log, host_first, host_count, list, st, d_sets, d_big, d_small));
  uint4 *res = reinterpret_cast<uint4 *>(d_scratch);
  unsigned long long *have = reinterpret_cast<unsigned long long *>(d_have);
  const uint32_t n_sets = (uint32_t)list.sets.size();
  if (list.big)
    hipLaunchKernelGGL((b3w_bao_set_ingest_kernel<(int)B3W_TILE, PACKED>), dim3((uint32_t)list.big), dim3(B3W_TILE), 0, st, d_sets, d_big, group_log, d_slices, d_roots, d_arena,
                       d_outboards, d_chunk_status, have, res);
  if (list.small)
    hipLaunchKernelGGL((b3w_bao_set_ingest_kernel<64, PACKED>), dim3((uint32_t)list.small), dim3(64), 0, st, d_sets, d_small, group_log, d_slices, d_roots, d_arena, d_outboards,
                       d_chunk_status, have, res + list.big);
  hipLaunchKernelGGL(b3w_bao_set_reduce_kernel, dim3((n_sets + 3) / 4), dim3(256), 0, st, d_sets, n_sets, res, d_set_status,
                     reinterpret_cast<unsigned long long *>(d_set_first_bad));
  return batch_launched(ctx, st, PACKED ? "bao set slice ingest packed launch" : "bao set slice ingest launch");
}

}  // namespace

extern "C" {

int32_t b3w_bao_set_slice_arena_device(b3w_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                       uint32_t n_files, uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files,
                                       const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices, void *stream) {
  const char *call = "bao set slice arena";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_offsets || !host_lens || !d_outboards || !host_files || !host_first || !host_count || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  SetList list;
  B3W_TRY(set_list_ok(ctx, call, d_arena, arena_bytes, host_offsets, host_lens, n_files, host_files, host_first, host_count, n_ranges, list));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const SetDev *d_sets = nullptr;
  const SetRow<(int)B3W_TILE> *d_big = nullptr;
  const SetRow<64> *d_small = nullptr;
  B3W_TRY(set_table(ctx, host_offsets, host_lens, n_files, group_log, host_first, host_count, list, st, d_sets, d_big, d_small));
  if (list.big) hipLaunchKernelGGL(b3w_bao_set_slice_kernel<(int)B3W_TILE>, dim3((uint32_t)list.big), dim3(B3W_TILE), 0, st, d_sets, d_big, group_log, d_arena, d_outboards, d_slices);
  if (list.small) hipLaunchKernelGGL(b3w_bao_set_slice_kernel<64>, dim3((uint32_t)list.small), dim3(64), 0, st, d_sets, d_small, group_log, d_arena, d_outboards, d_slices);
  return batch_launched(ctx, st, "bao set slice arena launch");
}

int32_t b3w_bao_set_slice_ingest_device(b3w_ctx *ctx, uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *host_offsets, const uint64_t *host_lens,
                                        uint32_t n_files, uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                        const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                        int32_t *d_set_status, uint64_t *d_set_first_bad, int32_t *d_chunk_status, uint64_t *d_have, void *d_scratch,
                                        uint64_t scratch_bytes, void *stream) {
  return set_slice_ingest<false>(ctx, d_arena, arena_bytes, host_offsets, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_first, host_count,
                                 n_ranges, d_slices, d_set_status, d_set_first_bad, d_chunk_status, d_have, d_scratch, scratch_bytes, stream);
}

int32_t b3w_bao_set_slice_ingest_packed_device(b3w_ctx *ctx, uint8_t *d_chunks, uint64_t chunks_bytes, const uint64_t *host_lens, uint32_t n_files,
                                               uint32_t group_log, uint8_t *d_outboards, const uint32_t *d_roots, const uint32_t *host_files,
                                               const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                               int32_t *d_set_status, uint64_t *d_set_first_bad, int32_t *d_chunk_status, uint64_t *d_have,
                                               void *d_scratch, uint64_t scratch_bytes, void *stream) {
  return set_slice_ingest<true>(ctx, d_chunks, chunks_bytes, nullptr, host_lens, n_files, group_log, d_outboards, d_roots, host_files, host_first, host_count,
                                n_ranges, d_slices, d_set_status, d_set_first_bad, d_chunk_status, d_have, d_scratch, scratch_bytes, stream);
}

// the arena call's table and grids; a row's slot (beside the table) is that of its block's first listed chunk in the packed buffer
int32_t b3w_bao_set_slice_packed_device(b3w_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, const uint64_t *host_lens, uint32_t n_files,
                                        uint32_t group_log, const uint8_t *d_outboards, const uint32_t *host_files, const uint64_t *host_first,
                                        const uint64_t *host_count, uint32_t n_ranges, uint8_t *d_slices, void *stream) {
  const char *call = "bao set slice packed";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_ranges) return B3W_OK;
  if (!host_lens || !d_outboards || !host_files || !host_first || !host_count || !d_slices) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards & 7) || ((uintptr_t)d_slices & 15)) return refuse(ctx, call, "d_outboards is not 8-byte or d_slices not 16-byte aligned");
  SetList list;
  B3W_TRY(set_list_ok(ctx, call, nullptr, 0, nullptr, host_lens, n_files, host_files, host_first, host_count, n_ranges, list));
  const PkLayout pk = b3w_int_packed_layout(host_lens, b3w_int_update_ranges(host_lens, host_files, host_first, host_count, n_ranges), group_log);
  B3W_TRY(packed_ok(ctx, call, SparseSrc{d_packed, packed_bytes, nullptr}, pk));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const SetDev *d_sets = nullptr;
  const SetRow<(int)B3W_TILE> *d_big = nullptr;
  const SetRow<64> *d_small = nullptr;
  const uint64_t *d_slot = nullptr;
  B3W_TRY(set_table<true>(ctx, host_lens, n_files, group_log, host_first, host_count, list, st, d_sets, d_big, d_small, d_slot,
                          [](uint32_t) { return 0ull; },
                          [&](uint64_t s, uint64_t blk, uint64_t B) {
                            const SetEnt &e = list.sets[s];
                            return b3w_int_set_row_slot(pk, e.file, host_lens[e.file], group_log, host_first + e.range_first, host_count + e.range_first,
                                                        e.range_end - e.range_first, blk * B);
                          }));
  if (list.big)
    hipLaunchKernelGGL(b3w_bao_set_slice_packed_kernel<(int)B3W_TILE>, dim3((uint32_t)list.big), dim3(B3W_TILE), 0, st, d_sets, d_big, d_slot, group_log, d_packed,
                       d_outboards, d_slices);
  if (list.small)
    hipLaunchKernelGGL(b3w_bao_set_slice_packed_kernel<64>, dim3((uint32_t)list.small), dim3(64), 0, st, d_sets, d_small, d_slot + list.big, group_log, d_packed,
                       d_outboards, d_slices);
  return batch_launched(ctx, st, "bao set slice packed launch");
}

// ---- step records of the wanted chunks of set slices ----------------------------------------------------------------------------------
int32_t b3w_sample_plan_set_slices_device(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, const uint32_t *d_roots, const uint32_t *host_files,
                                          const uint64_t *host_first, const uint64_t *host_count, uint32_t n_ranges, const uint8_t *d_slices,
                                          uint32_t *d_records, int32_t *d_chunk_status, int32_t *d_set_status, uint64_t *d_set_first_bad, void *d_scratch,
                                          uint64_t scratch_bytes, void *stream) {
  const char *call = "sample plan set slices";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(nova_ok(ctx));
  if (!n_ranges) return B3W_OK;
  if (!host_lens || !d_roots || !host_files || !host_first || !host_count || !d_slices || !d_records || !d_chunk_status || !d_set_status || !d_set_first_bad)
    return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_slices & 15) || ((uintptr_t)d_roots & 3)) return refuse(ctx, call, "d_slices is not 16-byte or d_roots not 4-byte aligned");
  if (((uintptr_t)d_records & 3) || ((uintptr_t)d_chunk_status & 3)) return refuse(ctx, call, "d_records or d_chunk_status is not 4-byte aligned");
  if (((uintptr_t)d_set_status & 3) || ((uintptr_t)d_set_first_bad & 7)) return refuse(ctx, call, "d_set_status is not 4-byte or d_set_first_bad not 8-byte aligned");
  SetList list;
  B3W_TRY(set_list_ok(ctx, call, nullptr, 0, nullptr, host_lens, n_files, host_files, host_first, host_count, n_ranges, list));
  if (scratch_bytes < (list.big + list.small) * 16) return refuse(ctx, call, "the scratch is smaller than b3w_bao_set_slice_ingest_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 15)) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const SetDev *d_sets = nullptr;
  const SetRow<(int)B3W_TILE> *d_big = nullptr;
  const SetRow<64> *d_small = nullptr;
  const uint64_t *d_base = nullptr;
  // a row carries the first record row of its first wanted chunk: the runs' first rows (O(depth) a run), then O(depth) a row
  const std::vector<uint64_t> run_row = b3w_int_range_row_first(host_lens, host_files, host_first, host_count, n_ranges);
  B3W_TRY(set_table<true>(ctx, host_lens, n_files, 0, host_first, host_count, list, st, d_sets, d_big, d_small, d_base,
                          [](uint32_t) { return 0ull; },
                          [&](uint64_t s, uint64_t blk, uint64_t B) {
                            const SetEnt &e = list.sets[s];
                            return b3w_int_set_row_base(host_lens[e.file], host_first + e.range_first, host_count + e.range_first, e.range_end - e.range_first,
                                                        run_row.data() + e.range_first, blk * B);
                          }));
  uint4 *res = reinterpret_cast<uint4 *>(d_scratch);
  const uint32_t n_sets = (uint32_t)list.sets.size();
  if (list.big)
    hipLaunchKernelGGL(b3w_sample_plan_set_kernel<(int)B3W_TILE>, dim3((uint32_t)list.big), dim3(B3W_TILE), 0, st, d_sets, d_big, d_base, d_slices, d_roots, d_records,
                       d_chunk_status, res);
  if (list.small)
    hipLaunchKernelGGL(b3w_sample_plan_set_kernel<64>, dim3((uint32_t)list.small), dim3(64), 0, st, d_sets, d_small, d_base + list.big, d_slices, d_roots, d_records,
                       d_chunk_status, res + list.big);
  hipLaunchKernelGGL(b3w_bao_set_reduce_kernel, dim3((n_sets + 3) / 4), dim3(256), 0, st, d_sets, n_sets, res, d_set_status,
                     reinterpret_cast<unsigned long long *>(d_set_first_bad));
  return batch_launched(ctx, st, "sample plan set slices launch");
}

}  // extern "C"

// ---- set slices in windows: one set's slice taken in as it arrives (b3wit.h "set slices in windows") ----------------------------------
// A host object: the set's row table (built once, the one-shot call's rows), the rows' cuts, the caller's device pointers and how far
// the slice has come.  No device memory and no event of its own: the carried area and the rows' results lie in the caller's scratch.
struct b3w_bao_set_stream {
  b3w_ctx *ctx = nullptr;
  uint64_t len = 0;
  uint32_t gl = 0;
  bool packed = false, shrt = false, finished = false;
  uint8_t *dest = nullptr, *ob = nullptr, *carry = nullptr;
  const uint32_t *root = nullptr;
  unsigned long long *have = nullptr, *first_bad = nullptr;
  int32_t *chunk_status = nullptr, *set_status = nullptr;
  uint4 *res = nullptr;
  uint64_t row_cap = 0, row_bytes = 0, next = 0;           // the rows a window may have; a table row's bytes; the first row not pushed
  std::vector<uint64_t> cut;                               // n_rows + 1
  std::vector<uint8_t> rows;                               // SetRow<64> or SetRow<B3W_TILE>, in the table's order
};

namespace {

// the session's rows [i, j) into the staging behind their SetDev: the places in front of the window's cut marked as carried, and what
// the push's tail must carry on - a depth's last node above a block that lies in this window
template <int B>
void set_stream_rows(const b3w_bao_set_stream *s, uint64_t i, uint64_t j, uint8_t *staging, SetStreamFold &fold) {
  const uint64_t at = s->cut[i];
  SetRow<B> *out = reinterpret_cast<SetRow<B> *>(staging);
  memcpy(out, s->rows.data() + i * sizeof(SetRow<B>), (size_t)((j - i) * sizeof(SetRow<B>)));
  for (uint64_t r = 0; r < j - i; ++r)
    for (uint32_t t = 0; t < SET_UP && out[r].up[t]; ++t) {
      if (out[r].up[t] < at) out[r].up[t] = SET_CARRIED | (16 + 64ull * t);
      else fold.src[t] = out[r].up[t] - at;
    }
}

template <int B, bool PACKED>
void set_stream_launch(const b3w_bao_set_stream *s, uint32_t n, const uint8_t *d_table, const uint8_t *d_window, hipStream_t st) {
  hipLaunchKernelGGL((b3w_bao_set_ingest_kernel<B, PACKED, true>), dim3(n), dim3(B), 0, st, reinterpret_cast<const SetDev *>(d_table),
                     reinterpret_cast<const SetRow<B> *>(d_table + sizeof(SetDev)), s->gl, d_window, s->root, s->dest, s->ob, s->chunk_status, s->have, s->res,
                     (const uint8_t *)s->carry);
}

}  // namespace

extern "C" {

int32_t b3w_bao_set_slice_stream_begin(b3w_ctx *ctx, uint64_t len, uint32_t group_log, const uint64_t *host_first, const uint64_t *host_count,
                                       uint32_t n_ranges, const uint32_t *d_root, uint32_t dest_kind, uint8_t *d_dest, uint64_t dest_bytes,
                                       uint8_t *d_outboard, uint64_t *d_have, int32_t *d_chunk_status, int32_t *d_set_status, uint64_t *d_set_first_bad,
                                       void *d_scratch, uint64_t scratch_bytes, void *stream, b3w_bao_set_stream **out_session) {
  const char *call = "bao set slice stream begin";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  if (!out_session) return refuse(ctx, call, "a null session pointer");
  *out_session = nullptr;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (dest_kind != B3W_BAO_SET_STREAM_ARENA && dest_kind != B3W_BAO_SET_STREAM_PACKED) return refuse(ctx, call, "an unknown destination kind");
  const bool packed = dest_kind == B3W_BAO_SET_STREAM_PACKED;
  if (((uintptr_t)d_have & 7) || ((uintptr_t)d_chunk_status & 3)) return refuse(ctx, call, "d_have is not 8-byte or d_chunk_status not 4-byte aligned");
  if (!n_ranges) return refuse(ctx, call, "a set has at least one run");
  if ((!packed && !d_outboard) || !d_root || !host_first || !host_count || !d_set_status || !d_set_first_bad) return refuse(ctx, call, "a null pointer");
  if ((uintptr_t)d_outboard & 7) return refuse(ctx, call, "d_outboard is not 8-byte aligned");
  if (((uintptr_t)d_set_status & 3) || ((uintptr_t)d_set_first_bad & 7)) return refuse(ctx, call, "d_set_status is not 4-byte or d_set_first_bad not 8-byte aligned");
  const std::vector<uint32_t> files(n_ranges, 0);
  const uint64_t off0 = 0;
  SetList list;
  B3W_TRY(set_list_ok(ctx, call, d_dest, dest_bytes, packed ? nullptr : &off0, &len, 1, files.data(), host_first, host_count, n_ranges, list));
  if (packed) B3W_TRY(slots_ok(ctx, call, d_dest, dest_bytes, list.chunks));
  if (scratch_bytes < B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES + 16) return refuse(ctx, call, "the scratch is smaller than b3w_bao_set_slice_stream_scratch_bytes says for the least window");
  if (!d_scratch || ((uintptr_t)d_scratch & 15)) return refuse(ctx, call, "the scratch is null or not 16-byte aligned");
  ON_DEVICE(ctx);
  b3w_bao_set_stream *s = new b3w_bao_set_stream;
  const SetEnt &e = list.sets[0];
  b3w_int_set_stream_cuts(len, host_first, host_count, n_ranges, list, s->cut);
  s->shrt = e.shrt;
  const uint64_t n_rows = s->cut.size() - 1, B = s->shrt ? 64 : B3W_TILE;
  s->ctx = ctx; s->len = len; s->gl = group_log; s->packed = packed;
  s->dest = d_dest; s->ob = d_outboard; s->root = d_root;
  s->have = reinterpret_cast<unsigned long long *>(d_have); s->first_bad = reinterpret_cast<unsigned long long *>(d_set_first_bad);
  s->chunk_status = d_chunk_status; s->set_status = d_set_status;
  s->carry = reinterpret_cast<uint8_t *>(d_scratch);
  s->res = reinterpret_cast<uint4 *>(s->carry + B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES);
  s->row_cap = (scratch_bytes - B3W_BAO_SET_SLICE_STREAM_CARRY_BYTES) / 16;
  if (s->row_cap > n_rows) s->row_cap = n_rows;
  s->row_bytes = s->shrt ? sizeof(SetRow<64>) : sizeof(SetRow<(int)B3W_TILE>);
  s->rows.resize((size_t)(n_rows * s->row_bytes));
  uint64_t last = ~0ull, made = 0;
  bool fits = e.rows == n_rows && e.shrt == s->shrt;
  for (uint64_t i = 0; i < n_ranges && fits; ++i)
    for (uint64_t blk = host_first[i] / B; blk <= (host_first[i] + host_count[i] - 1) / B && fits; ++blk) {
      if (blk == last) continue;
      last = blk;
      uint8_t *at = s->rows.data() + made++ * s->row_bytes;
      fits = s->shrt ? set_make_row<64>(*reinterpret_cast<SetRow<64> *>(at), 0, blk, len, host_first, host_count, n_ranges, list.ufirst.data(), list.rank.data())
                     : set_make_row<(int)B3W_TILE>(*reinterpret_cast<SetRow<(int)B3W_TILE> *>(at), 0, blk, len, host_first, host_count, n_ranges, list.ufirst.data(), list.rank.data());
    }
  if (!fits) { delete s; return refuse(ctx, call, "the rows do not add up");   /* (never: the cuts and the list count the same rows) */ }
  int32_t rc = B3W_OK;
  hipStream_t st = (hipStream_t)stream;
  // the ring's slots grown now, so that a push allocates nothing (a slot in flight keeps its size until a push needs it)
  for (uint32_t k = 0; k < b3w_ctx::B3W_MANY_SLOTS && rc == B3W_OK; ++k) {
    b3w_ctx::ManySlot *slot = nullptr;
    rc = many_staging(ctx, sizeof(SetDev) + s->row_cap * s->row_bytes, &slot);
  }
  if (rc == B3W_OK) {
    hipError_t err = hipMemsetAsync(d_set_status, 0, 4, st);
    if (err == hipSuccess) err = hipMemsetAsync(d_set_first_bad, 0xff, 8, st);
    if (err != hipSuccess) rc = hip_fail(ctx, err, "bao set slice stream begin: hipMemsetAsync");
  }
  if (rc != B3W_OK) { delete s; return rc; }
  *out_session = s;
  return B3W_OK;
}

int32_t b3w_bao_set_slice_stream_push(b3w_bao_set_stream *s, uint64_t offset, const uint8_t *d_window, uint64_t bytes, void *stream) {
  const char *call = "bao set slice stream push";
  if (!s) return B3W_E_BAD_ARGUMENT;
  b3w_ctx *ctx = s->ctx;
  const uint64_t n_rows = s->cut.size() - 1, i = s->next;
  if (s->finished) return refuse(ctx, call, "the session is finished");
  if (i == n_rows) return refuse(ctx, call, "the slice has been pushed to its end");
  if (!d_window || !bytes) return refuse(ctx, call, "a null window or no bytes");
  if (offset != s->cut[i]) return refuse(ctx, call, "out of order: the window starts at slice byte " + std::to_string(offset) + ", the last one ended at " + std::to_string(s->cut[i]));
  if (bytes > s->cut[n_rows] - offset) return refuse(ctx, call, "the window reaches past the slice's end (" + std::to_string(s->cut[n_rows]) + " bytes)");
  const uint64_t j = (uint64_t)(std::lower_bound(s->cut.begin() + (size_t)i + 1, s->cut.end(), offset + bytes) - s->cut.begin());
  if (s->cut[j] != offset + bytes) return refuse(ctx, call, "the window does not end on a cut: slice byte " + std::to_string(offset + bytes) + " lies inside row " + std::to_string(j - 1) + ", which ends at " + std::to_string(s->cut[j]));
  if (((uintptr_t)d_window & 15) != (i ? 0u : 8u)) return refuse(ctx, call, i ? "the window's first byte is not 16-byte aligned" : "the first window's first byte does not lie at 8 modulo 16");
  if (j - i > s->row_cap) return refuse(ctx, call, "the window has " + std::to_string(j - i) + " rows, the scratch holds the results of " + std::to_string(s->row_cap));
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t up_bytes = sizeof(SetDev) + (j - i) * s->row_bytes;
  b3w_ctx::ManySlot *slot = nullptr;
  B3W_TRY(many_staging(ctx, up_bytes, &slot));
  // the set as this window sees it: its slice "starts" a cut in front of the window; pad: the header is carried
  *reinterpret_cast<SetDev *>(slot->h) = SetDev{s->len, 0, 0, offset, 0, 0, 0, 0, (uint32_t)(j - i), i ? 1u : 0u};
  SetStreamFold fold;
  for (uint32_t t = 0; t < SET_UP; ++t) fold.src[t] = ~0ull;
  fold.n_rows = (uint32_t)(j - i); fold.header = i ? 0u : 1u;
  if (s->shrt) set_stream_rows<64>(s, i, j, slot->h + sizeof(SetDev), fold);
  else set_stream_rows<(int)B3W_TILE>(s, i, j, slot->h + sizeof(SetDev), fold);
  // (as many_upload: a copy that was not enqueued reads nothing, so the slot stays free; once it is enqueued many_launched releases it)
  HIP_TRY(ctx, hipMemcpyAsync(slot->d, slot->h, (size_t)up_bytes, hipMemcpyHostToDevice, st));
  const uint32_t n = (uint32_t)(j - i);
  if (s->shrt) {
    if (s->packed) set_stream_launch<64, true>(s, n, slot->d, d_window, st); else set_stream_launch<64, false>(s, n, slot->d, d_window, st);
  } else {
    if (s->packed) set_stream_launch<(int)B3W_TILE, true>(s, n, slot->d, d_window, st); else set_stream_launch<(int)B3W_TILE, false>(s, n, slot->d, d_window, st);
  }
  hipLaunchKernelGGL(b3w_bao_set_stream_fold_kernel, dim3(1), dim3(256), 0, st, fold, d_window, (const uint4 *)s->res, s->set_status, s->first_bad, s->carry);
  B3W_TRY(many_launched(ctx, slot, st, "bao set slice stream push launch"));
  s->next = j;
  return B3W_OK;
}

int32_t b3w_bao_set_slice_stream_finish(b3w_bao_set_stream *s) {
  if (!s) return B3W_E_BAD_ARGUMENT;
  const uint64_t n_rows = s->cut.size() - 1;
  if (s->finished) return refuse(s->ctx, "bao set slice stream finish", "the session is finished");
  if (s->next != n_rows) return refuse(s->ctx, "bao set slice stream finish", std::to_string(n_rows - s->next) + " of " + std::to_string(n_rows) + " rows have not been pushed: the slice is at byte " + std::to_string(s->cut[s->next]) + " of " + std::to_string(s->cut[n_rows]));
  s->finished = true;
  return B3W_OK;
}

void b3w_bao_set_slice_stream_free(b3w_bao_set_stream *s) { delete s; }

}  // extern "C"
