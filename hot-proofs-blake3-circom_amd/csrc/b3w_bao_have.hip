// b3w_bao_have.hip — the arrival bitmap of a batch of files and the run lists made from it ("the arrival bitmap" in b3wit.h).
//
// Layout (b3w_bao_have_layout): file f owns ceil(num_chunks(len_f) / 64) words of 64 bits from word word_first[f]; chunk c is bit c & 63
// of word word_first[f] + (c >> 6); the bits at and above the chunk count in a file's last word are pad bits, masked by every reader.
// The bits are set by b3w_bao_slice_ingest_kernel<K, true> (b3w_bao.hip).  Here:
//   b3w_bao_have_count_kernel    a lane per word: the word's SELECTED mask (below), the number of runs that start in it; a workgroup of
//                                1 024 words leaves its total in the scratch; the per-file counts are zeroed
//   b3w_bao_have_scan_kernel     one workgroup: the exclusive scan of the workgroups' totals in place, the grand total to *d_n_runs
//   b3w_bao_have_rows_kernel     the masks again, the workgroup's scan of the starts on top of its scanned total: the lane of a run's first
//                                chunk writes the row's file and first chunk, the lane of its last chunk writes the chunk behind it into
//                                the count's place; the set bits of every file counted into d_file_have
//   b3w_bao_have_sub_kernel      count = (the chunk behind the run) - first, for the rows written
//   b3w_bao_have_pack_kernel     a bitmap from packed unit statuses, a lane per word, every word written whole
//   b3w_bao_diff_kernel          a bitmap of the chunks two versions of a file share, from the CVs their outboards store (described
//                                where it stands), a wave per word, every word written whole
//   b3w_bao_delta_*_kernel       outboard deltas (described where they stand): mark and compact (the provider), check and write (the
//                                replica), count for both; the scan between them is b3w_bao_have_scan_kernel
// No workgroup waits for another: each level of the scan is a launch.
//
// The selected mask of a word at chunk granularity: a unit is a field of F = 1 << group_log bits, and for group_log <= 6 no field
// straddles a word.  With the pad bits read as ones, AND-folding the word over 1, 2, .. F / 2 leaves at a field's lowest bit whether the
// whole field is set; that bit times (1 << F) - 1 fills the field.  PRESENT selects those fields, MISSING the others, both clipped to
// the valid bits — so a ragged last unit is judged by the chunks it has and a run ends at the file's last chunk.  A run starts at a
// selected bit whose predecessor (the previous word's top bit, inside one file) is not selected, and ends likewise; the runs that ended
// before a word are the runs that started before it, less the one that comes in through bit 0, so one scan numbers both.
#include "b3w_internal.h"
#include "b3w_bao_tree.h"

namespace {

constexpr uint32_t HAVE_WG = 1024;                       // words a workgroup of the run kernels (a lane each)
constexpr uint64_t HAVE_MAX_WORDS = 1ull << 26;

// the tables behind each other in the staging: word_first [n_files + 1], n_chunks [n_files], unit_first [n_files] (the pack call's)
struct HaveTables { const uint64_t *word_first, *n_chunks, *unit_first; };
__host__ __device__ __forceinline__ HaveTables have_tables_at(const uint64_t *tab, uint32_t n_files) {
  return HaveTables{tab, tab + n_files + 1, tab + 2 * (uint64_t)n_files + 1};
}

// the file that owns word w: the last f with word_first[f] <= w (every file has a word, so word_first rises strictly)
__device__ __forceinline__ uint32_t have_file_of(const uint64_t *__restrict__ word_first, uint32_t n_files, uint64_t w) {
  uint32_t lo = 0, hi = n_files;                          // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (word_first[mid] <= w) lo = mid; else hi = mid;
  }
  return lo;
}

// the bits of word i (of its file) that are chunks of a file of n chunks
__device__ __forceinline__ uint64_t have_valid(uint64_t i, uint64_t n) {
  const uint64_t left = n - i * 64;
  return left >= 64 ? ~0ull : (1ull << left) - 1;
}

__device__ __forceinline__ uint64_t have_selected(uint64_t bits, uint64_t valid, uint32_t gl, uint32_t kind) {
  uint64_t x = bits | ~valid;
  for (uint32_t k = 0; k < gl; ++k) x &= x >> (1u << k);
  uint64_t low = 1;                                       // the lowest bit of every field
  for (uint32_t k = gl; k < 6; ++k) low |= low << (1u << k);
  const uint64_t full = gl == 6 ? 0ull - (x & 1) : (x & low) * ((1ull << (1u << gl)) - 1);
  return (kind == B3W_BAO_HAVE_PRESENT ? full : ~full) & valid;
}

struct HaveWord { uint32_t f; uint64_t i, bits, valid, starts, ends; uint32_t cont; bool live; };

// word w's file, place, run starts and ends (live false behind the last word: everything zero)
__device__ __forceinline__ HaveWord have_word(const uint64_t *__restrict__ have, HaveTables t, uint32_t n_files, uint64_t n_words, uint64_t w, uint32_t gl,
                                              uint32_t kind) {
  HaveWord r{};
  r.live = w < n_words;
  if (!r.live) return r;
  r.f = have_file_of(t.word_first, n_files, w);
  const uint64_t first = t.word_first[r.f], last = t.word_first[r.f + 1] - 1, n = t.n_chunks[r.f];
  r.i = w - first;
  r.bits = have[w];
  r.valid = have_valid(r.i, n);
  const uint64_t m = have_selected(r.bits, r.valid, gl, kind);
  const uint64_t prev_top = w > first ? have_selected(have[w - 1], ~0ull, gl, kind) >> 63 : 0;
  const uint64_t next_low = w < last ? have_selected(have[w + 1], have_valid(r.i + 1, n), gl, kind) & 1 : 0;
  r.cont = (uint32_t)(prev_top & m & 1);                  // a run comes in through bit 0
  r.starts = m & ~((m << 1) | prev_top);
  r.ends = m & ~((m >> 1) | (next_low << 63));
  return r;
}

// exclusive scan of v over the workgroup's HAVE_WG lanes (wave shuffles, then the waves' totals in LDS) -> the lane's prefix; total: all lanes'
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *lds /* HAVE_WG / 64 + 1 */, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const uint32_t up = __shfl_up(inc, d);
    if (lane >= (uint32_t)d) inc += up;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t k = 0; k < HAVE_WG / 64; ++k) { const uint32_t x = lds[k]; lds[k] = run; run += x; }
    lds[HAVE_WG / 64] = run;
  }
  __syncthreads();
  total = lds[HAVE_WG / 64];
  return lds[wave] + inc - v;
}

__global__ __launch_bounds__(HAVE_WG) void b3w_bao_have_count_kernel(const uint64_t *__restrict__ have, const uint64_t *__restrict__ tab, uint32_t n_files, uint64_t n_words,
                                                                     uint32_t gl, uint32_t kind, uint64_t *__restrict__ wg_totals,
                                                                     uint64_t *__restrict__ file_have) {
  __shared__ uint32_t lds[HAVE_WG / 64 + 1];
  const uint64_t w = (uint64_t)blockIdx.x * HAVE_WG + threadIdx.x;
  if (file_have && w < n_files) file_have[w] = 0;         // (n_files <= n_words: the grid covers them)
  const HaveWord r = have_word(have, have_tables_at(tab, n_files), n_files, n_words, w, gl, kind);
  uint32_t total;
  (void)block_scan((uint32_t)__popcll(r.starts), lds, total);
  if (threadIdx.x == 0) wg_totals[blockIdx.x] = total;
}

// one workgroup: wg_totals [n] becomes its exclusive scan, *n_runs the sum
__global__ __launch_bounds__(HAVE_WG) void b3w_bao_have_scan_kernel(uint64_t *__restrict__ wg_totals, uint32_t n, uint64_t *__restrict__ n_runs) {
  __shared__ uint64_t sums[HAVE_WG];
  const uint32_t per = (n + HAVE_WG - 1) / HAVE_WG, a = threadIdx.x * per, b = a + per < n ? a + per : n;
  uint64_t mine = 0;
  for (uint32_t k = a; k < b; ++k) mine += wg_totals[k];
  sums[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t run = 0;
    for (uint32_t k = 0; k < HAVE_WG; ++k) { const uint64_t x = sums[k]; sums[k] = run; run += x; }
    *n_runs = run;
  }
  __syncthreads();
  uint64_t run = sums[threadIdx.x];
  for (uint32_t k = a; k < b; ++k) { const uint64_t x = wg_totals[k]; wg_totals[k] = run; run += x; }
}

__global__ __launch_bounds__(HAVE_WG) void b3w_bao_have_rows_kernel(const uint64_t *__restrict__ have, const uint64_t *__restrict__ tab, uint32_t n_files, uint64_t n_words,
                                                                    uint32_t gl, uint32_t kind, const uint64_t *__restrict__ wg_first, uint64_t capacity,
                                                                    uint32_t *__restrict__ run_file, uint64_t *__restrict__ run_first,
                                                                    uint64_t *__restrict__ run_count, unsigned long long *__restrict__ file_have) {
  __shared__ uint32_t lds[HAVE_WG / 64 + 1];
  const uint64_t w = (uint64_t)blockIdx.x * HAVE_WG + threadIdx.x;
  const HaveWord r = have_word(have, have_tables_at(tab, n_files), n_files, n_words, w, gl, kind);
  uint32_t total;
  const uint64_t before = wg_first[blockIdx.x] + block_scan((uint32_t)__popcll(r.starts), lds, total);
  if (capacity) {
    uint64_t row = before;
    for (uint64_t s = r.starts; s && row < capacity; s &= s - 1, ++row) {
      run_file[row] = r.f;
      run_first[row] = r.i * 64 + (uint64_t)(__ffsll((unsigned long long)s) - 1);
    }
    row = before - r.cont;
    for (uint64_t e = r.ends; e && row < capacity; e &= e - 1, ++row) run_count[row] = r.i * 64 + (uint64_t)__ffsll((unsigned long long)e);
  }
  if (file_have) {
    // the set chunks of a file: the lanes of one file in a wave added up (a file's words are neighbours), one atomic a file and wave
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t f = r.live ? r.f : 0xffffffffu;
    uint32_t cnt = (uint32_t)__popcll(r.bits & r.valid);
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const uint32_t up = __shfl_up(cnt, d), uf = __shfl_up(f, d);
      if (lane >= (uint32_t)d && uf == f) cnt += up;
    }
    const uint32_t nf = __shfl_down(f, 1);
    if (r.live && (lane == 63 || nf != f)) atomicAdd(file_have + f, (unsigned long long)cnt);
  }
}

__global__ __launch_bounds__(256) void b3w_bao_have_sub_kernel(const uint64_t *__restrict__ n_runs, uint64_t capacity, const uint64_t *__restrict__ run_first,
                                                               uint64_t *__restrict__ run_count) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x, n = *n_runs < capacity ? *n_runs : capacity;
  if (row < n) run_count[row] -= run_first[row];
}

__global__ __launch_bounds__(256) void b3w_bao_have_pack_kernel(const uint8_t *__restrict__ status, const uint64_t *__restrict__ tab, uint32_t n_files, uint64_t n_words, uint32_t gl,
                                                                uint64_t *__restrict__ have) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_words) return;
  const HaveTables t = have_tables_at(tab, n_files);
  const uint32_t f = have_file_of(t.word_first, n_files, w);
  const uint64_t i = w - t.word_first[f], n = t.n_chunks[f];
  const uint64_t chunks = n - i * 64 < 64 ? n - i * 64 : 64, F = 1ull << gl;
  const uint8_t *st = status + t.unit_first[f] + ((i * 64) >> gl);
  uint64_t bits = 0;
  for (uint64_t c = 0, u = 0; c < chunks; c += F, ++u)
    if (st[u] == 0) bits |= (gl == 6 ? ~0ull : ((1ull << F) - 1)) << c;
  have[w] = bits & have_valid(i, n);
}

// ---- the chunks two versions of a file share, from their outboards alone (b3wit.h "outboard diff") ---------------------------------
// A wave is a word of the bitmap and a lane a chunk of it.  A unit is 2^G chunks, G the larger of the two group_logs, so a word holds
// whole units: the lane of a unit's first chunk finds where each outboard stores the unit's CV (diff_cv_at: a half of its parent's
// node, read at the coarser level in the finer outboard; the root where the unit is the whole file) and compares the 32 bytes, the
// ballot is the word at the units' lowest bits, one multiplication fills the fields as have_selected does, lane 0 stores the word
// whole.  The pair of a word is found in SGPRs (the wave index is made uniform).  Nothing is hashed; a half node is 8-byte aligned and
// a root 4-byte, and no load assumes more.
// the staging: word_first [n_pairs + 1], then four words a pair: chunk counts (a low, b high), a's and b's outboard's first byte, the
// files (a low, b high)
constexpr uint32_t DIFF_WG = 256;

__device__ __forceinline__ bool cv_equal(const uint8_t *a, const uint8_t *b, bool roots) {
  if (roots) {
    const uint32_t *x = reinterpret_cast<const uint32_t *>(a), *y = reinterpret_cast<const uint32_t *>(b);
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d |= x[k] ^ y[k];
    return d == 0;
  }
  const uint64_t *x = reinterpret_cast<const uint64_t *>(a), *y = reinterpret_cast<const uint64_t *>(b);
  uint64_t d = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) d |= x[k] ^ y[k];
  return d == 0;
}

__global__ __launch_bounds__(DIFF_WG) void b3w_bao_diff_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *obs_a,
                                                               const uint32_t *roots_a, uint32_t gl_a, const uint8_t *obs_b, const uint32_t *roots_b,
                                                               uint32_t gl_b, uint64_t *__restrict__ same) {
  const uint64_t w = (uint64_t)blockIdx.x * (DIFF_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_words) return;
  const uint32_t lane = threadIdx.x & 63, G = gl_a > gl_b ? gl_a : gl_b, F = 1u << G;
  const uint32_t p = have_file_of(tab, n_pairs, w);
  const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + 4ull * p;
  const uint64_t i = w - tab[p], c = i * 64 + lane;
  const uint32_t na = (uint32_t)rec[0], nb = (uint32_t)(rec[0] >> 32);
  bool eq = false;
  if (c < nb && !(lane & (F - 1)) && diff_unit_comparable(na, nb, (uint32_t)(c >> G), G)) {
    const uint32_t u = (uint32_t)(c >> G);
    const bool whole = nb <= F;
    const uint8_t *cv_a = whole ? reinterpret_cast<const uint8_t *>(roots_a + 8ull * (uint32_t)rec[3]) : obs_a + rec[1] + diff_cv_at(na, gl_a, u, G);
    const uint8_t *cv_b = whole ? reinterpret_cast<const uint8_t *>(roots_b + 8ull * (uint32_t)(rec[3] >> 32)) : obs_b + rec[2] + diff_cv_at(nb, gl_b, u, G);
    eq = cv_equal(cv_a, cv_b, whole);
  }
  const uint64_t low = __ballot(eq);
  const uint64_t bits = G == 6 ? 0ull - (low & 1) : low * ((1ull << F) - 1);
  if (lane == 0) same[w] = bits & have_valid(i, nb);
}

// ---- outboard deltas: b's parent nodes that a does not hold, served and verified on arrival (b3wit.h "outboard delta") --------------
// Both calls keep the diff kernel's shape: a wave is a word of a pair's bitmap (bit p: b's node p is in the blob), a lane a node.  What
// a lane decides about its node is b3w_bao_tree.h's (delta_node_same, delta_check_node, delta_copy_from), shared with the host mirrors;
// a node's span and the places of the stored CVs come from walks down from the root, at most 30 steps each.  A node's rank in the blob
// is (the set bits of the pair's words in front of its word) + (those below it in its word): the first from the have_runs scan over
// ALL pairs' words - a lane per word counts, the workgroups' totals are scanned by b3w_bao_have_scan_kernel, and a word's prefix is
// its workgroup's first plus its own place in the workgroup (delta_prefix).
//   provider  mark (the ballot of "not SAME" is the word, stored whole into the blob), count, scan, compact (a lane copies its node to
//             its rank while the rank is below the extent's capacity; a thread per pair writes the header and k as found)
//   replica   count (over the blob's own bitmap; the pairs' keys reset), scan, check (a thread per pair the header; a lane its node:
//             one parent compression per present node; the least key of a pair by atomicMin), write (gated on the pair's key: present
//             nodes from the blob, absent ones from a's outboard; a thread per pair the status, the first bad node and the length)
// The staging: word_first [n_pairs + 1], then eight words a pair: chunk counts (a low, b high), a's outboard's first byte (~0: the
// replica holds nothing), b's outboard's (provider), the files (a low, b high), the blob's first byte, the nodes its extent holds,
// len_b, the output outboard's first byte (replica).  A blob is UNTRUSTED: every node read is behind a rank below the capacity.
constexpr uint32_t DELTA_WG = 256, DELTA_REC = 8;
static_assert(DELTA_MALFORMED == B3W_BAO_DELTA_MALFORMED && DELTA_BAD_HASH == B3W_BAO_DELTA_BAD_HASH && DELTA_NOT_HELD == B3W_BAO_DELTA_NOT_HELD, "b3wit.h");

__device__ __forceinline__ DeltaSides delta_sides(const uint64_t *rec, const uint8_t *obs_a, const uint32_t *roots_a, const uint32_t *roots_b, uint32_t g) {
  DeltaSides s;
  const bool has_a = rec[1] != ~0ull;
  const uint32_t F1 = (1u << g) - 1;
  s.ob_a = has_a ? obs_a + rec[1] : nullptr;
  s.root_a = has_a && roots_a ? reinterpret_cast<const uint8_t *>(roots_a + 8ull * (uint32_t)rec[3]) : nullptr;
  s.root_b = roots_b ? reinterpret_cast<const uint8_t *>(roots_b + 8ull * (uint32_t)(rec[3] >> 32)) : nullptr;
  s.na = (uint32_t)rec[0]; s.nb = (uint32_t)(rec[0] >> 32);
  s.ua = (s.na + F1) >> g; s.ub = (s.nb + F1) >> g;
  s.g = g;
  return s;
}
// the set bits in front of word w of all pairs' words (w = n_words: all of them)
__device__ __forceinline__ uint64_t delta_prefix(const uint64_t *__restrict__ wg_first, const uint32_t *__restrict__ word_rank, uint64_t n_words, uint64_t w) {
  return w < n_words ? wg_first[w / HAVE_WG] + word_rank[w] : wg_first[-1];      // (the grand total lies in front of the workgroups' firsts)
}
__device__ __forceinline__ void copy_node(uint8_t *dst, const uint8_t *src) {
  uint64_t v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = reinterpret_cast<const uint64_t *>(src)[k];
#pragma unroll
  for (int k = 0; k < 8; ++k) reinterpret_cast<uint64_t *>(dst)[k] = v[k];
}

__global__ __launch_bounds__(DELTA_WG) void b3w_bao_delta_mark_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *obs_a,
                                                                      const uint32_t *roots_a, const uint8_t *obs_b, const uint32_t *roots_b, uint32_t g,
                                                                      uint8_t *__restrict__ delta) {
  const uint64_t w = (uint64_t)blockIdx.x * (DELTA_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_words) return;
  const uint32_t lane = threadIdx.x & 63, i = have_file_of(tab, n_pairs, w);
  const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
  const uint64_t j = w - tab[i];
  const uint32_t p = (uint32_t)(j * 64 + lane);
  const DeltaSides s = delta_sides(rec, obs_a, roots_a, roots_b, g);
  const bool differs = p < s.ub - 1 && !delta_node_same(s, obs_b + rec[2], p);
  const uint64_t word = __ballot(differs);
  if (lane == 0) *reinterpret_cast<uint64_t *>(delta + rec[4] + 16 + 8 * j) = word;
}

// a lane per word of the blobs' bitmaps: its count's place in the workgroup to word_rank, the workgroup's total to wg_totals; keys
// (the replica's): reset for every pair (the grid covers the pairs)
__global__ __launch_bounds__(HAVE_WG) void b3w_bao_delta_count_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *__restrict__ delta,
                                                                      uint64_t *__restrict__ wg_totals, uint32_t *__restrict__ word_rank, uint64_t *__restrict__ keys) {
  __shared__ uint32_t lds[HAVE_WG / 64 + 1];
  const uint64_t w = (uint64_t)blockIdx.x * HAVE_WG + threadIdx.x;
  if (keys && w < n_pairs) keys[w] = DELTA_OK;
  uint32_t pop = 0;
  if (w < n_words) {
    const uint32_t i = have_file_of(tab, n_pairs, w);
    const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
    pop = (uint32_t)__popcll(*reinterpret_cast<const uint64_t *>(delta + rec[4] + 16 + 8 * (w - tab[i])));
  }
  uint32_t total;
  const uint32_t before = block_scan(pop, lds, total);
  if (w < n_words) word_rank[w] = before;
  if (threadIdx.x == 0) wg_totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(DELTA_WG) void b3w_bao_delta_compact_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *__restrict__ obs_b,
                                                                         const uint64_t *__restrict__ wg_first, const uint32_t *__restrict__ word_rank,
                                                                         uint8_t *__restrict__ delta, uint64_t *__restrict__ n_nodes) {
  const uint64_t t = (uint64_t)blockIdx.x * DELTA_WG + threadIdx.x;
  if (t < n_pairs) {                                       // the pair's header: len_b, k as found
    const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * t;
    const uint64_t k = delta_prefix(wg_first, word_rank, n_words, tab[t + 1]) - delta_prefix(wg_first, word_rank, n_words, tab[t]);
    uint64_t *head = reinterpret_cast<uint64_t *>(delta + rec[4]);
    head[0] = rec[6];
    head[1] = k;
    n_nodes[t] = k;
  }
  const uint64_t w = (uint64_t)blockIdx.x * (DELTA_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_words) return;
  const uint32_t lane = threadIdx.x & 63, i = have_file_of(tab, n_pairs, w);
  const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
  const uint64_t j = w - tab[i], W = tab[i + 1] - tab[i];
  uint8_t *blob = delta + rec[4];
  const uint64_t word = *reinterpret_cast<const uint64_t *>(blob + 16 + 8 * j);
  if (!((word >> lane) & 1)) return;
  const uint64_t r = delta_prefix(wg_first, word_rank, n_words, w) - delta_prefix(wg_first, word_rank, n_words, tab[i]) + (uint64_t)__popcll(word & ((1ull << lane) - 1));
  if (r >= rec[5]) return;                                 // behind the extent: counted, not written
  copy_node(blob + 16 + 8 * W + 64 * r, obs_b + rec[2] + 8 + 64 * (j * 64 + lane));
}

__global__ __launch_bounds__(DELTA_WG) void b3w_bao_delta_check_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *obs_a,
                                                                       const uint32_t *roots_a, const uint32_t *roots_b, uint32_t g, const uint8_t *__restrict__ delta,
                                                                       const uint64_t *__restrict__ wg_first, const uint32_t *__restrict__ word_rank,
                                                                       unsigned long long *__restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * DELTA_WG + threadIdx.x;
  if (t < n_pairs) {
    const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * t;
    const uint64_t count = delta_prefix(wg_first, word_rank, n_words, tab[t + 1]) - delta_prefix(wg_first, word_rank, n_words, tab[t]);
    const uint64_t key = delta_check_head(delta + rec[4], rec[6], rec[5], count);
    if (key != DELTA_OK) atomicMin(keys + t, (unsigned long long)key);
  }
  const uint64_t w = (uint64_t)blockIdx.x * (DELTA_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_words) return;
  const uint32_t lane = threadIdx.x & 63, i = have_file_of(tab, n_pairs, w);
  const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
  const uint64_t first = tab[i], base = delta_prefix(wg_first, word_rank, n_words, first);
  const uint8_t *blob = delta + rec[4];
  const DeltaSides s = delta_sides(rec, obs_a, roots_a, roots_b, g);
  const auto rank = [&](uint32_t q) {
    const uint64_t word = *reinterpret_cast<const uint64_t *>(blob + 16 + 8 * (uint64_t)(q >> 6));
    return delta_prefix(wg_first, word_rank, n_words, first + (q >> 6)) - base + (uint64_t)__popcll(word & ((1ull << (q & 63)) - 1));
  };
  const uint64_t key = delta_check_node(s, blob, rec[5], (uint32_t)((w - first) * 64 + lane), rank);
  if (key != DELTA_OK) atomicMin(keys + i, (unsigned long long)key);
}

__global__ __launch_bounds__(DELTA_WG) void b3w_bao_delta_write_kernel(const uint64_t *__restrict__ tab, uint32_t n_pairs, uint64_t n_words, const uint8_t *obs_a, uint32_t g,
                                                                       const uint8_t *delta, const uint64_t *__restrict__ wg_first, const uint32_t *__restrict__ word_rank,
                                                                       const uint64_t *__restrict__ keys, uint8_t *out, int32_t *__restrict__ status,
                                                                       uint64_t *__restrict__ first_bad) {
  const uint64_t t = (uint64_t)blockIdx.x * DELTA_WG + threadIdx.x;
  if (t < n_pairs) {
    const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * t;
    const uint64_t key = keys[t];
    status[t] = key == DELTA_OK ? 0 : (int32_t)(key & 3);
    first_bad[t] = key == DELTA_OK ? ~0ull : key >> 2;
    if (key == DELTA_OK) *reinterpret_cast<uint64_t *>(out + rec[7]) = rec[6];
  }
  const uint64_t w = (uint64_t)blockIdx.x * (DELTA_WG / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_words) return;
  const uint32_t lane = threadIdx.x & 63, i = have_file_of(tab, n_pairs, w);
  if (keys[i] != DELTA_OK) return;                         // a pair with a status keeps its output as it was
  const uint64_t *rec = tab + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
  const uint64_t first = tab[i], j = w - first, W = tab[i + 1] - first;
  const DeltaSides s = delta_sides(rec, obs_a, nullptr, nullptr, g);
  const uint32_t p = (uint32_t)(j * 64 + lane);
  if (p >= s.ub - 1) return;
  const uint8_t *blob = delta + rec[4], *src;
  const uint64_t word = *reinterpret_cast<const uint64_t *>(blob + 16 + 8 * j);
  if ((word >> lane) & 1) {
    const uint64_t r = delta_prefix(wg_first, word_rank, n_words, w) - delta_prefix(wg_first, word_rank, n_words, first) + (uint64_t)__popcll(word & ((1ull << lane) - 1));
    src = blob + 16 + 8 * W + 64 * r;                      // (r < k <= the capacity: the pair passed)
  } else {
    const uint64_t at = delta_copy_from(s, p);
    if (!at) return;
    src = s.ob_a + at;
  }
  uint8_t *dst = out + rec[7] + 8 + 64ull * p;
  if (src != dst) copy_node(dst, src);                     // (in place: a's own node stays where it is)
}

// the tables into the staging and on their way to the device -> their device addresses
int32_t have_tables(b3w_ctx *ctx, const uint64_t *host_lens, uint32_t n_files, bool units, uint32_t group_log, hipStream_t st, const uint64_t *&t) {
  const uint64_t words = (uint64_t)n_files * (units ? 3 : 2) + 1;
  B3W_TRY(b3w_int_batch_staging(ctx, words * 8));
  uint64_t *h = reinterpret_cast<uint64_t *>(ctx->h_batch);
  (void)b3w_bao_have_layout(host_lens, n_files, h);
  for (uint32_t f = 0; f < n_files; ++f) h[(uint64_t)n_files + 1 + f] = num_chunks(host_lens[f]);
  if (units) {
    uint64_t at = 0;                                      // b3w_bao_verify_layout without its last entry
    for (uint32_t f = 0; f < n_files; ++f) { h[2 * (uint64_t)n_files + 1 + f] = at; at += n_units(host_lens[f], group_log); }
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)(words * 8), hipMemcpyHostToDevice, st));
  t = reinterpret_cast<const uint64_t *>(ctx->d_batch);
  return B3W_OK;
}

uint64_t have_words(const uint64_t *lens, uint32_t n_files) {
  uint64_t at = 0;
  for (uint32_t f = 0; f < n_files; ++f) at += (num_chunks(lens[f]) + 63) / 64;
  return at;
}

}  // namespace

extern "C" {

uint64_t b3w_bao_have_runs_scratch_bytes(const uint64_t *host_lens, uint32_t n_files) {
  if (!host_lens) return 0;
  const uint64_t wgs = (have_words(host_lens, n_files) + HAVE_WG - 1) / HAVE_WG;
  return (wgs * 8 + 15) & ~15ull;                        // a workgroup's total, then its first row
}

int32_t b3w_bao_have_runs_device(b3w_ctx *ctx, const uint64_t *d_have, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log, uint32_t kind,
                                 uint64_t capacity, uint32_t *d_run_file, uint64_t *d_run_first, uint64_t *d_run_count, uint64_t *d_n_runs,
                                 uint64_t *d_file_have, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao have runs";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (kind != B3W_BAO_HAVE_MISSING && kind != B3W_BAO_HAVE_PRESENT) return refuse(ctx, call, "kind is neither B3W_BAO_HAVE_MISSING nor B3W_BAO_HAVE_PRESENT");
  if (!d_n_runs || ((uintptr_t)d_n_runs & 7)) return refuse(ctx, call, "d_n_runs is null or not 8-byte aligned");
  if (capacity && (!d_run_file || !d_run_first || !d_run_count)) return refuse(ctx, call, "a null row array with a capacity above 0");
  if (((uintptr_t)d_run_file & 3) || ((uintptr_t)d_run_first & 7) || ((uintptr_t)d_run_count & 7) || ((uintptr_t)d_file_have & 7)) return refuse(ctx, call, "d_run_file is not 4-byte aligned, or d_run_first, d_run_count or d_file_have not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (!n_files) {
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipMemsetAsync(d_n_runs, 0, 8, st));
    return B3W_OK;
  }
  if (!host_lens || !d_have || ((uintptr_t)d_have & 7)) return refuse(ctx, call, "host_lens or d_have is null, or d_have not 8-byte aligned");
  const uint64_t n_words = have_words(host_lens, n_files);
  if (n_words > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 bitmap words");
  const uint32_t wgs = (uint32_t)((n_words + HAVE_WG - 1) / HAVE_WG);
  if (scratch_bytes < (((uint64_t)wgs * 8 + 15) & ~15ull)) return refuse(ctx, call, "the scratch is smaller than b3w_bao_have_runs_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 7)) return refuse(ctx, call, "the scratch is null or not 8-byte aligned");
  uint64_t most = 0;                                      // the rows there can be: ceil(units / 2) a file
  for (uint32_t f = 0; f < n_files; ++f) most += (n_units(host_lens[f], group_log) + 1) / 2;
  ON_DEVICE(ctx);
  const uint64_t *t = nullptr;
  B3W_TRY(have_tables(ctx, host_lens, n_files, false, 0, st, t));
  uint64_t *wg = reinterpret_cast<uint64_t *>(d_scratch);
  hipLaunchKernelGGL(b3w_bao_have_count_kernel, dim3(wgs), dim3(HAVE_WG), 0, st, d_have, t, n_files, n_words, group_log, kind, wg, d_file_have);
  hipLaunchKernelGGL(b3w_bao_have_scan_kernel, dim3(1), dim3(HAVE_WG), 0, st, wg, wgs, d_n_runs);
  if (capacity || d_file_have)
    hipLaunchKernelGGL(b3w_bao_have_rows_kernel, dim3(wgs), dim3(HAVE_WG), 0, st, d_have, t, n_files, n_words, group_log, kind, wg, capacity, d_run_file, d_run_first,
                       d_run_count, reinterpret_cast<unsigned long long *>(d_file_have));
  const uint64_t rows = capacity < most ? capacity : most;
  if (rows) hipLaunchKernelGGL(b3w_bao_have_sub_kernel, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, st, d_n_runs, capacity, d_run_first, d_run_count);
  return b3w_int_batch_launched(ctx, st, "bao have runs launch");
}

int32_t b3w_bao_have_from_status_device(b3w_ctx *ctx, const uint8_t *d_unit_status, const uint64_t *host_lens, uint32_t n_files, uint32_t group_log,
                                        uint64_t *d_have, void *stream) {
  const char *call = "bao have from status";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_files) return B3W_OK;
  if (!d_unit_status || !host_lens || !d_have || ((uintptr_t)d_have & 7)) return refuse(ctx, call, "a null pointer, or d_have not 8-byte aligned");
  const uint64_t n_words = have_words(host_lens, n_files);
  if (n_words > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 bitmap words");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *t = nullptr;
  B3W_TRY(have_tables(ctx, host_lens, n_files, true, group_log, st, t));
  hipLaunchKernelGGL(b3w_bao_have_pack_kernel, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, st, d_unit_status, t, n_files, n_words, group_log, d_have);
  return b3w_int_batch_launched(ctx, st, "bao have from status launch");
}

int32_t b3w_bao_outboard_diff_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                     uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, uint32_t group_log_a,
                                     const uint64_t *host_lens_b, const uint64_t *host_ob_first_b, const uint8_t *d_outboards_b,
                                     uint64_t outboards_b_bytes, const uint32_t *d_roots_b, uint32_t n_files_b, uint32_t group_log_b,
                                     const uint32_t *host_pair_a, const uint32_t *host_pair_b, uint32_t n_pairs, const uint64_t *host_word_first,
                                     uint64_t *d_same, void *stream) {
  const char *call = "bao outboard diff";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log_a));
  B3W_TRY(group_log_ok(ctx, call, group_log_b));
  if (!n_pairs) return B3W_OK;
  if (!host_lens_a || !host_ob_first_a || !d_outboards_a || !d_roots_a || !host_lens_b || !host_ob_first_b || !d_outboards_b || !d_roots_b || !host_pair_a ||
      !host_pair_b || !host_word_first || !d_same)
    return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards_a & 7) || ((uintptr_t)d_outboards_b & 7) || ((uintptr_t)d_roots_a & 3) || ((uintptr_t)d_roots_b & 3) || ((uintptr_t)d_same & 7))
    return refuse(ctx, call, "d_outboards_a, d_outboards_b or d_same is not 8-byte aligned, or d_roots_a or d_roots_b not 4-byte aligned");
  if (n_pairs > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 bitmap words");      // (a pair has a word at least)
  ON_DEVICE(ctx);
  const uint64_t words = 5ull * n_pairs + 1;
  B3W_TRY(b3w_int_batch_staging(ctx, words * 8));
  uint64_t *h = reinterpret_cast<uint64_t *>(ctx->h_batch);
  uint64_t n_words = 0;                                   // one pass checks a pair and writes its record; a refusal launches nothing
  for (uint32_t i = 0; i < n_pairs; ++i) {
    const uint32_t fa = host_pair_a[i], fb = host_pair_b[i];
    const auto pair = [i] { return "pair " + std::to_string(i); };
    if (fa >= n_files_a || fb >= n_files_b) return refuse(ctx, call, pair() + " names a file that is not below its side's file count");
    const uint64_t na = num_chunks(host_lens_a[fa]), nb = num_chunks(host_lens_b[fb]);
    if (na > DIFF_MAX_CHUNKS || nb > DIFF_MAX_CHUNKS) return refuse(ctx, call, pair() + " has a file of more than 2^30 chunks");
    const uint64_t oa = host_ob_first_a[fa], ob = host_ob_first_b[fb];
    if ((oa & 7) || (ob & 7)) return refuse(ctx, call, pair() + ": an outboard's place is not 8-byte aligned");
    const uint64_t sa = group_outboard_bytes(host_lens_a[fa], group_log_a), sb = group_outboard_bytes(host_lens_b[fb], group_log_b);
    if (oa > outboards_a_bytes || sa > outboards_a_bytes - oa || ob > outboards_b_bytes || sb > outboards_b_bytes - ob)
      return refuse(ctx, call, pair() + ": an outboard reaches past its buffer's bytes");
    if (host_word_first[i] != n_words) return refuse(ctx, call, "host_word_first is not b3w_bao_have_layout of the pairs' b lengths at " + pair());
    h[i] = n_words;
    uint64_t *rec = h + (uint64_t)n_pairs + 1 + 4ull * i;
    rec[0] = na | nb << 32;
    rec[1] = oa;
    rec[2] = ob;
    rec[3] = fa | (uint64_t)fb << 32;
    n_words += (nb + 63) / 64;
    if (n_words > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 bitmap words");
  }
  if (host_word_first[n_pairs] != n_words) return refuse(ctx, call, "host_word_first is not b3w_bao_have_layout of the pairs' b lengths at its last entry");
  h[n_pairs] = n_words;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)(words * 8), hipMemcpyHostToDevice, st));
  const uint32_t per = DIFF_WG / 64;
  hipLaunchKernelGGL(b3w_bao_diff_kernel, dim3((uint32_t)((n_words + per - 1) / per)), dim3(DIFF_WG), 0, st, reinterpret_cast<const uint64_t *>(ctx->d_batch), n_pairs,
                     n_words, d_outboards_a, d_roots_a, group_log_a, d_outboards_b, d_roots_b, group_log_b, d_same);
  return b3w_int_batch_launched(ctx, st, "bao outboard diff launch");
}

}  // extern "C"

// ---- outboard deltas: what both entry points check and prepare, then the entry points ------------------------------------------------
namespace {

bool ranges_meet(const void *p, uint64_t n, const void *q, uint64_t m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return n && m && a < b + m && b < a + n;
}
uint64_t delta_pair_words(const uint64_t *lens_b, const uint32_t *pair_b, uint32_t n_pairs, uint32_t n_files_b, uint32_t g, bool &ok) {
  uint64_t at = 0;
  ok = true;
  for (uint32_t i = 0; i < n_pairs; ++i) {
    const uint32_t fb = pair_b ? pair_b[i] : i;
    if (fb >= n_files_b) { ok = false; return 0; }
    at += delta_words(n_units(lens_b[fb], g));
  }
  return at;
}
uint64_t delta_scratch(uint64_t n_words, uint32_t n_pairs) {
  const uint64_t most = n_words > n_pairs ? n_words : n_pairs, wgs = most ? (most + HAVE_WG - 1) / HAVE_WG : 1;
  return (8 * (1 + wgs + (uint64_t)n_pairs) + 4 * n_words + 15) & ~15ull;      // the total, the workgroups' firsts, the pairs' keys, the words' ranks
}

struct DeltaPlan { uint64_t n_words; uint32_t wgs; const uint64_t *tab; uint64_t *total, *wg, *keys; uint32_t *word_rank; };

// the checks both calls share and the table of pairs into the staging; nothing is launched or written to the device before it returns.
// The provider passes ob_first_b and no out_first, the replica the other way round.
int32_t delta_prepare(b3w_ctx *ctx, const char *call, const uint64_t *lens_a, const uint64_t *ob_first_a, const uint8_t *d_a, uint64_t a_bytes, uint32_t n_files_a,
                      const uint64_t *lens_b, const uint64_t *ob_first_b, uint64_t b_bytes, uint32_t n_files_b, uint32_t g, const uint32_t *pair_a,
                      const uint32_t *pair_b, uint32_t n_pairs, const uint64_t *delta_first, uint64_t delta_bytes, const uint64_t *out_first, const uint8_t *d_out,
                      uint64_t out_bytes, bool in_place, void *d_scratch, uint64_t scratch_bytes, hipStream_t st, DeltaPlan &plan) {
  if (n_pairs > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 pairs");
  const uint64_t words = (uint64_t)n_pairs * (1 + DELTA_REC) + 1;
  B3W_TRY(b3w_int_batch_staging(ctx, words * 8));
  uint64_t *h = reinterpret_cast<uint64_t *>(ctx->h_batch);
  uint64_t n_words = 0, out_end = 0;
  for (uint32_t i = 0; i < n_pairs; ++i) {
    const uint32_t fa = pair_a[i], fb = pair_b[i];
    const auto pair = [i] { return "pair " + std::to_string(i); };
    const bool has_a = fa != B3W_BAO_DELTA_NO_A;
    if ((has_a && fa >= n_files_a) || fb >= n_files_b) return refuse(ctx, call, pair() + " names a file that is not below its side's file count");
    const uint64_t na = has_a ? num_chunks(lens_a[fa]) : 0, nb = num_chunks(lens_b[fb]);
    if (na > DIFF_MAX_CHUNKS || nb > DIFF_MAX_CHUNKS) return refuse(ctx, call, pair() + " has a file of more than 2^30 chunks");
    const uint64_t ub = n_units(lens_b[fb], g), W = delta_words(ub);
    uint64_t oa = ~0ull;
    if (has_a) {
      oa = ob_first_a[fa];
      if (oa & 7) return refuse(ctx, call, pair() + ": an outboard's place is not 8-byte aligned");
      const uint64_t sa = group_outboard_bytes(lens_a[fa], g);
      if (oa > a_bytes || sa > a_bytes - oa) return refuse(ctx, call, pair() + ": an outboard reaches past its buffer's bytes");
    }
    uint64_t ob = 0;
    if (ob_first_b) {
      ob = ob_first_b[fb];
      if (ob & 7) return refuse(ctx, call, pair() + ": an outboard's place is not 8-byte aligned");
      const uint64_t sb = group_outboard_bytes(lens_b[fb], g);
      if (ob > b_bytes || sb > b_bytes - ob) return refuse(ctx, call, pair() + ": an outboard reaches past its buffer's bytes");
    }
    const uint64_t d0 = delta_first[i], d1 = delta_first[i + 1];
    if ((d0 & 7) || (d1 & 7)) return refuse(ctx, call, "host_delta_first is not 8-byte aligned at " + pair());
    if (d1 < d0) return refuse(ctx, call, "host_delta_first does not rise at " + pair() + ": the extents overlap");
    if (d1 > delta_bytes) return refuse(ctx, call, pair() + ": the blob's extent reaches past delta_bytes");
    if (d1 - d0 < 16 + 8 * W) return refuse(ctx, call, pair() + ": the blob's extent is too small for its header and bitmap");
    uint64_t oo = 0;
    if (out_first) {
      oo = out_first[i];
      const uint64_t so = group_outboard_bytes(lens_b[fb], g);
      if (oo & 7) return refuse(ctx, call, pair() + ": the output outboard's place is not 8-byte aligned");
      if (oo > out_bytes || so > out_bytes - oo) return refuse(ctx, call, pair() + ": the output outboard reaches past its buffer's bytes");
      if (i && oo < out_end) return refuse(ctx, call, pair() + ": the output outboards do not lie in rising order, or two of them overlap");
      out_end = oo + so;
      if (in_place && !(has_a && n_units(lens_a[fa], g) == ub && d_out + oo == d_a + oa))
        return refuse(ctx, call, pair() + ": the output buffer overlaps a's outboards, and this pair's output is not a's outboard of the same unit count at the same place");
    }
    h[i] = n_words;
    uint64_t *rec = h + (uint64_t)n_pairs + 1 + (uint64_t)DELTA_REC * i;
    rec[0] = na | nb << 32;
    rec[1] = oa;
    rec[2] = ob;
    rec[3] = (has_a ? fa : 0) | (uint64_t)fb << 32;
    rec[4] = d0;
    rec[5] = (d1 - d0 - 16 - 8 * W) / 64;
    rec[6] = lens_b[fb];
    rec[7] = oo;
    n_words += W;
    if (n_words > HAVE_MAX_WORDS) return refuse(ctx, call, "more than 2^26 bitmap words");
  }
  h[n_pairs] = n_words;
  if (scratch_bytes < delta_scratch(n_words, n_pairs)) return refuse(ctx, call, "the scratch is smaller than b3w_bao_outboard_delta_scratch_bytes says");
  if (!d_scratch || ((uintptr_t)d_scratch & 7)) return refuse(ctx, call, "the scratch is null or not 8-byte aligned");
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, ctx->h_batch, (size_t)(words * 8), hipMemcpyHostToDevice, st));
  const uint64_t most = n_words > n_pairs ? n_words : n_pairs;
  plan.n_words = n_words;
  plan.wgs = (uint32_t)((most + HAVE_WG - 1) / HAVE_WG);
  plan.tab = reinterpret_cast<const uint64_t *>(ctx->d_batch);
  plan.total = reinterpret_cast<uint64_t *>(d_scratch);
  plan.wg = plan.total + 1;
  plan.keys = plan.wg + plan.wgs;
  plan.word_rank = reinterpret_cast<uint32_t *>(plan.keys + n_pairs);
  return B3W_OK;
}
// the grid of the kernels that give a wave to a word and a thread to a pair
uint32_t delta_grid(const DeltaPlan &p, uint32_t n_pairs) {
  const uint64_t a = (p.n_words + DELTA_WG / 64 - 1) / (DELTA_WG / 64), b = ((uint64_t)n_pairs + DELTA_WG - 1) / DELTA_WG;
  return (uint32_t)(a > b ? a : b);
}

}  // namespace
extern "C" {

uint64_t b3w_bao_outboard_delta_scratch_bytes(const uint64_t *host_lens_b, uint32_t n_files_b, const uint32_t *host_pair_b, uint32_t n_pairs, uint32_t group_log) {
  if (!host_lens_b || group_log > B3W_BAO_MAX_GROUP_LOG) return 0;
  bool ok;
  const uint64_t n_words = delta_pair_words(host_lens_b, host_pair_b, n_pairs, n_files_b, group_log, ok);
  return ok ? delta_scratch(n_words, n_pairs) : 0;
}

int32_t b3w_bao_outboard_delta_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                      uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, const uint64_t *host_lens_b,
                                      const uint64_t *host_ob_first_b, const uint8_t *d_outboards_b, uint64_t outboards_b_bytes, const uint32_t *d_roots_b,
                                      uint32_t n_files_b, uint32_t group_log_a, uint32_t group_log_b, const uint32_t *host_pair_a, const uint32_t *host_pair_b,
                                      uint32_t n_pairs, const uint64_t *host_delta_first, uint8_t *d_delta, uint64_t delta_bytes, uint64_t *d_n_nodes,
                                      void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao outboard delta";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log_a));
  B3W_TRY(group_log_ok(ctx, call, group_log_b));
  if (group_log_a != group_log_b) return refuse(ctx, call, "the two sides have different group_logs (b3w_bao_outboard_diff_device takes those)");
  if (!n_pairs) return B3W_OK;
  if (!host_lens_b || !host_ob_first_b || !d_outboards_b || !d_roots_b || !host_pair_a || !host_pair_b || !host_delta_first || !d_delta || !d_n_nodes)
    return refuse(ctx, call, "a null pointer");
  if (n_files_a && (!host_lens_a || !host_ob_first_a || !d_outboards_a || !d_roots_a)) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards_a & 7) || ((uintptr_t)d_outboards_b & 7) || ((uintptr_t)d_roots_a & 3) || ((uintptr_t)d_roots_b & 3) || ((uintptr_t)d_delta & 7) ||
      ((uintptr_t)d_n_nodes & 7))
    return refuse(ctx, call, "d_outboards_a, d_outboards_b, d_delta or d_n_nodes is not 8-byte aligned, or d_roots_a or d_roots_b not 4-byte aligned");
  if (ranges_meet(d_delta, delta_bytes, d_outboards_a, n_files_a ? outboards_a_bytes : 0) || ranges_meet(d_delta, delta_bytes, d_outboards_b, outboards_b_bytes))
    return refuse(ctx, call, "the blob buffer overlaps an outboard buffer");
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  DeltaPlan p;
  B3W_TRY(delta_prepare(ctx, call, host_lens_a, host_ob_first_a, d_outboards_a, outboards_a_bytes, n_files_a, host_lens_b, host_ob_first_b, outboards_b_bytes, n_files_b,
                        group_log_a, host_pair_a, host_pair_b, n_pairs, host_delta_first, delta_bytes, nullptr, nullptr, 0, false, d_scratch, scratch_bytes, st, p));
  const uint32_t per = DELTA_WG / 64;
  if (p.n_words)
    hipLaunchKernelGGL(b3w_bao_delta_mark_kernel, dim3((uint32_t)((p.n_words + per - 1) / per)), dim3(DELTA_WG), 0, st, p.tab, n_pairs, p.n_words, d_outboards_a, d_roots_a,
                       d_outboards_b, d_roots_b, group_log_a, d_delta);
  hipLaunchKernelGGL(b3w_bao_delta_count_kernel, dim3(p.wgs), dim3(HAVE_WG), 0, st, p.tab, n_pairs, p.n_words, d_delta, p.wg, p.word_rank, (uint64_t *)nullptr);
  hipLaunchKernelGGL(b3w_bao_have_scan_kernel, dim3(1), dim3(HAVE_WG), 0, st, p.wg, p.wgs, p.total);
  hipLaunchKernelGGL(b3w_bao_delta_compact_kernel, dim3(delta_grid(p, n_pairs)), dim3(DELTA_WG), 0, st, p.tab, n_pairs, p.n_words, d_outboards_b, p.wg, p.word_rank, d_delta,
                     d_n_nodes);
  return b3w_int_batch_launched(ctx, st, "bao outboard delta launch");
}

int32_t b3w_bao_outboard_delta_apply_device(b3w_ctx *ctx, const uint64_t *host_lens_a, const uint64_t *host_ob_first_a, const uint8_t *d_outboards_a,
                                            uint64_t outboards_a_bytes, const uint32_t *d_roots_a, uint32_t n_files_a, const uint64_t *host_lens_b,
                                            const uint32_t *d_roots_b, uint32_t n_files_b, uint32_t group_log, const uint32_t *host_pair_a,
                                            const uint32_t *host_pair_b, uint32_t n_pairs, const uint64_t *host_delta_first, const uint8_t *d_delta,
                                            uint64_t delta_bytes, const uint64_t *host_ob_first_out, uint8_t *d_outboards_out, uint64_t outboards_out_bytes,
                                            int32_t *d_pair_status, uint64_t *d_first_bad, void *d_scratch, uint64_t scratch_bytes, void *stream) {
  const char *call = "bao outboard delta apply";
  if (!ctx) return B3W_E_BAD_ARGUMENT;
  B3W_TRY(group_log_ok(ctx, call, group_log));
  if (!n_pairs) return B3W_OK;
  if (!host_lens_b || !d_roots_b || !host_pair_a || !host_pair_b || !host_delta_first || !d_delta || !host_ob_first_out || !d_outboards_out || !d_pair_status ||
      !d_first_bad)
    return refuse(ctx, call, "a null pointer");
  if (n_files_a && (!host_lens_a || !host_ob_first_a || !d_outboards_a || !d_roots_a)) return refuse(ctx, call, "a null pointer");
  if (((uintptr_t)d_outboards_a & 7) || ((uintptr_t)d_outboards_out & 7) || ((uintptr_t)d_roots_a & 3) || ((uintptr_t)d_roots_b & 3) || ((uintptr_t)d_delta & 7) ||
      ((uintptr_t)d_first_bad & 7) || ((uintptr_t)d_pair_status & 3))
    return refuse(ctx, call, "d_outboards_a, d_outboards_out, d_delta or d_first_bad is not 8-byte aligned, or d_roots_a, d_roots_b or d_pair_status not 4-byte aligned");
  if (ranges_meet(d_outboards_out, outboards_out_bytes, d_delta, delta_bytes)) return refuse(ctx, call, "the output buffer overlaps the blob buffer");
  const bool in_place = ranges_meet(d_outboards_out, outboards_out_bytes, d_outboards_a, n_files_a ? outboards_a_bytes : 0);
  ON_DEVICE(ctx);
  hipStream_t st = (hipStream_t)stream;
  DeltaPlan p;
  B3W_TRY(delta_prepare(ctx, call, host_lens_a, host_ob_first_a, d_outboards_a, outboards_a_bytes, n_files_a, host_lens_b, nullptr, 0, n_files_b, group_log, host_pair_a,
                        host_pair_b, n_pairs, host_delta_first, delta_bytes, host_ob_first_out, d_outboards_out, outboards_out_bytes, in_place, d_scratch, scratch_bytes,
                        st, p));
  hipLaunchKernelGGL(b3w_bao_delta_count_kernel, dim3(p.wgs), dim3(HAVE_WG), 0, st, p.tab, n_pairs, p.n_words, d_delta, p.wg, p.word_rank, p.keys);
  hipLaunchKernelGGL(b3w_bao_have_scan_kernel, dim3(1), dim3(HAVE_WG), 0, st, p.wg, p.wgs, p.total);
  hipLaunchKernelGGL(b3w_bao_delta_check_kernel, dim3(delta_grid(p, n_pairs)), dim3(DELTA_WG), 0, st, p.tab, n_pairs, p.n_words, d_outboards_a, d_roots_a, d_roots_b,
                     group_log, d_delta, p.wg, p.word_rank, reinterpret_cast<unsigned long long *>(p.keys));
  hipLaunchKernelGGL(b3w_bao_delta_write_kernel, dim3(delta_grid(p, n_pairs)), dim3(DELTA_WG), 0, st, p.tab, n_pairs, p.n_words, d_outboards_a, group_log, d_delta, p.wg,
                     p.word_rank, p.keys, d_outboards_out, d_pair_status, d_first_bad);
  return b3w_int_batch_launched(ctx, st, "bao outboard delta apply launch");
}

}  // extern "C"
