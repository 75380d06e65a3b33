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
