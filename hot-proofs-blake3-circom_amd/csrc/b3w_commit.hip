// b3w_commit.hip — on-device consumer #2: Pedersen commitments of witness bodies where they lie in HBM.
//
// What arecibo does with a step witness right after `synthesize` (rust_fold/src/main.rs:166-179
// -> RecursiveSNARK::prove_step -> commit to W): C = sum_i w_i * G_i over the group whose scalar field is the
// circuit's field — BN254 G1 for the bn128 builds, the Vesta curve for the --prime vesta build (y^2 = x^3 + b, a = 0).
// The generators are the caller's (arecibo derives its commitment key from a label; pass that key), so the result
// is comparable with the prover's own commitment; tests check it against an independent big-integer implementation.
//
// The witness is almost all bits: of 24 093 compression slots ~23 500 hold 0 or 1, the rest 32/34-bit words (nova:
// plus 67 256-bit inverses).  So the multi-scalar multiplication is turned into "add precomputed points":
//   set-up   every slot is cut into its bits ("virtual slots": slot, bit k; V = 53 k compression, 58 k nova O2) with
//            the point 2^k * G_slot each (b3w_commit_setup_kernel); W = 12 consecutive virtual slots form a WINDOW whose
//            4 095 non-empty subset sums are tabulated (b3w_commit_window_kernel: 4.5 k windows x 4 095 affine points = 1.2 GB; or W = 16:
//            3.3 k windows x 65 535 points = 14 GB);
//   commit   32 or 64 lanes per witness: they stream the body once and pack its virtual-slot bits into LDS (records mode:
//            the same bits from the witness's 3.7-11 KB TRACE image — no body at all); lane t then owns
//            windows t, t + T, ...: it skips ahead to its next NON-ZERO window and the wave does one mixed (XYZZ +
//            affine) addition with the tabulated point — no doublings, one addition per W slots, no zero work in lock
//            step; an LDS tree shared by the workgroup's witnesses adds the partial sums; a second kernel normalises them, one thread per witness
//            (Fermat inversion), and stores the affine points.
// Arithmetic: 256-bit Montgomery, modulus passed at run time.  The per-slot doubling chains of the set-up use the textbook
// CIOS on eight 32-bit limbs; the table, commit and normalise kernels use nine 29-bit limbs (radix 2^261, lazy reduction: see the
// F9 section of b3w_commit_arith.h), in which a limb product is a single v_mad_u64_u32.  Complete handling of the exceptional cases
// (infinity, P + P, P - P) so that related generators cannot break it.  The arithmetic itself lives in b3w_commit_arith.h, which
// the host can compile too (tests/commit_arith_harness.cpp).
// Domain: bodies of the batch kernels (every bit slot holds 0 or 1, words fit their slot's width); a slot holding
// anything else (e.g. a body of the exact kernel with a 254-bit input) flags the witness (status 103) instead of
// producing a wrong commitment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "b3w_kernels.h"
#include "b3w_atoms.h"
#include "b3w_commit_arith.h"

namespace {

__device__ __forceinline__ Fp load_fp(const uint32_t *p) {
  const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
  Fp r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void store_fp(uint32_t *p, const Fp &v) {
  reinterpret_cast<uint4 *>(p)[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  reinterpret_cast<uint4 *>(p)[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// ---- set-up: points[first_v[s] + k] = 2^k * G_s (affine, Montgomery radix 2^261, eight 32-bit words) for every committed slot s.
// One workgroup per slot, thread t takes bits t, t + 64, ...: t doublings to get there (a single thread walking all 256
// bits of a field-element slot, with an inversion per bit, was the whole key set-up time of the 12-bit tables).
__global__ __launch_bounds__(64) void b3w_commit_setup_kernel(const uint32_t *__restrict__ gens /* nslots x 16 words, standard form */,
                                                              const uint32_t *__restrict__ first_v, const uint32_t *__restrict__ nbits,
                                                              uint32_t nslots, uint32_t *__restrict__ points, B3wCurve C) {
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  if (s >= nslots) return;
  const uint32_t nb = nbits[s], v0 = first_v[s];
  if (t >= nb) return;
  Fp r2;
#pragma unroll
  for (int i = 0; i < 8; ++i) r2.l[i] = C.r2[i];
  Jac P;
  P.X = fp_mul(load_fp(gens + (uint64_t)s * 16), r2, C);
  P.Y = fp_mul(load_fp(gens + (uint64_t)s * 16 + 8), r2, C);
#pragma unroll
  for (int i = 0; i < 8; ++i) P.Z.l[i] = C.one[i];
  Fp c32;                                                 // 32 in Montgomery form: the other kernels' radix is 2^261
#pragma unroll
  for (int k = 0; k < 8; ++k) c32.l[k] = C.one[k];
#pragma unroll 1
  for (int k = 0; k < 5; ++k) c32 = fp_dbl(c32, C);
#pragma unroll 1
  for (uint32_t i = 0; i < t; ++i) P = jac_dbl(P, C);
#pragma unroll 1
  for (uint32_t k = t; k < nb; k += 64) {
    Fp x, y;
    if (k == 0) { x = P.X; y = P.Y; } else jac_to_affine(P, x, y, C);
    store_fp(points + (uint64_t)(v0 + k) * 16, fp_mul(x, c32, C));
    store_fp(points + (uint64_t)(v0 + k) * 16 + 8, fp_mul(y, c32, C));
    if (k + 64 < nb)
#pragma unroll 1
      for (int i = 0; i < 64; ++i) P = jac_dbl(P, C);
  }
}

// ---- set-up 1b (O2 nova circuits): invtab[(j * 2 + neg) * nk + mag - 1] = (+-1 / mag mod r) * G of the slot that holds the inverse of
// IsZero gadget j, for mag = 1 ... nk (affine, radix 2^261, eight 32-bit words; (0, 0) where that slot is not committed).  A step has 67
// such slots — 256 virtual bit slots, i.e. sixteen 16-bit windows each, 39 % of what a folded O2 key commits — but their values
// are 1 / k for a SMALL signed k the step's inputs determine (k = -depth, -block_count, n_blocks - 1 - block_count,
// total_depth - i - 2 - depth: circuits/blake3_nova.circom:19-23,65-72,136-144), the same 2 048-entry table of inverses the
// witness kernels use: records mode adds ONE tabulated point per gadget instead of sixteen.
// One thread per entry: 255 doublings and the additions of the scalar's bits (set-up only: 8 ms for 67 x 2 047 entries).
__global__ __launch_bounds__(64) void b3w_commit_invtab_kernel(const uint32_t *__restrict__ gens /* nslots x 16 words, standard form */,
                                                               const uint32_t *__restrict__ inv_slot /* 67: committed slot index or ~0 */,
                                                               const uint32_t *__restrict__ inverses /* 8 words per magnitude, standard form; entry 0 unused */,
                                                               uint32_t njobs, uint32_t nk, uint32_t *__restrict__ invtab, B3wCurve C) {
  const uint64_t gid = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (uint64_t)njobs * nk) return;
  const uint32_t j = (uint32_t)(gid / nk), mag = (uint32_t)(gid % nk) + 1u;
  uint32_t *o = invtab + ((uint64_t)j * 2 * nk + mag - 1u) * 16, *on = o + (uint64_t)nk * 16;        // 1 / mag, -1 / mag
  const uint32_t s = inv_slot[j];
  if (s == 0xFFFFFFFFu) { store_fp(o, fp_zero()); store_fp(o + 8, fp_zero()); store_fp(on, fp_zero()); store_fp(on + 8, fp_zero()); return; }
  Fp r2;
#pragma unroll
  for (int i = 0; i < 8; ++i) r2.l[i] = C.r2[i];
  const Fp gx = fp_mul(load_fp(gens + (uint64_t)s * 16), r2, C), gy = fp_mul(load_fp(gens + (uint64_t)s * 16 + 8), r2, C);
  const uint32_t *sc = inverses + 8ull * mag;
  Jac R = jac_infinity();
#pragma unroll 1
  for (int b = 255; b >= 0; --b) {
    R = jac_dbl(R, C);
    if ((sc[b >> 5] >> (b & 31)) & 1u) R = jac_madd(R, gx, gy, C);
  }
  Fp x, y, c32;
  jac_to_affine(R, x, y, C);
#pragma unroll
  for (int k = 0; k < 8; ++k) c32.l[k] = C.one[k];
#pragma unroll 1
  for (int k = 0; k < 5; ++k) c32 = fp_dbl(c32, C);         // 32 in Montgomery form: the commit kernel's radix is 2^261
  const Fp xo = fp_mul(x, c32, C);
  store_fp(o, xo);
  store_fp(o + 8, fp_mul(y, c32, C));
  store_fp(on, xo);
  store_fp(on + 8, fp_mul(fp_sub(fp_zero(), y, C), c32, C));
}

// ---- set-up 2: table[win * (2^W - 1) + m - 1] = sum of the window's virtual-slot points selected by the bits of m
// (affine, radix 2^261, eight 32-bit words; infinity = (0, 0)).  A thread walks K = 4 consecutive entries in Gray-code
// order — the first from scratch, each next one is the previous +/- one point — and the four share one inversion
// (Montgomery's trick), so an entry costs ~3 additions and a quarter of an inversion instead of W/2 additions and a
// whole one.  The thread's projective results and prefix products wait in LDS ([entry][limb][thread]: conflict-free).
#define B3W_WINDOW_K 4
template <int W>
__global__ __launch_bounds__(64) void b3w_commit_window_kernel(const uint32_t *__restrict__ points, uint32_t nwin,
                                                               uint32_t *__restrict__ table, B3wCurve C, B3wCurve9 C9) {
  constexpr int K = B3W_WINDOW_K;
  constexpr uint32_t CHUNKS = (1u << W) / K;                  // per window
  __shared__ uint32_t lds[5 * K * 9 * 64];                    // X, Y, ZZ, ZZZ, prefix product of the ZZ * ZZZ
  const uint32_t tid = threadIdx.x;
  const uint64_t gid = (uint64_t)blockIdx.x * 64 + tid;
  if (gid >= (uint64_t)nwin * CHUNKS) return;                 // no barriers below: every thread uses its own LDS column
  const uint32_t win = (uint32_t)(gid / CHUNKS), g0 = (uint32_t)(gid % CHUNKS) * K;
  auto at = [&](int what, int e, int l) -> uint32_t & { return lds[((what * K + e) * 9 + l) * 64 + tid]; };
  // -> false for (0, 0): a generator given as the point at infinity (or a multiple of one) adds nothing.  j9_madd leaves that
  // filter to its caller; without it (0, 0) went into the sum as if it were a point, and every entry that took it together with a
  // finite point came out off the curve (tests/test_gpu_commit_arith.py: test_infinity_among_finite_sums)
  auto point = [&](uint32_t b, bool negate, F9 &x, F9 &y) {
    const uint32_t *pt = points + (uint64_t)(win * W + b) * 16;
    const Fp px = load_fp(pt);
    Fp py = load_fp(pt + 8);
    if (fp_is_zero(px) && fp_is_zero(py)) return false;
    if (negate) py = fp_sub(fp_zero(), py, C);
    x = to29(px); y = to29(py);
    return true;
  };
  J9 acc = j9_infinity();
  const uint32_t m0 = g0 ^ (g0 >> 1);
#pragma unroll 1
  for (uint32_t b = 0; b < (uint32_t)W; ++b) {
    if (!((m0 >> b) & 1)) continue;
    F9 x, y;
    if (point(b, false, x, y)) j9_madd(acc, x, y, C9);
  }
#pragma unroll 1
  for (int e = 0; e < K; ++e) {
    if (e > 0) {                                              // Gray code: entry g differs from g - 1 in bit ctz(g)
      const uint32_t g = g0 + e, m = g ^ (g >> 1), b = (uint32_t)__builtin_ctz(g);
      F9 x, y;
      if (point(b, !((m >> b) & 1), x, y)) j9_madd(acc, x, y, C9);
    }
    const F9 A = acc.inf ? one29(C9) : mul29(acc.ZZ, acc.ZZZ, C9);      // what has to be inverted: 1/ZZ = ZZZ / A, 1/ZZZ = ZZ / A
#pragma unroll
    for (int l = 0; l < 9; ++l) {
      at(0, e, l) = acc.X.l[l]; at(1, e, l) = acc.Y.l[l];
      at(2, e, l) = acc.inf ? 0u : acc.ZZ.l[l]; at(3, e, l) = acc.inf ? 0u : acc.ZZZ.l[l];
    }
    F9 c;                                                     // prefix product of the (finite) As
    if (e == 0) c = A;
    else {
#pragma unroll
      for (int l = 0; l < 9; ++l) c.l[l] = at(4, e - 1, l);
      c = mul29(c, A, C9);
    }
#pragma unroll
    for (int l = 0; l < 9; ++l) at(4, e, l) = c.l[l];
  }
  F9 inv;
#pragma unroll
  for (int l = 0; l < 9; ++l) inv.l[l] = at(4, K - 1, l);
  inv = inv29(inv, C.pm2, C9);                                // 1 / (A_0 ... A_{K-1})
#pragma unroll 1
  for (int e = K - 1; e >= 0; --e) {
    F9 X, Y, ZZ, ZZZ, ia = inv;
    uint32_t z = 0;
#pragma unroll
    for (int l = 0; l < 9; ++l) { X.l[l] = at(0, e, l); Y.l[l] = at(1, e, l); ZZ.l[l] = at(2, e, l); ZZZ.l[l] = at(3, e, l); z |= ZZ.l[l]; }
    if (z) {                                                  // finite: it took part in the product
      if (e > 0) {
        F9 c;
#pragma unroll
        for (int l = 0; l < 9; ++l) c.l[l] = at(4, e - 1, l);
        ia = mul29(inv, c, C9);                               // 1 / A_e
      }
      inv = mul29(inv, mul29(ZZ, ZZZ, C9), C9);
    }
    const uint32_t g = g0 + e, m = g ^ (g >> 1);
    if (m == 0) continue;                                     // the empty subset has no entry
    Fp x = fp_zero(), y = fp_zero();
    if (z) {
      uint32_t hi;
      x = from29(mul29(X, mul29(ia, ZZZ, C9), C9), hi); x = fp_reduce_once(x, hi, C);
      y = from29(mul29(Y, mul29(ia, ZZ, C9), C9), hi); y = fp_reduce_once(y, hi, C);
    }
    uint32_t *o = table + ((uint64_t)win * B3W_COMMIT_ENTRIES(W) + m - 1) * 16;
    store_fp(o, x);
    store_fp(o + 8, y);
  }
}

// ---- commit: T lanes per witness.
//   phase 1  the lanes stream the body once (coalesced, 32 bytes per lane and step) and assemble the witness's
//            virtual-slot bits as one bit string in LDS (bit v = virtual slot v; 6.7 KB for the compression circuit);
//            the domain check lives here, where every word of an element is at hand anyway.  This phase waits on HBM,
//            the next one on the ALU: waves of different workgroups in different phases share a SIMD and overlap.
//            (Gathering the bits window by window — 12-16 dependent scattered loads each — cost 43 % of the kernel;
//            as a separate streaming kernel in front, 30 %.)
//   phase 2  lane t adds the tabulated points of the witness's non-zero windows t, t + T, ...
//   phase 3  LDS tree over the T partial sums (in the bit string's place).
template <int T, int WPB, int W, class CV>        // threads per witness, witnesses per workgroup (T * WPB threads), window width, field
__global__ __launch_bounds__(T * WPB) __attribute__((amdgpu_waves_per_eu(3, 3))) void b3w_commit_kernel(const uint8_t *__restrict__ bodies, uint32_t n, uint64_t pitch,
                                                         uint32_t first_slot, uint32_t nslots,
                                                         const uint32_t *__restrict__ slotdesc /* per committed slot: first virtual slot | width code << 24 */,
                                                         const uint32_t *__restrict__ images /* or null: TRACE images, word j of witness w at [j * img_row + w] */,
                                                         uint32_t img_row, const uint2 *__restrict__ runs, uint32_t nruns,
                                                         uint32_t region_words /* LDS words per witness: max(bit string, 36 T) */,
                                                         const uint32_t *__restrict__ table /* radix 2^261 */, uint32_t nwin,
                                                         uint32_t *__restrict__ sums /* n x B3W_COMMIT_SUM_WORDS: X Y ZZ ZZZ in 29-bit limbs */,
                                                         int32_t *__restrict__ status,
                                                         const uint32_t *__restrict__ invtab /* or null: the O2 nova circuits' inverse points, b3w_commit_invtab_kernel */,
                                                         uint32_t inv_nk, const uint32_t *__restrict__ invmeta /* bodies mode: gadget slots, input slots, first virtual slots */,
                                                         const uint32_t *__restrict__ aux /* bodies mode: the prime, then 1 / k as scalars */,
                                                         unsigned long long *__restrict__ adds /* or null: += mixed additions of phase 2 (b3w_commit_key_counts) */, CV C) {
  extern __shared__ uint32_t lds[];
  __shared__ uint32_t bad[WPB];
  // invtab: per IsZero gadget of the step 0 = nothing to add (k = 0: the inverse is 0; or a rejected step), +-mag = the tabulated
  // point of 1 / k (both signs are in the table), INV_WINDOWS = k beyond the table: the slot's bits go through the windows like any other slot's
  constexpr int32_t INV_WINDOWS = (int32_t)0x80000000;
  __shared__ int32_t kinv[WPB][B3W_NOVA_ISZERO];
  const uint32_t sub = threadIdx.x / T, t = threadIdx.x % T;       // which witness of the workgroup, lane within it
  const uint32_t w = blockIdx.x * WPB + sub;
  const bool live = w < n;
  uint32_t *packed = lds + sub * region_words;
  for (uint32_t i = t; i < region_words; i += T) packed[i] = 0;
  if (t == 0) bad[sub] = 0;
  if (images && invtab) {
    const uint32_t *img = images + (live ? w : 0);
    const bool ok = live && img[(uint64_t)B3W_LDS_OKWORD * img_row] != 0;
    for (uint32_t j = t; j < B3W_NOVA_ISZERO; j += T) {        // the gadgets' arguments, as the TRACE phase of the witness kernel derives them
      const int64_t depth = img[(uint64_t)(B3W_LDS_NV + NV_DEPTH) * img_row];
      int64_t k;
      if (j == 0) k = -depth;
      else if (j == 1) k = -(int64_t)img[(uint64_t)(B3W_LDS_NV + NV_BLOCK_COUNT) * img_row];
      else if (j == 2) k = (int64_t)img[(uint64_t)(B3W_LDS_NV + NV_N_BLOCKS) * img_row] - 1 - (int64_t)img[(uint64_t)(B3W_LDS_NV + NV_BLOCK_COUNT) * img_row];
      else k = (int64_t)img[(uint64_t)(B3W_LDS_NV + NV_TOTAL_DEPTH) * img_row] - (int64_t)(j - 3) - 2 - depth;
      const uint64_t mag = k < 0 ? (uint64_t)(-k) : (uint64_t)k;
      kinv[sub][j] = !ok || mag == 0 ? 0 : mag > inv_nk ? INV_WINDOWS : k < 0 ? -(int32_t)mag : (int32_t)mag;
    }
  } else if (!images) {
    // bodies mode: the same arguments from the body's four input slots — and the point is taken only if the body's inverse slot
    // IS +-1 / k (the context's scalar table), whatever the rest of the body says; everything else goes through the windows
    const uint4 *wbody = reinterpret_cast<const uint4 *>(bodies + (uint64_t)(live ? w : 0) * pitch);
    uint32_t inw[4] = {0, 0, 0, 0};
    bool words = live && invtab != nullptr;
    if (words)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t sidx = invmeta[B3W_NOVA_ISZERO + q];
        const uint4 a = wbody[(uint64_t)sidx * 2], b = wbody[(uint64_t)sidx * 2 + 1];
        inw[q] = a.x;
        words = words && !(a.y | a.z | a.w | b.x | b.y | b.z | b.w);
      }
    for (uint32_t j = t; j < B3W_NOVA_ISZERO; j += T) {
      int32_t res = INV_WINDOWS;
      const uint32_t sl = words ? invmeta[j] : 0xFFFFFFFFu;
      const int64_t depth = inw[3];
      const int64_t k = j == 0 ? -depth : j == 1 ? -(int64_t)inw[1] : j == 2 ? (int64_t)inw[0] - 1 - (int64_t)inw[1] : (int64_t)inw[2] - (int64_t)(j - 3) - 2 - depth;
      const uint64_t mag = k < 0 ? (uint64_t)(-k) : (uint64_t)k;
      if (sl != 0xFFFFFFFFu && mag <= inv_nk) {
        const uint4 va = wbody[((uint64_t)first_slot + sl) * 2], vb = wbody[((uint64_t)first_slot + sl) * 2 + 1];
        const uint32_t v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
        uint32_t diff = 0;
        if (mag == 0) {                                        // IsZero(0): the inverse slot holds 0 — nothing to add
#pragma unroll
          for (int i = 0; i < 8; i++) diff |= v[i];
          if (!diff) res = 0;
        } else {
          const uint32_t *e = aux + 16 + 8 * mag;              // 1 / mag; a negative argument's inverse is p - 1 / mag
          uint64_t br = 0;
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)aux[i] - e[i] - br;
            br = (d >> 63) & 1;
            diff |= v[i] ^ (k < 0 ? (uint32_t)d : e[i]);
          }
          if (!diff) res = k < 0 ? -(int32_t)mag : (int32_t)mag;
        }
      }
      kinv[sub][j] = res;
    }
  }
  __syncthreads();
  if (images) {
    // records mode: the witness is an expansion of its TRACE image (3.7-11 KB) through the slot table, so its bits are
    // pieces of image words: run r = `len` bits of image word `src` from bit `sh` on, at bit v0 of the bit string
    const uint32_t *img = images + (live ? w : 0);
    const bool ok = live && img[(uint64_t)B3W_LDS_OKWORD * img_row] != 0;              // a rejected step leaves the string empty
    for (uint32_t r = t; r < nruns; r += T) {
      const uint2 e = runs[r];
      if (invtab) {                                          // an inverse whose point is tabulated stays out of the bit string
        const uint32_t src = e.y & 0xFFFFu;
        if (src >= B3W_LDS_WIDE && src < B3W_LDS_WIDE + 8u * B3W_NOVA_ISZERO && kinv[sub][(src - B3W_LDS_WIDE) >> 3] != INV_WINDOWS) continue;
      }
      const uint32_t len = (e.x >> 24) + 1u, x = ok ? img[(uint64_t)(e.y & 0xFFFFu) * img_row] >> (e.y >> 16) : 0u;
      const uint32_t piece = len == 32 ? x : x & ((1u << len) - 1u);
      if (piece) {
        const uint32_t v = e.x & 0xFFFFFFu;
        atomicOr(&packed[v >> 5], piece << (v & 31));
        if (v & 31) atomicOr(&packed[(v >> 5) + 1], piece >> (32 - (v & 31)));
      }
    }
  } else {
    const uint4 *body = reinterpret_cast<const uint4 *>(bodies + (uint64_t)(live ? w : 0) * pitch) + (uint64_t)first_slot * 2;
    auto put32 = [&](uint32_t v, uint32_t x) {
      if (!x) return;
      atomicOr(&packed[v >> 5], x << (v & 31));
      if (v & 31) atomicOr(&packed[(v >> 5) + 1], x >> (32 - (v & 31)));
    };
    const uint64_t mine = T == 64 ? ~0ull : (threadIdx.x & 32) ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;   // my witness's lanes of the wave
    bool wrong = false;
    constexpr int U = 8;                                        // steps in flight: 8 x (32 + 4) bytes per lane
#pragma unroll 1
    for (uint32_t s0 = 0; s0 < nslots; s0 += T * U) {
      uint4 a[U], b[U];
      uint32_t d[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t sl = s0 + u * T + t;
        a[u] = make_uint4(0, 0, 0, 0); b[u] = a[u]; d[u] = 0xFFFFFFFFu;          // code 255: not a slot
        if (live && sl < nslots) { a[u] = body[(uint64_t)sl * 2]; b[u] = body[(uint64_t)sl * 2 + 1]; d[u] = slotdesc[sl]; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t v0 = d[u] & 0xFFFFFFu, code = d[u] >> 24, hi = b[u].x | b[u].y | b[u].z | b[u].w;
        const uint32_t vbase = __shfl(v0, 0, T);
        const uint64_t run = __ballot(code == 0 && v0 == vbase + t), ones = __ballot(a[u].x & 1);
        if ((run & mine) == mine) {                             // T consecutive bit slots: one ballot
          wrong |= a[u].x > 1 || (a[u].y | a[u].z | a[u].w | hi);
          if (t == 0) {
            const uint64_t mk = T == 64 ? ones : (threadIdx.x & 32) ? ones >> 32 : ones & 0xFFFFFFFFull;
            put32(vbase, (uint32_t)mk);
            if (T == 64) put32(vbase + 32, (uint32_t)(mk >> 32));
          }
        } else if (code == 0) { wrong |= a[u].x > 1 || (a[u].y | a[u].z | a[u].w | hi); put32(v0, a[u].x & 1); }
        else if (code == 1) { wrong |= (a[u].y | a[u].z | a[u].w | hi) != 0; put32(v0, a[u].x); }
        else if (code == 2) { wrong |= (a[u].z | a[u].w | hi) != 0; put32(v0, a[u].x); put32(v0 + 32, a[u].y); }
        else if (code == 3) { put32(v0, a[u].x); put32(v0 + 32, a[u].y); put32(v0 + 64, a[u].z); put32(v0 + 96, a[u].w);
                              put32(v0 + 128, b[u].x); put32(v0 + 160, b[u].y); put32(v0 + 192, b[u].z); put32(v0 + 224, b[u].w); }
        else if (code == 5) {                                  // a nova inverse slot (v0 = the gadget): tabulated, or eight words like any 256-bit slot
          if (kinv[sub][v0] == INV_WINDOWS) {
            const uint32_t vv = invmeta ? invmeta[B3W_NOVA_ISZERO + 4 + v0] : 0u;
            put32(vv, a[u].x); put32(vv + 32, a[u].y); put32(vv + 64, a[u].z); put32(vv + 96, a[u].w);
            put32(vv + 128, b[u].x); put32(vv + 160, b[u].y); put32(vv + 192, b[u].z); put32(vv + 224, b[u].w);
          }
        }
        else if (code >= 8 && code < 40) { wrong |= (a[u].y | a[u].z | a[u].w | hi) != 0; put32(v0, (a[u].x >> (code - 8)) & 1u); }   // folded key: one bit of a word
        // (code 4: a slot folded into others' generators — nothing to add)
      }
    }
    if (wrong) bad[sub] = 1;
  }
  __syncthreads();
  J9 acc = j9_infinity();
  uint32_t win = live ? t : nwin, nadd = 0;
  while (true) {
    // skip ahead to this lane's next window with a set bit
    uint32_t m = 0;
    while (win < nwin) {
      if (W == 16) m = (packed[win >> 1] >> ((win & 1) * 16)) & 0xFFFFu;
      else {
        const uint32_t bit = win * W;
        m = (uint32_t)(((((uint64_t)packed[(bit >> 5) + 1]) << 32 | packed[bit >> 5]) >> (bit & 31)) & ((1u << W) - 1u));
      }
      if (m) break;
      win += T;
    }
    const bool has = win < nwin;
    if (!__any(has)) break;
    if (has) {
      const uint32_t *pt = table + ((uint64_t)win * B3W_COMMIT_ENTRIES(W) + m - 1) * 16;
      const Fp x2 = load_fp(pt), y2 = load_fp(pt + 8);
      if (!(fp_is_zero(x2) && fp_is_zero(y2))) {           // (0, 0) is not on these curves (b != 0): the table's infinity
        j9_madd(acc, to29(x2), to29(y2), C);
        nadd++;
      }
      win += T;
    }
  }
  if (invtab && live)
    for (uint32_t j = t; j < B3W_NOVA_ISZERO; j += T) {        // one tabulated point per IsZero gadget (y negated for a negative argument)
      const int32_t kc = kinv[sub][j];
      if (kc == 0 || kc == INV_WINDOWS) continue;
      const uint32_t *pt = invtab + (((uint64_t)j * 2 + (kc < 0 ? 1u : 0u)) * inv_nk + (uint32_t)(kc < 0 ? -kc : kc) - 1u) * 16;
      const Fp x2 = load_fp(pt), y2 = load_fp(pt + 8);
      if (fp_is_zero(x2) && fp_is_zero(y2)) continue;          // (the gadget's slot is not committed)
      j9_madd(acc, to29(x2), to29(y2), C);
      nadd++;
    }
  if (adds) {                                                // (uniform: a statistics pass, b3w_commit_key_count)
    for (int o = 32; o >= 1; o >>= 1) nadd += __shfl_xor(nadd, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(adds, (unsigned long long)nadd);
  }
  __syncthreads();                                           // every lane is done with the bit string: the tree takes its place
  // LDS tree over each witness's T partial sums (infinity travels as ZZ = 0).  The additions of all WPB witnesses of a
  // level are dealt to the first threads of the workgroup, so whole waves drop out instead of running half empty
  // (one witness per wave spent 6 nearly empty wave-wide additions here: 10 % of the kernel).
  auto put = [&](uint32_t *dst, const J9 &a) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { dst[i] = a.X.l[i]; dst[9 + i] = a.Y.l[i]; dst[18 + i] = a.inf ? 0u : a.ZZ.l[i]; dst[27 + i] = a.inf ? 0u : a.ZZZ.l[i]; }
  };
  auto get = [&](const uint32_t *src) {
    J9 a;
    uint32_t z = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { a.X.l[i] = src[i]; a.Y.l[i] = src[9 + i]; a.ZZ.l[i] = src[18 + i]; a.ZZZ.l[i] = src[27 + i]; z |= src[18 + i]; }
    a.inf = z == 0;
    return a;
  };
  put(packed + t * 36, acc);
  __syncthreads();
  for (uint32_t st = T / 2; st >= 1; st >>= 1) {
    if (threadIdx.x < WPB * st) {
      uint32_t *m = lds + (threadIdx.x / st) * region_words + (threadIdx.x % st) * 36;
      J9 a = get(m);
      j9_add(a, get(m + st * 36), C);
      put(m, a);
    }
    __syncthreads();
  }
  if (live) for (uint32_t i = t; i < 36; i += T) sums[(uint64_t)w * B3W_COMMIT_SUM_WORDS + i] = packed[i];   // normalised by the next kernel
  if (live && t == 0 && status) status[w] = bad[sub] ? 103 : 0;
}

// ---- normalise: one THREAD per witness (a Fermat inversion is 380 dependent multiplications: on thread 0 of the commit
// workgroup it took longer than the workgroup's whole share of additions); affine, standard form, 64 bytes per point
template <class CV>
__global__ __launch_bounds__(64) void b3w_commit_normalize_kernel(const uint32_t *__restrict__ sums, uint32_t n, uint8_t *__restrict__ out,
                                                                  B3wCurve C, CV C9) {
  const uint32_t w = blockIdx.x * 64 + threadIdx.x;
  if (w >= n) return;
  F9 co[4];                                                  // X, Y, ZZ, ZZZ (tidy < 2p)
  uint32_t z = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 9; ++i) co[c].l[i] = sums[(uint64_t)w * B3W_COMMIT_SUM_WORDS + c * 9 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) z |= co[2].l[i];
  Fp x = fp_zero(), y = fp_zero();                           // infinity -> (0, 0)
  if (z) {
    const F9 ia = inv29(mul29(co[2], co[3], C9), C.pm2, C9);  // 1 / (ZZ * ZZZ): 1/ZZ = ZZZ * ia, 1/ZZZ = ZZ * ia
    F9 unit;
#pragma unroll
    for (int i = 0; i < 9; ++i) unit.l[i] = i == 0 ? 1u : 0u;
    const F9 xs = mul29(mul29(co[0], mul29(ia, co[3], C9), C9), unit, C9);    // out of Montgomery form: < 2p
    const F9 ys = mul29(mul29(co[1], mul29(ia, co[2], C9), C9), unit, C9);
    uint32_t hi;
    x = from29(xs, hi); x = fp_reduce_once(x, hi, C);
    y = from29(ys, hi); y = fp_reduce_once(y, hi, C);
  }
  uint32_t *o = reinterpret_cast<uint32_t *>(out + (uint64_t)w * 64);
  store_fp(o, x);
  store_fp(o + 8, y);
}

// ---- normalise MANY: a thread takes B3W_NORMALIZE_K consecutive witnesses and inverts the product of their ZZ * ZZZ once
// (Montgomery's trick, as the window kernel above): 95 + 14 multiplications a witness instead of 390, and — the point — launched once
// for all the witnesses of a pass it fills the machine, where the per-batch launch was a chain of dependent multiplications on one
// wave per CU.  The sums are read twice (144 bytes a witness).
#define B3W_NORMALIZE_K 4
template <class CV>
__global__ __launch_bounds__(64) void b3w_commit_normalize_many_kernel(const uint32_t *__restrict__ sums, uint64_t n, uint8_t *__restrict__ out,
                                                                       B3wCurve C, CV C9) {
  constexpr int K = B3W_NORMALIZE_K;
  const uint64_t w0 = ((uint64_t)blockIdx.x * 64 + threadIdx.x) * K;
  if (w0 >= n) return;
  auto coord = [&](uint64_t w, int c) {
    F9 v;
#pragma unroll
    for (int i = 0; i < 9; ++i) v.l[i] = sums[w * B3W_COMMIT_SUM_WORDS + c * 9 + i];
    return v;
  };
  auto is_zero = [](const F9 &v) { uint32_t z = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) z |= v.l[i];
    return z == 0; };
  F9 pre[K];                                                 // prefix products of the finite witnesses' ZZ * ZZZ (infinity: the product so far)
#pragma unroll
  for (int e = 0; e < K; ++e) {
    const uint64_t w = w0 + e;
    F9 a = one29(C9);
    if (w < n) {
      const F9 zz = coord(w, 2);
      if (!is_zero(zz)) a = mul29(zz, coord(w, 3), C9);
    }
    pre[e] = e == 0 ? a : mul29(pre[e - 1], a, C9);
  }
  F9 inv = inv29(pre[K - 1], C.pm2, C9);                      // 1 / (A_0 ... A_{K-1})
  F9 unit;
#pragma unroll
  for (int i = 0; i < 9; ++i) unit.l[i] = i == 0 ? 1u : 0u;
#pragma unroll
  for (int e = K - 1; e >= 0; --e) {
    const uint64_t w = w0 + e;
    if (w >= n) continue;                                      // (its A was one: nothing to take out of `inv`)
    const F9 zz = coord(w, 2);
    Fp x = fp_zero(), y = fp_zero();                           // infinity -> (0, 0)
    if (!is_zero(zz)) {
      const F9 zzz = coord(w, 3);
      const F9 ia = e > 0 ? mul29(inv, pre[e - 1], C9) : inv;  // 1 / A_e
      inv = mul29(inv, mul29(zz, zzz, C9), C9);
      const F9 xs = mul29(mul29(coord(w, 0), mul29(ia, zzz, C9), C9), unit, C9);    // 1 / ZZ = ZZZ / A; out of Montgomery form: < 2p
      const F9 ys = mul29(mul29(coord(w, 1), mul29(ia, zz, C9), C9), unit, C9);     // 1 / ZZZ = ZZ / A
      uint32_t hi;
      x = from29(xs, hi); x = fp_reduce_once(x, hi, C);
      y = from29(ys, hi); y = fp_reduce_once(y, hi, C);
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(out + w * 64);
    store_fp(o, x);
    store_fp(o + 8, y);
  }
}

}  // namespace

extern "C" int b3w_launch_commit_setup(const uint32_t *d_gens, const uint32_t *d_first_v, const uint32_t *d_nbits, uint32_t nslots,
                                       uint32_t *d_points, const B3wCurve *curve, hipStream_t stream) {
  if (!nslots) return 0;
  hipLaunchKernelGGL(b3w_commit_setup_kernel, dim3(nslots), dim3(64), 0, stream, d_gens, d_first_v, d_nbits, nslots, d_points, *curve);
  return (int)hipGetLastError();
}

extern "C" int b3w_launch_commit_windows(const uint32_t *d_points, uint32_t nwin, uint32_t window, uint32_t *d_table, const B3wCurve *curve, hipStream_t stream) {
  if (!nwin) return 0;
  if (!B3W_COMMIT_WINDOW_OK(window)) return (int)hipErrorInvalidValue;
  const uint64_t total = (uint64_t)nwin * ((1u << window) / B3W_WINDOW_K);      // threads: B3W_WINDOW_K entries each
  const dim3 grid((uint32_t)((total + 63) / 64));
  const B3wCurve9 c9 = make_curve9(*curve);
  if (window == B3W_COMMIT_WINDOW_XL)
    hipLaunchKernelGGL(b3w_commit_window_kernel<B3W_COMMIT_WINDOW_XL>, grid, dim3(64), 0, stream, d_points, nwin, d_table, *curve, c9);
  else if (window == B3W_COMMIT_WINDOW_LARGE)
    hipLaunchKernelGGL(b3w_commit_window_kernel<B3W_COMMIT_WINDOW_LARGE>, grid, dim3(64), 0, stream, d_points, nwin, d_table, *curve, c9);
  else
    hipLaunchKernelGGL(b3w_commit_window_kernel<B3W_COMMIT_WINDOW_SMALL>, grid, dim3(64), 0, stream, d_points, nwin, d_table, *curve, c9);
  return (int)hipGetLastError();
}

extern "C" int b3w_launch_commit(const uint8_t *d_bodies, uint32_t n, uint64_t pitch, uint32_t first_slot, uint32_t nslots,
                                 const uint32_t *d_slotdesc, const uint32_t *d_images /* or null */, uint32_t img_row, const uint32_t *d_runs,
                                 uint32_t nruns, const uint32_t *d_table, uint32_t nwin, uint32_t window,
                                 uint32_t *d_sums /* n * B3W_COMMIT_SUM_WORDS scratch */, uint8_t *d_out, int32_t *d_status,
                                 const uint32_t *d_invtab, uint32_t inv_nk, const uint32_t *d_invmeta, const uint32_t *d_aux,
                                 unsigned long long *d_adds, const B3wCurve *curve, hipStream_t stream) {
  if (!n) return 0;
  if (!d_images && !(d_invtab && d_invmeta && d_aux)) { d_invtab = nullptr; d_invmeta = nullptr; }      // (bodies mode needs all three)
  if (!B3W_COMMIT_WINDOW_OK(window)) return (int)hipErrorInvalidValue;
  const uint32_t bits_words = (nwin * window + 31) / 32 + 2;   // one packed witness in LDS (nova O1: 13.5 KB)
  if (bits_words * 4 > 32 * 1024) return (int)hipErrorInvalidValue;
  const B3wCurve9 c9 = make_curve9(*curve);
  // lanes per witness: 32 (two witnesses per wave) for small batches of the compression circuit, 64 for large ones and for
  // the longer nova witnesses (measured at both window widths).  Virtual slots: 53 k compression, 58 k nova O2, 108 k nova O1.
  static const int env_tpw = getenv("B3W_COMMIT_THREADS") ? atoi(getenv("B3W_COMMIT_THREADS")) : 0;
  const int tpw = window > B3W_COMMIT_WINDOW_LARGE ? 64 : env_tpw ? env_tpw : ((uint64_t)nwin * window > 55200 || n >= 8192) ? 64 : 32;
  bool vesta = true;                                           // the modulus with compile-time limbs?
  for (int i = 0; i < 9; ++i) vesta = vesta && c9.p[i] == B3wCurve9Vesta::P(i);
  vesta = vesta && c9.inv == B3wCurve9Vesta::INV() && tpw == 64;
  B3wCurve9Vesta c9v;
  static_cast<B3wCurve9 &>(c9v) = c9;
#define B3W_COMMIT_LAUNCH(T, WPB, W, CV, cv)                                                                              \
  {                                                                                                                       \
    const uint32_t region = bits_words > 36u * T ? bits_words : 36u * T;                                                  \
    if ((size_t)region * WPB * 4 > 64 * 1024) return (int)hipErrorInvalidValue;   /* LDS of one workgroup (nova O1: 54 KB) */ \
    hipLaunchKernelGGL((b3w_commit_kernel<T, WPB, W, CV>), dim3((n + WPB - 1) / WPB), dim3(T * WPB), region * WPB * 4, stream, d_bodies, n, \
                       pitch, first_slot, nslots, d_slotdesc, d_images, img_row, reinterpret_cast<const uint2 *>(d_runs), nruns, region, d_table, nwin, \
                       d_sums, d_status, d_invtab, inv_nk, d_invmeta, d_aux, d_adds, cv);                                         \
  }
  if (window == B3W_COMMIT_WINDOW_XL) {                        // (the wide table: 64 lanes a witness only)
    if (vesta) B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_XL, B3wCurve9Vesta, c9v)
    else B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_XL, B3wCurve9, c9)
  } else if (window == B3W_COMMIT_WINDOW_LARGE) {
    if (vesta) B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_LARGE, B3wCurve9Vesta, c9v)
    else if (tpw == 64) B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_LARGE, B3wCurve9, c9)
    else B3W_COMMIT_LAUNCH(32, 2, B3W_COMMIT_WINDOW_LARGE, B3wCurve9, c9)
  } else {
    if (vesta) B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_SMALL, B3wCurve9Vesta, c9v)
    else if (tpw == 64) B3W_COMMIT_LAUNCH(64, 4, B3W_COMMIT_WINDOW_SMALL, B3wCurve9, c9)
    else B3W_COMMIT_LAUNCH(32, 2, B3W_COMMIT_WINDOW_SMALL, B3wCurve9, c9)
  }
#undef B3W_COMMIT_LAUNCH
  if (!d_out) return (int)hipGetLastError();                  // (the sums are normalised later: b3w_launch_commit_normalize)
  if (vesta) hipLaunchKernelGGL(b3w_commit_normalize_kernel<B3wCurve9Vesta>, dim3((n + 63) / 64), dim3(64), 0, stream, d_sums, n, d_out, *curve, c9v);
  else hipLaunchKernelGGL(b3w_commit_normalize_kernel<B3wCurve9>, dim3((n + 63) / 64), dim3(64), 0, stream, d_sums, n, d_out, *curve, c9);
  return (int)hipGetLastError();
}

extern "C" int b3w_launch_commit_normalize(const uint32_t *d_sums, uint64_t n, uint8_t *d_out, const B3wCurve *curve, hipStream_t stream) {
  if (!n) return 0;
  const B3wCurve9 c9 = make_curve9(*curve);
  const uint64_t threads = (n + B3W_NORMALIZE_K - 1) / B3W_NORMALIZE_K;
  hipLaunchKernelGGL(b3w_commit_normalize_many_kernel<B3wCurve9>, dim3((uint32_t)((threads + 63) / 64)), dim3(64), 0, stream, d_sums, n, d_out, *curve, c9);
  return (int)hipGetLastError();
}

extern "C" int b3w_launch_commit_invtab(const uint32_t *d_gens, const uint32_t *d_inv_slot, const uint32_t *d_inverses, uint32_t njobs, uint32_t nk,
                                        uint32_t *d_invtab, const B3wCurve *curve, hipStream_t stream) {
  if (!njobs || !nk) return 0;
  const uint64_t total = (uint64_t)njobs * nk;
  hipLaunchKernelGGL(b3w_commit_invtab_kernel, dim3((uint32_t)((total + 63) / 64)), dim3(64), 0, stream, d_gens, d_inv_slot, d_inverses, njobs, nk, d_invtab,
                     *curve);
  return (int)hipGetLastError();
}
