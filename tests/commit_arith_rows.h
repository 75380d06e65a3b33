// commit_arith_rows.h — one row of the arithmetic table: apply ONE routine of csrc/b3w_commit_arith.h to the operands of a row and
// write its raw result.  Test infrastructure (tests/commit_arith_cases.py makes the rows and judges the results;
// tests/commit_arith_harness.cpp runs them on the CPU).  It loads, calls and stores — nothing here computes.  Written
// __host__ __device__ like the header, so that a device probe (one thread per row) can run the same text.
#pragma once
#include "b3w_commit_arith.h"

#define B3W_PROBE_IN 80        // words per row: operation, argument, operands
#define B3W_PROBE_OUT 72       // words per result
// fields / instantiations (the table's `field`)
#define B3W_PROBE_BN254 0          // BN254 base field, B3wCurve9
#define B3W_PROBE_PASTA 1          // the Pasta field P_VESTA_BASE, B3wCurve9
#define B3W_PROBE_PASTA_CONST 2    // the same field, B3wCurve9Vesta (modulus as compile-time constants)
#define B3W_PROBE_FIELDS 3

enum B3wProbeOp : uint32_t {
  // eight 32-bit limbs; operands 8 words each
  PR_FP_ADD = 1, PR_FP_SUB, PR_FP_MUL, PR_FP_SQR, PR_FP_INV, PR_FP_DBL,
  PR_FP_REDUCE_ONCE,                 // a, arg = hi
  PR_JAC_DBL, PR_JAC_MADD, PR_JAC_ADD, PR_JAC_TO_AFFINE,     // points X Y Z (24 words); madd: P, x2, y2
  // nine 29-bit limbs; operands 9 words each
  PR_MUL29 = 20, PR_SQR29, PR_MULADD29, PR_CN29, PR_RED29, PR_ADD29, PR_SUB29, PR_NEG29,
  PR_SHL29,                          // a, arg = shift
  PR_IS_KP29,                        // a, arg = k  ->  0 / 1
  PR_S_IS_ZERO, PR_S_ADD, PR_S_SUB, PR_S_DBL, PR_INV29,
  PR_TO29,                           // 8 words -> 9
  PR_FROM29,                         // 9 words -> from29's 8 words, hi, then fp_reduce_once of them (8 words)
  PR_J9_DBL = 40, PR_J9_MADD, PR_J9_ADD,   // points X Y ZZ ZZZ (36 words), arg bit 0 = P.inf, bit 1 = Q.inf; madd: P, x2, y2.  -> 36 words, inf
  PR_CONSTS = 50,                    // -> the B3wCurve (33 words), then the B3wCurve9 (32 words) the routines were given
};

namespace {

__host__ __device__ __forceinline__ Fp pr_ld8(const uint32_t *p) { Fp r; for (int i = 0; i < 8; ++i) r.l[i] = p[i]; return r; }
__host__ __device__ __forceinline__ F9 pr_ld9(const uint32_t *p) { F9 r; for (int i = 0; i < 9; ++i) r.l[i] = p[i]; return r; }
__host__ __device__ __forceinline__ void pr_st8(uint32_t *p, const Fp &v) { for (int i = 0; i < 8; ++i) p[i] = v.l[i]; }
__host__ __device__ __forceinline__ void pr_st9(uint32_t *p, const F9 &v) { for (int i = 0; i < 9; ++i) p[i] = v.l[i]; }
__host__ __device__ __forceinline__ Jac pr_ldjac(const uint32_t *p) { Jac r; r.X = pr_ld8(p); r.Y = pr_ld8(p + 8); r.Z = pr_ld8(p + 16); return r; }
__host__ __device__ __forceinline__ void pr_stjac(uint32_t *p, const Jac &v) { pr_st8(p, v.X); pr_st8(p + 8, v.Y); pr_st8(p + 16, v.Z); }
__host__ __device__ __forceinline__ J9 pr_ldj9(const uint32_t *p, bool inf) {
  J9 r; r.X = pr_ld9(p); r.Y = pr_ld9(p + 9); r.ZZ = pr_ld9(p + 18); r.ZZZ = pr_ld9(p + 27); r.inf = inf; return r;
}
__host__ __device__ __forceinline__ void pr_stj9(uint32_t *p, const J9 &v) {
  pr_st9(p, v.X); pr_st9(p + 9, v.Y); pr_st9(p + 18, v.ZZ); pr_st9(p + 27, v.ZZZ); p[36] = v.inf ? 1u : 0u;
}

template <class CV>
__host__ __device__ void b3w_commit_probe_row(const uint32_t *in /* B3W_PROBE_IN */, uint32_t *out /* B3W_PROBE_OUT */, const B3wCurve &C, const CV &C9) {
  const uint32_t op = in[0], arg = in[1];
  const uint32_t *a = in + 2;
  for (int i = 0; i < B3W_PROBE_OUT; ++i) out[i] = 0;
  switch (op) {
    case PR_FP_ADD: pr_st8(out, fp_add(pr_ld8(a), pr_ld8(a + 8), C)); break;
    case PR_FP_SUB: pr_st8(out, fp_sub(pr_ld8(a), pr_ld8(a + 8), C)); break;
    case PR_FP_MUL: pr_st8(out, fp_mul(pr_ld8(a), pr_ld8(a + 8), C)); break;
    case PR_FP_SQR: pr_st8(out, fp_sqr(pr_ld8(a), C)); break;
    case PR_FP_INV: pr_st8(out, fp_inv(pr_ld8(a), C)); break;
    case PR_FP_DBL: pr_st8(out, fp_dbl(pr_ld8(a), C)); break;
    case PR_FP_REDUCE_ONCE: pr_st8(out, fp_reduce_once(pr_ld8(a), arg, C)); break;
    case PR_JAC_DBL: pr_stjac(out, jac_dbl(pr_ldjac(a), C)); break;
    case PR_JAC_MADD: pr_stjac(out, jac_madd(pr_ldjac(a), pr_ld8(a + 24), pr_ld8(a + 32), C)); break;
    case PR_JAC_ADD: pr_stjac(out, jac_add(pr_ldjac(a), pr_ldjac(a + 24), C)); break;
    case PR_JAC_TO_AFFINE: { Fp x, y; jac_to_affine(pr_ldjac(a), x, y, C); pr_st8(out, x); pr_st8(out + 8, y); break; }
    case PR_MUL29: pr_st9(out, mul29(pr_ld9(a), pr_ld9(a + 9), C9)); break;
    case PR_SQR29: pr_st9(out, sqr29(pr_ld9(a), C9)); break;
    case PR_MULADD29: pr_st9(out, muladd29(pr_ld9(a), pr_ld9(a + 9), pr_ld9(a + 18), pr_ld9(a + 27), C9)); break;
    case PR_CN29: pr_st9(out, cn29(pr_ld9(a))); break;
    case PR_RED29: pr_st9(out, red29(pr_ld9(a), C9)); break;
    case PR_ADD29: pr_st9(out, add29(pr_ld9(a), pr_ld9(a + 9))); break;
    case PR_SUB29: pr_st9(out, sub29(pr_ld9(a), pr_ld9(a + 9), C9)); break;
    case PR_NEG29: pr_st9(out, neg29(pr_ld9(a), C9)); break;
    case PR_SHL29: pr_st9(out, shl29(pr_ld9(a), (int)arg)); break;
    case PR_IS_KP29: out[0] = is_kp29(pr_ld9(a), arg, C9) ? 1u : 0u; break;
    case PR_S_IS_ZERO: out[0] = s_is_zero(pr_ld9(a), C9) ? 1u : 0u; break;
    case PR_S_ADD: pr_st9(out, s_add(pr_ld9(a), pr_ld9(a + 9), C9)); break;
    case PR_S_SUB: pr_st9(out, s_sub(pr_ld9(a), pr_ld9(a + 9), C9)); break;
    case PR_S_DBL: pr_st9(out, s_dbl(pr_ld9(a), C9)); break;
    case PR_INV29: pr_st9(out, inv29(pr_ld9(a), C.pm2, C9)); break;
    case PR_TO29: pr_st9(out, to29(pr_ld8(a))); break;
    case PR_FROM29: { uint32_t hi; const Fp v = from29(pr_ld9(a), hi); pr_st8(out, v); out[8] = hi; pr_st8(out + 9, fp_reduce_once(v, hi, C)); break; }
    case PR_J9_DBL: { J9 P = pr_ldj9(a, arg & 1u); j9_dbl(P, C9); pr_stj9(out, P); break; }
    case PR_J9_MADD: { J9 P = pr_ldj9(a, arg & 1u); j9_madd(P, pr_ld9(a + 36), pr_ld9(a + 45), C9); pr_stj9(out, P); break; }
    case PR_J9_ADD: { J9 P = pr_ldj9(a, arg & 1u); j9_add(P, pr_ldj9(a + 36, (arg >> 1) & 1u), C9); pr_stj9(out, P); break; }
    case PR_CONSTS: {
      for (int i = 0; i < 8; ++i) { out[i] = C.p[i]; out[8 + i] = C.r2[i]; out[16 + i] = C.one[i]; out[24 + i] = C.pm2[i]; }
      out[32] = C.inv;
      for (int i = 0; i < 9; ++i) { out[33 + i] = C9.P(i); out[42 + i] = C9.sp4[i]; out[51 + i] = C9.one[i]; }   // (P, INV: what the routines read)
      out[60] = C9.INV(); out[61] = C9.mu; out[62] = C9.kp0[0]; out[63] = C9.kp0[1]; out[64] = C9.kp0[2];
      break;
    }
    default: out[B3W_PROBE_OUT - 1] = 0xBADC0DEu; break;
  }
}

}  // namespace
