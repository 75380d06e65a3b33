// b3w_commit_arith.h — the field and group arithmetic of the commitment kernels (b3w_commit.hip) and the host builders of
// their constants, in a header a plain C++ compiler can read too: every routine is __host__ __device__, and without hipcc
// the qualifiers are empty.  tests/commit_arith_harness.cpp drives exactly this text on the CPU (tests/test_commit_arith_cpu.py).
// The unnamed namespace keeps the routines local to each file that includes the header, as they were when they lived in
// b3w_commit.hip.
#pragma once
#include <stdint.h>
#include <string.h>
#include "b3w_commit_curve.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline       // (forcing it would make one function of a host caller that dispatches over every routine)
#endif

namespace {

struct Fp { uint32_t l[8]; };
struct Jac { Fp X, Y, Z; };          // Z == 0: the point at infinity

__host__ __device__ __forceinline__ bool fp_is_zero(const Fp &a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.l[i];
  return o == 0;
}
__host__ __device__ __forceinline__ bool fp_eq(const Fp &a, const Fp &b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.l[i] ^ b.l[i];
  return o == 0;
}
__host__ __device__ __forceinline__ Fp fp_zero() { Fp r; for (int i = 0; i < 8; ++i) r.l[i] = 0; return r; }

// r = a - p if a >= p (a < 2p, `hi` = the ninth limb of a)
__host__ __device__ __forceinline__ Fp fp_reduce_once(const Fp &a, uint32_t hi, const B3wCurve &C) {
  Fp d;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.l[i] - C.p[i] - br;
    d.l[i] = (uint32_t)t;
    br = (uint32_t)(t >> 63);
  }
  const bool ge = hi != 0 || br == 0;      // a >= p
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = ge ? d.l[i] : a.l[i];
  return r;
}
__host__ __device__ __forceinline__ Fp fp_add(const Fp &a, const Fp &b, const B3wCurve &C) {
  Fp s;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.l[i] + b.l[i] + c;
    s.l[i] = (uint32_t)t;
    c = (uint32_t)(t >> 32);
  }
  return fp_reduce_once(s, c, C);
}
__host__ __device__ __forceinline__ Fp fp_sub(const Fp &a, const Fp &b, const B3wCurve &C) {
  Fp d;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.l[i] - b.l[i] - br;
    d.l[i] = (uint32_t)t;
    br = (uint32_t)(t >> 63);
  }
  uint32_t c = 0;                          // + p when it went negative
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)d.l[i] + (br ? C.p[i] : 0u) + c;
    d.l[i] = (uint32_t)t;
    c = (uint32_t)(t >> 32);
  }
  return d;
}
__host__ __device__ __forceinline__ Fp fp_dbl(const Fp &a, const B3wCurve &C) { return fp_add(a, a, C); }

// Montgomery product a * b / 2^256 mod p (CIOS)
__host__ __device__ __forceinline__ Fp fp_mul(const Fp &a, const Fp &b, const B3wCurve &C) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c += (uint64_t)a.l[j] * b.l[i] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[8] = (uint32_t)c;
    t[9] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * C.inv;
    c = (uint64_t)m * C.p[0] + t[0];
    c >>= 32;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      c += (uint64_t)m * C.p[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[7] = (uint32_t)c;
    t[8] = t[9] + (uint32_t)(c >> 32);
  }
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = t[i];
  return fp_reduce_once(r, t[8], C);
}
// Montgomery square: the 28 cross products once, doubled, plus the 8 squares (36 limb products, not 64), then the
// reduction of the 512-bit product.  1.17x the rate of fp_mul(a, a) on gfx950 (tools/ubench/fpmul_peak.hip).
__host__ __device__ __forceinline__ Fp fp_sqr(const Fp &a, const B3wCurve &C) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = i + 1; j < 8; ++j) {
      c += (uint64_t)a.l[i] * a.l[j] + t[i + j];
      t[i + j] = (uint32_t)c;
      c >>= 32;
    }
    t[i + 8] = (uint32_t)c;
  }
  uint32_t top = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t n = (t[i] << 1) | top;
    top = t[i] >> 31;
    t[i] = n;
  }
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.l[i] * a.l[i] + t[2 * i];
    t[2 * i] = (uint32_t)c;
    c >>= 32;
    c += t[2 * i + 1];
    t[2 * i + 1] = (uint32_t)c;
    c >>= 32;
  }
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t m = t[i] * C.inv;
    uint64_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      d += (uint64_t)m * C.p[j] + t[i + j];
      t[i + j] = (uint32_t)d;
      d >>= 32;
    }
    d += (uint64_t)t[i + 8] + carry;
    t[i + 8] = (uint32_t)d;
    carry = (uint32_t)(d >> 32);
  }
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = t[i + 8];
  return fp_reduce_once(r, carry, C);
}

// a^(p-2): Fermat inversion (a != 0)
__host__ __device__ Fp fp_inv(const Fp &a, const B3wCurve &C) {
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = C.one[i];
  for (int i = 255; i >= 0; --i) {
    r = fp_sqr(r, C);
    if ((C.pm2[i >> 5] >> (i & 31)) & 1) r = fp_mul(r, a, C);
  }
  return r;
}

__host__ __device__ __forceinline__ Jac jac_infinity() { Jac r; r.X = fp_zero(); r.Y = fp_zero(); r.Z = fp_zero(); return r; }

// 2P, a = 0 (dbl-2009-l)
__host__ __device__ __forceinline__ Jac jac_dbl(const Jac &P, const B3wCurve &C) {
  if (fp_is_zero(P.Z) || fp_is_zero(P.Y)) return jac_infinity();
  const Fp A = fp_sqr(P.X, C), B = fp_sqr(P.Y, C), Cc = fp_sqr(B, C);
  Fp D = fp_sub(fp_sub(fp_sqr(fp_add(P.X, B, C), C), A, C), Cc, C);
  D = fp_dbl(D, C);
  const Fp E = fp_add(fp_dbl(A, C), A, C), F = fp_sqr(E, C);
  Jac R;
  R.X = fp_sub(F, fp_dbl(D, C), C);
  Fp c8 = fp_dbl(fp_dbl(fp_dbl(Cc, C), C), C);
  R.Y = fp_sub(fp_mul(E, fp_sub(D, R.X, C), C), c8, C);
  R.Z = fp_dbl(fp_mul(P.Y, P.Z, C), C);
  return R;
}

// P + (x2, y2, 1) (madd-2007-bl) with the exceptional cases
__host__ __device__ __forceinline__ Jac jac_madd(const Jac &P, const Fp &x2, const Fp &y2, const B3wCurve &C) {
  if (fp_is_zero(x2) && fp_is_zero(y2)) return P;        // (0, 0) is not on these curves (b != 0): the table's infinity
  if (fp_is_zero(P.Z)) {
    Jac R; R.X = x2; R.Y = y2;
#pragma unroll
    for (int i = 0; i < 8; ++i) R.Z.l[i] = C.one[i];
    return R;
  }
  const Fp Z1Z1 = fp_sqr(P.Z, C), U2 = fp_mul(x2, Z1Z1, C), S2 = fp_mul(fp_mul(y2, P.Z, C), Z1Z1, C);
  const Fp H = fp_sub(U2, P.X, C), rr = fp_sub(S2, P.Y, C);
  if (fp_is_zero(H)) {
    if (!fp_is_zero(rr)) return jac_infinity();        // P + (-P)
    Jac Q; Q.X = x2; Q.Y = y2;
#pragma unroll
    for (int i = 0; i < 8; ++i) Q.Z.l[i] = C.one[i];
    return jac_dbl(Q, C);                               // P + P
  }
  const Fp HH = fp_sqr(H, C), I = fp_dbl(fp_dbl(HH, C), C), J = fp_mul(H, I, C), r = fp_dbl(rr, C), V = fp_mul(P.X, I, C);
  Jac R;
  R.X = fp_sub(fp_sub(fp_sqr(r, C), J, C), fp_dbl(V, C), C);
  R.Y = fp_sub(fp_mul(r, fp_sub(V, R.X, C), C), fp_dbl(fp_mul(P.Y, J, C), C), C);
  R.Z = fp_sub(fp_sub(fp_sqr(fp_add(P.Z, H, C), C), Z1Z1, C), HH, C);
  return R;
}

// P + Q (add-2007-bl) with the exceptional cases
__host__ __device__ __forceinline__ Jac jac_add(const Jac &P, const Jac &Q, const B3wCurve &C) {
  if (fp_is_zero(P.Z)) return Q;
  if (fp_is_zero(Q.Z)) return P;
  const Fp Z1Z1 = fp_sqr(P.Z, C), Z2Z2 = fp_sqr(Q.Z, C);
  const Fp U1 = fp_mul(P.X, Z2Z2, C), U2 = fp_mul(Q.X, Z1Z1, C);
  const Fp S1 = fp_mul(fp_mul(P.Y, Q.Z, C), Z2Z2, C), S2 = fp_mul(fp_mul(Q.Y, P.Z, C), Z1Z1, C);
  const Fp H = fp_sub(U2, U1, C), rr = fp_sub(S2, S1, C);
  if (fp_is_zero(H)) return fp_is_zero(rr) ? jac_dbl(P, C) : jac_infinity();
  const Fp I = fp_sqr(fp_dbl(H, C), C), J = fp_mul(H, I, C), r = fp_dbl(rr, C), V = fp_mul(U1, I, C);
  Jac R;
  R.X = fp_sub(fp_sub(fp_sqr(r, C), J, C), fp_dbl(V, C), C);
  R.Y = fp_sub(fp_mul(r, fp_sub(V, R.X, C), C), fp_dbl(fp_mul(S1, J, C), C), C);
  R.Z = fp_mul(fp_sub(fp_sub(fp_sqr(fp_add(P.Z, Q.Z, C), C), Z1Z1, C), Z2Z2, C), H, C);
  return R;
}

// Jacobian (Montgomery) -> affine (Montgomery); infinity -> (0, 0)
__host__ __device__ void jac_to_affine(const Jac &P, Fp &x, Fp &y, const B3wCurve &C) {
  if (fp_is_zero(P.Z)) { x = fp_zero(); y = fp_zero(); return; }
  const Fp zi = fp_inv(P.Z, C), zi2 = fp_sqr(zi, C);
  x = fp_mul(P.X, zi2, C);
  y = fp_mul(P.Y, fp_mul(zi2, zi, C), C);
}

// =====================================================================================================================
// The commit kernel's own arithmetic: the same field in NINE 29-BIT LIMBS, Montgomery radix 2^261.
// Every column of a 9 x 9 limb product (plus the reduction's) fits one 64-bit accumulator, so a limb product is ONE
// v_mad_u64_u32 whose addend is the accumulator itself: no carry moves (the 8 x 32-bit CIOS above spends three quarters
// of its instructions on them).  172 G multiplications/s against 93 (tools/ubench/fpmul29_peak.hip).
// Values are LAZY: a value is any representative below 2^261 (>= 64p); limbs may exceed 29 bits between operations.
// Each routine states what it needs and what it gives:  "tidy" = limbs 0..7 below 2^29;  "< kp" = the value's bound.
//   mul29 / sqr29   limb bounds la * lb < 1.52 * 2^60; a < Ap, b < Bp  ->  tidy, < (AB/64 + 1)p
//   cn29            any limbs  ->  tidy, same value
//   red29           any limbs, value < 2^261  ->  tidy, < 2p   (one-word Barrett quotient, never too large, at most 1 short)
//   a + sp4 - b     b tidy < 2p  ->  value a + 4p - b, limbs < a's + 2^30   (sp4 = 4p with every limb lifted by 2^29)
#define M29 0x1FFFFFFFu
struct F9 { uint32_t l[9]; };
struct J9 { F9 X, Y, ZZ, ZZZ; bool inf; };  // the point (X / ZZ, Y / ZZZ), ZZ^3 = ZZZ^2 ("XYZZ" coordinates: a mixed addition is
                                             // 8M + 2S, one squaring less than Jacobian); between additions all four are tidy < 2p
struct B3wCurve9 {
  uint32_t p[9];        // modulus
  uint32_t sp4[9];      // 4p, limb i lifted by 2^29 and lowered by the 1 it lent to limb i - 1
  uint32_t one[9];      // 2^261 mod p
  uint32_t inv;         // -p^-1 mod 2^29
  uint32_t mu;          // floor(2^269 / p) (or 1 less)
  uint32_t kp0[3];      // limb 0 of 3p, 4p, 5p: the filter in front of the exact "H = 0 mod p" test
  __host__ __device__ __forceinline__ uint32_t P(int i) const { return p[i]; }
  __host__ __device__ __forceinline__ uint32_t INV() const { return inv; }
};
// The Vesta base field with its modulus as compile-time constants: p = 2^254 + (126 bits) has limb 0 = 1, limbs 5..7 = 0
// and limb 8 = 2^22, so a third of the reduction's multiplications fold away (same layout, chosen by the launcher
// when the key's modulus is this one).
struct B3wCurve9Vesta : B3wCurve9 {
  __host__ __device__ static constexpr uint32_t P(int i) {
    return i == 0 ? 0x1u : i == 1 ? 0x9698768u : i == 2 ? 0x133e46e6u : i == 3 ? 0xd31f812u : i == 4 ? 0x224u : i == 8 ? 0x400000u : 0u;
  }
  __host__ __device__ static constexpr uint32_t INV() { return M29; }
};

template <class CV>
__host__ __device__ __forceinline__ F9 mul29(const F9 &a, const F9 &b, const CV &C) {
  uint64_t acc = 0;
  uint32_t m[9];
  F9 r;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (uint64_t)m[i] * C.P(k - i);
    m[k] = ((uint32_t)acc * C.INV()) & M29;
    acc += (uint64_t)m[k] * C.P(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (uint64_t)m[i] * C.P(k - i);
    r.l[k - 9] = (uint32_t)acc & M29;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}
// (a b + c d) / 2^261: two products, ONE reduction.  Column bound: 9 (la lb + lc ld) + 9 * 2^58 < 2^64, i.e.
// la lb + lc ld < 1.52 * 2^60 (e.g. 2^29 x 1.5 * 2^30 and 2^30 x 2^29); a < Ap ... d < Dp  ->  tidy, < ((AB + CD)/64 + 1)p
template <class CV>
__host__ __device__ __forceinline__ F9 muladd29(const F9 &a, const F9 &b, const F9 &c, const F9 &d, const CV &C) {
  uint64_t acc = 0;
  uint32_t m[9];
  F9 r;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) { acc += (uint64_t)a.l[i] * b.l[k - i]; acc += (uint64_t)c.l[i] * d.l[k - i]; }
#pragma unroll
    for (int i = 0; i < k; ++i) acc += (uint64_t)m[i] * C.P(k - i);
    m[k] = ((uint32_t)acc * C.INV()) & M29;
    acc += (uint64_t)m[k] * C.P(0);
    acc >>= 29;
  }
#pragma unroll
  for (int k = 9; k < 17; ++k) {
#pragma unroll
    for (int i = k - 8; i < 9; ++i) { acc += (uint64_t)a.l[i] * b.l[k - i]; acc += (uint64_t)c.l[i] * d.l[k - i]; }
#pragma unroll
    for (int i = k - 8; i < 9; ++i) acc += (uint64_t)m[i] * C.P(k - i);
    r.l[k - 9] = (uint32_t)acc & M29;
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}
template <class CV>
__host__ __device__ __forceinline__ F9 sqr29(const F9 &a, const CV &C) {      // limbs < 2^30
  uint64_t acc = 0;
  uint32_t m[9], d[9];
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) d[i] = a.l[i] << 1;
#pragma unroll
  for (int k = 0; k < 17; ++k) {
#pragma unroll
    for (int i = (k > 8 ? k - 8 : 0); 2 * i < k; ++i) acc += (uint64_t)d[i] * a.l[k - i];
    if (!(k & 1)) acc += (uint64_t)a.l[k / 2] * a.l[k / 2];
    if (k < 9) {
#pragma unroll
      for (int i = 0; i < k; ++i) acc += (uint64_t)m[i] * C.P(k - i);
      m[k] = ((uint32_t)acc * C.INV()) & M29;
      acc += (uint64_t)m[k] * C.P(0);
    } else {
#pragma unroll
      for (int i = k - 8; i < 9; ++i) acc += (uint64_t)m[i] * C.P(k - i);
      r.l[k - 9] = (uint32_t)acc & M29;
    }
    acc >>= 29;
  }
  r.l[8] = (uint32_t)acc;
  return r;
}
__host__ __device__ __forceinline__ F9 cn29(F9 a) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { a.l[i + 1] += a.l[i] >> 29; a.l[i] &= M29; }
  return a;
}
template <class CV>
__host__ __device__ __forceinline__ F9 red29(const F9 &a, const CV &C) {
  const uint32_t top = (a.l[8] + (a.l[7] >> 29)) >> 13;            // value / 2^245, rounded down (< 2^16)
  const uint32_t q = (top * C.mu) >> 24;                           // floor(value / p) or 1 less
  int64_t acc = 0;
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    acc += (int64_t)(uint64_t)a.l[i];
    acc -= (int64_t)((uint64_t)q * C.P(i));
    r.l[i] = i < 8 ? (uint32_t)acc & M29 : (uint32_t)acc;
    acc >>= 29;
  }
  return r;
}
__host__ __device__ __forceinline__ F9 add29(const F9 &a, const F9 &b) {
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + b.l[i];
  return r;
}
template <class CV>
__host__ __device__ __forceinline__ F9 sub29(const F9 &a, const F9 &b, const CV &C) {     // a + 4p - b   (b tidy < 2p)
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + (C.sp4[i] - b.l[i]);
  return r;
}
template <class CV>
__host__ __device__ __forceinline__ F9 neg29(const F9 &b, const CV &C) {                  // 4p - b
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = C.sp4[i] - b.l[i];
  return r;
}
__host__ __device__ __forceinline__ F9 shl29(const F9 &a, int s) {
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] << s;
  return r;
}
// tidy a == k * p ?
template <class CV>
__host__ __device__ __forceinline__ bool is_kp29(const F9 &a, uint32_t k, const CV &C) {
  uint32_t c = 0, o = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const uint32_t t = k * C.P(i) + c;
    o |= (i < 8 ? t & M29 : t) ^ a.l[i];
    c = t >> 29;
  }
  return o == 0;
}
// the safe forms (tidy < 2p in, tidy < 2p out) for the rare paths and the tree
template <class CV>
__host__ __device__ __forceinline__ F9 s_add(const F9 &a, const F9 &b, const CV &C) { return red29(add29(a, b), C); }
template <class CV>
__host__ __device__ __forceinline__ F9 s_sub(const F9 &a, const F9 &b, const CV &C) { return red29(sub29(a, b, C), C); }
template <class CV>
__host__ __device__ __forceinline__ F9 s_dbl(const F9 &a, const CV &C) { return red29(shl29(a, 1), C); }
template <class CV>
__host__ __device__ __forceinline__ bool s_is_zero(const F9 &a, const CV &C) { return is_kp29(a, 0, C) || is_kp29(a, 1, C); }
template <class CV>
__host__ __device__ __forceinline__ F9 one29(const CV &C) {
  F9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = C.one[i];
  return r;
}

// a^(p-2) (Fermat), a tidy < 2p and != 0 mod p; pm2 = p - 2 in eight 32-bit words
template <class CV>
__host__ __device__ __forceinline__ F9 inv29(const F9 &a, const uint32_t *pm2, const CV &C) {
  F9 r = one29(C);
#pragma unroll 1
  for (int i = 255; i >= 0; --i) {
    r = sqr29(r, C);
    if ((pm2[i >> 5] >> (i & 31)) & 1) r = mul29(r, a, C);
  }
  return r;
}

__host__ __device__ __forceinline__ F9 to29(const Fp &a) {                   // eight 32-bit words -> nine 29-bit limbs
  F9 r;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int bit = 29 * k, w = bit >> 5, sh = bit & 31;
    uint64_t v = a.l[w];
    if (w + 1 < 8) v |= (uint64_t)a.l[w + 1] << 32;
    r.l[k] = (uint32_t)(v >> sh) & M29;
  }
  return r;
}
__host__ __device__ __forceinline__ Fp from29(const F9 &a, uint32_t &hi) {     // tidy -> eight words + the bits above 2^256
  uint32_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int bit = 29 * k, w = bit >> 5, sh = bit & 31;
    const uint64_t v = (uint64_t)a.l[k] << sh;
    t[w] |= (uint32_t)v;
    if (w + 1 < 9) t[w + 1] |= (uint32_t)(v >> 32);
  }
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = t[i];
  hi = t[8];
  return r;
}

__host__ __device__ __forceinline__ J9 j9_infinity() {
  J9 r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.X.l[i] = r.Y.l[i] = r.ZZ.l[i] = r.ZZZ.l[i] = 0;
  r.inf = true;
  return r;
}
// P = 2P (dbl-2008-s-1, a = 0), safe forms
template <class CV>
__host__ __device__ __forceinline__ void j9_dbl(J9 &P, const CV &C) {
  if (P.inf) return;
  if (s_is_zero(P.Y, C)) { P.inf = true; return; }
  const F9 U = s_dbl(P.Y, C), V = sqr29(U, C), W = mul29(U, V, C), S = mul29(P.X, V, C);
  const F9 XX = sqr29(P.X, C), M = s_add(s_dbl(XX, C), XX, C);
  const F9 X3 = s_sub(sqr29(M, C), s_dbl(S, C), C);
  const F9 Y3 = s_sub(mul29(M, s_sub(S, X3, C), C), mul29(W, P.Y, C), C);
  P.ZZ = mul29(V, P.ZZ, C);
  P.ZZZ = mul29(W, P.ZZZ, C);
  P.X = X3; P.Y = Y3;
}
// P += (x2, y2): madd-2008-s with lazy values; x2, y2 tidy < p; (0, 0) (the table's infinity) is filtered by the caller.
// Bounds: inputs X1, Y1, ZZ1, ZZZ1 tidy < 2p  ->  outputs the same.
template <class CV>
__host__ __device__ __forceinline__ void j9_madd(J9 &P, const F9 &x2, const F9 &y2, const CV &C) {
  if (P.inf) {
    P.X = x2; P.Y = y2; P.ZZ = one29(C); P.ZZZ = one29(C); P.inf = false;
    return;
  }
  const F9 U2 = mul29(x2, P.ZZ, C), S2 = mul29(y2, P.ZZZ, C);      // < 2p
  const F9 Pd = cn29(sub29(U2, P.X, C));                           // tidy, in (2p, 6p): = 0 mod p iff 3p, 4p or 5p
  const F9 R = cn29(sub29(S2, P.Y, C));                            // likewise
  if (Pd.l[0] == C.kp0[0] || Pd.l[0] == C.kp0[1] || Pd.l[0] == C.kp0[2]) {
    if (is_kp29(Pd, 3, C) || is_kp29(Pd, 4, C) || is_kp29(Pd, 5, C)) {
      if (!(is_kp29(R, 3, C) || is_kp29(R, 4, C) || is_kp29(R, 5, C))) { P.inf = true; return; }     // P + (-P)
      P.X = x2; P.Y = y2; P.ZZ = one29(C); P.ZZZ = one29(C);
      j9_dbl(P, C);                                                                                  // P + P
      return;
    }
  }
  const F9 PP = sqr29(Pd, C);                                      // < 2p   (36 / 64 + 1)
  const F9 PPP = mul29(Pd, PP, C), Q = mul29(P.X, PP, C);          // < 2p
  const F9 X3 = red29(add29(add29(sqr29(R, C), neg29(PPP, C)), shl29(neg29(Q, C), 1)), C);    // R^2 - PPP - 2Q  (< 14p before)
  P.Y = muladd29(R, sub29(Q, X3, C), neg29(P.Y, C), PPP, C);       // R (Q - X3) + (4p - Y1) PPP: (6 * 5.1 + 4 * 1.2)/64 + 1 < 2p
  P.X = X3;
  P.ZZ = mul29(P.ZZ, PP, C);
  P.ZZZ = mul29(P.ZZZ, PPP, C);
}
// P += Q (add-2008-s), safe forms
template <class CV>
__host__ __device__ __forceinline__ void j9_add(J9 &P, const J9 &Q, const CV &C) {
  if (Q.inf) return;
  if (P.inf) { P.X = Q.X; P.Y = Q.Y; P.ZZ = Q.ZZ; P.ZZZ = Q.ZZZ; P.inf = false; return; }
  const F9 U1 = mul29(P.X, Q.ZZ, C), U2 = mul29(Q.X, P.ZZ, C);
  const F9 S1 = mul29(P.Y, Q.ZZZ, C), S2 = mul29(Q.Y, P.ZZZ, C);
  const F9 Pd = s_sub(U2, U1, C), R = s_sub(S2, S1, C);
  if (s_is_zero(Pd, C)) {
    if (s_is_zero(R, C)) j9_dbl(P, C); else P.inf = true;
    return;
  }
  const F9 PP = sqr29(Pd, C), PPP = mul29(Pd, PP, C), Qq = mul29(U1, PP, C);
  const F9 X3 = s_sub(s_sub(sqr29(R, C), PPP, C), s_dbl(Qq, C), C);
  P.Y = s_sub(mul29(R, s_sub(Qq, X3, C), C), mul29(S1, PPP, C), C);
  P.ZZ = mul29(mul29(P.ZZ, Q.ZZ, C), PP, C);
  P.ZZZ = mul29(mul29(P.ZZZ, Q.ZZZ, C), PPP, C);
  P.X = X3;
}

// ---- host: the constants of a curve
// 256-bit helpers for the curve constants (host, little-endian u32 limbs)
bool u256_geq(const uint32_t a[8], const uint32_t b[8]) { for (int i = 7; i >= 0; --i) if (a[i] != b[i]) return a[i] > b[i]; return true; }
void u256_sub_host(uint32_t a[8], const uint32_t b[8]) {
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a[i] - b[i] - br; a[i] = (uint32_t)t; br = (t >> 63) & 1; }
}
void u256_double_mod(uint32_t a[8], const uint32_t p[8]) {            // a = 2a mod p (a < p < 2^255)
  uint32_t c = 0;
  for (int i = 0; i < 8; i++) { const uint32_t n = (a[i] << 1) | c; c = a[i] >> 31; a[i] = n; }
  if (c || u256_geq(a, p)) u256_sub_host(a, p);
}
B3wCurve make_curve(const uint64_t p64[4]) {
  B3wCurve C{};
  memcpy(C.p, p64, 32);
  uint32_t x[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 256; i++) u256_double_mod(x, C.p);
  memcpy(C.one, x, 32);
  for (int i = 0; i < 256; i++) u256_double_mod(x, C.p);
  memcpy(C.r2, x, 32);
  memcpy(C.pm2, C.p, 32);
  const uint32_t two[8] = {2, 0, 0, 0, 0, 0, 0, 0};
  u256_sub_host(C.pm2, two);
  uint32_t inv = C.p[0];                                             // Newton: inv = p^-1 mod 2^32
  for (int i = 0; i < 5; i++) inv *= 2u - C.p[0] * inv;
  C.inv = 0u - inv;
  return C;
}
const uint64_t Q_BN254[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
const uint64_t P_VESTA_BASE[4] = {0x992d30ed00000001ull, 0x224698fc094cf91bull, 0x0ull, 0x4000000000000000ull};

// the 29-bit constants of a curve
void u288_split29(const uint32_t w[9], uint32_t out[9]) {
  for (int k = 0; k < 9; ++k) {
    const int bit = 29 * k, i = bit >> 5, sh = bit & 31;
    uint64_t v = w[i];
    if (i + 1 < 9) v |= (uint64_t)w[i + 1] << 32;
    out[k] = (uint32_t)(v >> sh) & (k < 8 ? M29 : 0xFFFFFFFFu);
  }
}
B3wCurve9 make_curve9(const B3wCurve &C) {
  B3wCurve9 D{};
  uint32_t w[9];
  for (int i = 0; i < 8; ++i) w[i] = C.p[i];
  w[8] = 0;
  u288_split29(w, D.p);
  uint32_t p4[9];                                              // 4p
  for (int i = 0; i < 9; ++i) p4[i] = (i < 8 ? C.p[i] << 2 : 0u) | (i > 0 ? C.p[i - 1] >> 30 : 0u);
  u288_split29(p4, D.sp4);
  for (int i = 0; i < 8; ++i) D.sp4[i] += (1u << 29) - (i > 0 ? 1u : 0u);
  D.sp4[8] -= 1u;
  uint32_t x[8];
  for (int i = 0; i < 8; ++i) x[i] = C.one[i];
  for (int k = 0; k < 5; ++k) u256_double_mod(x, C.p);          // 2^261 mod p
  for (int i = 0; i < 8; ++i) w[i] = x[i];
  w[8] = 0;
  u288_split29(w, D.one);
  D.inv = C.inv & M29;
  const uint64_t phi = ((uint64_t)C.p[7] << 32) | C.p[6];      // p >> 192
  D.mu = (uint32_t)((((unsigned __int128)1) << 77) / ((unsigned __int128)phi + 1));
  for (uint32_t k = 3; k <= 5; ++k) D.kp0[k - 3] = (k * D.p[0]) & M29;
  return D;
}

}  // namespace
