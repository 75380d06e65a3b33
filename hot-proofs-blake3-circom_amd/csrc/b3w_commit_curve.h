// b3w_commit_curve.h — the field constants of a commitment curve (shared by b3w_kernels.h and the HIP-free b3w_commit_arith.h)
#pragma once
#include <stdint.h>

// Field of the curve's coordinates:
struct B3wCurve {
  uint32_t p[8];      // modulus, little-endian limbs
  uint32_t r2[8];     // 2^512 mod p   (into Montgomery form)
  uint32_t one[8];    // 2^256 mod p   (1 in Montgomery form)
  uint32_t pm2[8];    // p - 2         (Fermat inversion exponent)
  uint32_t inv;       // -p^-1 mod 2^32
};
