// b3w_blake3_cv.h — the BLAKE3 compression and tree shape that host code and device code share: b3w_blake3_dev.h puts the device-only
// helpers on top of it, b3w_bao_tree.h the bao arithmetic.  Compiles as HIP (host and device) and as plain C++ (b3w_bao_host.cpp in a
// sanitizer build without hipcc).  Everything lives in an anonymous namespace: each file that includes it gets its own copy.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define B3W_HD __host__ __device__
#define B3W_HD_INLINE __host__ __device__ __forceinline__
#define B3W_UNROLL _Pragma("unroll")
#else
#define B3W_HD
#define B3W_HD_INLINE inline __attribute__((always_inline))
#define B3W_UNROLL
#endif

namespace {

B3W_HD_INLINE uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

#define B3_G(a, b, c, d, x, y)                                       \
  v[a] = v[a] + v[b] + (x); v[d] = rotr(v[d] ^ v[a], 16);            \
  v[c] = v[c] + v[d];       v[b] = rotr(v[b] ^ v[c], 12);            \
  v[a] = v[a] + v[b] + (y); v[d] = rotr(v[d] ^ v[a], 8);             \
  v[c] = v[c] + v[d];       v[b] = rotr(v[b] ^ v[c], 7);

// plain BLAKE3 compression, first 8 output words (BLAKE3 spec 2.2; the circuit's Blake3Compression
// computes the same function, circuits/blake3_compression.circom:171-228).  Host-callable too: the bao host calls
// (b3w_bao_host.cpp) hash chunks and nodes with it.
B3W_HD void blake3_cv(const uint32_t h[8], const uint32_t m_in[16], uint32_t t0, uint32_t t1, uint32_t b, uint32_t d,
                          uint32_t out[8]) {
  uint32_t v[16], m[16];
  B3W_UNROLL
  for (int i = 0; i < 8; ++i) v[i] = h[i];
  v[8] = 0x6A09E667u; v[9] = 0xBB67AE85u; v[10] = 0x3C6EF372u; v[11] = 0xA54FF53Au;
  v[12] = t0; v[13] = t1; v[14] = b; v[15] = d;
  B3W_UNROLL
  for (int i = 0; i < 16; ++i) m[i] = m_in[i];
  B3W_UNROLL
  for (int r = 0; r < 7; ++r) {
    B3_G(0, 4, 8, 12, m[0], m[1]) B3_G(1, 5, 9, 13, m[2], m[3]) B3_G(2, 6, 10, 14, m[4], m[5]) B3_G(3, 7, 11, 15, m[6], m[7])
    B3_G(0, 5, 10, 15, m[8], m[9]) B3_G(1, 6, 11, 12, m[10], m[11]) B3_G(2, 7, 8, 13, m[12], m[13]) B3_G(3, 4, 9, 14, m[14], m[15])
    const uint32_t t[16] = {m[2], m[6], m[3], m[10], m[7], m[0], m[4], m[13], m[1], m[11], m[12], m[5], m[9], m[14], m[15], m[8]};
    B3W_UNROLL
    for (int i = 0; i < 16; ++i) m[i] = t[i];
  }
  B3W_UNROLL
  for (int i = 0; i < 8; ++i) out[i] = v[i] ^ v[i + 8];
}

B3W_HD_INLINE void iv(uint32_t h[8]) {
  h[0] = 0x6A09E667u; h[1] = 0xBB67AE85u; h[2] = 0x3C6EF372u; h[3] = 0xA54FF53Au;
  h[4] = 0x510E527Fu; h[5] = 0x9B05688Cu; h[6] = 0x1F83D9ABu; h[7] = 0x5BE0CD19u;
}

// number of parent nodes above chunk c in BLAKE3's tree over n chunks (left subtree = largest power
// of two strictly below n)
B3W_HD inline uint32_t path_len(uint64_t c, uint64_t n) {
  uint32_t p = 0;
  while (n > 1) {
    uint64_t k = 1;
    while (k * 2 < n) k *= 2;
    if (c < k) n = k; else { c -= k; n -= k; }
    p++;
  }
  return p;
}

}  // namespace
