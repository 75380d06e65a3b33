// commit_arith_harness.cpp — the commit kernels' field and group arithmetic (csrc/b3w_commit_arith.h) on the CPU, under
// AddressSanitizer + UBSan (tests/test_commit_arith_cpu.py builds and runs it).  No GPU, no HIP.
//   commit_arith_harness <rows.bin> <results.bin>
// rows.bin: u32 field (B3W_PROBE_BN254 / _PASTA / _PASTA_CONST), u32 n, then n rows of B3W_PROBE_IN words (tests/commit_arith_cases.py);
// results.bin: n results of B3W_PROBE_OUT words (tests/commit_arith_rows.h applies a row).
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "commit_arith_rows.h"

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s rows.bin results.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t head[2];
  if (fread(head, 4, 2, f) != 2 || head[0] >= B3W_PROBE_FIELDS) { fprintf(stderr, "bad header\n"); return 2; }
  const uint32_t field = head[0], n = head[1];
  std::vector<uint32_t> rows((size_t)n * B3W_PROBE_IN), out((size_t)n * B3W_PROBE_OUT);
  if (fread(rows.data(), 4, rows.size(), f) != rows.size()) { fprintf(stderr, "short rows\n"); return 2; }
  fclose(f);
  const B3wCurve C = make_curve(field == B3W_PROBE_BN254 ? Q_BN254 : P_VESTA_BASE);
  const B3wCurve9 c9 = make_curve9(C);
  B3wCurve9Vesta c9v;
  static_cast<B3wCurve9 &>(c9v) = c9;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t *in = rows.data() + (size_t)r * B3W_PROBE_IN;
    uint32_t *res = out.data() + (size_t)r * B3W_PROBE_OUT;
    if (field == B3W_PROBE_PASTA_CONST) b3w_commit_probe_row(in, res, C, c9v);
    else b3w_commit_probe_row(in, res, C, c9);
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  if (fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
  fclose(f);
  printf("rows %u field %u\n", n, field);
  return 0;
}
