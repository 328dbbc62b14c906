// sq8_core_test.cpp — stand-alone driver of dingo-store_amd/csrc/
// dg_sq8_core.h for tests/test_ivf_sq8_cpu.py (no GPU, no HIP).
//
//   sq8_core_test                 self-check, prints OK
//   sq8_core_test codec IN OUT    IN: int32 n, then n x (x, vmin, vdiff) f32.
//                                 OUT: n code bytes, n f32 decodes of (code,
//                                 vmin, vdiff), n f32 steps of vdiff.
//   sq8_core_test offset d nrows_pad
//                                 one line per (dim, row): the byte offset
//
// The self-check demands that the chunk offsets of every (dim < d16, row <
// nrows_pad) are a permutation of 0 .. d16 * nrows_pad - 1 (no slack, no
// overlap), that a lane's 16-byte load holds the four k-steps of four rows,
// and that every code decodes back to itself.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dingo-store_amd/csrc/dg_sq8_core.h"

static bool layout_ok(int32_t d, int32_t nrows_pad) {
  const int32_t d16 = dg_sq8_dims_pad(d);
  const int64_t bytes = dg_sq8_chunk_bytes(d, nrows_pad);
  if (d16 % 16 || d16 < d || d16 - d >= 16 || bytes != (int64_t)d16 * nrows_pad)
    return false;
  std::vector<int> seen((size_t)bytes, 0);
  for (int32_t dim = 0; dim < d16; dim++)
    for (int32_t row = 0; row < nrows_pad; row++) {
      const int64_t o = dg_sq8_chunk_offset(dim, row, nrows_pad);
      if (o < 0 || o >= bytes) return false;
      seen[(size_t)o]++;
      // the load of lane (g = dim & 3, row & ~3) at k-period dim >> 4
      const int64_t base =
          ((int64_t)(4 * (dim >> 4) + (dim & 3)) * nrows_pad + (row & ~3)) * 4;
      if (o != base + 4 * ((dim >> 2) & 3) + (row & 3)) return false;
    }
  for (int c : seen)
    if (c != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    for (int32_t d : {1, 4, 15, 16, 17, 32, 100, 208})
      for (int32_t nrp : {4, 8, 12, 256, 1024})
        if (!layout_ok(d, nrp)) {
          printf("FAIL layout d %d nrows_pad %d\n", d, nrp);
          return 1;
        }
    const float ranges[][2] = {{0.0f, 1.0f},      {-3.5f, 7.25f},
                               {1e-30f, 1e-30f},  {-1e30f, 2e30f},
                               {5.0f, 0.0f},      {0.1f, 1e-3f}};
    for (const auto& r : ranges)
      for (int c = 0; c < 256; c++) {
        const float x = dg_sq8_decode((uint8_t)c, r[0], r[1]);
        const int want = r[1] > 0.0f ? c : 0;
        if (!std::isfinite(x) || dg_sq8_encode(x, r[0], r[1]) != want) {
          printf("FAIL round trip code %d range %g %g\n", c, r[0], r[1]);
          return 1;
        }
      }
    if (dg_sq8_encode(-1.0f, 0.0f, 1.0f) != 0 ||
        dg_sq8_encode(2.0f, 0.0f, 1.0f) != 255 ||
        dg_sq8_encode(1.0f, 0.0f, 1.0f) != 255 ||
        dg_sq8_encode(0.0f, 0.0f, 1.0f) != 0 ||
        dg_sq8_encode(7.0f, 5.0f, 0.0f) != 0 ||
        dg_sq8_decode(0, 5.0f, 0.0f) != 5.0f ||
        dg_sq8_step(255.0f) != 1.0f) {
      printf("FAIL fixed points\n");
      return 1;
    }
    printf("OK\n");
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "codec")) {
    FILE* in = fopen(argv[2], "rb");
    int32_t n = 0;
    if (!in || fread(&n, 4, 1, in) != 1 || n < 0) return 3;
    std::vector<float> v((size_t)n * 3);
    if (fread(v.data(), 4, v.size(), in) != v.size()) return 3;
    fclose(in);
    std::vector<uint8_t> code((size_t)n);
    std::vector<float> dec((size_t)n), step((size_t)n);
    for (int32_t i = 0; i < n; i++) {
      const float x = v[3 * (size_t)i], lo = v[3 * (size_t)i + 1],
                  w = v[3 * (size_t)i + 2];
      code[(size_t)i] = dg_sq8_encode(x, lo, w);
      dec[(size_t)i] = dg_sq8_decode(code[(size_t)i], lo, w);
      step[(size_t)i] = dg_sq8_step(w);
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 3;
    fwrite(code.data(), 1, code.size(), out);
    fwrite(dec.data(), 4, dec.size(), out);
    fwrite(step.data(), 4, step.size(), out);
    fclose(out);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "offset")) {
    const int32_t d = atoi(argv[2]), nrp = atoi(argv[3]);
    for (int32_t dim = 0; dim < dg_sq8_dims_pad(d); dim++)
      for (int32_t row = 0; row < nrp; row++)
        printf("%d %d %lld\n", dim, row,
               (long long)dg_sq8_chunk_offset(dim, row, nrp));
    return 0;
  }
  fprintf(stderr, "usage: sq8_core_test [codec IN OUT | offset d nrows_pad]\n");
  return 2;
}
