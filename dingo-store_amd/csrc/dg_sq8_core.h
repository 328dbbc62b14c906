// dg_sq8_core.h — the 8-bit scalar-quantiser codec of DG_STORAGE_SQ8 and the
// byte layout of its scanned chunks (DESIGN.md §SQ8 row storage).  No HIP
// here: the kernels, the host code, the loaders and
// tests/host/sq8_core_test.cpp all include this one definition.
//
// The codec restates faiss QT_8bit with per-dimension ranges (vmin, vdiff),
// all in f32:
//   encode  t = vdiff > 0 ? (x - vmin) / vdiff : 0, clamped to [0, 1];
//           code = (uint8)(int)(255.0f * t)       (out of range saturates)
//   decode  vmin + ((code + 0.5f) / 255.0f) * vdiff
// Each function rounds every operation on its own (no fused multiply-add),
// so the host and the device produce the same bits.
#pragma once
#include <cstdint>

#if defined(__clang__)
#define DG_SQ8_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DG_SQ8_NO_CONTRACT
#endif

constexpr uint8_t dg_sq8_encode(float x, float vmin, float vdiff) {
  DG_SQ8_NO_CONTRACT
  float t = vdiff > 0.0f ? (x - vmin) / vdiff : 0.0f;
  if (!(t > 0.0f)) t = 0.0f;  // NaN too; add and upsert refuse it earlier
  if (t > 1.0f) t = 1.0f;
  return (uint8_t)(int)(255.0f * t);
}

constexpr float dg_sq8_decode(uint8_t code, float vmin, float vdiff) {
  DG_SQ8_NO_CONTRACT
  const float t = ((float)code + 0.5f) / 255.0f;
  const float s = t * vdiff;
  return vmin + s;
}

// The scan folds the affine decode into the query:
//   q . x = cq + sum_j (q_j * step_j) * code_j,
//   step_j = vdiff_j / 255, cq = sum_j q_j * (vmin_j + step_j / 2).
constexpr float dg_sq8_step(float vdiff) { return vdiff / 255.0f; }

// Chunk layout: with d16 = ceil(d/16)*16 (dims past d hold code 0) and
// nrows_pad = ceil(nrows/4)*4 (rows past nrows hold code 0) a chunk is
// [d16/16 kp][4 g][nrows_pad/4 quads][4 h][4 x] bytes, the code of dim
// 16kp + 4h + g of row 4*quad + x.  A lane's 16-byte load at
// ((4kp + g) * nrows_pad + row) * 4 (row a multiple of 4: the byte offsets
// of the f32 layout) is the B operand (k = g) of the four k-steps 4kp + h
// for four consecutive rows.
constexpr int32_t dg_sq8_dims_pad(int32_t d) { return (d + 15) & ~15; }

constexpr int64_t dg_sq8_chunk_bytes(int32_t d, int32_t nrows_pad) {
  return (int64_t)dg_sq8_dims_pad(d) * nrows_pad;
}

constexpr int64_t dg_sq8_chunk_offset(int32_t dim, int32_t row,
                                      int32_t nrows_pad) {
  return ((int64_t)(4 * (dim >> 4) + (dim & 3)) * (nrows_pad >> 2) +
          (row >> 2)) * 16 +
         ((dim >> 2) & 3) * 4 + (row & 3);
}
