// dg_scan_split.h — how a list's 16-query tiles are divided between the two
// kernels of the fused f32-MFMA scan (DESIGN.md §Pair scan).  No HIP here:
// the kernels, the host launcher and tests/host/scan_split_test.cpp all
// include this one definition.
//
// A list probed by nql queries has T = ceil(nql / 16) tiles.  The pair
// kernel (k_ivf_scan_mfma2) takes pairs p = 0 .. floor(T/2)-1, i.e. tiles 2p
// and 2p+1, and k_ivf_scan_mfma starts at tile 2*floor(T/2): everything
// when T = 1, the odd last tile when T is odd, nothing when T is even.
// With pairing off the pair kernel is not launched and k_ivf_scan_mfma
// starts at tile 0.
#pragma once
#include <cstdint>

constexpr int32_t kScanTileQ = 16;  // queries per MFMA tile

constexpr int32_t dg_scan_tiles(int32_t nql) {
  return (nql + kScanTileQ - 1) / kScanTileQ;
}

// pairs of tiles the pair kernel scans for a list probed by nql queries
constexpr int32_t dg_scan_pairs(int32_t nql, bool pairing) {
  return pairing ? dg_scan_tiles(nql) / 2 : 0;
}

// bytes of the pair kernel's operand image: nq queries and one zero query,
// each ceil(d/16) periods of 16 floats
constexpr int64_t dg_scan_qimage_bytes(int64_t nq, int32_t d) {
  return (nq + 1) * (int64_t)((d + 15) / 16) * 64;
}

// The pair kernel is an instance of the 16-query rung of the tile ladder
// (d <= 2304), can find two tiles only with more than 16 queries, and
// addresses the operand image with 32-bit byte offsets.
constexpr bool dg_scan_pair_applies(int32_t d, int64_t nq) {
  return d <= 2304 && nq > kScanTileQ &&
         dg_scan_qimage_bytes(nq, d) < ((int64_t)1 << 32);
}

// first tile left to k_ivf_scan_mfma (it runs tiles up to dg_scan_tiles)
constexpr int32_t dg_scan_single_first(int32_t nql, bool pairing) {
  return 2 * dg_scan_pairs(nql, pairing);
}
