// scan_split_test.cpp — stand-alone driver of dingo-store_amd/csrc/
// dg_scan_split.h for tests/test_scan_split_cpu.py (no GPU, no HIP).
//
//   scan_split_test            self-check, prints OK
//   scan_split_test table N    one line per nql = 0 .. N and pairing = 0, 1:
//                              "nql pairing tiles pairs single_first"
//   scan_split_test applies d nq
//                              "applies image_bytes"
//
// The self-check walks the two kernels' tile loops as they are written
// (pair p takes tiles 2p and 2p+1 and needs tile 2p whole and tile 2p+1
// non-empty; the single-tile kernel runs from single_first to the end) and
// demands that every tile is taken exactly once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dingo-store_amd/csrc/dg_scan_split.h"

static bool cover_once(int32_t nql, bool pairing) {
  const int32_t T = dg_scan_tiles(nql);
  std::vector<int> taken((size_t)T, 0);
  for (int32_t p = 0; p < dg_scan_pairs(nql, pairing); p++) {
    const int32_t t0 = 2 * kScanTileQ * p;
    const int32_t qt1 = nql - t0 - kScanTileQ;  // before the clamp to 16
    if (2 * p + 1 >= T || qt1 < 1) return false;
    taken[(size_t)(2 * p)]++;
    taken[(size_t)(2 * p + 1)]++;
  }
  for (int32_t t0 = kScanTileQ * dg_scan_single_first(nql, pairing);
       t0 < nql; t0 += kScanTileQ)
    taken[(size_t)(t0 / kScanTileQ)]++;
  for (int c : taken)
    if (c != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    for (int32_t nql = 0; nql <= 4096; nql++)
      for (int pairing = 0; pairing < 2; pairing++)
        if (!cover_once(nql, pairing != 0)) {
          printf("FAIL nql %d pairing %d\n", nql, pairing);
          return 1;
        }
    if (dg_scan_pairs(16, true) != 0 || dg_scan_pairs(17, true) != 1 ||
        dg_scan_single_first(33, true) != 2 ||
        dg_scan_single_first(33, false) != 0 ||
        dg_scan_pair_applies(768, 16) || !dg_scan_pair_applies(768, 17) ||
        dg_scan_pair_applies(2308, 1024) || !dg_scan_pair_applies(2304, 17)) {
      printf("FAIL fixed points\n");
      return 1;
    }
    printf("OK\n");
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "table")) {
    for (int32_t nql = 0; nql <= atoi(argv[2]); nql++)
      for (int pairing = 0; pairing < 2; pairing++)
        printf("%d %d %d %d %d\n", nql, pairing, dg_scan_tiles(nql),
               dg_scan_pairs(nql, pairing != 0),
               dg_scan_single_first(nql, pairing != 0));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "applies")) {
    const int32_t d = atoi(argv[2]);
    const int64_t nq = atoll(argv[3]);
    printf("%d %lld\n", dg_scan_pair_applies(d, nq) ? 1 : 0,
           (long long)dg_scan_qimage_bytes(nq, d));
    return 0;
  }
  fprintf(stderr, "usage: scan_split_test [table N | applies d nq]\n");
  return 2;
}
