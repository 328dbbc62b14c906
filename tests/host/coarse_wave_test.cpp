// coarse_wave_test.cpp — stand-alone driver of dingo-store_amd/csrc/
// dg_coarse_wave.h for tests/test_coarse_wave_cpu.py (no GPU, no HIP).
//
//   coarse_wave_test                 self-check, prints OK
//   coarse_wave_test consts          "cap threads inv_threads inv_max_nlist"
//   coarse_wave_test applies np nlist
//                                    "applies"
//   coarse_wave_test offsets nlist   "applies per_thread"
//
// The self-check walks k_inv_offsets' ownership (thread t takes the lists
// from min(t * per, nlist) to min(that + per, nlist)) and demands that every
// list is owned exactly once for every nlist the predicate admits.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dingo-store_amd/csrc/dg_coarse_wave.h"

static bool owned_once(int32_t nlist) {
  const int32_t per = dg_inv_offsets_per_thread(nlist);
  int64_t next = 0;  // the ranges must tile [0, nlist) in thread order
  for (int32_t t = 0; t < kInvOffsetsThreads; t++) {
    const int64_t lo = (int64_t)t * per < nlist ? (int64_t)t * per : nlist;
    const int64_t hi = lo + per < nlist ? lo + per : nlist;
    if (lo != next && lo != nlist) return false;
    if (lo < nlist) next = hi;
  }
  return next == nlist;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    for (int32_t nlist = 1; nlist <= kInvOffsetsMaxNlist; nlist++)
      if (!dg_inv_offsets_applies(nlist) || !owned_once(nlist)) {
        printf("FAIL offsets nlist %d\n", nlist);
        return 1;
      }
    if (dg_inv_offsets_applies(0) ||
        dg_inv_offsets_applies(kInvOffsetsMaxNlist + 1) ||
        kCoarseWaveMaxNp < 128 || kInvOffsetsMaxNlist < 65536 ||
        !dg_coarse_wave_applies(kCoarseWaveMaxNp, kCoarseWaveMaxNp + 1) ||
        dg_coarse_wave_applies(kCoarseWaveMaxNp + 1, 1 << 20) ||
        dg_coarse_wave_applies(32, 32) || dg_coarse_wave_applies(33, 32) ||
        !dg_coarse_wave_applies(31, 32) || !dg_coarse_wave_applies(1, 2) ||
        dg_coarse_wave_applies(0, 2) || dg_coarse_wave_applies(1, 1)) {
      printf("FAIL fixed points\n");
      return 1;
    }
    printf("OK\n");
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d %d %d\n", kCoarseWaveMaxNp, kCoarseWaveThreads,
           kInvOffsetsThreads, kInvOffsetsMaxNlist);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "applies")) {
    printf("%d\n",
           dg_coarse_wave_applies(atoi(argv[2]), atoi(argv[3])) ? 1 : 0);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "offsets")) {
    const int32_t nlist = atoi(argv[2]);
    printf("%d %d\n", dg_inv_offsets_applies(nlist) ? 1 : 0,
           dg_inv_offsets_per_thread(nlist));
    return 0;
  }
  fprintf(stderr,
          "usage: coarse_wave_test [consts | applies np nlist | "
          "offsets nlist]\n");
  return 2;
}
