// dg_coarse_wave.h — when the one-pass coarse probe selection
// (k_coarse_select, DESIGN.md §Coarse probe selection) and the single-block
// inverted-offset scan (k_inv_offsets) apply.  No HIP here: the kernels, the
// host launcher and tests/host/coarse_wave_test.cpp all include this one
// definition.
//
// k_coarse_select keeps the np selected (key, list) pairs of a query in a
// fixed LDS array of kCoarseWaveMaxNp entries, so np is capped there; it
// selects, so it needs np < nlist (np == nlist probes every list and has no
// selection).  Any nlist is covered: the block loops over the row, and a row
// shorter than one wave only leaves lanes idle.  Everything else keeps
// k_select_dense + k_probe_unpack.
#pragma once
#include <cstdint>

constexpr int32_t kCoarseWaveMaxNp = 128;    // >= the default nprobe of 80
constexpr int32_t kCoarseWaveThreads = 256;  // 4 waves per query

constexpr bool dg_coarse_wave_applies(int32_t np, int32_t nlist) {
  return np >= 1 && np < nlist && np <= kCoarseWaveMaxNp;
}

// k_inv_offsets scans the per-list probe counts in one block, each thread
// taking ceil(nlist / kInvOffsetsThreads) consecutive lists; past this bound
// the serial part per thread would outgrow the launches it saves and the
// two-kernel scan + two cursor copies stay.
constexpr int32_t kInvOffsetsThreads = 1024;
constexpr int32_t kInvOffsetsMaxNlist = 65536;

constexpr bool dg_inv_offsets_applies(int32_t nlist) {
  return nlist >= 1 && nlist <= kInvOffsetsMaxNlist;
}

constexpr int32_t dg_inv_offsets_per_thread(int32_t nlist) {
  return (nlist + kInvOffsetsThreads - 1) / kInvOffsetsThreads;
}
