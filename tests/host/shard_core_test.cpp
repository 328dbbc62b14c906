// shard_core_test.cpp — stand-alone driver of dingo-store_amd/csrc/
// dg_shard_core.h for tests/test_shard_core_cpu.py (no GPU, no HIP).
//
//   shard_core_test                      self-check, prints OK
//   shard_core_test shard S id...        dg_shard_of(id, S) per id
//   shard_core_test balance N S          rows per shard of ids 0 .. N-1
//   shard_core_test merge FILE           merges the lists in FILE
//
// FILE is text: "n_lists nq k_in k_out metric", then n_lists * nq * k_in
// lines "dist_bits_hex id" in [list][query][pos] order.  The answer is two
// blocks of nq * k_out lines "dist_bits_hex id": the scalar host merge, then
// the rank placement the GPU kernel performs (one dg_merge_rank per input
// element), which also verifies that the ranks of a query are a permutation.
//
// The self-check runs both on random lists with ties and pads and compares
// them; it is what a -fsanitize=address,undefined build of this file runs.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dingo-store_amd/csrc/dg_shard_core.h"

static uint32_t f2u(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float u2f(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// the kernel's work on the host: every input element places itself
static bool rank_place(int32_t n_lists, int64_t nq, int32_t k_in,
                       int32_t k_out, int32_t metric,
                       const std::vector<float>& dists,
                       const std::vector<int64_t>& ids,
                       std::vector<float>* out_dist,
                       std::vector<int64_t>* out_ids) {
  const int64_t per_q = (int64_t)n_lists * k_in;
  out_dist->assign((size_t)nq * k_out, -12345.f);
  out_ids->assign((size_t)nq * k_out, -777);
  std::vector<char> seen;
  for (int64_t q = 0; q < nq; q++) {
    seen.assign((size_t)per_q, 0);
    for (int32_t s = 0; s < n_lists; s++)
      for (int32_t p = 0; p < k_in; p++) {
        const int64_t rank = dg_merge_rank(dists.data(), ids.data(), n_lists,
                                           nq, k_in, metric, q, s, p);
        if (rank < 0 || rank >= per_q || seen[(size_t)rank]) {
          fprintf(stderr, "rank %" PRId64 " of (q %" PRId64 ", s %d, p %d) "
                  "is out of range or taken\n", rank, q, s, p);
          return false;
        }
        seen[(size_t)rank] = 1;
        const int64_t j = (int64_t)s * k_in + p;
        if (rank < k_out) {
          const int64_t self = dg_merge_list_base(nq, k_in, q, s) + p;
          const bool pad = ids[(size_t)self] < 0;
          (*out_dist)[(size_t)(q * k_out + rank)] =
              pad ? 0.0f : dists[(size_t)self];
          (*out_ids)[(size_t)(q * k_out + rank)] = pad ? -1 : ids[(size_t)self];
        }
        for (int64_t r = per_q + j; r < k_out; r += per_q) {
          (*out_dist)[(size_t)(q * k_out + r)] = 0.0f;
          (*out_ids)[(size_t)(q * k_out + r)] = -1;
        }
      }
  }
  return true;
}

static uint64_t g_rng = 0x1234567ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

static int self_check() {
  // routing: the finaliser of 0 is a published splitmix64 value
  if (dg_shard_hash(0) != 0xE220A8397B1DCDAFull) {
    fprintf(stderr, "dg_shard_hash(0) = %016" PRIx64 "\n", dg_shard_hash(0));
    return 1;
  }
  if (!(dg_order_f32(-0.0f) < dg_order_f32(0.0f)) ||
      dg_order_f32(-0.0f) + 1 != dg_order_f32(0.0f) ||
      !(dg_order_f32(-1.0f) < dg_order_f32(-0.0f)) ||
      !(dg_order_f32(3.0e38f) < dg_order_f32(u2f(0x7f800000u)))) {
    fprintf(stderr, "dg_order_f32 is not monotone\n");
    return 1;
  }
  const int shapes[][4] = {{1, 1, 1, 1},  {2, 3, 1, 1},   {3, 5, 10, 10},
                           {8, 2, 65, 10}, {32, 1, 7, 100}, {3, 4, 10, 40},
                           {4, 9, 5, 5},   {2, 1, 2048, 2048}};
  int cases = 0;
  for (const auto& sh : shapes)
    for (int metric = 0; metric < 2; metric++) {
      const int32_t L = sh[0], k_in = sh[2], k_out = sh[3];
      const int64_t nq = sh[1];
      std::vector<float> d((size_t)L * nq * k_in);
      std::vector<int64_t> id(d.size());
      for (int32_t t = 0; t < L; t++)
        for (int64_t q = 0; q < nq; q++) {
          // a sorted list from a small value set (ties across lists), a
          // random fill, the rest pads with dist 0.0
          const int32_t fill = (int32_t)(rnd() % (uint32_t)(k_in + 1));
          std::vector<int> v((size_t)fill);
          for (auto& e : v) e = (int)(rnd() % 7);
          for (size_t a = 1; a < v.size(); a++)  // insertion sort
            for (size_t b = a; b > 0 && v[b - 1] > v[b]; b--) {
              const int tmp = v[b];
              v[b] = v[b - 1];
              v[b - 1] = tmp;
            }
          const int64_t base = dg_merge_list_base(nq, k_in, q, t);
          for (int32_t p = 0; p < k_in; p++) {
            const bool real = p < fill;
            const float key = real ? (float)v[(size_t)p] * 0.5f : 0.0f;
            d[(size_t)(base + p)] = real && metric ? -key : key;
            id[(size_t)(base + p)] =
                real ? (int64_t)t * 100000 + q * 3000 + p : -1;
          }
        }
      std::vector<float> hd((size_t)nq * k_out), rd;
      std::vector<int64_t> hi((size_t)nq * k_out), ri;
      dg_merge_lists_host(L, nq, k_in, k_out, metric, d.data(), id.data(),
                          hd.data(), hi.data());
      if (!rank_place(L, nq, k_in, k_out, metric, d, id, &rd, &ri)) return 1;
      for (size_t i = 0; i < hd.size(); i++)
        if (f2u(hd[i]) != f2u(rd[i]) || hi[i] != ri[i]) {
          fprintf(stderr, "shape %d %d %d %d metric %d: slot %zu differs\n",
                  L, (int)nq, k_in, k_out, metric, i);
          return 1;
        }
      cases++;
    }
  printf("self-check: %d cases\nOK\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (!strcmp(argv[1], "shard") && argc >= 3) {
    const int32_t S = atoi(argv[2]);
    for (int i = 3; i < argc; i++)
      printf("%d\n", dg_shard_of((int64_t)strtoull(argv[i], nullptr, 0), S));
    return 0;
  }
  if (!strcmp(argv[1], "balance") && argc == 4) {
    const int64_t n = atoll(argv[2]);
    const int32_t S = atoi(argv[3]);
    std::vector<int64_t> cnt((size_t)S, 0);
    for (int64_t i = 0; i < n; i++) cnt[(size_t)dg_shard_of(i, S)]++;
    for (int32_t s = 0; s < S; s++) printf("%" PRId64 "\n", cnt[(size_t)s]);
    return 0;
  }
  if (!strcmp(argv[1], "merge") && argc == 3) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    int L, k_in, k_out, metric;
    long long nq;
    if (fscanf(f, "%d %lld %d %d %d", &L, &nq, &k_in, &k_out, &metric) != 5 ||
        L < 1 || L > 32 || nq < 1 || k_in < 1 || k_out < 1)
      return 2;
    std::vector<float> d((size_t)L * nq * k_in);
    std::vector<int64_t> id(d.size());
    for (size_t i = 0; i < d.size(); i++) {
      unsigned bits;
      long long v;
      if (fscanf(f, "%x %lld", &bits, &v) != 2) return 2;
      d[i] = u2f(bits);
      id[i] = v;
    }
    fclose(f);
    std::vector<float> hd((size_t)nq * k_out), rd;
    std::vector<int64_t> hi((size_t)nq * k_out), ri;
    dg_merge_lists_host(L, nq, k_in, k_out, metric, d.data(), id.data(),
                        hd.data(), hi.data());
    if (!rank_place(L, nq, k_in, k_out, metric, d, id, &rd, &ri)) return 3;
    for (size_t i = 0; i < hd.size(); i++)
      printf("%08x %lld\n", f2u(hd[i]), (long long)hi[i]);
    for (size_t i = 0; i < rd.size(); i++)
      printf("%08x %lld\n", f2u(rd[i]), (long long)ri[i]);
    return 0;
  }
  fprintf(stderr, "usage: see the head of shard_core_test.cpp\n");
  return 2;
}
