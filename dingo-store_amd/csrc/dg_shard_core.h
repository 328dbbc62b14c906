// dg_shard_core.h — shard routing and the merge order of the sharded index
// (dg_sharded_*, dg_merge_topk).  Header-only and free of HIP, like
// dg_batch_core.h: the host code, the merge kernel and the CPU test
// (tests/host/shard_core_test.cpp) all read the order from here, so there is
// one statement of it.  When a HIP compiler reads this file the functions are
// also device functions; nothing else changes.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DG_SHARD_HD __host__ __device__ inline
#else
#define DG_SHARD_HD inline
#endif

// ---- routing ----
// Stateless: the splitmix64 finaliser of the id, modulo the shard count.  An
// id always lives on the same shard, so upsert and remove route without a
// global map and ids stay unique across shards.
DG_SHARD_HD uint64_t dg_shard_hash(int64_t id) {
  uint64_t z = (uint64_t)id + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
DG_SHARD_HD int32_t dg_shard_of(int64_t id, int32_t n_shards) {
  return (int32_t)(dg_shard_hash(id) % (uint64_t)n_shards);
}

// ---- merge order ----
// n_lists best-first lists per query; element (list, pos) is smaller than
// another iff (is_pad, key, list, pos) is lexicographically smaller.  is_pad
// is id < 0; key is the order-preserving u32 image of the distance (L2) or of
// the negated score (IP, COSINE), the mapping of pack_cand / dec_f32 in
// kernels.hip.cpp: -0.0 sorts directly before +0.0, +inf after every finite
// value, and a real +inf still precedes every pad.  (is_pad, key) is packed
// into one integer, dg_merge_key; list and pos break its ties.
// Shard results tie-break by internal row and their pad rows carry dist 0.0,
// so under this order every shard's list is sorted whatever its own tie rule.
DG_SHARD_HD uint32_t dg_order_f32(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (int32_t)u < 0 ? ~u : (u | 0x80000000u);
}
// metric: 0 = L2 (distance as it is), otherwise the score is negated
DG_SHARD_HD uint64_t dg_merge_key(int32_t metric, float dist, int64_t id) {
  uint32_t u;
  memcpy(&u, &dist, 4);
  if (metric != 0) u ^= 0x80000000u;
  float key;
  memcpy(&key, &u, 4);
  return ((uint64_t)(id < 0 ? 1 : 0) << 32) | dg_order_f32(key);
}

// Layout of the inputs: dists / ids are [n_lists][nq][k_in], so list t of
// query q starts at ((t * nq) + q) * k_in.
DG_SHARD_HD int64_t dg_merge_list_base(int64_t nq, int32_t k_in, int64_t q,
                                       int32_t t) {
  return ((int64_t)t * nq + q) * k_in;
}

// number of elements of one sorted list whose key is < key (strict) or
// <= key (!strict)
DG_SHARD_HD int32_t dg_merge_bound(const float* dists, const int64_t* ids,
                                   int32_t k_in, int32_t metric, uint64_t key,
                                   bool strict) {
  int32_t lo = 0, hi = k_in;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const uint64_t m = dg_merge_key(metric, dists[mid], ids[mid]);
    if (strict ? m < key : m <= key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Rank placement: the final position of element (q, s, p) among the
// n_lists * k_in elements of query q.  Lists before s contribute their
// elements <= e (they win ties), lists after s their elements < e, and s
// itself the p elements in front.  The order being total, the ranks of one
// query are a permutation of 0 .. n_lists * k_in - 1.
DG_SHARD_HD int64_t dg_merge_rank(const float* dists, const int64_t* ids,
                                  int32_t n_lists, int64_t nq, int32_t k_in,
                                  int32_t metric, int64_t q, int32_t s,
                                  int32_t p) {
  const int64_t self = dg_merge_list_base(nq, k_in, q, s) + p;
  const uint64_t key = dg_merge_key(metric, dists[self], ids[self]);
  int64_t rank = p;
  for (int32_t t = 0; t < n_lists; t++) {
    if (t == s) continue;
    const int64_t b = dg_merge_list_base(nq, k_in, q, t);
    rank += dg_merge_bound(dists + b, ids + b, k_in, metric, key, t > s);
  }
  return rank;
}

// ---- the merge, stated on the host ----
// Scalar n-way merge under the same order: the reference the kernel
// (k_merge_lists, which places by dg_merge_rank) is tested against.  Real
// elements keep their distance bits; pads come out as -1 / 0.0f, also in the
// slots at or beyond n_lists * k_in.
#if !defined(__HIP_DEVICE_COMPILE__)
inline void dg_merge_lists_host(int32_t n_lists, int64_t nq, int32_t k_in,
                                int32_t k_out, int32_t metric,
                                const float* dists, const int64_t* ids,
                                float* out_dist, int64_t* out_ids) {
  int32_t head[32];
  for (int64_t q = 0; q < nq; q++) {
    for (int32_t t = 0; t < n_lists; t++) head[t] = 0;
    for (int32_t r = 0; r < k_out; r++) {
      int32_t best = -1;
      uint64_t best_key = 0;
      for (int32_t t = 0; t < n_lists; t++) {
        if (head[t] >= k_in) continue;
        const int64_t i = dg_merge_list_base(nq, k_in, q, t) + head[t];
        const uint64_t key = dg_merge_key(metric, dists[i], ids[i]);
        if (best < 0 || key < best_key) {  // ties stay with the smaller list
          best = t;
          best_key = key;
        }
      }
      float od = 0.0f;
      int64_t oi = -1;
      if (best >= 0) {
        const int64_t i = dg_merge_list_base(nq, k_in, q, best) + head[best]++;
        if (ids[i] >= 0) {
          od = dists[i];
          oi = ids[i];
        }
      }
      out_dist[q * k_out + r] = od;
      out_ids[q * k_out + r] = oi;
    }
  }
}
#endif
