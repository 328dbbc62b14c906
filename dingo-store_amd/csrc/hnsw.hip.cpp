// hnsw.hip.cpp — k_hnsw_search, the graph search of DG_INDEX_HNSW on gfx950.
//
// One wave per query (a block is one wave, so the kernel has no block-wide
// barrier at all).  The kernel restates the reference search of
// dg_hnsw_core.h exactly: greedy descent on the upper
// levels, then the level-0 beam with the candidate set C and the result set W
// as two ascending arrays of packed (key bits << 32 | node) in LDS, sized
// from ef' at launch.  A popped node's unvisited neighbours are collected
// with one returning vector atomic per lane on the query's own exact visited
// bitmap, their rows are gathered four at a time by the whole wave (16 B per
// lane per load, the loads of four rows issued before the first reduction),
// and they are admitted one after the other in list order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_internal.h"

namespace {

constexpr int kWave = 64;
constexpr int kNbMax = 256;  // maxM0 of nlinks = 128

__device__ __forceinline__ uint32_t h_enc_f32(float x) {
  uint32_t u = __float_as_uint(x);
  return (int32_t)u < 0 ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float h_dec_f32(uint32_t e) {
  uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t h_pack(float key, uint32_t node) {
  return ((uint64_t)h_enc_f32(key) << 32) | node;
}

// The lanes of one wave run in lockstep and the LDS serves a wave's
// instructions in order; what is left to do is to keep the compiler from
// moving LDS accesses across the point where lanes exchange data.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// ascending array a[0..cnt): insert x (no equal element exists: a node
// enters each array once)
__device__ __forceinline__ void sorted_insert(uint64_t* a, int& cnt,
                                              uint64_t x, int lane) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  for (int top = cnt; top > lo; top -= kWave) {  // top chunk first
    const int i = top - 1 - lane;
    const bool act = i >= lo;
    uint64_t v = 0;
    if (act) v = a[i];
    wave_sync();
    if (act) a[i + 1] = v;
    wave_sync();
  }
  if (lane == 0) a[lo] = x;
  wave_sync();
  cnt++;
}

__device__ __forceinline__ void pop_front(uint64_t* a, int& cnt, int lane) {
  for (int base = 1; base < cnt; base += kWave) {
    const int i = base + lane;
    const bool act = i < cnt;
    uint64_t v = 0;
    if (act) v = a[i];
    wave_sync();
    if (act) a[i - 1] = v;
    wave_sync();
  }
  cnt--;
}

// keys of the rows nb_node[0..m) into nb_key: the whole wave on each row,
// four rows in flight
template <bool kL2>
__device__ __forceinline__ void compute_keys(const float* __restrict__ rows,
                                             int32_t d, const float* q,
                                             const uint32_t* nb_node,
                                             float* nb_key, int m, int lane) {
  const int d4 = d >> 2;
  const float4* q4 = (const float4*)q;
  for (int j = 0; j < m; j += 4) {
    const float4* r0 = (const float4*)(rows + (size_t)nb_node[j] * d);
    const float4* r1 =
        (const float4*)(rows + (size_t)nb_node[min(j + 1, m - 1)] * d);
    const float4* r2 =
        (const float4*)(rows + (size_t)nb_node[min(j + 2, m - 1)] * d);
    const float4* r3 =
        (const float4*)(rows + (size_t)nb_node[min(j + 3, m - 1)] * d);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = lane; i < d4; i += kWave) {
      const float4 x0 = r0[i], x1 = r1[i], x2 = r2[i], x3 = r3[i];
      const float4 qv = q4[i];
      if (kL2) {
        float t;
        t = qv.x - x0.x; a0 += t * t; t = qv.y - x0.y; a0 += t * t;
        t = qv.z - x0.z; a0 += t * t; t = qv.w - x0.w; a0 += t * t;
        t = qv.x - x1.x; a1 += t * t; t = qv.y - x1.y; a1 += t * t;
        t = qv.z - x1.z; a1 += t * t; t = qv.w - x1.w; a1 += t * t;
        t = qv.x - x2.x; a2 += t * t; t = qv.y - x2.y; a2 += t * t;
        t = qv.z - x2.z; a2 += t * t; t = qv.w - x2.w; a2 += t * t;
        t = qv.x - x3.x; a3 += t * t; t = qv.y - x3.y; a3 += t * t;
        t = qv.z - x3.z; a3 += t * t; t = qv.w - x3.w; a3 += t * t;
      } else {
        a0 += qv.x * x0.x + qv.y * x0.y + qv.z * x0.z + qv.w * x0.w;
        a1 += qv.x * x1.x + qv.y * x1.y + qv.z * x1.z + qv.w * x1.w;
        a2 += qv.x * x2.x + qv.y * x2.y + qv.z * x2.z + qv.w * x2.w;
        a3 += qv.x * x3.x + qv.y * x3.y + qv.z * x3.z + qv.w * x3.w;
      }
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    a3 = wave_sum(a3);
    if (lane < 4 && j + lane < m) {
      const float s = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
      nb_key[j + lane] = kL2 ? s : 0.0f - s;
    }
  }
  wave_sync();
}

template <bool kL2>
__global__ __launch_bounds__(kWave) void k_hnsw_search(
    const dgk::hnsw_graph g, const float* __restrict__ queries,
    int32_t d_user, int32_t k, int32_t efp, uint32_t* __restrict__ visited,
    int64_t vwords, float* __restrict__ out_dist,
    int64_t* __restrict__ out_ids, unsigned long long* __restrict__ counters,
    int32_t* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const int32_t d = g.d;
  float* q = (float*)smem;
  uint64_t* C = (uint64_t*)(smem + (size_t)d * 4);
  uint64_t* W = C + efp;
  uint32_t* nb_node = (uint32_t*)(W + efp + 2);
  float* nb_key = (float*)(nb_node + kNbMax);
  uint32_t* nb_adm = (uint32_t*)(nb_key + kNbMax);
  uint32_t* vis = visited + qi * vwords;
  const uint32_t n = (uint32_t)g.n;

  // the query: pad columns are zero; cosine: x * (1 / (sqrt(sum x^2) + 1e-30))
  {
    const float* qsrc = queries + qi * (int64_t)d_user;
    float s = 0.f;
    for (int j = lane; j < d; j += kWave) {
      const float v = j < d_user ? qsrc[j] : 0.f;
      q[j] = v;
      s += v * v;
    }
    if (g.metric == DG_METRIC_COSINE) {
      const float inv = 1.0f / (sqrtf(wave_sum(s)) + 1e-30f);
      for (int j = lane; j < d; j += kWave) q[j] *= inv;
    }
  }
  wave_sync();

  unsigned long long expansions = 0, evals = 0;
  bool bad = false;
  int cntC = 0, cntW = 0;

  if (lane == 0) nb_node[0] = (uint32_t)g.entry;
  wave_sync();
  compute_keys<kL2>(g.rows, d, q, nb_node, nb_key, 1, lane);
  evals = 1;
  uint64_t cur = h_pack(nb_key[0], (uint32_t)g.entry);
  wave_sync();

  // ---- upper levels: greedy, deleted flags and filters play no part ----
  for (int32_t level = g.max_level; level >= 1 && !bad; level--) {
    for (uint32_t step = 0;; step++) {
      const uint32_t c = (uint32_t)cur;
      if (step > n || g.levels[c] < level) {
        bad = true;
        break;
      }
      const int64_t li = g.up_off[c] + level - 1;
      const int m = min(max(g.up_cnt[li], 0), g.maxM);
      for (int t = lane; t < m; t += kWave) {
        const uint32_t e = g.up_links[li * g.maxM + t];
        if (e >= n) bad = true;
        nb_node[t] = e < n ? e : c;
      }
      bad = __any(bad);
      wave_sync();
      compute_keys<kL2>(g.rows, d, q, nb_node, nb_key, m, lane);
      evals += m;
      uint64_t best = cur;
      for (int t = lane; t < m; t += kWave)
        best = min(best, h_pack(nb_key[t], nb_node[t]));
      for (int off = 32; off; off >>= 1)
        best = min(best, (uint64_t)__shfl_xor((long long)best, off, kWave));
      wave_sync();
      if (best == cur || bad) break;
      cur = best;
    }
  }

  // ---- level 0 ----
  if (!bad) {
    const uint32_t ep = (uint32_t)cur;
    if (lane == 0) {
      atomicOr(&vis[ep >> 5], 1u << (ep & 31));
      C[0] = cur;
      if ((g.pass[ep >> 5] >> (ep & 31)) & 1) W[0] = cur;
    }
    cntC = 1;
    cntW = (int)((g.pass[ep >> 5] >> (ep & 31)) & 1);
    wave_sync();
    // a node enters C once at most, so n pops end every search; the cap
    // keeps a corrupt graph or a bug from spinning on a shared machine
    for (uint32_t iter = 0; cntC > 0; iter++) {
      const uint64_t c0 = C[0];
      if (cntW == efp && c0 > W[cntW - 1]) break;
      if (iter > n) {
        bad = true;
        break;
      }
      wave_sync();
      pop_front(C, cntC, lane);
      expansions++;
      const uint32_t c = (uint32_t)c0;
      const int cnt = min(max(g.cnt0[c], 0), g.maxM0);
      int m = 0;
      for (int base = 0; base < cnt; base += kWave) {
        const int t = base + lane;
        bool fresh = false;
        uint32_t e = 0;
        if (t < cnt) {
          e = g.links0[(size_t)c * g.maxM0 + t];
          if (e < n) {
            const uint32_t bit = 1u << (e & 31);
            fresh = !(atomicOr(&vis[e >> 5], bit) & bit);
          } else {
            bad = true;
          }
        }
        const uint64_t mask = __ballot(fresh);
        if (fresh) {
          const int at = m + __popcll(mask & ((1ull << lane) - 1));
          nb_node[at] = e;
          nb_adm[at] = (g.pass[e >> 5] >> (e & 31)) & 1;
        }
        m += __popcll(mask);
      }
      bad = __any(bad);
      if (bad) break;
      wave_sync();
      compute_keys<kL2>(g.rows, d, q, nb_node, nb_key, m, lane);
      evals += m;
      for (int j = 0; j < m; j++) {
        const uint64_t x = h_pack(nb_key[j], nb_node[j]);
        const bool adm = nb_adm[j] != 0;
        if (cntW < efp || x < W[cntW - 1]) {
          if (cntC < efp) {
            sorted_insert(C, cntC, x, lane);
          } else if (x < C[cntC - 1]) {
            cntC--;
            sorted_insert(C, cntC, x, lane);
          }
          if (adm) {
            sorted_insert(W, cntW, x, lane);
            if (cntW > efp) cntW--;
          }
        }
      }
    }
  }
  wave_sync();

  if (bad) {
    if (lane == 0) atomicOr(flag, 1);
    cntW = 0;
  }
  for (int i = lane; i < k; i += kWave) {
    float dist = 0.f;
    int64_t id = -1;
    if (i < cntW) {
      const uint64_t w = W[i];
      const float key = h_dec_f32((uint32_t)(w >> 32));
      dist = kL2 ? key : -key;
      id = g.ids[(uint32_t)w];
    }
    out_dist[qi * k + i] = dist;
    out_ids[qi * k + i] = id;
  }
  if (lane == 0) {
    atomicAdd(&counters[0], expansions);
    atomicAdd(&counters[1], evals);
  }
}

}  // namespace

namespace dgk {

size_t hnsw_search_lds(int32_t d, int32_t efp) {
  return (size_t)d * 4 + ((size_t)2 * efp + 2) * 8 + (size_t)kNbMax * 12;
}

void hnsw_search(hipStream_t s, const hnsw_graph& g, const float* queries,
                 int64_t nq, int32_t d_user, int32_t k, int32_t efp,
                 uint32_t* visited, int64_t vwords, float* out_dist,
                 int64_t* out_ids, unsigned long long* counters,
                 int32_t* flag) {
  const size_t lds = hnsw_search_lds(g.d, efp);
  if (g.metric == DG_METRIC_L2)
    hipLaunchKernelGGL(k_hnsw_search<true>, dim3((unsigned)nq), dim3(kWave),
                       lds, s, g, queries, d_user, k, efp, visited, vwords,
                       out_dist, out_ids, counters, flag);
  else
    hipLaunchKernelGGL(k_hnsw_search<false>, dim3((unsigned)nq), dim3(kWave),
                       lds, s, g, queries, d_user, k, efp, visited, vwords,
                       out_dist, out_ids, counters, flag);
}

}  // namespace dgk
